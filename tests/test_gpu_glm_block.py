"""A correlation block of three or four factor terms (GLM(..., correlated=[glm.block(..)]), idhmc_create_glm_block) on
the device.  Models with a sampled K x K correlation matrix among K terms are bit-identical to the CPU oracle running the C restatement
of section 26 (tests/test_glm_block_cpu.py, through oracle.OracleModel.custom, fed the expanded matrix of glm.expand_factors) and within
1e-12 of numpy, in both device forms: one chain per wavefront (evaluation, leapfrog, the stepsize search; NUTS at L >= 512) and the
matrix-core gradient of the NUTS kernel, under both metrics.  No tolerance on the device side.  Then: a K = 2 block against an engine
built with glm.pair, the create function with no block, several responses, the device summaries of [beta | a | sigma | R | phi], and
exact stationarity on a model whose posterior is its LKJ prior.  Every context compiles its source with hipRTC."""
import ctypes as C

import numpy as np
import pytest
from scipy import special, stats

import stationarity as S
import test_glm_struct_cpu as STRUCT
from test_glm_block_cpu import (betas, c_source_block, make_block, numpy_density_block, nz_of, oracle_params_block, start_block)
from test_glm_hier_cpu import SHAPE, consts
from test_glm_priors_cpu import LOG_HALF_STUDENT_T, NORMAL, STUDENT_T
from test_gpu_glm_corr import NULL_SOURCE, fma_twin
from test_gpu_glm_factors import SHORT, same_bits
from test_gpu_glm_slopes import run_engines
from test_gpu_summary import assert_histogram, assert_summary
from test_summary_cpu import range_twin, summary_twin

pytestmark = pytest.mark.gpu

# name: (family, Dd, (levels, valued, index it is drawn on) per term, the group of each term (None: no groups), the block's rows as term
# indices, eta, local scales with a slab on the columns of this ROW (or None), the term with an AR(1) structure (or None), D, padded
# length, matrix cores)
SHAPES = {
    "one tile": ("POISSON_LOG", 20, ((15, False, 0), (15, True, 0), (15, True, 0)), (0, 1, 2), (0, 1, 2), 2.0, None, None, 71, 128, 1),
    "across 128": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, ((20, False, 0), (20, True, 1), (20, True, 0), (20, True, 1)), (0, 1, 2, 3), (2, 0, 3, 1), 2.0,
                   None, None, 191, 256, 1),
    "L = 512": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, ((120, False, 0), (120, True, 0), (120, True, 0)), (0, 1, 2), (0, 1, 2), 1.0, None, None, 467, 512, 0),
    "no groups": ("POISSON_LOG", 1, ((5, False, 0), (5, True, 0), (5, False, 1)), None, (0, 1, 2), 2.0, None, None, 1 + 15 + 3, 128, 1),
    "prior arrays": ("POISSON_LOG", 8, ((6, False, 0), (6, True, 0), (6, True, 0)), (0, 1, 2), (1, 2, 0), 0.0, None, None, 8 + 18 + 3 + 3, 128, 1),
    "local": ("POISSON_LOG", 10, ((12, False, 0), (12, True, 0), (12, True, 0)), (0, 1, 2), (0, 1, 2), 2.0, 1, None, 10 + 36 + 3 + 12 + 3, 128, 1),
    "local per wave": ("POISSON_LOG", 100, ((90, False, 0), (90, True, 0), (90, True, 0)), (0, 1, 2), (0, 1, 2), 2.0, 1, None,
                       100 + 270 + 3 + 90 + 3, 512, 0),
    "ar1": ("POISSON_LOG", 8, ((6, False, 0), (6, True, 0), (6, True, 0), (9, False, 1)), (0, 1, 2, 3), (0, 1, 2), 2.0, None, 3,
            8 + 27 + 4 + 3 + 1, 128, 1),
}
BIG = ("POISSON_LOG", 100, ((300, False, 0), (300, True, 0), (300, True, 0)), (0, 1, 2), (0, 1, 2), 2.0, None, None, 1006, 1024, 0)
SLAB = 2.0
AR_ETA = 2.0
C_ = 18


def spec(shape):
    return BIG if shape == "L = 1024" else SHAPES[shape]


def dims(shape):
    """Dx, A, H, J, nz, Sz"""
    family, Dd, terms, groups, order, eta, loc, ar, D, L, form = spec(shape)
    Dx = Dd + sum(t[0] for t in terms)
    return (Dx, SHAPE[family][2], 0 if groups is None else max(groups) + 1, 0 if loc is None else terms[order[loc]][0], nz_of(len(order)),
            0 if ar is None else 1)


def offsets(shape):
    family, Dd, terms = spec(shape)[:3]
    return [Dd + sum(t[0] for t in terms[:f]) for f in range(len(terms))]


def row_offsets(shape):
    """the first column of the term in each row of the block"""
    off = offsets(shape)
    return [off[t] for t in spec(shape)[4]]


def problem(idhmc, shape, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,), local (Dx,) or None, slab): data from the family's own model; values are 0.5 N(0, 1), terms with
    the same index id share one index array"""
    family, Dd, terms, groups, order, eta, loc, ar, D, L, form = spec(shape)
    rng = np.random.default_rng(n + Dd if seed is None else seed)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    z = X @ (0.5 * rng.standard_normal(Dd) / np.sqrt(Dd))
    index, factors = {}, []
    for N, valued, iid in terms:
        if iid not in index or index[iid].max() >= N:
            index[iid] = rng.integers(0, N, n)
        idx, w = index[iid], 0.5 * rng.standard_normal(n)
        z = z + (w if valued else 1.0) * (0.3 * rng.standard_normal(N))[idx]
        factors.append(idhmc.glm.term(idx, values=w, levels=N) if valued else (idx, N))
    Y = rng.poisson(np.exp(z)).astype(float) if family == "POISSON_LOG" else z + 0.5 * rng.standard_normal(n)
    Dx, off = dims(shape)[0], offsets(shape)
    grp = np.full(Dx, -1, np.int32)
    if groups is not None:
        for f, g in enumerate(groups):
            grp[off[f]:off[f] + terms[f][0]] = g
    local = None
    if loc is not None:
        local = np.zeros(Dx, np.int32)
        o = row_offsets(shape)[loc]
        local[o:o + terms[order[loc]][0]] = 1
    return X, Y, factors, grp, local, SLAB if loc is not None else None


def shape_priors(shape, eta=None):
    """normal and Student-t on u, log half-t on the scales and the lambdas, the defaults on the block's zetas with eta > 0 and on the
    AR(1) zeta, Student-t(3) entries on the block's zetas with eta = 0"""
    Dx, A, H, J, nz, Sz = dims(shape)
    D = spec(shape)[8]
    eta = spec(shape)[5] if eta is None else eta
    rng = np.random.default_rng(D)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:Dx:2] = STUDENT_T
    kind[Dx + A:D - nz - Sz] = LOG_HALF_STUDENT_T
    nu[kind == STUDENT_T], nu[kind == LOG_HALF_STUDENT_T] = 4.0, 3.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx + A:D - nz - Sz] = 1.0
    z0 = D - nz - Sz
    if eta > 0.0:
        kind[z0:z0 + nz], nu[z0:z0 + nz], mu[z0:z0 + nz], tau[z0:z0 + nz] = NORMAL, 0.0, 0.0, 1.0
    else:
        kind[z0:z0 + nz], nu[z0:z0 + nz] = STUDENT_T, 3.0
    kind[D - Sz:], nu[D - Sz:], mu[D - Sz:], tau[D - Sz:] = NORMAL, 0.0, 0.0, 1.0
    return kind, nu, mu, tau


def structs_of(shape):
    """(off, N, kind) of the structured slot, for the restatement"""
    ar = spec(shape)[7]
    return () if ar is None else ((offsets(shape)[ar], spec(shape)[2][ar][0], STRUCT.AR1),)


def model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, correlated="shape", **kw):
    g = idhmc.glm
    family, Dd, terms, groups, order, eta, loc, ar = spec(shape)[:8]
    corr = [g.block(order, eta)] if correlated == "shape" else correlated
    if ar is not None:
        kw.setdefault("structured", [g.ar1(ar, AR_ETA)])
    return make_block(idhmc, family, X, Y, factors, None if groups is None else grp, local, slab, kind, nu, mu, tau, corr, **kw)


def oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau):
    family, D = spec(shape)[0], spec(shape)[8]
    Xe = idhmc.glm.expand_factors(X, factors)
    st = structs_of(shape)
    N = spec(shape)[2][spec(shape)[4][0]][0]
    return oracle.OracleModel.custom(D, c_source_block(family),
                                     oracle_params_block(Xe, Y, SHAPE[family][2], grp, local, slab, kind, nu, row_offsets(shape), N, spec(shape)[5], st,
                                                         [AR_ETA] * len(st), consts(family), mu, tau), str(tmp_path))


def start(shape, n_chains, seed=0):
    """start_block with zetas of both signs in every chain"""
    Dx, A, H, J, nz, Sz = dims(shape)
    q = start_block(spec(shape)[0], n_chains, Dx, H, J, nz, seed, Sz=Sz)
    z0 = q.shape[1] - nz - Sz
    q[:, z0], q[:, z0 + 1] = np.abs(q[:, z0]) + 0.1, -np.abs(q[:, z0 + 1]) - 0.1
    return q


def check_numpy(idhmc, eng, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, ends):
    family = spec(shape)[0]
    if spec(shape)[7] is not None:
        return                                              # (next to a structure the twin alone is the reference)
    Xe = idhmc.glm.expand_factors(X, factors)
    N = spec(shape)[2][spec(shape)[4][0]][0]
    q, g, lq = eng.q, eng.grad, eng.lq
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_block(family, Xe, Y, q[c], grp, np.zeros(Xe.shape[1], int) if local is None else local, slab, kind,
                                                           nu, row_offsets(shape), N, spec(shape)[5], mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


def test_the_shapes_are_what_they_are_there_for(idhmc):
    lane = lambda c: ((c & 127) >> 1, c >> 7, c & 1)           # lane, chunk, component of a coordinate
    for name in list(SHAPES) + ["L = 1024"]:
        family, Dd, terms, groups, order, eta, loc, ar, D, L, form = spec(name)
        Dx, A, H, J, nz, Sz = dims(name)
        assert Dx + A + H + J + nz + Sz == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))), name
        assert len(set(order)) == len(order) and len({terms[t][0] for t in order}) == 1 and (ar is None or ar not in order)
    assert [spec(s)[8] for s in ("one tile", "across 128", "L = 512", "L = 1024")] == [71, 191, 467, 1006]
    # "one tile": partners 15 and 30 columns away, in other lanes, one index array
    assert row_offsets("one tile") == [20, 35, 50] and all(lane(c)[0] != lane(c + 15)[0] != lane(c + 30)[0] for c in range(20, 35))
    X, Y, factors, grp, local, slab = problem(idhmc, "one tile", 130)
    assert factors[0][0] is factors[1].index is factors[2].index
    # "across 128": rows (2, 0, 3, 1) -> first columns 140, 100, 160, 120: rows not in term order, row 3's partners behind it and in front,
    # row 3 (columns 120..139) on both sides of column 128, two index arrays
    assert row_offsets("across 128") == [140, 100, 160, 120] and {lane(c)[1] for c in range(120, 140)} == {0, 1}
    assert {lane(c)[1] for c in range(100, 120)} == {0} and {lane(c)[1] for c in range(140, 180)} == {1}
    X, Y, factors, grp, local, slab = problem(idhmc, "across 128", 130)
    assert factors[0][0] is factors[2].index and factors[1].index is factors[3].index and factors[0][0] is not factors[1].index
    # "L = 512": 3 x 120 levels over chunks 0 .. 3, the zetas in chunk 3
    assert row_offsets("L = 512") == [100, 220, 340] and lane(464)[1] == 3 and any(lane(c)[1] != lane(c + 120)[1] for c in range(100, 220))
    # "L = 1024": chunks 4 .. 7 hold columns and the zetas
    assert row_offsets("L = 1024") == [100, 400, 700] and lane(700)[1] == 5 and lane(1003)[1] == 7
    # "prior arrays": eta = 0 and Student-t(3) entries on the zetas; "local": the slab's local scales on row 1's columns
    kind, nu, mu, tau = shape_priors("prior arrays")
    assert list(kind[-3:]) == [STUDENT_T] * 3 and list(nu[-3:]) == [3.0] * 3 and spec("prior arrays")[5] == 0.0
    X, Y, factors, grp, local, slab = problem(idhmc, "local", 130)
    assert slab == SLAB and list(np.flatnonzero(local)) == list(range(22, 34)) and row_offsets("local")[1] == 22
    # "local per wave": the same at L = 512, the second mix under kLocal in the per-wave form
    X, Y, factors, grp, local, slab = problem(idhmc, "local per wave", 37)
    assert list(np.flatnonzero(local)) == list(range(190, 280)) and spec("local per wave")[9:] == (512, 0)
    # "ar1": the block's zetas, then the AR(1) zeta
    assert dims("ar1") == (35, 0, 4, 0, 3, 1) and structs_of("ar1") == ((26, 9, STRUCT.AR1),) and dims("no groups")[2] == 0
    q = start("ar1", 4)
    assert np.all(q[:, -4] > 0) and np.all(q[:, -3] < 0)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1, 130])
def test_density_leapfrog_search_and_nuts(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the shape runs, then the stepsize search: bit-identical to oracle chains on the C
    twin, within 1e-12 of numpy"""
    family, Dd, terms, groups, order, eta, loc, ar, D, L, form = SHAPES[shape]
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    assert (m.D, m.BK, m.Bz, m.P, m.Dx) == (D, len(order), nz_of(len(order)), 0, dims(shape)[0])
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D
    bt, be = eng.glm_block()
    assert bt.dtype == np.int32 and list(bt) == list(order) and be == eta and eng.glm_pairs() == (None, None, None)
    assert np.array_equal(eng.glm_priors()[0], kind) and np.array_equal(eng.glm_priors()[1], nu)       # the public kinds: no 5 comes back
    args = (idhmc, eng, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, (0, C_ - 1))
    q = start(shape, C_)
    eng.set_q(q)
    check_numpy(*args)
    run_engines([eng], chains, D, q, shape)
    check_numpy(*args)
    eng.refresh_momentum(0)
    eng.find_initial_stepsize()
    ref = []
    for ch in chains:
        ch.rand_p(0)
        rc, e = ch.find_initial_stepsize()
        assert rc == 0
        ref.append(e)
    assert same_bits(eng.eps, ref) and eng.poll_abort() == 0
    eng.close()


@pytest.mark.parametrize("shape", ["across 128", "L = 512"])
def test_shared_metric(idhmc, oracle, tmp_path, shape):
    """the same stages on a shared unit metric (METRIC_SHARED: the other instantiation of the NUTS kernel), in both forms"""
    family, Dd, terms, groups, order, eta, loc, ar, D, L, form = SHAPES[shape]
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4, metric_mode=idhmc.METRIC_SHARED), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.padded_dim() == L
    run_engines([eng], chains, D, start(shape, C_), shape)
    eng.close()


def test_chunks_past_the_fourth(idhmc, oracle, tmp_path):
    """K = 3 with 3 x 300 levels, D = 1006, L = 1024 (NCH = 8, the shared metric): columns, partners and the zetas in chunks 4 .. 7; 8
    oracle chains.  The one test at this size: its time is the hipRTC compile."""
    shape = "L = 1024"
    family, Dd, terms, groups, order, eta, loc, ar, D, L, form = BIG
    n_chains = 8
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    eng = idhmc.Engine(m, n_chains, idhmc.default_options(max_depth=4, metric_mode=idhmc.METRIC_SHARED), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(n_chains)]
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D == 1006
    run_engines([eng], chains, D, start(shape, n_chains), shape)
    eng.close()


# ---- the anchor: a block of two is the pair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Dd,form", [(15, 20, 1), (150, 100, 0)], ids=["matrix-cores", "per-wave"])
def test_a_block_of_two_is_the_pair(idhmc, N, Dd, form):
    """the same data, priors and seed through glm.block((0, 1)) and through glm.pair(0, 1): after a short warm-up the draws, the tree
    statistics and the stepsizes are bit-equal, in both forms"""
    g = idhmc.glm
    rng = np.random.default_rng(N)
    n, n_chains, draws_n = 60, 8, 6
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    s = rng.integers(0, N, n)
    w = 0.5 * rng.standard_normal(n)
    Y = rng.poisson(np.exp(0.3 * rng.standard_normal(n))).astype(float)
    factors = [(s, N), g.term(s, values=w, levels=N)]
    kw = g.correlated_effects(Dd, [N, N], [(0, 1)], eta=1.5, scale=g.half_student_t(3))
    kb = dict(kw, correlated=[g.block((0, 1), 1.5)])
    out = []
    for k in (kw, kb):
        eng = idhmc.Engine(idhmc.GLM(X, Y, g.POISSON_LOG, factors=factors, **k), n_chains, idhmc.default_options(**SHORT), seed=77)
        assert eng.glm_form() == form
        draws, st = eng.mcmc_with_warmup(draws_n)
        out.append((draws, st, eng.eps, eng.lq, eng.grad))
        assert eng.poll_abort() == 0
        eng.close()
    (d0, s0, e0, l0, g0), (d1, s1, e1, l1, g1) = out
    assert same_bits(d0, d1) and np.array_equal(s0, s1) and same_bits(e0, e1) and same_bits(l0, l1) and same_bits(g0, g1)
    assert len(np.unique(e0)) > 1 and np.isfinite(d0).all()


def test_no_block_through_the_new_entry_point(idhmc):
    """idhmc_create_glm_block with block = NULL, and with K = 0 and term NULL, against the same model through the entry point Engine
    takes for it: the same form, footprint and bits"""
    from inplacedhmc_jl_amd import _lib
    shape = "one tile"
    family, Dd, terms, groups, order, eta, loc, ar, D, L, form = SHAPES[shape]
    n = 130
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind[:-3], nu[:-3], mu[:-3], tau[:-3], correlated=None)
    assert m.BK == 0 and m.D == D - 3
    opt = idhmc.default_options(max_depth=4)
    lib = idhmc.load_library()
    ip = C.POINTER(C.c_int32)
    engs = [idhmc.Engine(m, C_, opt, seed=3)]
    for bk in (None, _lib.GlmBlock(K=0)):
        desc = m.glm_desc()
        pr = _lib.GlmPriors(kind=m.prior_kind.ctypes.data_as(ip), nu=m.prior_nu.ctypes.data_as(C.POINTER(C.c_double)))
        fc = _lib.GlmFactors(F=m.F, levels=m.levels.ctypes.data_as(ip), index=m.factor_index.ctypes.data_as(ip))
        fv = _lib.GlmFactorValues(values=m.factor_values.ctypes.data_as(C.POINTER(C.c_double)), has=m.factor_has.ctypes.data_as(ip))
        h = C.c_void_p()
        _lib.check(lib.idhmc_create_glm_block(C.byref(h), 0, C_, 0, C.byref(desc), C.byref(pr), None, C.byref(fc), C.byref(fv), None, None, None,
                                              None if bk is None else C.byref(bk), 1, 0, C.byref(opt), 3))
        eng = idhmc.Engine._adopt(m, h, C_, opt)     # an Engine around that context
        engs.append(eng)
    for e in engs:
        assert e.glm_form() == form and e.glm_block() == (None, None) and e.glm_pairs() == (None, None, None)
    assert engs[0].device_bytes() == engs[1].device_bytes() == engs[2].device_bytes()
    run_engines(engs, None, D - 3, start(shape, C_)[:, :-3], shape)
    for e in engs:
        e.close()


def test_responses_are_single_response_oracle_chains(idhmc, oracle, tmp_path):
    """M = 3 responses of R = 2 chains on "one tile": every chain is bit-identical to the single-response oracle chain on its Y (the
    same global chain id)"""
    shape = "one tile"
    family, Dd, terms, groups, order, eta, loc, ar, D, L, form = SHAPES[shape]
    M, R, n = 3, 2, 130
    X, Y0, factors, grp, local, slab = problem(idhmc, shape, n)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [rng.poisson(np.maximum(Y0, 0.5)).astype(float) for _ in range(M - 1)])[:, :, None]
    kind, nu, mu, tau = shape_priors(shape)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, chains_per_response=R), M * R, opt, seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form and list(eng.glm_block()[0]) == [0, 1, 2]
    q = start(shape, M * R)
    eng.set_q(q)
    eps = 0.02
    eng.set_eps(eps)
    eng.nuts_transition(1)
    q1 = eng.q
    eng.nuts_transitions(2, 2)
    q3, lq3, g3 = eng.q, eng.lq, eng.grad
    assert eng.poll_abort() == 0
    eng.close()
    for m in range(M):
        om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y[m], factors, grp, local, slab, kind, nu, mu, tau)
        for c in range(R * m, R * m + R):
            ch = oracle.OracleChain(om, oopt, seed=13, chain_id=c)
            ch.set_q(q[c])
            ch.sample_tree(eps, 1)
            assert same_bits(q1[c], ch.q[:D]), c
            ch.sample_tree(eps, 2)
            ch.sample_tree(eps, 3)
            assert same_bits(q3[c], ch.q[:D]) and same_bits(lq3[c], ch.lq) and same_bits(g3[c], ch.grad[:D]), c


# ---- the summaries --------------------------------------------------------------------------------------------------------------------
def factors_twin(zeta, dexp):
    """(z, c) per zeta by the device's expressions, dexp the oracle's"""
    z, c = [], []
    for x in zeta:
        s = np.float64(dexp(-abs(x)))
        t = s * s
        d = 1.0 + t
        z.append(np.copysign((1.0 - t) / d, x))
        c.append((2.0 * s) / d)
    return z, c


def l_twin(z, c, j, i):
    """L_ji = coef(j, -1, i) in section 26's association"""
    o, s = nz_of(j), None
    for t in range(i):
        s = c[o + t] if s is None else s * c[o + t]
    if i == j:
        return np.float64(1.0) if s is None else s
    return z[o + i] if s is None else z[o + i] * s


def theta_block_twin(draws, shape, grp, dexp):
    """[..., D] sampled coordinates -> [beta | a raw | sigma | R lower, row-major | phi] by section 26's expressions, a structured term
    by section 23's scan (shapes without local scales)"""
    Dx, A, H, J, nz, Sz = dims(shape)
    assert J == 0
    K = len(spec(shape)[4])
    N = spec(shape)[2][spec(shape)[4][0]][0]
    offs = row_offsets(shape)
    draws = np.asarray(draws, dtype=np.float64)
    out = draws.copy()
    flat, oflat = draws.reshape(-1, draws.shape[-1]), out.reshape(-1, draws.shape[-1])
    D = flat.shape[1]
    for r in range(flat.shape[0]):
        q = flat[r]
        e = [dexp(q[Dx + A + g]) for g in range(H)]
        z, c = factors_twin(q[D - Sz - nz:D - Sz], dexp)
        ut = q[:Dx].copy()
        for o, Ns, kd in structs_of(shape):
            (phi,), (cs,) = factors_twin(q[D - 1:], dexp)
            oflat[r, D - 1] = phi
            ut[o:o + Ns] = STRUCT.scan_twin(q[o:o + Ns], phi, cs)
        for j in range(1, K):
            for k in range(N):
                x = l_twin(z, c, j, j) * q[offs[j] + k]
                for i in range(j):
                    x = fma_twin(l_twin(z, c, j, i), q[offs[i] + k], x)
                ut[offs[j] + k] = x
            for i in range(j):
                if i == 0:
                    x = l_twin(z, c, j, 0)
                else:
                    x = l_twin(z, c, j, i) * l_twin(z, c, i, i)
                    for k in range(i):
                        x = fma_twin(l_twin(z, c, j, k), l_twin(z, c, i, k), x)
                oflat[r, D - Sz - nz + nz_of(j) + i] = x
        for j in range(Dx):
            oflat[r, j] = ut[j] * e[grp[j]] if grp[j] >= 0 else ut[j]
        for g in range(H):
            oflat[r, Dx + A + g] = e[g]
    return out


@pytest.mark.parametrize("shape", ["one tile", "across 128", "ar1"])
def test_summaries_of_the_reported_vector(idhmc, oracle, shape):
    """summary_add_draws of host draws, and one mcmc_summary, against the host twins of [beta | a | sigma | R | phi]: K = 3, K = 4 with the
    rows not in term order, and K = 3 next to an AR(1) term (the other theta kernel)"""
    family, Dd, terms, groups, order, eta, loc, ar, D, L, form = SHAPES[shape]
    Dx, A, H, J, nz, Sz = dims(shape)
    n_chains, N, G, bins = 16, 6, 8, 16
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau), n_chains, idhmc.default_options(max_depth=4), seed=21)
    dexp = oracle.lib().orc_exp_export
    draws = np.stack([start(shape, n_chains, seed=k) for k in range(N)])
    z0 = D - Sz - nz
    draws[0, 0, z0:z0 + nz], draws[1, 1, z0 + nz - 1], draws[2, 2, z0:z0 + nz] = 800.0, -40.0, 0.0
    theta = theta_block_twin(draws, shape, grp, dexp)
    assert theta.shape == draws.shape and theta[0, 0, z0] == 1.0 and np.all(theta[2, 2, z0:z0 + nz] == 0.0) and np.isfinite(theta).all()
    eng.summary_begin(chains_per_group=G, bins=bins)
    assert eng.summary_dims() == (n_chains // G, G, D, bins)
    eng.summary_add_draws(draws[:2])
    eng.summary_set_range(span=3.0)
    eng.summary_add_draws(draws[2:])
    got = eng.summary()
    assert_summary(got, summary_twin(theta, G), "host draws")
    s = summary_twin(theta[:2], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 3.0, bins)
    assert_histogram(got, theta[2:], G, lo, hi, "host draws")
    eng.summary_end()
    # sampled: the same transitions stored, then reduced on the device
    q0 = start(shape, n_chains)
    eng.set_eps(0.02)
    eng.set_q(q0)
    stored, _ = eng.mcmc(N, 3, store_draws=True, store_stats=False)
    eng.set_q(q0)
    got = eng.mcmc_summary(N, 3, pilot=2, chains_per_group=G, bins=bins)
    th = theta_block_twin(stored, shape, grp, dexp)
    assert np.all(got.n == N * G) and np.all(got.binned == (N - 2) * G)
    assert_summary(got, summary_twin(th, G), "mcmc_summary")
    s = summary_twin(th[:2], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 6.0, bins)
    assert_histogram(got, th[2:], G, lo, hi, "mcmc_summary")
    m = eng.model
    assert np.allclose(th[..., :Dx], idhmc.glm.coefficients(m, stored), rtol=1e-12, atol=1e-300)
    assert np.allclose(th[..., z0:z0 + nz], idhmc.glm.correlations(m, stored), rtol=1e-12, atol=1e-15)
    assert np.allclose(th[..., D - Sz:], idhmc.glm.autocorrelations(m, stored), rtol=1e-12, atol=1e-15)
    assert eng.poll_abort() == 0
    eng.close()


# ---- exact stationarity: a likelihood that is constant, so the posterior is the prior ---------------------------------------------------
@pytest.mark.parametrize("N,form,eps", [(15, 1, 0.25), (120, 0, 0.12)], ids=["L128-matrix-cores", "L512-per-wave"])
def test_nuts_leaves_the_prior_exact(idhmc, N, form, eps):
    """K = 4, eta = 1: 4096 chains start at exact draws from the prior -- u ~ N, half-t(4) group scales, zeta_ji = atanh(2 Beta(b_i, b_i)
    - 1) with b = (2, 1.5, 1) by column, which is LKJ(1) -- and make 8 transitions at a fixed stepsize: u = F(q) per coordinate stays
    uniform (tests/stationarity.py, its FWER); all six correlations R_ji are judged against their LKJ marginal, (R + 1) / 2 ~
    Beta(eta - 1 + K / 2 = 2, 2); zeta_10 and zeta_21 judged against Beta(eta, eta) -- the exponents without (K - 2 - i) / 2 -- are
    rejected"""
    n_chains, K, H, eta = 4096, 4, 4, 1.0
    nz = nz_of(K)
    Dx = 1 + K * N
    D = Dx + H + nz
    rng = np.random.default_rng(17)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[Dx:Dx + H], nu[Dx:Dx + H] = LOG_HALF_STUDENT_T, 4.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx:], mu[-nz:] = 1.0, 0.0
    grp = np.r_[-1, np.repeat(np.arange(K), N)].astype(np.int32)
    idx = np.zeros(1, np.int64)
    g = idhmc.glm
    fac = [(idx, N)] + [g.term(idx, values=np.array([0.7 - 0.4 * t]), levels=N) for t in range(1, K)]
    m = idhmc.GLM(np.ones((1, 1)), np.array([2.0]), NULL_SOURCE, None, mu, tau, groups=grp, prior_kind=kind, prior_nu=nu, factors=fac,
                  correlated=[g.block((0, 1, 2, 3), eta)])
    eng = idhmc.Engine(m, n_chains, idhmc.default_options(max_depth=8), seed=5)
    assert eng.glm_form() == form and eng.D == D
    be = betas(K, eta)
    assert list(be) == [2.0, 2.0, 1.5, 2.0, 1.5, 1.0]
    q0 = np.empty((n_chains, D))
    q0[:, :Dx] = mu[:Dx] + rng.standard_normal((n_chains, Dx)) / np.sqrt(tau[:Dx])
    for c in range(Dx, Dx + H):
        q0[:, c] = mu[c] + np.log(np.abs(rng.standard_t(nu[c], n_chains)))
    for e in range(nz):
        q0[:, D - nz + e] = np.arctanh(2.0 * rng.beta(be[e], be[e], n_chains) - 1.0)

    def prior_u(q):
        u = np.empty_like(q)
        u[:, :Dx] = special.ndtr((q[:, :Dx] - mu[:Dx]) * np.sqrt(tau[:Dx]))
        for c in range(Dx, Dx + H):
            u[:, c] = 2.0 * stats.t.cdf(np.exp(q[:, c] - mu[c]), nu[c]) - 1.0
        for e in range(nz):
            u[:, D - nz + e] = stats.beta(be[e], be[e]).cdf((np.tanh(q[:, D - nz + e]) + 1.0) / 2.0)
        return u
    eng.set_q(q0)
    assert np.isfinite(eng.lq).all()
    eng.set_eps(eps)
    eng.nuts_transitions(1, 8)
    q1, ts = eng.q, eng.tree_stats()
    assert eng.poll_abort() == 0
    eng.close()
    fam = S.Family()
    S.add_uniform(fam, prior_u(q1), "after 8 transitions")
    R = g.correlations(m, q1)
    S.add_uniform(fam, stats.beta(2.0, 2.0).cdf((R + 1.0) / 2.0), "the correlations against their LKJ marginal")
    moved = S.moved_fraction(q0, q1)
    print("N = %d: %s; moved %.3f; terminations %s" % (N, fam.report(), moved, S.terminations(ts)))
    S.assert_stationary(fam, "correlation block")
    assert moved > 0.9, moved
    ctl = S.Family()
    z = np.tanh(q1[:, [D - nz, D - nz + 2]])
    S.add_uniform(ctl, stats.beta(eta, eta).cdf((z + 1.0) / 2.0), "zeta_10 and zeta_21 against Beta(eta, eta)")
    S.assert_rejects(ctl, "correlation block")
