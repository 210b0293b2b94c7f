"""Correlated random effects (GLM(..., correlated=[glm.pair(..)]), idhmc_create_glm_corr) on the device.  Models with a
sampled correlation per pair of factor terms are bit-identical to the CPU oracle running the C restatement of section 22
(tests/test_glm_corr_cpu.py, through oracle.OracleModel.custom, fed the expanded matrix of glm.expand_factors) and within 1e-12 of
numpy, in both device forms: one chain per wavefront (evaluation, leapfrog; NUTS at L = 512) and the matrix-core gradient of the NUTS
kernel.  No tolerance on the device side.  Then: the anchor to the kernels of the model without pairs at zeta = +0, several responses,
a warm-up, the create function with no pairs against idhmc_create_glm_slopes, the device summaries of [beta | a | sigma | exp lambda |
rho], and exact stationarity on a model whose posterior is its prior.  Every context compiles its source with hipRTC, so engines are
shared across assertions."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
from scipy import special, stats

import stationarity as S
from test_glm_corr_cpu import c_source_corr, make_corr, numpy_density_corr, oracle_params_corr, start_corr
from test_glm_hier_cpu import SHAPE, consts
from test_glm_priors_cpu import LOG_HALF_STUDENT_T, NORMAL, STUDENT_T
from test_gpu_glm_factors import SHORT, same_bits
from test_gpu_glm_slopes import run_engines
from test_gpu_summary import assert_histogram, assert_summary
from test_summary_cpu import range_twin, summary_twin

pytestmark = pytest.mark.gpu

# name: (family, Dd, (levels, valued, index it is drawn on) per term, the group of each term (None: no groups), (first, second, eta) per
# pair, local scales with a slab on the columns of this term (or None), D, padded length, matrix cores)
SHAPES = {
    "one tile": ("POISSON_LOG", 20, ((15, False, 0), (15, True, 0)), (0, 1), ((0, 1, 2.0),), None, 20 + 30 + 2 + 1, 128, 1),
    "across 128": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, ((20, False, 0), (20, True, 1)), (0, 1), ((0, 1, 2.0),), None, 100 + 40 + 1 + 2 + 1, 256, 1),
    "L = 512": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, ((150, False, 0), (150, True, 0)), (0, 1), ((0, 1, 1.0),), None, 100 + 300 + 1 + 2 + 1, 512, 0),
    "two pairs": ("POISSON_LOG", 8, ((6, False, 0), (6, True, 0), (9, True, 1), (9, False, 1)), (0, 1, 2, 3), ((0, 1, 2.0), (3, 2, 0.0)), None,
                  8 + 30 + 4 + 2, 128, 1),
    "local": ("POISSON_LOG", 10, ((12, False, 0), (12, True, 0)), (0, 1), ((0, 1, 2.0),), 1, 10 + 24 + 2 + 12 + 1, 128, 1),
    "no groups": ("POISSON_LOG", 1, ((5, False, 0), (5, False, 1)), None, ((0, 1, 2.0),), None, 1 + 10 + 1, 128, 1),
}
SLAB = 2.0


def dims(shape):
    family, Dd, terms, groups, pairs, loc, D, L, form = SHAPES[shape]
    Dx = Dd + sum(t[0] for t in terms)
    return Dx, SHAPE[family][2], 0 if groups is None else max(groups) + 1, 0 if loc is None else terms[loc][0], len(pairs)


def offsets(shape):
    family, Dd, terms = SHAPES[shape][:3]
    return [Dd + sum(t[0] for t in terms[:f]) for f in range(len(terms))]


def pair_columns(shape):
    """(off_first, off_second, N) per pair: what the restatement's partner table is built from"""
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[a], off[b], terms[a][0]) for a, b, eta in SHAPES[shape][4]]


def problem(idhmc, shape, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,), local (Dx,) or None, slab): data from the family's own model; values are 0.5 N(0, 1), terms with
    the same index id share one index array"""
    family, Dd, terms, groups, pairs, loc, D, L, form = SHAPES[shape]
    rng = np.random.default_rng(n + Dd if seed is None else seed)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    z = X @ (0.5 * rng.standard_normal(Dd) / np.sqrt(Dd))
    index, factors = {}, []
    for N, valued, iid in terms:
        if iid not in index or index[iid].max() >= N:
            index[iid] = rng.integers(0, N, n)
        idx, w = index[iid], 0.5 * rng.standard_normal(n)
        z = z + (w if valued else 1.0) * (0.4 * rng.standard_normal(N))[idx]
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
        local[off[loc]:off[loc] + terms[loc][0]] = 1
    return X, Y, factors, grp, local, SLAB if loc is not None else None


def shape_priors(shape, eta=None):
    """normal and Student-t on u, log half-t on the scales and the lambdas, the defaults on a zeta with eta > 0, Student-t(3) on one with eta = 0"""
    Dx, A, H, J, P = dims(shape)
    D = SHAPES[shape][6]
    eta = [p[2] for p in SHAPES[shape][4]] if eta is None else eta
    rng = np.random.default_rng(D)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:Dx:2] = STUDENT_T
    kind[Dx + A:D - P] = LOG_HALF_STUDENT_T
    nu[kind == STUDENT_T], nu[kind == LOG_HALF_STUDENT_T] = 4.0, 3.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx + A:D - P] = 1.0
    for p in range(P):
        cz = D - P + p
        kind[cz], nu[cz], mu[cz], tau[cz] = (NORMAL, 0.0, 0.0, 1.0) if eta[p] > 0.0 else (STUDENT_T, 3.0, mu[cz], tau[cz])
    return kind, nu, mu, tau


def model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, pairs="shape", **kw):
    g = idhmc.glm
    corr = [g.pair(a, b, e) for a, b, e in SHAPES[shape][4]] if pairs == "shape" else pairs
    return make_corr(idhmc, SHAPES[shape][0], X, Y, factors, None if SHAPES[shape][3] is None else grp, local, slab, kind, nu, mu, tau, corr, **kw)


def oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau):
    family, D = SHAPES[shape][0], SHAPES[shape][6]
    Xe = idhmc.glm.expand_factors(X, factors)
    eta = [p[2] for p in SHAPES[shape][4]]
    return oracle.OracleModel.custom(D, c_source_corr(family), oracle_params_corr(Xe, Y, SHAPE[family][2], grp, local, slab, kind, nu, pair_columns(shape),
                                                                                 eta, consts(family), mu, tau), str(tmp_path))


def start(shape, C_, seed=0):
    """start_corr with, for two pairs, one zeta positive and one negative"""
    Dx, A, H, J, P = dims(shape)
    q = start_corr(SHAPES[shape][0], C_, Dx, H, J, P, seed)
    if P == 2:
        q[:, -2], q[:, -1] = np.abs(q[:, -2]) + 0.1, -np.abs(q[:, -1]) - 0.1
    return q


def check_numpy(idhmc, eng, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, ends):
    family, D = SHAPES[shape][0], SHAPES[shape][6]
    Xe = idhmc.glm.expand_factors(X, factors)
    q, g, lq = eng.q, eng.grad, eng.lq
    eta = [p[2] for p in SHAPES[shape][4]]
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_corr(family, Xe, Y, q[c], grp, np.zeros(Xe.shape[1], int) if local is None else local, slab, kind, nu,
                                                          pair_columns(shape), eta, mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


def test_the_shapes_are_what_they_are_there_for(idhmc):
    lane = lambda c: ((c & 127) >> 1, c >> 7, c & 1)           # lane, chunk, component of a coordinate
    for name, (family, Dd, terms, groups, pairs, loc, D, L, form) in SHAPES.items():
        Dx, A, H, J, P = dims(name)
        assert Dx + A + H + J + P == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))), name
        for a, b, eta in pairs:
            assert terms[a][0] == terms[b][0] and a != b
    # "one tile": the partner of column c is c + 15 -- another lane and the other component; one index, (1 + x | s)
    assert pair_columns("one tile") == [(20, 35, 15)]
    assert all(lane(c)[0] != lane(c + 15)[0] and lane(c)[2] != lane(c + 15)[2] and lane(c)[1] == lane(c + 15)[1] == 0 for c in range(20, 35))
    X, Y, factors, grp, local, slab = problem(idhmc, "one tile", 130)
    assert factors[0][0] is factors[1].index and factors[1].values is not None and lane(52) == (26, 0, 0)
    # "across 128": columns 100..119 and 120..139, the second term on both sides of column 128, two index arrays
    assert pair_columns("across 128") == [(100, 120, 20)] and 120 < 128 < 139 and lane(127)[1] == 0 and lane(128) == (0, 1, 0)
    assert {lane(c)[1] for c in range(100, 120)} == {0} and {lane(c)[1] for c in range(120, 140)} == {0, 1}
    X, Y, factors, grp, local, slab = problem(idhmc, "across 128", 130)
    assert factors[0][0] is not factors[1].index and not np.array_equal(factors[0][0], factors[1].index)
    # "L = 512": 150 + 150 levels over chunks 0..3, partners in different chunks; zeta is coordinate 403
    assert pair_columns("L = 512") == [(100, 250, 150)] and all(lane(c)[1] != lane(c + 150)[1] for c in range(100, 250)) and lane(403)[1] == 3
    # "two pairs": the second pair's first term lies behind its second; eta = (2, 0), the second zeta with a Student-t entry
    assert pair_columns("two pairs") == [(8, 14, 6), (29, 20, 9)]
    kind, nu, mu, tau = shape_priors("two pairs")
    assert (kind[-2], mu[-2], tau[-2], nu[-2]) == (0, 0.0, 1.0, 0.0) and (kind[-1], nu[-1]) == (STUDENT_T, 3.0)
    q = start("two pairs", 18)
    assert np.all(q[:, -2] > 0) and np.all(q[:, -1] < 0)
    # "local": the slab's local scales sit on the second (the slope) term's columns, which are paired
    X, Y, factors, grp, local, slab = problem(idhmc, "local", 130)
    assert slab == SLAB and list(np.flatnonzero(local)) == list(range(22, 34)) and pair_columns("local") == [(10, 22, 12)]
    # "no groups"
    assert dims("no groups") == (11, 0, 0, 0, 1)
    # the anchor's starts: every u, and every product of a value with a coefficient, far above 1e-100
    for name in ("one tile", "L = 512"):
        X, Y, factors, grp, local, slab = problem(idhmc, name, 130)
        q = start(name, 18)
        Dx = dims(name)[0]
        assert np.all(np.abs(q[:, :Dx]) > 1e-100)
        w = np.asarray(factors[1].values)
        prod = w[None, :] * q[:, offsets(name)[1] + factors[1].index]
        assert np.all(np.abs(w[w != 0.0]) > 1e-8) and np.all(np.abs(prod[prod != 0.0]) > 1e-100)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1, 130])
def test_density_leapfrog_and_nuts(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the shape runs: bit-identical to oracle chains on the C twin, within 1e-12 of numpy"""
    family, Dd, terms, groups, pairs, loc, D, L, form = SHAPES[shape]
    C_ = 18
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    assert (m.D, m.P, m.Dx) == (D, len(pairs), dims(shape)[0])
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D
    first, second, eta = eng.glm_pairs()
    assert first.dtype == second.dtype == np.int32 and eta.dtype == np.float64
    assert [(int(a), int(b), float(e)) for a, b, e in zip(first, second, eta)] == list(pairs)
    assert np.array_equal(eng.glm_priors()[0], kind) and np.array_equal(eng.glm_priors()[1], nu)       # the public kinds: no 5 comes back
    args = (idhmc, eng, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, (0, C_ - 1))
    q = start(shape, C_)
    eng.set_q(q)
    check_numpy(*args)
    run_engines([eng], chains, D, q, shape)
    check_numpy(*args)
    eng.close()


@pytest.mark.parametrize("shape", ["one tile", "L = 512"])
def test_zeta_zero_is_the_model_without_the_pair(idhmc, oracle, tmp_path, shape):
    """The anchor to the parent's kernels: every zeta = +0, eta = 0 and a normal entry on zeta.  lq and grad[:, :D - P] are the bits of an
    engine on the same model without `correlated` at the same leading coordinates: after evaluation (the per-wave form), and after a
    NUTS transition at eps = 1e-300 -- no coordinate above 1e-100 moves, zeta stays so small that rho = +-0 and c = 1, and the state the
    transition leaves was evaluated by the form the shape runs in the NUTS kernel (the matrix cores for "one tile").  grad at zeta is
    the twin's."""
    family, Dd, terms, groups, pairs, loc, D, L, form = SHAPES[shape]
    Dx, A, H, J, P = dims(shape)
    C_, n = 18, 130
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape, eta=[0.0])
    kind[-1], nu[-1], mu[-1], tau[-1] = NORMAL, 0.0, 0.0, 1.5
    g = idhmc.glm
    opt = idhmc.default_options(max_depth=4)
    engC = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, pairs=[g.pair(0, 1, 0.0)]), C_, opt, seed=3)
    engP = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind[:-1], nu[:-1], mu[:-1], tau[:-1], pairs=None), C_, opt, seed=3)
    assert engC.glm_form() == engP.glm_form() == form and engC.D == engP.D + 1 == D and engP.glm_pairs() == (None, None, None)
    Xe = g.expand_factors(X, factors)
    om = oracle.OracleModel.custom(D, c_source_corr(family), oracle_params_corr(Xe, Y, A, grp, local, slab, kind, nu, pair_columns(shape), [0.0],
                                                                                consts(family), mu, tau), str(tmp_path))
    q = start(shape, C_)
    q[:, -1] = 0.0
    assert np.all(np.abs(q[:, :Dx]) > 1e-100) and not np.signbit(q[:, -1]).any()
    engC.set_q(q)
    engP.set_q(q[:, :-1])

    def same_leading(stage):
        gC, gP = engC.grad, engP.grad
        assert same_bits(engC.lq, engP.lq) and same_bits(gC[:, :-1], gP), stage
        qC = engC.q
        assert same_bits(qC[:, :-1], q[:, :-1]) and same_bits(engP.q, q[:, :-1]), stage
        for c in range(C_):
            l_t, g_t = om.logdensity_and_gradient(qC[c])
            assert same_bits(g_t, gC[c]) and same_bits(l_t, engC.lq[c]) and g_t[-1] != 0.0, (stage, c)
    same_leading("evaluation")
    for e in (engC, engP):
        e.set_eps(1e-300)
        e.nuts_transition(1)
        assert (e.tree_stats()["steps"] >= 1).all() and e.poll_abort() == 0
    assert np.all(np.abs(engC.q[:, -1]) < 1e-290)
    same_leading("a transition that moves nothing")
    engC.close()
    engP.close()


def test_responses_are_single_response_oracle_chains(idhmc, oracle, tmp_path):
    """M = 4 responses of R = 3 chains on "one tile": every chain is bit-identical to the single-response oracle chain on its Y (the
    same global chain id)"""
    shape = "one tile"
    family, Dd, terms, groups, pairs, loc, D, L, form = SHAPES[shape]
    M, R, n = 4, 3, 130
    X, Y0, factors, grp, local, slab = problem(idhmc, shape, n)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [rng.poisson(np.maximum(Y0, 0.5)).astype(float) for _ in range(M - 1)])[:, :, None]
    kind, nu, mu, tau = shape_priors(shape)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, chains_per_response=R), M * R, opt, seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form and list(eng.glm_pairs()[2]) == [2.0]
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


def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path):
    """a 40-transition warm-up with per-chain adaptation on "one tile", then 8 draws: stepsizes, draws and records are the twin's"""
    shape = "one tile"
    family, Dd, terms, groups, pairs, loc, D, L, form = SHAPES[shape]
    C_, N = 8, 8
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 130)
    kind, nu, mu, tau = shape_priors(shape)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau), C_, idhmc.default_options(**SHORT), seed=77)
    draws, stats_ = eng.mcmc_with_warmup(N)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, C_, oracle.default_options(**SHORT), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps) and len(np.unique(oeps)) > 1
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats_.T, ost[:, :N])
    assert eng.poll_abort() == 0 and eng.glm_form() == form
    eng.close()


def test_no_pairs_through_the_new_entry_point(idhmc):
    """idhmc_create_glm_corr with pairs = NULL, and with P = 0 and its arrays NULL, against the same model through
    idhmc_create_glm_slopes: the same form, footprint and bits"""
    from inplacedhmc_jl_amd import _lib
    shape = "one tile"
    family, Dd, terms, groups, pairs, loc, D, L, form = SHAPES[shape]
    C_, n = 18, 130
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind[:-1], nu[:-1], mu[:-1], tau[:-1], pairs=None)
    assert m.P == 0 and m.D == D - 1
    opt = idhmc.default_options(max_depth=4)
    lib = idhmc.load_library()
    ip = C.POINTER(C.c_int32)
    engs = [idhmc.Engine(m, C_, opt, seed=3)]
    for pp in (None, _lib.GlmPairs(P=0)):
        desc = m.glm_desc()
        pr = _lib.GlmPriors(kind=m.prior_kind.ctypes.data_as(ip), nu=m.prior_nu.ctypes.data_as(C.POINTER(C.c_double)))
        fc = _lib.GlmFactors(F=m.F, levels=m.levels.ctypes.data_as(ip), index=m.factor_index.ctypes.data_as(ip))
        fv = _lib.GlmFactorValues(values=m.factor_values.ctypes.data_as(C.POINTER(C.c_double)), has=m.factor_has.ctypes.data_as(ip))
        h = C.c_void_p()
        _lib.check(lib.idhmc_create_glm_corr(C.byref(h), 0, C_, 0, C.byref(desc), C.byref(pr), None, C.byref(fc), C.byref(fv),
                                             None if pp is None else C.byref(pp), 1, 0, C.byref(opt), 3))
        eng = idhmc.Engine._adopt(m, h, C_, opt)     # an Engine around that context
        engs.append(eng)
    for e in engs:
        assert e.glm_form() == form and e.glm_pairs() == (None, None, None) and list(e.glm_factor_values()[0]) == [0, 1]
    assert engs[0].device_bytes() == engs[1].device_bytes() == engs[2].device_bytes()
    Dx, A, H, J, P = dims(shape)
    run_engines(engs, None, D - 1, start(shape, C_)[:, :-1], shape)
    for e in engs:
        e.close()


# ---- the summaries --------------------------------------------------------------------------------------------------------------------
def fma_twin(a, b, c):
    """fma(a, b, c) rounded once, through exact rationals (finite arguments)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def theta_corr_twin(draws, shape, grp, dexp):
    """[..., D] sampled coordinates -> [beta | a raw | sigma | rho] by section 22's expressions, dexp the oracle's (shapes without local scales)"""
    Dx, A, H, J, P = dims(shape)
    assert J == 0
    draws = np.asarray(draws, dtype=np.float64)
    out = draws.copy()
    flat, oflat = draws.reshape(-1, draws.shape[-1]), out.reshape(-1, draws.shape[-1])
    D = flat.shape[1]
    for r in range(flat.shape[0]):
        q = flat[r]
        e = [dexp(q[Dx + A + g]) for g in range(H)]
        ut = q[:Dx].copy()
        for p, (o1, o2, N) in enumerate(pair_columns(shape)):
            z = q[D - P + p]
            s = np.float64(dexp(-abs(z)))
            t = s * s
            d = 1.0 + t
            rho, c = np.copysign((1.0 - t) / d, z), (2.0 * s) / d
            oflat[r, D - P + p] = rho
            for k in range(N):
                ut[o2 + k] = fma_twin(rho, q[o1 + k], c * q[o2 + k])
        for j in range(Dx):
            oflat[r, j] = ut[j] * e[grp[j]] if grp[j] >= 0 else ut[j]
        for g in range(H):
            oflat[r, Dx + A + g] = e[g]
    return out


def test_summaries_of_the_reported_vector(idhmc, oracle):
    """"one tile": summary_add_draws of host draws, and one mcmc_summary, against the host twins of [beta | sigma | rho]"""
    shape = "one tile"
    family, Dd, terms, groups, pairs, loc, D, L, form = SHAPES[shape]
    Dx, A, H, J, P = dims(shape)
    C_, N, G, bins = 16, 6, 8, 16
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau), C_, idhmc.default_options(max_depth=4), seed=21)
    dexp = oracle.lib().orc_exp_export
    draws = np.stack([start(shape, C_, seed=k) for k in range(N)])
    draws[0, 0, -1], draws[1, 1, -1], draws[2, 2, -1] = 800.0, -40.0, 0.0          # rho = 1 exactly, nearly -1, +0
    theta = theta_corr_twin(draws, shape, grp, dexp)
    assert theta.shape == draws.shape and theta[0, 0, -1] == 1.0 and -1.0 <= theta[1, 1, -1] < -0.999 and theta[2, 2, -1] == 0.0
    eng.summary_begin(chains_per_group=G, bins=bins)
    assert eng.summary_dims() == (C_ // G, G, D, bins)
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
    q0 = start(shape, C_)
    eng.set_eps(0.02)
    eng.set_q(q0)
    stored, _ = eng.mcmc(N, 3, store_draws=True, store_stats=False)
    eng.set_q(q0)
    got = eng.mcmc_summary(N, 3, pilot=2, chains_per_group=G, bins=bins)
    th = theta_corr_twin(stored, shape, grp, dexp)
    assert np.all(got.n == N * G) and np.all(got.binned == (N - 2) * G)
    assert_summary(got, summary_twin(th, G), "mcmc_summary")
    s = summary_twin(th[:2], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 6.0, bins)
    assert_histogram(got, th[2:], G, lo, hi, "mcmc_summary")
    m = eng.model
    assert np.allclose(th[..., :Dx], idhmc.glm.coefficients(m, stored), rtol=1e-12, atol=1e-300)
    assert np.allclose(th[..., -1:], idhmc.glm.correlations(m, stored), rtol=1e-12, atol=1e-300)
    assert eng.poll_abort() == 0
    eng.close()


# ---- exact stationarity: a likelihood that is constant, so the posterior is the prior and its coordinates are independent ----------------
NULL_SOURCE = "__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)\n{\n    r = 0.0;\n    v = 0.0;\n}\n"


@pytest.mark.parametrize("N,form,eps", [(15, 1, 0.25), (150, 0, 0.12)], ids=["L128-matrix-cores", "L512-per-wave"])
def test_nuts_leaves_the_prior_exact(idhmc, N, form, eps):
    """4096 chains start at exact draws from the prior -- u ~ N, half-t(4) group scales, zeta = atanh(2 Beta(2, 2) - 1) under LKJ(2) -- and
    make 8 transitions at a fixed stepsize: u = F(q) per coordinate stays uniform (tests/stationarity.py, its FWER), with
    F_zeta = Beta(2, 2).cdf((tanh zeta + 1) / 2); zeta judged against N(0, 1) is rejected (its variance is (pi^2 - 6) / 12, about 0.32)"""
    C_, H, eta = 4096, 2, 2.0
    Dx = 1 + 2 * N
    D = Dx + H + 1
    rng = np.random.default_rng(17)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[Dx:Dx + H], nu[Dx:Dx + H] = LOG_HALF_STUDENT_T, 4.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx:], mu[-1] = 1.0, 0.0
    grp = np.r_[-1, [0] * N, [1] * N].astype(np.int32)
    idx = np.zeros(1, np.int64)
    g = idhmc.glm
    m = idhmc.GLM(np.ones((1, 1)), np.array([2.0]), NULL_SOURCE, None, mu, tau, groups=grp, prior_kind=kind, prior_nu=nu,
                  factors=[(idx, N), g.term(idx, values=np.array([0.7]), levels=N)], correlated=[g.pair(0, 1, eta)])
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=8), seed=5)
    assert eng.glm_form() == form and eng.D == D
    q0 = np.empty((C_, D))
    q0[:, :Dx] = mu[:Dx] + rng.standard_normal((C_, Dx)) / np.sqrt(tau[:Dx])
    for c in range(Dx, Dx + H):
        q0[:, c] = mu[c] + np.log(np.abs(rng.standard_t(nu[c], C_)))
    q0[:, -1] = np.arctanh(2.0 * rng.beta(eta, eta, C_) - 1.0)

    def prior_u(q):
        u = np.empty_like(q)
        u[:, :Dx] = special.ndtr((q[:, :Dx] - mu[:Dx]) * np.sqrt(tau[:Dx]))
        for c in range(Dx, Dx + H):
            u[:, c] = 2.0 * stats.t.cdf(np.exp(q[:, c] - mu[c]), nu[c]) - 1.0
        u[:, -1] = stats.beta(eta, eta).cdf((np.tanh(q[:, -1]) + 1.0) / 2.0)
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
    moved = S.moved_fraction(q0, q1)
    print("N = %d: %s; moved %.3f; terminations %s; var zeta %.3f" % (N, fam.report(), moved, S.terminations(ts), q1[:, -1].var()))
    S.assert_stationary(fam, "correlated pairs")
    assert moved > 0.9, moved
    ctl = S.Family()
    S.add_uniform(ctl, special.ndtr(q1[:, -1:]), "zeta against N(0, 1)")
    S.assert_rejects(ctl, "correlated pairs")
