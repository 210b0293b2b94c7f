"""Structured factor terms (GLM(..., structured=[glm.ar1(..) / glm.rw1(..)]), idhmc_create_glm_struct) on the device.
Models with an AR(1) or random-walk effect across a term's levels are bit-identical to the CPU oracle running the C restatement of
section 23 (tests/test_glm_struct_cpu.py, through oracle.OracleModel.custom, fed the expanded matrix of glm.expand_factors) and within
1e-12 of numpy, in both device forms: one chain per wavefront (evaluation, leapfrog, the stepsize search; NUTS at L = 512) and the
matrix-core gradient of the NUTS kernel, with a per-chain and a shared metric, on 37 chains.  No tolerance on the device side.  Then: the
anchor to the kernels of the model without the structure at zeta = +0, the create function with no structure against
idhmc_create_glm_corr, several responses with per-response adaptation, a warm-up, the device summaries of
[beta | a | sigma | exp lambda | rho | phi], and exact stationarity on a model whose posterior is its prior.  Every context compiles its
source with hipRTC, so engines are shared across assertions."""
import ctypes as C

import numpy as np
import pytest
from scipy import special, stats

import stationarity as S
from test_glm_hier_cpu import SHAPE, consts
from test_glm_priors_cpu import LOG_HALF_STUDENT_T, NORMAL, STUDENT_T
from test_glm_struct_cpu import (AR1, RW1, c_source_struct, fma_twin, make_struct, numpy_density_struct, oracle_params_struct, scan_twin,
                                 start_struct)
from test_gpu_glm_factors import SHORT, same_bits
from test_gpu_glm_pooling import against_single_responses, fixed_stage
from test_gpu_glm_slopes import run_engines
from test_gpu_summary import assert_histogram, assert_summary
from test_summary_cpu import range_twin, summary_twin

pytestmark = pytest.mark.gpu

# name: (family, Dd, (levels, valued, index it is drawn on) per term, the group of each term (None: no groups), (first, second, eta) per
# pair, (term, kind, eta) per structure, local scales with a slab on the columns of this term (or None), D, padded length, matrix cores,
# the n it runs at)
SHAPES = {
    "odd offset": ("POISSON_LOG", 3, ((5, False, 0),), (0,), (), ((0, AR1, 2.0),), None, 3 + 5 + 1 + 1, 128, 1, (1, 37)),
    "even offset": ("POISSON_LOG", 4, ((2, False, 0),), (0,), (), ((0, AR1, 0.0),), None, 4 + 2 + 1 + 1, 128, 1, (37,)),
    "across 128": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, ((60, True, 0),), (0,), (), ((0, AR1, 2.0),), None, 100 + 60 + 1 + 1 + 1, 256, 1, (130,)),
    "rw1": ("POISSON_LOG", 1, ((130, False, 0),), None, (), ((0, RW1, 0.0),), None, 1 + 130, 256, 1, (37,)),
    "two slots": ("POISSON_LOG", 8, ((9, True, 0), (6, False, 1), (6, False, 2), (6, True, 2)), (0, 1, 2, 3), ((2, 3, 2.0),),
                  ((0, AR1, 2.0), (1, RW1, 0.0)), 3, 8 + 27 + 4 + 6 + 1 + 1, 128, 1, (37,)),
    "L = 512": ("POISSON_LOG", 100, ((300, False, 0),), (0,), (), ((0, AR1, 1.0),), None, 100 + 300 + 1 + 1, 512, 0, (37,)),
}
SLAB = 2.0
C_ = 37


def dims(shape):
    """Dx, A, H, J, P, Sz"""
    family, Dd, terms, groups, pairs, structs, loc = SHAPES[shape][:7]
    Dx = Dd + sum(t[0] for t in terms)
    return (Dx, SHAPE[family][2], 0 if groups is None else max(groups) + 1, 0 if loc is None else terms[loc][0], len(pairs),
            sum(1 for s in structs if s[1] == AR1))


def offsets(shape):
    family, Dd, terms = SHAPES[shape][:3]
    return [Dd + sum(t[0] for t in terms[:f]) for f in range(len(terms))]


def pair_columns(shape):
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[a], off[b], terms[a][0]) for a, b, eta in SHAPES[shape][4]]


def struct_columns(shape):
    """(off, N, kind) per structure: what the restatement's level table is built from"""
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[t], terms[t][0], kd) for t, kd, eta in SHAPES[shape][5]]


def etas(shape):
    return [p[2] for p in SHAPES[shape][4]], [s[2] for s in SHAPES[shape][5]]


def problem(idhmc, shape, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,), local (Dx,) or None, slab): data from the family's own model; values are 1 + 0.5 N(0, 1), terms
    with the same index id share one index array"""
    family, Dd, terms, groups, pairs, structs, loc = SHAPES[shape][:7]
    rng = np.random.default_rng(n + Dd if seed is None else seed)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    z = X @ (0.5 * rng.standard_normal(Dd) / np.sqrt(Dd))
    index, factors = {}, []
    for N, valued, iid in terms:
        if iid not in index or index[iid].max() >= N:
            index[iid] = rng.integers(0, N, n)
        idx, w = index[iid], 1.0 + 0.5 * rng.standard_normal(n)
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
        local[off[loc]:off[loc] + terms[loc][0]] = 1
    return X, Y, factors, grp, local, SLAB if loc is not None else None


def shape_priors(shape, seta=None):
    """normal and Student-t on u, log half-t on the scales and the lambdas, the defaults on a zeta with eta > 0, Student-t(3) on one with
    eta = 0"""
    Dx, A, H, J, P, Sz = dims(shape)
    D = SHAPES[shape][7]
    eta, se = etas(shape)
    se = se if seta is None else seta
    ze = eta + [e for s, e in zip(SHAPES[shape][5], se) if s[1] == AR1]
    Z = P + Sz
    rng = np.random.default_rng(D)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:Dx:2] = STUDENT_T
    kind[Dx + A:D - Z] = LOG_HALF_STUDENT_T
    nu[kind == STUDENT_T], nu[kind == LOG_HALF_STUDENT_T] = 4.0, 3.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx + A:D - Z] = 1.0
    for p in range(Z):
        cz = D - Z + p
        kind[cz], nu[cz], mu[cz], tau[cz] = (NORMAL, 0.0, 0.0, 1.0) if ze[p] > 0.0 else (STUDENT_T, 3.0, mu[cz], tau[cz])
    return kind, nu, mu, tau


def model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, structured="shape", **kw):
    g = idhmc.glm
    corr = [g.pair(a, b, e) for a, b, e in SHAPES[shape][4]] or None
    st = [g.Structure(t, kd, e) for t, kd, e in SHAPES[shape][5]] if structured == "shape" else structured
    return make_struct(idhmc, SHAPES[shape][0], X, Y, factors, None if SHAPES[shape][3] is None else grp, local, slab, kind, nu, mu, tau, corr, st, **kw)


def oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, seta=None):
    family, D = SHAPES[shape][0], SHAPES[shape][7]
    Xe = idhmc.glm.expand_factors(X, factors)
    eta, se = etas(shape)
    return oracle.OracleModel.custom(D, c_source_struct(family), oracle_params_struct(Xe, Y, SHAPE[family][2], grp, local, slab, kind, nu, pair_columns(shape),
                                                                                     eta, struct_columns(shape), se if seta is None else seta,
                                                                                     consts(family), mu, tau), str(tmp_path))


def start(shape, chains, seed=0):
    Dx, A, H, J, P, Sz = dims(shape)
    return start_struct(SHAPES[shape][0], chains, Dx, H, J, P, Sz, seed)


def check_numpy(idhmc, eng, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, ends):
    family = SHAPES[shape][0]
    Xe = idhmc.glm.expand_factors(X, factors)
    q, g, lq = eng.q, eng.grad, eng.lq
    eta, se = etas(shape)
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_struct(family, Xe, Y, q[c], grp, np.zeros(Xe.shape[1], int) if local is None else local, slab, kind,
                                                            nu, pair_columns(shape), eta, struct_columns(shape), se, mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


def test_the_shapes_are_what_they_are_there_for(idhmc):
    lane = lambda c: ((c & 127) >> 1, c >> 7, c & 1)           # lane, chunk, component of a coordinate
    for name, (family, Dd, terms, groups, pairs, structs, loc, D, L, form, ns) in SHAPES.items():
        Dx, A, H, J, P, Sz = dims(name)
        assert Dx + A + H + J + P + Sz == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))), name
    stages = lambda N: int(np.ceil(np.log2(N)))
    # "odd offset": o = 3 is the .y of lane 1, o + N - 1 = 7 the .y of lane 3; N = 5 is no power of two: stages h = 1, 2, 4
    assert struct_columns("odd offset") == [(3, 5, AR1)] and lane(3) == (1, 0, 1) and lane(7) == (3, 0, 1) and stages(5) == 3
    # "even offset": o = 4 is the .x of lane 2 and level 1 its own .y; one stage; eta = 0 with a Student-t entry on zeta
    assert struct_columns("even offset") == [(4, 2, AR1)] and lane(4) == (2, 0, 0) and lane(5) == (2, 0, 1) and stages(2) == 1
    kind, nu, mu, tau = shape_priors("even offset")
    assert (kind[-1], nu[-1]) == (STUDENT_T, 3.0)
    # "across 128": levels 100..159 straddle column 128, so stages read across chunks; A = 1, a group, values; the matrix cores at L = 256
    assert struct_columns("across 128") == [(100, 60, AR1)] and lane(127)[1] == 0 and lane(128) == (0, 1, 0) and lane(159) == (15, 1, 1)
    assert {lane(c)[1] for c in range(100, 160)} == {0, 1} and stages(60) == 6
    X, Y, factors, grp, local, slab = problem(idhmc, "across 128", 130)
    assert factors[0].values is not None and set(grp[100:160]) == {0}
    # "rw1": 130 levels > 128 in columns 1..130, eight stages, no sampled coordinate and no group
    assert struct_columns("rw1") == [(1, 130, RW1)] and dims("rw1") == (131, 0, 0, 0, 0, 0) and lane(130) == (1, 1, 0) and stages(130) == 8
    # "two slots": AR1 N = 9 (four stages) with values and RW1 N = 6 (three) share the stage loop; a pair on two further terms whose
    # second carries the local scales with a slab: kCorr && kStruct && kLocal; the pair's zeta in front of the term's
    assert struct_columns("two slots") == [(8, 9, AR1), (17, 6, RW1)] and pair_columns("two slots") == [(23, 29, 6)]
    assert stages(9) == 4 and stages(6) == 3 and dims("two slots") == (35, 0, 4, 6, 1, 1)
    X, Y, factors, grp, local, slab = problem(idhmc, "two slots", 37)
    assert slab == SLAB and list(np.flatnonzero(local)) == list(range(29, 35)) and factors[0].values is not None
    # "L = 512": 300 levels over columns 100..399, chunks 0..3, nine stages; zeta is coordinate 401 in chunk 3
    assert struct_columns("L = 512") == [(100, 300, AR1)] and {lane(c)[1] for c in range(100, 400)} == {0, 1, 2, 3} and stages(300) == 9
    assert lane(401)[1] == 3


CASES = [(s, n) for s in SHAPES for n in SHAPES[s][10]]


@pytest.mark.parametrize("shape,n", CASES, ids=["%s-n%d" % c for c in CASES])
def test_density_leapfrog_search_and_nuts(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the shape runs, then the stepsize search: bit-identical to oracle chains on the C
    twin, within 1e-12 of numpy"""
    family, Dd, terms, groups, pairs, structs, loc, D, L, form, ns = SHAPES[shape]
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    Dx, A, H, J, P, Sz = dims(shape)
    assert (m.D, m.P, m.S, m.Sz, m.Dx) == (D, P, len(structs), Sz, Dx)
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D
    term, kd, eta = eng.glm_structs()
    assert term.dtype == kd.dtype == np.int32 and eta.dtype == np.float64
    assert [(int(a), int(b), float(e)) for a, b, e in zip(term, kd, eta)] == list(structs)
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


@pytest.mark.parametrize("shape", ["odd offset", "L = 512"])
def test_shared_metric(idhmc, oracle, tmp_path, shape):
    """the same stages on a shared unit metric (METRIC_SHARED: the other instantiation of the NUTS kernel), in both forms"""
    family, Dd, terms, groups, pairs, structs, loc, D, L, form, ns = SHAPES[shape]
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4, metric_mode=idhmc.METRIC_SHARED), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.padded_dim() == L
    run_engines([eng], chains, D, start(shape, C_), shape)
    eng.close()


@pytest.mark.parametrize("shape", ["odd offset", "L = 512"])
def test_zeta_zero_is_the_model_without_the_structure(idhmc, oracle, tmp_path, shape):
    """The anchor to the parent's kernels: zeta = +0, eta = 0 and a normal entry on zeta.  lq and grad[:, :D - 1] are the bits of an
    engine on the same model without `structured` at the same leading coordinates: after evaluation (the per-wave form), and after a
    NUTS transition at eps = 1e-300 -- no coordinate above 1e-100 moves, zeta stays so small that phi = +-0 and c = 1, and the state the
    transition leaves was evaluated by the form the shape runs in the NUTS kernel.  grad at zeta is the twin's."""
    family, Dd, terms, groups, pairs, structs, loc, D, L, form, ns = SHAPES[shape]
    Dx, A, H, J, P, Sz = dims(shape)
    n = 37
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape, seta=[0.0])
    kind[-1], nu[-1], mu[-1], tau[-1] = NORMAL, 0.0, 0.0, 1.5
    g = idhmc.glm
    opt = idhmc.default_options(max_depth=4)
    engS = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, structured=[g.ar1(0, 0.0)]), C_, opt, seed=3)
    engP = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind[:-1], nu[:-1], mu[:-1], tau[:-1], structured=None), C_, opt, seed=3)
    assert engS.glm_form() == engP.glm_form() == form and engS.D == engP.D + 1 == D and engP.glm_structs() == (None, None, None)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, seta=[0.0])
    q = start(shape, C_)
    q[:, -1] = 0.0
    assert np.all(np.abs(q[:, :Dx]) > 1e-100) and not np.signbit(q[:, -1]).any()
    engS.set_q(q)
    engP.set_q(q[:, :-1])

    def same_leading(stage):
        gS, gP = engS.grad, engP.grad
        assert same_bits(engS.lq, engP.lq) and same_bits(gS[:, :-1], gP), stage
        qS = engS.q
        assert same_bits(qS[:, :-1], q[:, :-1]) and same_bits(engP.q, q[:, :-1]), stage
        for c in range(C_):
            l_t, g_t = om.logdensity_and_gradient(qS[c])
            assert same_bits(g_t[:D], gS[c]) and same_bits(l_t, engS.lq[c]) and g_t[D - 1] != 0.0, (stage, c)
    same_leading("evaluation")
    for e in (engS, engP):
        e.set_eps(1e-300)
        e.nuts_transition(1)
        assert (e.tree_stats()["steps"] >= 1).all() and e.poll_abort() == 0
    assert np.all(np.abs(engS.q[:, -1]) < 1e-290)
    same_leading("a transition that moves nothing")
    engS.close()
    engP.close()


@pytest.mark.parametrize("null", [True, False], ids=["structs-NULL", "S-0"])
def test_no_structure_through_the_new_entry_point(idhmc, null):
    """idhmc_create_glm_struct with structs = NULL, or with S = 0 and its arrays NULL, against the same model through
    idhmc_create_glm_corr (what Engine calls for a model with pairs): the same form, footprint and bits"""
    from inplacedhmc_jl_amd import _lib
    shape = "two slots"
    family, Dd, terms, groups, pairs, structs, loc, D, L, form, ns = SHAPES[shape]
    n = 37
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, kind[:-1], nu[:-1], mu[:-1], tau[:-1], structured=None)
    assert m.S == 0 and m.P == 1 and m.D == D - 1
    opt = idhmc.default_options(max_depth=4)
    lib = idhmc.load_library()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    engs = [idhmc.Engine(m, C_, opt, seed=3)]
    for st in ((None,) if null else (_lib.GlmStructs(S=0),)):
        desc = m.glm_desc()
        pr = _lib.GlmPriors(kind=m.prior_kind.ctypes.data_as(ip), nu=m.prior_nu.ctypes.data_as(dp))
        lc = _lib.GlmLocal(local=m.local.ctypes.data_as(ip), slab_scale=m.slab_scale)
        fc = _lib.GlmFactors(F=m.F, levels=m.levels.ctypes.data_as(ip), index=m.factor_index.ctypes.data_as(ip))
        fv = _lib.GlmFactorValues(values=m.factor_values.ctypes.data_as(dp), has=m.factor_has.ctypes.data_as(ip))
        pp = _lib.GlmPairs(P=m.P, first=m.pair_first.ctypes.data_as(ip), second=m.pair_second.ctypes.data_as(ip), eta=m.pair_eta.ctypes.data_as(dp))
        h = C.c_void_p()
        _lib.check(lib.idhmc_create_glm_struct(C.byref(h), 0, C_, 0, C.byref(desc), C.byref(pr), C.byref(lc), C.byref(fc), C.byref(fv), C.byref(pp),
                                               None if st is None else C.byref(st), 1, 0, C.byref(opt), 3))
        eng = idhmc.Engine._adopt(m, h, C_, opt)     # an Engine around that context
        engs.append(eng)
    for e in engs:
        assert e.glm_form() == form and e.glm_structs() == (None, None, None) and list(e.glm_pairs()[0]) == [2]
    assert engs[0].device_bytes() == engs[1].device_bytes()
    run_engines(engs, None, D - 1, start(shape, C_)[:, :-1], shape)
    for e in engs:
        e.close()


class _Responses:
    """what test_gpu_glm_pooling.against_single_responses takes: M, R and the single-response model of each response"""

    def __init__(self, M, R, one):
        self.M, self.R, self.one = M, R, one


def _responses(idhmc, shape, M, R, n):
    X, Y0, factors, grp, local, slab = problem(idhmc, shape, n)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [rng.poisson(np.maximum(Y0, 0.5)).astype(float) for _ in range(M - 1)])[:, :, None]
    kind, nu, mu, tau = shape_priors(shape)
    full = model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, chains_per_response=R)
    return X, Y, factors, grp, local, slab, kind, nu, mu, tau, full


def test_responses_are_single_response_oracle_chains(idhmc, oracle, tmp_path):
    """M = 3 responses of R = 5 chains on "odd offset": at a fixed eps every chain is bit-identical to the single-response oracle chain
    on its Y (the same global chain id)"""
    shape = "odd offset"
    family, Dd, terms, groups, pairs, structs, loc, D, L, form, ns = SHAPES[shape]
    M, R = 3, 5
    X, Y, factors, grp, local, slab, kind, nu, mu, tau, full = _responses(idhmc, shape, M, R, 37)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(full, M * R, opt, seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form and list(eng.glm_structs()[2]) == [2.0]
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


def test_per_response_adaptation(idhmc):
    """chains_per_response with (EPS_PER_RESPONSE, METRIC_PER_RESPONSE): a tuning stage holds the bits of a single-response context per
    response under (EPS_GLOBAL, METRIC_POOLED), as section 16's tests ask of every model (responses 0 and 2 are compared)"""
    shape = "odd offset"
    M, R = 3, 5
    X, Y, factors, grp, local, slab, kind, nu, mu, tau, full = _responses(idhmc, shape, M, R, 37)
    pb = _Responses(M, R, lambda m: model(idhmc, shape, X, Y[m], factors, grp, local, slab, kind, nu, mu, tau))
    got = against_single_responses(idhmc, pb, full, fixed_stage(6, True), ("PER_RESPONSE", "PER_RESPONSE"), ("GLOBAL", "POOLED"), 5, which=(0, 2),
                                   max_depth=4)
    assert np.isfinite(got["draws"]).all() and len({got["eps"][R * m] for m in range(M)}) == M


def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path):
    """a 40-transition warm-up with per-chain adaptation on "odd offset", then 8 draws: stepsizes, draws and records are the twin's"""
    shape = "odd offset"
    family, Dd, terms, groups, pairs, structs, loc, D, L, form, ns = SHAPES[shape]
    chains, N = 8, 8
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau), chains, idhmc.default_options(**SHORT), seed=77)
    draws, stats_ = eng.mcmc_with_warmup(N)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, chains, oracle.default_options(**SHORT), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps) and len(np.unique(oeps)) > 1
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats_.T, ost[:, :N])
    assert eng.poll_abort() == 0 and eng.glm_form() == form
    eng.close()


# ---- the summaries --------------------------------------------------------------------------------------------------------------------
def theta_struct_twin(draws, shape, grp, dexp):
    """[..., D] sampled coordinates -> [beta | sigma | phi] by section 23's expressions with exact-rational fma, dexp the oracle's (shapes
    with one AR(1) term, no pair, no local scale, no auxiliary coordinate)"""
    Dx, A, H, J, P, Sz = dims(shape)
    assert (A, J, P, Sz) == (0, 0, 0, 1)
    (o, N, kd), = struct_columns(shape)
    draws = np.asarray(draws, dtype=np.float64)
    out = draws.copy()
    flat, oflat = draws.reshape(-1, draws.shape[-1]), out.reshape(-1, draws.shape[-1])
    D = flat.shape[1]
    for r in range(flat.shape[0]):
        q = flat[r]
        e = [dexp(q[Dx + g]) for g in range(H)]
        z = q[D - 1]
        s = np.float64(dexp(-abs(z)))
        t = s * s
        d = 1.0 + t
        phi, c = np.copysign((1.0 - t) / d, z), (2.0 * s) / d
        oflat[r, D - 1] = phi
        ut = q[:Dx].copy()
        ut[o:o + N] = scan_twin(q[o:o + N], phi, c)
        for j in range(Dx):
            oflat[r, j] = ut[j] * e[grp[j]] if grp[j] >= 0 else ut[j]
        for g in range(H):
            oflat[r, Dx + g] = e[g]
    return out


def test_summaries_of_the_reported_vector(idhmc, oracle):
    """"odd offset": summary_add_draws of host draws, and one mcmc_summary, against the host twins of [beta | sigma | phi]"""
    shape = "odd offset"
    family, Dd, terms, groups, pairs, structs, loc, D, L, form, ns = SHAPES[shape]
    Dx = dims(shape)[0]
    chains, N, G, bins = 16, 6, 8, 16
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau), chains, idhmc.default_options(max_depth=4), seed=21)
    dexp = oracle.lib().orc_exp_export
    draws = np.stack([start(shape, chains, seed=k) for k in range(N)])
    draws[0, 0, -1], draws[1, 1, -1], draws[2, 2, -1] = 800.0, -40.0, 0.0          # phi = 1 exactly, nearly -1, +0
    theta = theta_struct_twin(draws, shape, grp, dexp)
    assert theta.shape == draws.shape and theta[0, 0, -1] == 1.0 and -1.0 <= theta[1, 1, -1] < -0.999 and theta[2, 2, -1] == 0.0
    assert fma_twin(2.0, 3.0, 1.0) == 7.0
    eng.summary_begin(chains_per_group=G, bins=bins)
    assert eng.summary_dims() == (chains // G, G, D, bins)
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
    q0 = start(shape, chains)
    eng.set_eps(0.02)
    eng.set_q(q0)
    stored, _ = eng.mcmc(N, 3, store_draws=True, store_stats=False)
    eng.set_q(q0)
    got = eng.mcmc_summary(N, 3, pilot=2, chains_per_group=G, bins=bins)
    th = theta_struct_twin(stored, shape, grp, dexp)
    assert np.all(got.n == N * G) and np.all(got.binned == (N - 2) * G)
    assert_summary(got, summary_twin(th, G), "mcmc_summary")
    s = summary_twin(th[:2], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 6.0, bins)
    assert_histogram(got, th[2:], G, lo, hi, "mcmc_summary")
    m = eng.model
    assert np.allclose(th[..., :Dx], idhmc.glm.coefficients(m, stored), rtol=1e-12, atol=1e-300)
    assert np.allclose(th[..., -1:], idhmc.glm.autocorrelations(m, stored), rtol=1e-12, atol=1e-300)
    assert eng.poll_abort() == 0
    eng.close()


# ---- exact stationarity: a likelihood that is constant, so the posterior is the prior and its coordinates are independent ----------------
NULL_SOURCE = "__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)\n{\n    r = 0.0;\n    v = 0.0;\n}\n"


@pytest.mark.parametrize("N,form,eps", [(30, 1, 0.25), (300, 0, 0.12)], ids=["L128-matrix-cores", "L512-per-wave"])
def test_nuts_leaves_the_prior_exact(idhmc, N, form, eps):
    """4096 chains start at exact draws from the prior -- u ~ N, a half-t(4) group scale, zeta = atanh(2 Beta(2, 2) - 1) -- and make 8
    transitions at a fixed stepsize: u = F(q) per coordinate stays uniform (tests/stationarity.py, its FWER), with
    F_zeta = Beta(2, 2).cdf((tanh zeta + 1) / 2); zeta judged against N(0, 1) is rejected (its variance is (pi^2 - 6) / 12, about 0.32).
    The scan runs in every gradient and must leave no trace: the likelihood is constant"""
    chains, H, eta = 4096, 1, 2.0
    Dx = 1 + N
    D = Dx + H + 1
    rng = np.random.default_rng(17)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[Dx:Dx + H], nu[Dx:Dx + H] = LOG_HALF_STUDENT_T, 4.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx:], mu[-1] = 1.0, 0.0
    grp = np.r_[-1, [0] * N].astype(np.int32)
    idx = np.zeros(1, np.int64)
    g = idhmc.glm
    m = idhmc.GLM(np.ones((1, 1)), np.array([2.0]), NULL_SOURCE, None, mu, tau, groups=grp, prior_kind=kind, prior_nu=nu,
                  factors=[g.term(idx, values=np.array([0.7]), levels=N)], structured=[g.ar1(0, eta)])
    eng = idhmc.Engine(m, chains, idhmc.default_options(max_depth=8), seed=5)
    assert eng.glm_form() == form and eng.D == D
    q0 = np.empty((chains, D))
    q0[:, :Dx] = mu[:Dx] + rng.standard_normal((chains, Dx)) / np.sqrt(tau[:Dx])
    for c in range(Dx, Dx + H):
        q0[:, c] = mu[c] + np.log(np.abs(rng.standard_t(nu[c], chains)))
    q0[:, -1] = np.arctanh(2.0 * rng.beta(eta, eta, chains) - 1.0)

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
    S.assert_stationary(fam, "structured terms")
    assert moved > 0.9, moved
    ctl = S.Family()
    S.add_uniform(ctl, special.ndtr(q1[:, -1:]), "zeta against N(0, 1)")
    S.assert_rejects(ctl, "structured terms")
