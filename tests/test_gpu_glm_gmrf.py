"""GMRF terms (GLM(..., gmrf=[glm.gmrf(term, Q, sum_to_zero)]), idhmc_create_glm_gmrf) on the device.  Models with a
sparse precision on a term's levels are bit-identical to the CPU oracle running the C restatement of PRIOR row 6
(tests/test_glm_gmrf_cpu.py, through oracle.OracleModel.custom, fed the expanded matrix of glm.expand_factors) and within 1e-12 of numpy,
in both device forms: one chain per wavefront (evaluation, leapfrog, the stepsize search; NUTS at L = 512) and the matrix-core gradient
of the NUTS kernel, with a per-chain and a shared metric, on 37 chains.  No tolerance on the device side.  Then: the anchor to the
kernels of the model without the feature at Q = I, kappa = 0, the create function with no GMRF term against idhmc_create_glm_struct,
several responses, a warm-up, the device summaries of the unchanged reported vector, and exact stationarity on N(0, (Q + kappa 11')^-1).
Every context compiles its source with hipRTC, so engines are shared across assertions."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import stationarity as S
from test_glm_gmrf_cpu import c_source_gmrf, grid_edges, numpy_density_gmrf, oracle_params_gmrf
from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_priors_cpu import LOG_HALF_STUDENT_T, NORMAL, STUDENT_T
from test_glm_struct_cpu import AR1, start_struct
from test_gpu_glm_factors import SHORT, same_bits
from test_gpu_glm_slopes import run_engines
from test_gpu_glm_struct import NULL_SOURCE
from test_gpu_summary import assert_histogram, assert_summary
from test_summary_cpu import range_twin, summary_twin, theta_twin

pytestmark = pytest.mark.gpu

# name: (family, Dd, (levels, valued, index it is drawn on) per term, the group of each term (None: no groups), (first, second, eta) per
# pair, (term, kind, eta) per structure, (term, precision, kappa) per GMRF term, D, padded length, matrix cores, n)
SHAPES = {
    "icar": ("POISSON_LOG", 1, ((30, False, 0),), None, (), (), ((0, "icar 6x5", 0.0),), 1 + 30, 128, 1, 200),
    "rw2 odd offset": ("POISSON_LOG", 3, ((150, False, 0),), (0,), (), (), ((0, "rw2", 0.0),), 3 + 150 + 1, 256, 1, 37),
    "two terms": ("POISSON_LOG", 100, ((12, False, 0), (30, False, 1)), (0, 1), (), (), ((0, "seasonal 4", 0.0), (1, "icar 6x5", 2.0)),
                  100 + 42 + 2, 256, 1, 37),
    "complete 128": ("GAUSSIAN_IDENTITY_LOGSIGMA", 2, ((128, False, 0),), (0,), (), (), ((0, "complete", 0.5),), 2 + 128 + 1 + 1, 256, 1, 37),
    "rw2 per wave": ("POISSON_LOG", 100, ((300, False, 0),), (0,), (), (), ((0, "rw2", 0.0),), 100 + 300 + 1, 512, 0, 37),
    "composed": ("POISSON_LOG", 100, ((200, True, 0), (100, False, 1), (20, False, 2), (20, True, 2)), (0, 1, 2, 3), ((2, 3, 2.0),),
                 ((1, AR1, 2.0),), ((0, "scaled rw1", 0.25),), 100 + 340 + 4 + 1 + 1, 512, 0, 37),
}
C_ = 37


def precision(idhmc, name, N):
    g = idhmc.glm
    if name == "icar 6x5":
        assert N == 30
        return g.icar_precision(grid_edges(6, 5), 30)
    if name == "rw2":
        return g.rw2_precision(N)
    if name == "seasonal 4":
        return g.seasonal_precision(N, 4)
    if name == "complete":
        return (N + 1.0) * np.eye(N) - np.ones((N, N))            # the complete graph's D - W plus I: every row has N entries
    if name == "scaled rw1":
        return g.scale_precision(g.rw1_precision(N))
    assert name == "identity"
    return np.eye(N)


def dims(shape):
    """Dx, A, H, P, Sz"""
    family, Dd, terms, groups, pairs, structs = SHAPES[shape][:6]
    return (Dd + sum(t[0] for t in terms), SHAPE[family][2], 0 if groups is None else max(groups) + 1, len(pairs), sum(1 for s in structs if s[1] == AR1))


def offsets(shape):
    family, Dd, terms = SHAPES[shape][:3]
    return [Dd + sum(t[0] for t in terms[:f]) for f in range(len(terms))]


def pair_columns(shape):
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[a], off[b], terms[a][0]) for a, b, eta in SHAPES[shape][4]]


def struct_columns(shape):
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[t], terms[t][0], kd) for t, kd, eta in SHAPES[shape][5]]


def gmrf_columns(idhmc, shape, gmrfs=None):
    """(off, N, Q, kappa) per GMRF term: what the restatement's tables are built from"""
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[t], terms[t][0], precision(idhmc, qn, terms[t][0]), k) for t, qn, k in (SHAPES[shape][6] if gmrfs is None else gmrfs)]


def etas(shape):
    return [p[2] for p in SHAPES[shape][4]], [s[2] for s in SHAPES[shape][5]]


def problem(idhmc, shape, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,)): data from the family's own model; values are 1 + 0.5 N(0, 1), terms with the same index id
    share one index array"""
    family, Dd, terms, groups = SHAPES[shape][:4]
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
    return X, Y, factors, grp


def shape_priors(shape):
    """normal and Student-t coefficients, log half-t on the scales, the defaults on the zetas (eta > 0) and on every member of a GMRF term"""
    Dx, A, H, P, Sz = dims(shape)
    D, terms, off = SHAPES[shape][7], SHAPES[shape][2], offsets(shape)
    Z = P + Sz
    rng = np.random.default_rng(D)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:Dx:2] = STUDENT_T
    kind[Dx + A:D - Z] = LOG_HALF_STUDENT_T
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx + A:D - Z] = 1.0
    kind[D - Z:], mu[D - Z:], tau[D - Z:] = NORMAL, 0.0, 1.0
    for t, qn, k in SHAPES[shape][6]:
        sl = slice(off[t], off[t] + terms[t][0])
        kind[sl], mu[sl], tau[sl] = NORMAL, 0.0, 1.0
    nu[kind == STUDENT_T], nu[kind == LOG_HALF_STUDENT_T] = 4.0, 3.0
    return kind, nu, mu, tau


def model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau, gmrfs="shape", **kw):
    g = idhmc.glm
    family, terms = SHAPES[shape][0], SHAPES[shape][2]
    corr = [g.pair(a, b, e) for a, b, e in SHAPES[shape][4]] or None
    st = [g.Structure(t, kd, e) for t, kd, e in SHAPES[shape][5]] or None
    spec = SHAPES[shape][6] if gmrfs == "shape" else gmrfs
    gm = None if spec is None else [g.gmrf(t, precision(idhmc, qn, terms[t][0]), k) for t, qn, k in spec]
    return idhmc.GLM(X, Y, source(idhmc, family), consts(family), mu, tau, aux=SHAPE[family][2], groups=None if SHAPES[shape][3] is None else grp,
                     prior_kind=kind, prior_nu=nu, factors=factors, correlated=corr, structured=st, gmrf=gm, **kw)


def oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, kind, nu, mu, tau):
    family, D = SHAPES[shape][0], SHAPES[shape][7]
    Xe = idhmc.glm.expand_factors(X, factors)
    eta, se = etas(shape)
    return oracle.OracleModel.custom(D, c_source_gmrf(family), oracle_params_gmrf(Xe, Y, SHAPE[family][2], grp, None, None, kind, nu, pair_columns(shape),
                                                                                 eta, struct_columns(shape), se, gmrf_columns(idhmc, shape),
                                                                                 consts(family), mu, tau), str(tmp_path))


def start(shape, chains, seed=0):
    Dx, A, H, P, Sz = dims(shape)
    return start_struct(SHAPES[shape][0], chains, Dx, H, 0, P, Sz, seed)


def check_numpy(idhmc, eng, shape, X, Y, factors, grp, kind, nu, mu, tau, ends):
    family = SHAPES[shape][0]
    Xe = idhmc.glm.expand_factors(X, factors)
    q, g, lq = eng.q, eng.grad, eng.lq
    eta, se = etas(shape)
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_gmrf(family, Xe, Y, q[c], grp, np.zeros(Xe.shape[1], int), None, kind, nu, pair_columns(shape),
                                                          eta, struct_columns(shape), se, gmrf_columns(idhmc, shape), mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


def test_the_shapes_are_what_they_are_there_for(idhmc):
    lane = lambda c: ((c & 127) >> 1, c >> 7, c & 1)           # lane, chunk, component of a coordinate
    for name, (family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n) in SHAPES.items():
        Dx, A, H, P, Sz = dims(name)
        assert Dx + A + H + P + Sz == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))) and n in (37, 200), name
    assert {s[9] for s in SHAPES.values()} == {0, 1}                           # both forms occur
    # "icar": no group, pair or structure: kGmrf alone takes the matrix-core form's G row into registers; the intercept is dense
    assert dims("icar") == (31, 0, 0, 0, 0) and gmrf_columns(idhmc, "icar")[0][:2] == (1, 30)
    # "rw2 odd offset": o = 3 is a .y; rows reach two levels to either side, so levels 123..126 (columns 126..129) read across the chunk
    # boundary at 128 and every row reads both lane components
    (o, N, Q, k), = gmrf_columns(idhmc, "rw2 odd offset")
    assert (o, N) == (3, 150) and lane(3) == (1, 0, 1) and lane(127)[1] == 0 and lane(128) == (0, 1, 0) and np.count_nonzero(Q[124]) == 5
    assert set(np.flatnonzero(Q[124]) + o) == {125, 126, 127, 128, 129}
    # "two terms": two slots with a group each, kappa > 0 on the second only; the first slot's columns straddle nothing, the tables of the
    # second start behind the first's
    g2 = gmrf_columns(idhmc, "two terms")
    assert [(o, N, k) for o, N, Q, k in g2] == [(100, 12, 0.0), (112, 30, 2.0)] and lane(127)[1] == 0 and lane(141)[1] == 1
    # "complete 128": every row holds the full 128 entries; A = 1
    (o, N, Q, k), = gmrf_columns(idhmc, "complete 128")
    assert (o, N) == (2, 128) and (np.count_nonzero(Q, axis=1) == 128).all() and np.linalg.eigvalsh(Q).min() > 0.5
    # "rw2 per wave": 300 levels over columns 100..399, chunks 0..3, in the per-wave form with no other feature but the group
    assert gmrf_columns(idhmc, "rw2 per wave")[0][:2] == (100, 300) and {lane(c)[1] for c in range(100, 400)} == {0, 1, 2, 3}
    # "composed": the GMRF term carries values; an AR(1) term and a pair on other terms: kCorr && kStruct && kGmrf, per wave at L = 512
    assert dims("composed") == (440, 0, 4, 1, 1) and struct_columns("composed") == [(300, 100, AR1)] and pair_columns("composed") == [(400, 420, 20)]
    X, Y, factors, grp = problem(idhmc, "composed", 37)
    assert factors[0].values is not None and {lane(c)[1] for c in range(100, 300)} == {0, 1, 2}
    kind, nu, mu, tau = shape_priors("composed")
    assert set(kind[:100]) == {NORMAL, STUDENT_T} and set(kind[440:444]) == {LOG_HALF_STUDENT_T} and set(kind[100:300]) == {NORMAL}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_density_leapfrog_search_and_nuts(idhmc, oracle, tmp_path, shape):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the shape runs, then the stepsize search: bit-identical to oracle chains on the C
    twin, within 1e-12 of numpy"""
    family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n = SHAPES[shape]
    X, Y, factors, grp = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau)
    assert (m.D, m.G, m.Dx) == (D, len(gmrfs), dims(shape)[0])
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D
    term, kappa, nnz = eng.glm_gmrfs()
    assert term.dtype == np.int32 and kappa.dtype == np.float64 and nnz.dtype == np.int64
    assert [(int(a), float(b)) for a, b in zip(term, kappa)] == [(t, k) for t, qn, k in gmrfs]
    assert list(nnz) == [np.count_nonzero(Q) for o, N, Q, k in gmrf_columns(idhmc, shape)]
    assert np.array_equal(eng.glm_priors()[0], kind) and np.array_equal(eng.glm_priors()[1], nu)       # the public kinds: no 6 comes back
    args = (idhmc, eng, shape, X, Y, factors, grp, kind, nu, mu, tau, (0, C_ - 1))
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


@pytest.mark.parametrize("shape", ["icar", "composed"])
def test_shared_metric(idhmc, oracle, tmp_path, shape):
    """the same stages on a shared unit metric (METRIC_SHARED: the other instantiation of the NUTS kernel), in both forms"""
    family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n = SHAPES[shape]
    X, Y, factors, grp = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau)
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4, metric_mode=idhmc.METRIC_SHARED), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.padded_dim() == L
    run_engines([eng], chains, D, start(shape, C_), shape)
    eng.close()


def engine_through(idhmc, entry, m, opt, seed, gmrfs=()):
    """an Engine around the context `entry` (idhmc_create_glm_struct, or idhmc_create_glm_gmrf with gmrfs = (None,) or (a GlmGmrfs,))
    makes of model m: what Engine.__init__ sets"""
    from inplacedhmc_jl_amd import _lib
    lib = idhmc.load_library()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    desc = m.glm_desc()
    pr = _lib.GlmPriors(kind=m.prior_kind.ctypes.data_as(ip), nu=m.prior_nu.ctypes.data_as(dp))
    fc = _lib.GlmFactors(F=m.F, levels=m.levels.ctypes.data_as(ip), index=m.factor_index.ctypes.data_as(ip))
    fv = None if m.factor_has is None else C.byref(_lib.GlmFactorValues(values=m.factor_values.ctypes.data_as(dp), has=m.factor_has.ctypes.data_as(ip)))
    pp = None if not m.P else C.byref(_lib.GlmPairs(P=m.P, first=m.pair_first.ctypes.data_as(ip), second=m.pair_second.ctypes.data_as(ip),
                                                    eta=m.pair_eta.ctypes.data_as(dp)))
    st = None if not m.S else C.byref(_lib.GlmStructs(S=m.S, term=m.struct_term.ctypes.data_as(ip), kind=m.struct_kind.ctypes.data_as(ip),
                                                      eta=m.struct_eta.ctypes.data_as(dp)))
    h = C.c_void_p()
    extra = tuple(None if g is None else C.byref(g) for g in gmrfs)
    _lib.check(getattr(lib, entry)(C.byref(h), 0, C_, 0, C.byref(desc), C.byref(pr), None, C.byref(fc), fv, pp, st, *extra, 1, 0, C.byref(opt), seed))
    eng = idhmc.Engine._adopt(m, h, C_, opt)     # an Engine around that context
    return eng


@pytest.mark.parametrize("shape", ["icar", "rw2 per wave"], ids=["L128-matrix-cores", "L512-per-wave"])
def test_identity_precision_is_the_model_without_the_feature(idhmc, shape):
    """The anchor to the parent's kernels: Q = I and kappa = 0 on the shape's GMRF term through idhmc_create_glm_gmrf against the same
    model without `gmrf` through idhmc_create_glm_struct -- the normal row with mu = 0, tau = 1 on those columns: the same bits after
    evaluation, a leapfrog and four NUTS transitions, from starts without a zero"""
    family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n = SHAPES[shape]
    X, Y, factors, grp = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    opt = idhmc.default_options(max_depth=4)
    mG = model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau, gmrfs=[(gmrfs[0][0], "identity", 0.0)])
    mP = model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau, gmrfs=None)
    assert mG.G == 1 and mP.G == 0 and mG.D == mP.D == D
    engG = idhmc.Engine(mG, C_, opt, seed=3)
    engP = engine_through(idhmc, "idhmc_create_glm_struct", mP, opt, 3)
    assert engG.glm_form() == engP.glm_form() == form and engP.glm_gmrfs() == (None, None, None) and list(engG.glm_gmrfs()[2]) == [terms[gmrfs[0][0]][0]]
    q = start(shape, C_)
    assert (q != 0.0).all()
    run_engines([engG, engP], None, D, q, shape)
    assert engG.poll_abort() == 0
    engG.close()
    engP.close()


@pytest.mark.parametrize("null", [True, False], ids=["gmrfs-NULL", "G-0"])
def test_no_gmrf_through_the_new_entry_point(idhmc, null):
    """idhmc_create_glm_gmrf with gmrfs = NULL, or with G = 0 and its arrays NULL, against the same model through
    idhmc_create_glm_struct: the same form, footprint and bits"""
    from inplacedhmc_jl_amd import _lib
    shape = "two terms"
    family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n = SHAPES[shape]
    X, Y, factors, grp = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    m = model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau, gmrfs=None)
    assert m.G == 0 and m.H == 2
    opt = idhmc.default_options(max_depth=4)
    engs = [engine_through(idhmc, "idhmc_create_glm_struct", m, opt, 3), engine_through(idhmc, "idhmc_create_glm_gmrf", m, opt, 3, (None if null else _lib.GlmGmrfs(G=0),))]
    for e in engs:
        assert e.glm_form() == form and e.glm_gmrfs() == (None, None, None) and list(e.glm_factors()[0]) == [12, 30]
    assert engs[0].device_bytes() == engs[1].device_bytes()
    run_engines(engs, None, D, start(shape, C_), shape)
    for e in engs:
        e.close()


def test_the_tables_are_counted_in_the_footprint(idhmc):
    """device_bytes grows by the level table (L int32), start, col, val and nothing else against the model with Q = I"""
    shape = "icar"
    family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n = SHAPES[shape]
    X, Y, factors, grp = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    opt = idhmc.default_options(max_depth=4)
    sizes = []
    for qn in ("identity", "icar 6x5"):
        eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau, gmrfs=[(0, qn, 0.0)]), 4, opt, seed=3)
        sizes.append((eng.device_bytes(), int(eng.glm_gmrfs()[2][0])))
        eng.close()
    (b0, z0), (b1, z1) = sizes
    assert (z0, z1) == (30, 30 + 2 * len(grid_edges(6, 5))) and b1 - b0 == (4 + 8) * (z1 - z0)      # an int32 column and a double per entry


def test_responses_are_single_response_oracle_chains(idhmc, oracle, tmp_path):
    """M = 3 responses of R = 5 chains on "two terms": at a fixed eps every chain is bit-identical to the single-response oracle chain
    on its Y (the same global chain id)"""
    shape = "two terms"
    family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n = SHAPES[shape]
    M, R = 3, 5
    X, Y0, factors, grp = problem(idhmc, shape, 37)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [rng.poisson(np.maximum(Y0, 0.5)).astype(float) for _ in range(M - 1)])[:, :, None]
    kind, nu, mu, tau = shape_priors(shape)
    full = model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau, chains_per_response=R)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(full, M * R, opt, seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form and list(eng.glm_gmrfs()[1]) == [0.0, 2.0]
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
    for m in (0, 2):
        om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y[m], factors, grp, kind, nu, mu, tau)
        for c in range(R * m, R * m + R):
            ch = oracle.OracleChain(om, oopt, seed=13, chain_id=c)
            ch.set_q(q[c])
            ch.sample_tree(eps, 1)
            assert same_bits(q1[c], ch.q[:D]), c
            ch.sample_tree(eps, 2)
            ch.sample_tree(eps, 3)
            assert same_bits(q3[c], ch.q[:D]) and same_bits(lq3[c], ch.lq) and same_bits(g3[c], ch.grad[:D]), c


def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path):
    """a 40-transition warm-up with per-chain adaptation on "icar", then 8 draws: stepsizes, draws and records are the twin's"""
    shape = "icar"
    family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n = SHAPES[shape]
    chains, N = 8, 8
    X, Y, factors, grp = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau), chains, idhmc.default_options(**SHORT), seed=77)
    draws, stats_ = eng.mcmc_with_warmup(N)
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, kind, nu, mu, tau)
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, chains, oracle.default_options(**SHORT), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps) and len(np.unique(oeps)) > 1
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats_.T, ost[:, :N])
    assert eng.poll_abort() == 0 and eng.glm_form() == form
    eng.close()


def test_summaries_of_the_reported_vector_are_unchanged(idhmc, oracle):
    """"rw2 odd offset": no coordinate is added, so the device summaries are those of a model with groups, [beta | sigma]
    (test_summary_cpu.theta_twin): summary_add_draws of host draws and one mcmc_summary against the host twin, and glm.coefficients"""
    shape = "rw2 odd offset"
    family, Dd, terms, groups, pairs, structs, gmrfs, D, L, form, n = SHAPES[shape]
    Dx, A, H, P, Sz = dims(shape)
    chains, N, G, bins = 16, 6, 8, 16
    X, Y, factors, grp = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, kind, nu, mu, tau), chains, idhmc.default_options(max_depth=4), seed=21)
    dexp = oracle.lib().orc_exp_export
    draws = np.stack([start(shape, chains, seed=k) for k in range(N)])
    theta = theta_twin(draws, Dx, A, H, grp, dexp)
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
    q0 = start(shape, chains)
    eng.set_eps(0.02)
    eng.set_q(q0)
    stored, _ = eng.mcmc(N, 3, store_draws=True, store_stats=False)
    eng.set_q(q0)
    got = eng.mcmc_summary(N, 3, pilot=2, chains_per_group=G, bins=bins)
    th = theta_twin(stored, Dx, A, H, grp, dexp)
    assert np.all(got.n == N * G) and np.all(got.binned == (N - 2) * G)
    assert_summary(got, summary_twin(th, G), "mcmc_summary")
    assert np.allclose(th[..., :Dx], idhmc.glm.coefficients(eng.model, stored), rtol=1e-12, atol=1e-300)
    assert eng.poll_abort() == 0
    eng.close()


# ---- exact stationarity: a likelihood that is constant, so the posterior is the prior -----------------------------------------------------
@pytest.mark.parametrize("rows,cols,form,kappa,eps", [(6, 5, 1, 1.0, 0.15), (20, 15, 0, 0.02, 0.12)], ids=["L128-matrix-cores", "L512-per-wave"])
def test_nuts_leaves_the_gmrf_exact(idhmc, rows, cols, form, kappa, eps):
    """4096 chains start at exact draws from the prior -- an intercept ~ N, u ~ N(0, (Q + kappa 11')^-1) for the ICAR of a rows x cols
    grid, a half-t(4) group scale -- and make 8 transitions at a fixed stepsize: z = Lc^-1 u, Lc the Cholesky factor of numpy's inverse
    of Q + kappa 11', stays iid N(0, 1) (tests/stationarity.py, its FWER), and the other coordinates stay uniform under their priors;
    u judged against N(0, 1) per coordinate is rejected.  The likelihood is constant: the prior row alone moves u"""
    chains, N = 4096, rows * cols
    Dx = 1 + N
    D = Dx + 1
    rng = np.random.default_rng(17)
    g = idhmc.glm
    Q = g.icar_precision(grid_edges(rows, cols), N)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[Dx], nu[Dx] = LOG_HALF_STUDENT_T, 4.0
    mu, tau = np.zeros(D), np.ones(D)
    mu[0], tau[0], mu[Dx] = 0.3, 1.7, -0.2
    grp = np.r_[-1, [0] * N].astype(np.int32)
    m = idhmc.GLM(np.ones((1, 1)), np.array([2.0]), NULL_SOURCE, None, mu, tau, groups=grp, prior_kind=kind, prior_nu=nu,
                  factors=[g.term(np.zeros(1, np.int64), values=np.array([0.7]), levels=N)], gmrf=[g.gmrf(0, Q, sum_to_zero=kappa)])
    eng = idhmc.Engine(m, chains, idhmc.default_options(max_depth=8), seed=5)
    assert eng.glm_form() == form and eng.D == D
    Sigma = np.linalg.inv(Q + kappa * np.ones((N, N)))
    Lc = np.linalg.cholesky(0.5 * (Sigma + Sigma.T))
    q0 = np.empty((chains, D))
    q0[:, 0] = mu[0] + rng.standard_normal(chains) / np.sqrt(tau[0])
    q0[:, 1:Dx] = rng.standard_normal((chains, N)) @ Lc.T
    q0[:, Dx] = mu[Dx] + np.log(np.abs(rng.standard_t(nu[Dx], chains)))

    def whitened(q):
        return np.linalg.solve(Lc, q[:, 1:Dx].T).T

    def rest_u(q):
        return np.c_[stats.norm.cdf((q[:, 0] - mu[0]) * np.sqrt(tau[0])), 2.0 * stats.t.cdf(np.exp(q[:, Dx] - mu[Dx]), nu[Dx]) - 1.0]
    eng.set_q(q0)
    assert np.isfinite(eng.lq).all()
    eng.set_eps(eps)
    eng.nuts_transitions(1, 8)
    q1, ts = eng.q, eng.tree_stats()
    assert eng.poll_abort() == 0
    eng.close()
    fam = S.Family()
    S.add_gaussian(fam, whitened(q1), "u after 8 transitions")
    S.add_uniform(fam, rest_u(q1), "intercept and scale after 8 transitions")
    moved = S.moved_fraction(q0, q1)
    print("N = %d: %s; moved %.3f; terminations %s" % (N, fam.report(), moved, S.terminations(ts)))
    S.assert_stationary(fam, "GMRF terms")
    assert moved > 0.9, moved
    ctl = S.Family()
    S.add_gaussian(ctl, q1[:, 1:Dx], "u against iid N(0, 1)")
    S.assert_rejects(ctl, "GMRF terms")
