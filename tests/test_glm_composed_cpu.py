"""Correlated pairs, structured terms and GMRF terms (DESIGN sections 22, 23 and 25) on the shapes and flag combinations that
tests/test_gpu_glm_corr.py, tests/test_gpu_glm_struct.py and tests/test_gpu_glm_gmrf.py leave out: L = 1024 with each of the three, two
AR(1) terms with the larger one in the second slot, a scan of more than 512 levels, GMRF members in chunks j >= 4, an AR(1) term of
more than 128 levels and four blocks of observations on the matrix cores, local scales next to a structure without a pair and next to
a GMRF term, the three features at once on the matrix cores, two pairs across column 128 with D = L, and A = 4 at L = 256.  This file
holds the one table of shapes that tests/test_gpu_glm_composed.py runs on the device, and pins without a GPU what the device is
compared with: section 25's C restatement (tests/test_glm_gmrf_cpu.py, which takes local scales and two structure slots) agrees with
the numpy closed form on every row within 1e-12 of the magnitude of the terms summed; numpy's gradient is mpmath's derivative (40
digits) of a log density written from the definitions on one small model with every feature at once; and theta_composed_twin, the
reported vector [beta | a | sigma | exp lambda | rho | phi] of any row by the summary kernels' own expressions with exact-rational
fma, has the bits of the two twins it generalises and agrees with glm.coefficients, glm.correlations and glm.autocorrelations."""
import ctypes as C

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
from test_glm_factor_matrix_cpu import coop
from test_glm_gmrf_cpu import MAP5, c_source_gmrf, numpy_density_gmrf, oracle_params_gmrf
from test_glm_hier_cpu import SHAPE, consts
from test_glm_local_cpu import inv2_of
from test_glm_priors_cpu import LOG_HALF_STUDENT_T, NORMAL, STUDENT_T
from test_glm_struct_cpu import AR1, RW1, fma_twin, make_struct, scan_twin, start_struct
from test_gpu_glm_factors import same_bits
from test_gpu_glm_gmrf import precision

# name: (family, Dd, (levels, valued, index it is drawn on) per term, the group of each term, (first, second, eta) per pair, (term, kind,
# eta) per structure, (term, precision, kappa) per GMRF term, local scales with a slab on the columns of this term (or None), D, padded
# length, matrix cores, n)
SHAPES = {
    "everything 1024": ("POISSON_LOG", 100, ((520, True, 0), (150, False, 1), (60, False, 2), (60, True, 2)), (0, 1, 2, 3), ((2, 3, 2.0),),
                        ((0, AR1, 2.0),), ((1, "rw2", 0.5),), 3, 956, 1024, 0, 37),
    "two ar1 two gmrf 1024": ("POISSON_LOG", 100, ((130, False, 0), (600, True, 1), (30, False, 2), (12, False, 3)), (0, 1, 2, 3), (),
                              ((0, AR1, 2.0), (1, AR1, 0.0)), ((2, "icar 6x5", 2.0), (3, "seasonal 4", 0.5)), None, 878, 1024, 0, 37),
    "two ar1 coop": ("POISSON_LOG", 20, ((40, False, 0), (150, True, 1)), (0, 1), (), ((0, AR1, 2.0), (1, AR1, 0.0)), (), None, 214, 256, 1, 385),
    "composed coop": ("GAUSSIAN_IDENTITY_LOGSIGMA", 10, ((100, True, 0), (60, False, 1), (20, False, 2), (20, True, 2)), (0, 1, 2, 3), ((2, 3, 2.0),),
                      ((1, AR1, 2.0),), ((0, "scaled rw1", 0.25),), 3, 237, 256, 1, 130),
    "two pairs local D=L": ("POISSON_LOG", 20, ((70, True, 0), (70, False, 0), (30, False, 1), (30, True, 1)), (0, 1, 2, 3),
                            ((1, 0, 2.0), (2, 3, 0.0)), (), (), 3, 256, 256, 1, 385),
    "A4 per wave 256": ("TEST_A4", 20, ((150, False, 0), (30, False, 1)), (0, 1), (), ((0, AR1, 2.0),), ((1, "icar 6x5", 1.0),), None, 207, 256, 0, 130),
    "struct local no pair": ("POISSON_LOG", 150, ((200, False, 0), (40, False, 1)), (0, 1), (), ((0, RW1, 0.0),), (), 1, 432, 512, 0, 130),
    "gmrf local 128": ("POISSON_LOG", 8, ((30, False, 0), (20, True, 1)), (0, 1), (), (), ((0, "icar 6x5", 1.0),), 1, 80, 128, 1, 37),
}
SLAB = 2.0
C_ = 37


def dims(shape):
    """Dx, A, H, J, P, Sz"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc = SHAPES[shape][:8]
    return (Dd + sum(t[0] for t in terms), SHAPE[family][2], max(groups) + 1, 0 if loc is None else terms[loc][0], len(pairs),
            sum(1 for s in structs if s[1] == AR1))


def offsets(shape):
    family, Dd, terms = SHAPES[shape][:3]
    return [Dd + sum(t[0] for t in terms[:f]) for f in range(len(terms))]


def pair_columns(shape):
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[a], off[b], terms[a][0]) for a, b, eta in SHAPES[shape][4]]


def struct_columns(shape):
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[t], terms[t][0], kd) for t, kd, eta in SHAPES[shape][5]]


def gmrf_columns(idhmc, shape):
    """(off, N, Q, kappa) per GMRF term"""
    terms, off = SHAPES[shape][2], offsets(shape)
    return [(off[t], terms[t][0], precision(idhmc, qn, terms[t][0]), k) for t, qn, k in SHAPES[shape][6]]


def etas(shape):
    return [p[2] for p in SHAPES[shape][4]], [s[2] for s in SHAPES[shape][5]]


def stages(N):
    """the stages h = 1, 2, 4, .. < N of a scan over N levels"""
    return int(np.ceil(np.log2(N)))


def problem(idhmc, shape, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,), local (Dx,) or None, slab): tests/test_gpu_glm_gmrf.py's problem with the local scales of
    tests/test_gpu_glm_struct.py's, and for TEST_A4 the two columns of Y (the response and its covariate).  The first two observations
    have the last and the first level of every term: with 37 observations on 520 levels the levels past 512 would otherwise have no data,
    and what the h = 512 stage writes there would reach neither l nor the gradient"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc = SHAPES[shape][:8]
    rng = np.random.default_rng(n + Dd if seed is None else seed)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    z = X @ (0.5 * rng.standard_normal(Dd) / np.sqrt(Dd))
    index, factors = {}, []
    for N, valued, iid in terms:
        if iid not in index or index[iid].max() >= N:
            index[iid] = rng.integers(0, N, n)
            index[iid][:2] = N - 1, 0                          # both ends are observed: a scan's last stage reaches a level with data
        idx, w = index[iid], 1.0 + 0.5 * rng.standard_normal(n)
        z = z + (w if valued else 1.0) * (0.3 * rng.standard_normal(N))[idx]
        factors.append(idhmc.glm.term(idx, values=w, levels=N) if valued else (idx, N))
    if family == "POISSON_LOG":
        Y = rng.poisson(np.exp(z)).astype(float)
    elif family == "GAUSSIAN_IDENTITY_LOGSIGMA":
        Y = z + 0.5 * rng.standard_normal(n)
    else:
        a = AUX.TRUE_A["TEST_A4"]
        y1 = rng.uniform(-1.0, 1.0, n)
        Y = np.stack([z + a[1] * y1 + a[2] + np.exp(a[0] + a[3] * y1) * rng.standard_normal(n), y1], 1)
    Dx, off = dims(shape)[0], offsets(shape)
    grp = np.full(Dx, -1, np.int32)
    for f, g in enumerate(groups):
        grp[off[f]:off[f] + terms[f][0]] = g
    local = None
    if loc is not None:
        local = np.zeros(Dx, np.int32)
        local[off[loc]:off[loc] + terms[loc][0]] = 1
    return X, Y, factors, grp, local, SLAB if loc is not None else None


def shape_priors(shape, seta=None):
    """normal and Student-t(4) on u, log half-t(3) on the scales and the lambdas, the defaults on a zeta with eta > 0, Student-t(3) on
    one with eta = 0, the defaults on every member of a GMRF term"""
    Dx, A, H, J, P, Sz = dims(shape)
    D, terms, off = SHAPES[shape][8], SHAPES[shape][2], offsets(shape)
    eta, se = etas(shape)
    se = se if seta is None else seta
    ze = eta + [e for s, e in zip(SHAPES[shape][5], se) if s[1] == AR1]
    Z = P + Sz
    rng = np.random.default_rng(D)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:Dx:2] = STUDENT_T
    kind[Dx + A:D - Z] = LOG_HALF_STUDENT_T
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx + A:D - Z] = 1.0
    for t, qn, k in SHAPES[shape][6]:
        sl = slice(off[t], off[t] + terms[t][0])
        kind[sl], mu[sl], tau[sl] = NORMAL, 0.0, 1.0
    nu[kind == STUDENT_T], nu[kind == LOG_HALF_STUDENT_T] = 4.0, 3.0
    for p in range(Z):
        cz = D - Z + p
        kind[cz], nu[cz], mu[cz], tau[cz] = (NORMAL, 0.0, 0.0, 1.0) if ze[p] > 0.0 else (STUDENT_T, 3.0, mu[cz], tau[cz])
    return kind, nu, mu, tau


def model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, structured="shape", **kw):
    g = idhmc.glm
    terms = SHAPES[shape][2]
    corr = [g.pair(a, b, e) for a, b, e in SHAPES[shape][4]] or None
    st = ([g.Structure(t, kd, e) for t, kd, e in SHAPES[shape][5]] or None) if structured == "shape" else structured
    gm = [g.gmrf(t, precision(idhmc, qn, terms[t][0]), k) for t, qn, k in SHAPES[shape][6]] or None
    return make_struct(idhmc, SHAPES[shape][0], X, Y, factors, grp, local, slab, kind, nu, mu, tau, corr, st, gmrf=gm, **kw)


def oracle_model(idhmc, oracle, work, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, seta=None):
    """the C twin of the row in the directory `work`: one directory per family, or one per test"""
    family, D = SHAPES[shape][0], SHAPES[shape][8]
    Xe = idhmc.glm.expand_factors(X, factors)
    eta, se = etas(shape)
    return oracle.OracleModel.custom(D, c_source_gmrf(family),
                                     oracle_params_gmrf(Xe, Y, SHAPE[family][2], grp, local, slab, kind, nu, pair_columns(shape), eta,
                                                        struct_columns(shape), se if seta is None else seta, gmrf_columns(idhmc, shape),
                                                        consts(family), mu, tau), str(work))


def options(idhmc, shape, **kw):
    """default_options for the row: beyond D = 512 a GLM takes the shared metric only (the NUTS kernel's LDS budget), so the two rows at
    L = 1024 run METRIC_SHARED wherever a context is made"""
    if SHAPES[shape][8] > 512:
        kw.setdefault("metric_mode", idhmc.METRIC_SHARED)
    return idhmc.default_options(**kw)


def start(shape, chains, seed=0):
    """start_struct, and in every third chain (0, 3, ..) the AR(1) terms' zetas at 2 .. 2.5 in magnitude, the sign alternating: with
    zeta ~ U(-0.8, 0.8) alone |phi| <= 0.67, so p = phi^h is below an ulp of what it multiplies from h = 128 on and the late stages of a
    long scan -- h = 256 and 512 at 520 and 600 levels -- change no bit; at |phi| >= 0.96 phi^512 > 1e-9"""
    Dx, A, H, J, P, Sz = dims(shape)
    q = start_struct(SHAPES[shape][0], chains, Dx, H, J, P, Sz, seed)
    if Sz:
        c = np.arange(0, chains, 3)
        q[c, q.shape[1] - Sz:] = (np.where((c // 3) % 2 == 0, 1.0, -1.0) * (2.0 + 0.5 * np.abs(q[c, -1]) / 0.8))[:, None]
    return q


def numpy_reference(idhmc, shape, Xe, Y, q, grp, local, slab, kind, nu, mu, tau):
    eta, se = etas(shape)
    return numpy_density_gmrf(SHAPES[shape][0], Xe, Y, q, grp, np.zeros(Xe.shape[1], int) if local is None else local, slab, kind, nu,
                              pair_columns(shape), eta, struct_columns(shape), se, gmrf_columns(idhmc, shape), mu, tau)


def check_numpy(idhmc, eng, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, ends):
    Xe = idhmc.glm.expand_factors(X, factors)
    q, g, lq = eng.q, eng.grad, eng.lq
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_reference(idhmc, shape, Xe, Y, q[c], grp, local, slab, kind, nu, mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


def create_through_the_c_boundary(idhmc, m, chains, opt, seed):
    """idhmc_create_glm_gmrf on model m with every descriptor it has: (rc, handle, message).  m must stay alive while the handle does"""
    from inplacedhmc_jl_amd import _lib
    lib = idhmc.load_library()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    desc = m.glm_desc()
    pr = _lib.GlmPriors(kind=m.prior_kind.ctypes.data_as(ip), nu=m.prior_nu.ctypes.data_as(dp))
    lc = None if not m.J else C.byref(_lib.GlmLocal(local=m.local.ctypes.data_as(ip), slab_scale=m.slab_scale or 0.0))
    fc = _lib.GlmFactors(F=m.F, levels=m.levels.ctypes.data_as(ip), index=m.factor_index.ctypes.data_as(ip))
    fv = None if m.factor_has is None else C.byref(_lib.GlmFactorValues(values=m.factor_values.ctypes.data_as(dp), has=m.factor_has.ctypes.data_as(ip)))
    pp = None if not m.P else C.byref(_lib.GlmPairs(P=m.P, first=m.pair_first.ctypes.data_as(ip), second=m.pair_second.ctypes.data_as(ip),
                                                    eta=m.pair_eta.ctypes.data_as(dp)))
    st = None if not m.S else C.byref(_lib.GlmStructs(S=m.S, term=m.struct_term.ctypes.data_as(ip), kind=m.struct_kind.ctypes.data_as(ip),
                                                      eta=m.struct_eta.ctypes.data_as(dp)))
    gm = None if not m.G else C.byref(_lib.GlmGmrfs(G=m.G, term=m.gmrf_term.ctypes.data_as(ip), start=m.gmrf_start.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    col=m.gmrf_col.ctypes.data_as(ip), val=m.gmrf_val.ctypes.data_as(dp),
                                                    kappa=m.gmrf_kappa.ctypes.data_as(dp)))
    h = C.c_void_p()
    rc = lib.idhmc_create_glm_gmrf(C.byref(h), 0, chains, 0, C.byref(desc), C.byref(pr), lc, C.byref(fc), fv, pp, st, gm, 1, 0, C.byref(opt), seed)
    return rc, h, lib.idhmc_last_error()


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def lane(c):
    """lane, chunk, component of a coordinate"""
    return (c & 127) >> 1, c >> 7, c & 1


def test_the_shapes_are_what_they_are_there_for(idhmc):
    chunks = lambda o, N: {lane(c)[1] for c in range(o, o + N)}
    for name, (family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n) in SHAPES.items():
        Dx, A, H, J, P, Sz = dims(name)
        assert Dx + A + H + J + P + Sz == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))) and len(terms) <= 4, name
        # the form of the NUTS kernel re-derived from (L, A, metric): section 12's table
        assert form == coop(L, A) and (name == "A4 per wave 256" or form == coop(L, A, shared=True)), name
    assert {s[10] for s in SHAPES.values()} == {0, 1} and [s for s in SHAPES if SHAPES[s][8] > 512] == ["everything 1024", "two ar1 two gmrf 1024"]
    # "everything 1024": NCH = 8; kCorr && kStruct && kGmrf && kLocal per wave; 520 levels: ten stages, the last h = 512 with p = phi^512 by
    # nine squarings, reading four chunks away; the GMRF term's members (its rows and glm_gmrf_sums, kappa > 0) lie in chunks 4, 5, 6;
    # the pair and its local scales with the slab in chunk 6; both zetas in chunk 7
    assert SHAPES["everything 1024"][9] == 1024 == 128 * 8 and 128 * 7 < 956
    assert struct_columns("everything 1024") == [(100, 520, AR1)] and stages(520) == 10 and 1 << 9 == 512 < 520 and 512 // 128 == 4
    assert chunks(100, 520) == {0, 1, 2, 3, 4}
    # the h = 512 stage changes bits only where phi^512 is not below an ulp: every third start has |zeta| >= 2, the others never do
    z = start("everything 1024", C_)[:, -1]
    assert np.abs(z[0::3]).min() >= 2.0 and np.tanh(2.0) ** 512 > 1e-9 and np.tanh(0.8) ** 256 < 2.0 ** -60 and (z[0:7:3] > 0).tolist() == [True, False, True]
    assert np.abs(np.delete(z, np.arange(0, C_, 3))).max() <= 0.8
    z2 = start("two ar1 two gmrf 1024", C_)[:, -2:]
    assert np.abs(z2[0::3]).min() >= 2.0 and np.abs(z2[36]).min() >= 2.0         # chain 36, which the numpy comparison takes, is one of them
    (o, N, Q, k), = gmrf_columns(idhmc, "everything 1024")
    assert (o, N, k) == (620, 150, 0.5) and chunks(o, N) == {4, 5, 6} and min(chunks(o, N)) >= 4
    assert pair_columns("everything 1024") == [(770, 830, 60)] and chunks(770, 120) == {6} and dims("everything 1024") == (890, 0, 4, 60, 1, 1)
    X, Y, factors, grp, local, slab = problem(idhmc, "everything 1024", 37)
    assert slab == SLAB and list(np.flatnonzero(local)) == list(range(830, 890)) and factors[0].values is not None and lane(954)[1] == lane(955)[1] == 7
    assert factors[0].index[0] == 519 >= 512 and factors[0].index[1] == 0 and factors[0].values[0] != 0.0      # level 519 has data and reads level 7
    # "two ar1 two gmrf 1024": two sampled phi, slot 1 the larger one (the stage loop runs to max(n0, n1) = n1: ten stages against eight);
    # slot 1 has the h = 512 stage and carries values; its zeta has eta = 0 and a Student-t entry; two GMRF slots behind them, chunk 6
    assert struct_columns("two ar1 two gmrf 1024") == [(100, 130, AR1), (230, 600, AR1)] and (stages(130), stages(600)) == (8, 10) and 600 > 512
    assert chunks(230, 600) == {1, 2, 3, 4, 5, 6} and dims("two ar1 two gmrf 1024") == (872, 0, 4, 0, 0, 2)
    assert [(o, N, k) for o, N, Q, k in gmrf_columns(idhmc, "two ar1 two gmrf 1024")] == [(830, 30, 2.0), (860, 12, 0.5)] and chunks(830, 42) == {6}
    kind, nu, mu, tau = shape_priors("two ar1 two gmrf 1024")
    assert (kind[876], kind[877], nu[877]) == (NORMAL, STUDENT_T, 3.0) and set(kind[830:872]) == {NORMAL} and set(kind[872:876]) == {LOG_HALF_STUDENT_T}
    # "two ar1 coop": the same on the matrix cores: slot 1 larger (six stages and eight), 150 > 128 levels across column 128 with values
    # and a sampled phi, four blocks of observations, the last of one
    assert struct_columns("two ar1 coop") == [(20, 40, AR1), (60, 150, AR1)] and (stages(40), stages(150)) == (6, 8) and chunks(60, 150) == {0, 1}
    assert SHAPES["two ar1 coop"][10:] == (1, 385) and (385 + 127) // 128 == 4 and 385 - 3 * 128 == 1 and dims("two ar1 coop") == (210, 0, 2, 0, 0, 2)
    # "composed coop": kCorr && kStruct && kGmrf with A = 1 and local scales on the matrix cores; the AR(1) term straddles column 128; two
    # blocks of observations
    assert dims("composed coop") == (210, 1, 4, 20, 1, 1) and struct_columns("composed coop") == [(110, 60, AR1)] and chunks(110, 60) == {0, 1}
    assert [(o, N, k) for o, N, Q, k in gmrf_columns(idhmc, "composed coop")] == [(10, 100, 0.25)] and pair_columns("composed coop") == [(170, 190, 20)]
    X, Y, factors, grp, local, slab = problem(idhmc, "composed coop", 130)
    assert slab == SLAB and list(np.flatnonzero(local)) == list(range(190, 210)) and factors[0].values is not None and SHAPES["composed coop"][10] == 1
    # "two pairs local D=L": D == L, so the zetas are the last two columns of the last chunk, coordinates 254 and 255; in pair (1, 0) the
    # first term (columns 90..159, across column 128) lies behind its second (20..89); local scales with the slab on the second term of
    # the other pair, whose zeta has eta = 0; four blocks
    assert SHAPES["two pairs local D=L"][8] == SHAPES["two pairs local D=L"][9] == 256 and dims("two pairs local D=L") == (220, 0, 4, 30, 2, 0)
    assert pair_columns("two pairs local D=L") == [(90, 20, 70), (160, 190, 30)] and chunks(90, 70) == {0, 1} and 90 > 20
    assert [256 - 2 + p for p in range(2)] == [254, 255] and lane(255) == (63, 1, 1) and SHAPES["two pairs local D=L"][11] == 385
    kind, nu, mu, tau = shape_priors("two pairs local D=L")
    assert (kind[254], kind[255], nu[255]) == (NORMAL, STUDENT_T, 3.0)
    X, Y, factors, grp, local, slab = problem(idhmc, "two pairs local D=L", 385)
    assert list(np.flatnonzero(local)) == list(range(190, 220)) and factors[0].index is factors[1][0]
    # "A4 per wave 256": A = 4 at L = 256 is the per-wave form at NCH = 2 under both metrics, with an AR(1) term across column 128 and a
    # GMRF term; Y has the response and its covariate
    assert SHAPES["A4 per wave 256"][9:11] == (256, 0) and coop(256, 4) == coop(256, 4, shared=True) == 0 and dims("A4 per wave 256")[1] == 4
    assert struct_columns("A4 per wave 256") == [(20, 150, AR1)] and chunks(20, 150) == {0, 1} and problem(idhmc, "A4 per wave 256", 130)[1].shape == (130, 2)
    # "struct local no pair": kStruct && kLocal && !kCorr: GlmWave::grad takes qm = q and scans a second time after the blocks; a random
    # walk, so no sampled zeta; the local scales are on the other term
    assert dims("struct local no pair") == (390, 0, 2, 40, 0, 0) and SHAPES["struct local no pair"][4] == () and SHAPES["struct local no pair"][7] == 1
    assert struct_columns("struct local no pair") == [(150, 200, RW1)] and SHAPES["struct local no pair"][10] == 0
    # "gmrf local 128": kGmrf && kLocal on the matrix cores, the local scales on the other term, which carries values
    assert dims("gmrf local 128") == (58, 0, 2, 20, 0, 0) and SHAPES["gmrf local 128"][9:11] == (128, 1) and SHAPES["gmrf local 128"][7] == 1
    assert [(o, N, k) for o, N, Q, k in gmrf_columns(idhmc, "gmrf local 128")] == [(8, 30, 1.0)]


def indicator_matrix(shape, X, factors):
    """the expanded matrix from its definition: X in front, then w_f[i] (1.0 without values) at column off_f + idx_f[i], +0.0 elsewhere"""
    n, Dd = X.shape
    E = np.zeros((n, dims(shape)[0]))
    E[:, :Dd] = X
    for off, t in zip(offsets(shape), factors):
        idx, w = (t.index, t.values) if hasattr(t, "values") else (t[0], None)
        E[np.arange(n), off + np.asarray(idx)] = 1.0 if w is None else np.asarray(w)
    return E


@pytest.mark.parametrize("shape", list(SHAPES))
def test_table_arithmetic(idhmc, shape):
    """idhmc.GLM accepts the row with the table's D, P, S, Sz, G and the offsets and stage counts derived from it; glm.expand_factors has
    the bits of the matrix built from its definition"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    Dx, A, H, J, P, Sz = dims(shape)
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, *shape_priors(shape))
    assert (m.D, m.Dx, m.Dd, m.F, m.A, m.H, m.J, m.P, m.S, m.Sz, m.G, m.K) == (D, Dx, Dd, len(terms), A, H, J, P, len(structs), Sz, len(gmrfs), SHAPE[family][0])
    assert (m.slab_scale is None) == (loc is None) and 128 * (1 << int(np.ceil(np.log2((m.D + 127) // 128)))) == L
    off = offsets(shape)
    assert off[0] == Dd and all(off[f + 1] - off[f] == terms[f][0] for f in range(len(terms) - 1)) and off[-1] + terms[-1][0] == Dx
    assert [idhmc.glm.factor_columns(m, f).start for f in range(len(terms))] == off
    assert [stages(N) for o, N, kd in struct_columns(shape)] == [len([h for h in (1 << k for k in range(11)) if h < N]) for o, N, kd in struct_columns(shape)]
    E = indicator_matrix(shape, X, factors)
    assert E.shape == (n, Dx) and same_bits(E, idhmc.glm.expand_factors(X, factors))
    assert all(np.count_nonzero(E[:, o:o + t[0]], axis=1).max() <= 1 for o, t in zip(off, terms))


def test_every_shape_passes_the_argument_checks(idhmc):
    """idhmc_create_glm_gmrf with 37 chains: accepted, or stopped at the device check, which is past every argument check.  The rows at
    L = 1024 are refused with the per-chain metric, so every device test of them runs the shared one"""
    lib = idhmc.load_library()
    for shape in SHAPES:
        X, Y, factors, grp, local, slab = problem(idhmc, shape, SHAPES[shape][11])
        m = model(idhmc, shape, X, Y, factors, grp, local, slab, *shape_priors(shape))
        if SHAPES[shape][8] > 512:
            rc, h, msg = create_through_the_c_boundary(idhmc, m, C_, idhmc.default_options(max_depth=4), 3)
            assert rc == idhmc.ERR_BAD_ARG and b"with D > 512 needs metric_mode = SHARED" in msg, (shape, rc, msg)
        rc, h, msg = create_through_the_c_boundary(idhmc, m, C_, options(idhmc, shape, max_depth=4), 3)
        if rc == 0:
            lib.idhmc_destroy(h)
        assert rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg), (shape, rc, msg)


# ---- the twin against numpy, numpy against mpmath ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """one directory per family for the compiled restatement: a second family in a directory would run the first one's observation"""
    dirs = {}

    def of(family):
        if family not in dirs:
            dirs[family] = str(tmp_path_factory.mktemp("composed_" + family.lower()))
        return dirs[family]
    return of


@pytest.mark.parametrize("shape", list(SHAPES))
def test_twin_matches_numpy(idhmc, oracle, work, shape):
    """l and every gradient coordinate of the C twin within 1e-12 of the magnitude of numpy's terms, at three starts, the zetas flipped
    (zeta -> -zeta - 1) in the third: the precondition of the device file, which has no tolerance of its own"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    Dx, A, H, J, P, Sz = dims(shape)
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = shape_priors(shape)
    om = oracle_model(idhmc, oracle, work(family), shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    Xe = idhmc.glm.expand_factors(X, factors)
    for k in range(3):
        q = start(shape, 1, seed=k)[0]
        if k == 2:
            q[D - P - Sz:] = -q[D - P - Sz:] - 1.0
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_reference(idhmc, shape, Xe, Y, q, grp, local, slab, kind, nu, mu, tau)
        assert np.isfinite(lq) and abs(lq - l_ref) <= 1e-12 * lscale, (k, lq, l_ref)
        assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), (k, np.max(np.abs(g[:D] - g_ref) / gscale))


def test_numpy_gradient_is_mpmath_derivative_of_the_composed_model(idhmc):
    """Every feature at once on a few levels each: a Gaussian likelihood with a sampled log sigma (A = 1), Dd = 2, an AR(1) term of 4 levels
    with values (Beta(2, 2) on (phi + 1) / 2) and one of 3 levels (a normal entry on its zeta), a pair of terms of 3 levels on one index
    (LKJ eta = 2) whose second carries values and local scales with a slab, and an ICAR term over the 5-region map with kappa = 0.75;
    every term has a sampled scale.  These are five terms, one more than a model may have: numpy's density, like the twin's, works on
    column ranges and does not know.  The log density is written in mpmath from b = sigma .* (L u), the sequential recurrence
    ut_k = phi ut_{k-1} + sqrt(1 - phi^2) u_k, st = s / sqrt(1 + s^2 / S^2) and -1/2 u'Qu - 1/2 kappa (sum u)^2, and differentiated
    numerically at 40 digits; numpy's l and gradient are within 1e-12 of their terms' magnitude"""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(4)
    n, Dd, Ns, S, kappa, eta = 16, 2, (4, 3, 3, 3, 5), 2.0, 0.75, 2.0
    off = [Dd + sum(Ns[:f]) for f in range(5)]
    Dx = Dd + sum(Ns)
    A, H, J, P, Sz = 1, 5, 3, 1, 2
    D = Dx + A + H + J + P + Sz
    X = 0.5 * rng.standard_normal((n, Dd))
    t0, t1, t2, t4 = (rng.integers(0, N, n) for N in (4, 3, 3, 5))
    w0, w3 = 1.0 + 0.5 * rng.standard_normal(n), 1.0 + 0.5 * rng.standard_normal(n)
    Y = rng.standard_normal(n)
    Xe = np.zeros((n, Dx))
    Xe[:, :Dd] = X
    r = np.arange(n)
    Xe[r, off[0] + t0], Xe[r, off[1] + t1], Xe[r, off[2] + t2], Xe[r, off[3] + t2], Xe[r, off[4] + t4] = w0, 1.0, 1.0, w3, 1.0
    grp = np.full(Dx, -1)
    for f in range(5):
        grp[off[f]:off[f] + Ns[f]] = f
    local = np.zeros(Dx, int)
    local[off[3]:off[3] + 3] = 1
    Q = idhmc.glm.icar_precision(MAP5, 5)
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    mu[off[4]:off[4] + 5], tau[off[4]:off[4] + 5] = 0.0, 1.0
    zp, za0, za1 = D - 3, D - 2, D - 1
    for cz in (zp, za0):
        mu[cz], tau[cz] = 0.0, 1.0
    pairs, structs, gm = [(off[2], off[3], 3)], [(off[0], 4, AR1), (off[1], 3, AR1)], [(off[4], 5, Q, kappa)]
    f_ = lambda x: mp.mpf(float(x))

    def logp(*q):
        u, a, om, lam = q[:Dx], q[Dx], q[Dx + A:Dx + A + H], q[Dx + A + H:Dx + A + H + J]
        sig = [mp.exp(o) for o in om]
        walks = []
        for (o, N, kd), z in zip(structs, (q[za0], q[za1])):
            phi = mp.tanh(z)
            c = mp.sqrt(1 - phi * phi)
            ut = [u[o]]
            for k in range(1, N):
                ut.append(phi * ut[-1] + c * u[o + k])
            walks.append(ut)
        rho = mp.tanh(q[zp])
        mix = [rho * u[off[2] + k] + mp.sqrt(1 - rho * rho) * u[off[3] + k] for k in range(3)]
        st = []
        for k in range(3):
            s = sig[3] * mp.exp(lam[k])
            st.append(s / mp.sqrt(1 + s * s / (S * S)))
        total = mp.mpf(0)
        for i in range(n):
            z = sum(f_(X[i, j]) * u[j] for j in range(Dd))
            z += f_(w0[i]) * sig[0] * walks[0][t0[i]] + sig[1] * walks[1][t1[i]]
            z += sig[2] * u[off[2] + t2[i]] + f_(w3[i]) * st[t2[i]] * mix[t2[i]]
            z += sig[4] * u[off[4] + t4[i]]
            e = (f_(Y[i]) - z) / mp.exp(a)
            total += -e * e / 2 - a
        for j in list(range(off[4])) + list(range(Dx, zp)) + [za1]:
            total -= f_(tau[j]) * (q[j] - f_(mu[j])) ** 2 / 2
        ug = u[off[4]:off[4] + 5]
        for i in range(5):
            for j in range(5):
                total -= f_(Q[i, j]) * ug[i] * ug[j] / 2
        total -= mp.mpf(kappa) * sum(ug) ** 2 / 2
        return total + eta * mp.log(1 - rho * rho) + eta * mp.log(1 - mp.tanh(q[za0]) ** 2)

    for seed, zetas in enumerate(((0.7, -1.3, 0.4), (-0.9, 0.2, -1.1))):
        r_ = np.random.default_rng(seed)
        q = np.r_[r_.uniform(-0.8, 0.8, Dx), np.log(0.8) + r_.uniform(-0.2, 0.2), np.log(0.6) + r_.uniform(-0.3, 0.3, H), r_.uniform(-0.7, 0.7, J), zetas]
        l, g, ls, gs = numpy_density_gmrf("GAUSSIAN_IDENTITY_LOGSIGMA", Xe, Y, q, grp, local, S, np.zeros(D, int), np.zeros(D), pairs, [eta], structs,
                                          [eta, 0.0], gm, mu, tau)
        qm = [f_(x) for x in q]
        assert abs(float(logp(*qm) - mp.mpf(float(l)))) <= 1e-12 * ls
        for j in range(D):
            order = tuple(1 if i == j else 0 for i in range(D))
            ref = mp.diff(logp, tuple(qm), order)
            assert abs(float(ref - mp.mpf(float(g[j])))) <= 1e-12 * gs[j] + 1e-300, (seed, j, float(ref), g[j])


# ---- the reported vector ----------------------------------------------------------------------------------------------------------------
def theta_composed_twin(draws, Dx, A, H, J, P, Sz, grp, local, inv2, pairs, structs, dexp):
    """[..., D] sampled coordinates [u | a | omega | lambda | zeta of the pairs | zeta of the AR(1) terms] -> the reported vector
    [beta | a raw | sigma | exp lambda | rho | phi] by the expressions of k_summary_struct_theta and k_summary_corr_theta, fma through
    exact rationals, dexp the oracle's: the scan of every structure slot (phi and c of its own zeta, 1 and 1 for a random walk), then
    the pairs' mix, then the scale: e_g f with the slab (i = 1 / s, nn = fma(i, i, inv2), 1 / sqrt(nn)) on a flagged column, e_g on
    another column of a group.  pairs: (first column, second column, levels); structs: (column, levels, kind)"""
    draws = np.asarray(draws, dtype=np.float64)
    out = draws.copy()
    flat, oflat = draws.reshape(-1, draws.shape[-1]), out.reshape(-1, draws.shape[-1])
    D = flat.shape[1]
    assert D == Dx + A + H + J + P + Sz and len(pairs) == P and sum(1 for s in structs if s[2] == AR1) == Sz
    lam = {int(c): Dx + A + H + k for k, c in enumerate(np.flatnonzero(local))} if J else {}
    assert len(lam) == J

    def rho_c(z):
        s = np.float64(dexp(-abs(z)))
        t = s * s
        d = 1.0 + t
        return np.copysign((1.0 - t) / d, z), (2.0 * s) / d

    for r in range(flat.shape[0]):
        q = flat[r]
        e = [np.float64(dexp(q[Dx + A + g])) for g in range(H)]
        ut = q[:Dx].copy()
        z = 0
        for o, N, kd in structs:
            phi, c = np.float64(1.0), np.float64(1.0)
            if kd == AR1:
                phi, c = rho_c(q[D - Sz + z])
                z += 1
            ut[o:o + N] = scan_twin(q[o:o + N], phi, c)
        for p, (o1, o2, N) in enumerate(pairs):
            rho, c = rho_c(q[D - Sz - P + p])
            for k in range(N):
                ut[o2 + k] = fma_twin(rho, q[o1 + k], c * ut[o2 + k])
        for j in range(Dx):
            if j in lam:
                f = np.float64(dexp(q[lam[j]]))
                s = e[grp[j]] * f if H and grp[j] >= 0 else f
                st = s
                if inv2 != 0.0:
                    iv = np.float64(1.0) / s
                    st = np.float64(1.0) / np.sqrt(np.float64(fma_twin(iv, iv, inv2)))
                oflat[r, j] = ut[j] * st
            else:
                oflat[r, j] = ut[j] * e[grp[j]] if H and grp[j] >= 0 else ut[j]
        for d in range(Dx + A, D - P - Sz):
            oflat[r, d] = dexp(q[d])
        for d in range(D - P - Sz, D):
            oflat[r, d] = rho_c(q[d])[0]
    return out


def theta_of_shape(draws, shape, grp, local, slab, dexp):
    """theta_composed_twin on a row of the table"""
    return theta_composed_twin(draws, *dims(shape), grp, local, inv2_of(slab), pair_columns(shape), struct_columns(shape), dexp)


def assert_host_helpers(idhmc, m, shape, draws, th):
    """th = theta_composed_twin(draws) against glm.coefficients, glm.correlations and glm.autocorrelations, which round every product
    where the twin fuses it.  A coefficient is a sum (the scan's, the mix's) that may cancel, so its bound is the project's 1e-12 of the
    magnitude of the terms summed: glm.coefficients at |u| and |zeta|, where every term of every sum has its magnitude and none
    cancels.  rho and phi are no sums: 1e-12 relative"""
    Dx, A, H, J, P, Sz = dims(shape)
    D = draws.shape[-1]
    g = idhmc.glm
    mags = np.array(draws, dtype=np.float64)
    mags[..., :Dx], mags[..., D - P - Sz:] = np.abs(mags[..., :Dx]), np.abs(mags[..., D - P - Sz:])
    err = np.abs(th[..., :Dx] - g.coefficients(m, draws))
    assert np.all(err <= 1e-12 * g.coefficients(m, mags) + 1e-300), np.max(err / (g.coefficients(m, mags) + 1e-300))
    assert np.allclose(th[..., D - Sz - P:D - Sz], g.correlations(m, draws), rtol=1e-12, atol=1e-300)
    assert np.allclose(th[..., D - Sz:], g.autocorrelations(m, draws), rtol=1e-12, atol=1e-300) and g.autocorrelations(m, draws).shape[-1] == Sz


def test_theta_twin_has_the_bits_of_the_twins_it_generalises(idhmc, oracle):
    """on "odd offset" of tests/test_gpu_glm_struct.py theta_struct_twin's bits, on "one tile" of tests/test_gpu_glm_corr.py
    theta_corr_twin's, with the ends of zeta among the draws"""
    import test_gpu_glm_corr as GC
    import test_gpu_glm_struct as GS
    dexp = oracle.lib().orc_exp_export
    for mod, shape, old in ((GS, "odd offset", GS.theta_struct_twin), (GC, "one tile", GC.theta_corr_twin)):
        X, Y, factors, grp, local, slab = mod.problem(idhmc, shape, 37)
        draws = np.stack([mod.start(shape, 6, seed=k) for k in range(3)])
        draws[0, 0, -1], draws[1, 1, -1], draws[2, 2, -1] = 800.0, -40.0, 0.0
        d = mod.dims(shape)
        Dx, A, H, J, P, Sz = d if len(d) == 6 else d + (0,)
        assert J == 0 and local is None
        structs = GS.struct_columns(shape) if mod is GS else []
        got = theta_composed_twin(draws, Dx, A, H, J, P, Sz, grp, np.zeros(Dx, int), 0.0, mod.pair_columns(shape), structs, dexp)
        assert same_bits(got, old(draws, shape, grp, dexp)), shape
        assert got[0, 0, -1] == 1.0 and got[2, 2, -1] == 0.0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_theta_twin_agrees_with_the_host_helpers(idhmc, oracle, shape):
    """within 1e-12 of glm.coefficients, glm.correlations and glm.autocorrelations (assert_host_helpers) on two draws of four chains of
    every row, the first of them with |zeta| >= 2 on the AR(1) terms; a raw, sigma and exp lambda are dexp's"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    Dx, A, H, J, P, Sz = dims(shape)
    g = idhmc.glm
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    m = model(idhmc, shape, X, Y, factors, grp, local, slab, *shape_priors(shape))
    draws = np.stack([start(shape, 4, seed=k) for k in range(2)])
    th = theta_of_shape(draws, shape, grp, local, slab, oracle.lib().orc_exp_export)
    assert th.shape == draws.shape and np.isfinite(th).all()
    assert_host_helpers(idhmc, m, shape, draws, th)
    assert same_bits(th[..., Dx:Dx + A], draws[..., Dx:Dx + A])
    assert np.allclose(th[..., Dx + A:Dx + A + H], g.group_scales(m, draws), rtol=1e-12, atol=0)
    assert np.allclose(th[..., Dx + A + H:Dx + A + H + J], g.local_scales(m, draws), rtol=1e-12, atol=0)
