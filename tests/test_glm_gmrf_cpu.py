"""GMRF terms (GLM(..., gmrf=[glm.gmrf(term, Q, sum_to_zero)]), idhmc_create_glm_gmrf) without a GPU: glm.gmrf and the
constructor's validation, the precision builders against their definitions, glm.scale_precision against numpy.linalg.pinv, the C
boundary's argument checks, and the C restatement of PRIOR row 6 (the header comment of idhmc_glm_coords.hpp) against a numpy density
-1/2 u'Qu - 1/2 kappa (1'u)^2, whose gradient is held against mpmath's differentiation (40 digits) of the log density written straight
from the model.

The restatement is C_BODY_STRUCT of tests/test_glm_struct_cpu.py with the GMRF tables added to its params and row 6 to its prior loop:
params are [n, K, nc, A, H, J, P, S, Sz, inv2, G, R, Z, mu (D), tau (D), kind (D, as doubles; 6 marks a member of a GMRF term), nu (D),
c (nc), grp (Dx), local (Dx), cpart (Dx), spart (Dx), N and kind of the two structure slots, gpart (Dx, as doubles: -1 or k + 1024 slot),
kappa of the two GMRF slots, start (R + 1, R = the rows of both slots), col (Z entries), val (Z), X row-major, Y row-major].  The GPU
tests (tests/test_gpu_glm_gmrf.py) hand the same source to the oracle."""
import ctypes as C

import numpy as np
import pytest

import test_glm_hier_cpu as HIER
import test_glm_struct_cpu as ST
from test_glm_corr_cpu import _pairs_struct, _priors_struct
from test_glm_factors_cpu import SUBJECT, _data, _factors_struct
from test_glm_hier_cpu import SHAPE, consts
from test_glm_priors_cpu import NORMAL, STUDENT_T
from test_glm_slopes_cpu import DOSE, _values_struct
from test_glm_struct_cpu import AR1, RW1, _local_struct, _structs_struct

GMRF_KIND = 6      # the device table's (and the restatement's) mark of a member of a GMRF term; never a public kind

_SUMS = """    double g_S[2] = {0.0, 0.0}, g_R[2][128];
    int g_n[2] = {0, 0};
    for (int r = 0; r < 128; ++r) g_R[0][r] = g_R[1][r] = 0.0;
    for (int j = 0; j < Dx; ++j)
        if (gp[j] >= 0.0) {
            const int i = (int)gp[j] >> 10;
            g_n[i]++;
            g_R[i][j & 127] = g_R[i][j & 127] + q[j];
        }
    for (int i = 0; i < NG; ++i)
        if (gk[i] > 0.0) g_S[i] = orc_tree128(g_R[i]);
"""
_ROW6 = """        } else if (k == 6) {
            const int ge = (int)gp[j], i = ge >> 10, lv = ge & 1023, o = j - lv, rb = i ? g_n[0] : 0;
            double s = gk[i] > 0.0 ? gk[i] * g_S[i] : 0.0;
            for (long e = (long)gst[rb + lv]; e < (long)gst[rb + lv + 1]; ++e) s = fma(gval[e], q[o + (int)gcol[e]], s);
            T[r] = fma(q[j], s, T[r]);
            grad[j] = G - s;
        } else if (k == 5) {"""


def _body():
    s = ST.C_BODY_STRUCT
    loop = "    for (int j = 0; j < D; ++j) {\n        const double d = q[j] - mu[j], G = grad[j], t = tau[j], f = nu[j];"
    for old, new in (("const double inv2 = params[9];",
                      "const double inv2 = params[9];\n    const int NG = (int)params[10], GR = (int)params[11], GNZ = (int)params[12];"),
                     ("*mu = params + 10,", "*mu = params + 13,"),
                     ("*X = sk + 2,", "*gp = sk + 2, *gk = gp + Dx, *gst = gk + 2, *gcol = gst + GR + 1, *gval = gcol + GNZ,\n                 *X = gval + GNZ,"),
                     (loop, _SUMS + loop), ("        } else if (k == 5) {", _ROW6)):
        assert s.count(old) == 1, old
        s = s.replace(old, new)
    return s


C_BODY_GMRF = _body()


def c_source_gmrf(family):
    """C_BODY_GMRF around the family's observation, as test_glm_struct_cpu.c_source_struct builds on HIER.c_source_hier"""
    body = HIER.c_source_hier(family)
    head, tail = HIER.C_BODY_HIER.split("%s")
    assert body.startswith(head) and body.endswith(tail)
    return C_BODY_GMRF % body[len(head):len(body) - len(tail)]


def csr(Q):
    """(indptr, indices, data) of a dense Q: its non-zero entries and its whole diagonal, as glm.gmrf keeps them"""
    Q = np.asarray(Q, float)
    keep = (Q != 0.0) | np.eye(Q.shape[0], dtype=bool)
    rows, cols = np.nonzero(keep)
    return np.r_[0, np.cumsum(keep.sum(1))].astype(np.int64), cols.astype(np.int32), Q[rows, cols]


def oracle_params_gmrf(Xe, Y, A, grp, local, S, kind, nu, pairs, eta, structs, seta, gmrfs, c=None, mu=None, tau=None):
    """test_glm_struct_cpu.oracle_params_struct with gmrfs = [(off, N, Q dense, kappa)] per slot: their members get the mark 6"""
    base = ST.oracle_params_struct(Xe, Y, A, grp, local, S, kind, nu, pairs, eta, structs, seta, c, mu, tau)
    n, Dx = Xe.shape
    D = (base.size - 10 - (0 if c is None else np.asarray(c).size) - 4 * Dx - 4 - n * Dx - np.asarray(Y).size) // 4
    gp, gk, start, col, val = np.full(Dx, -1.0), np.zeros(2), [np.zeros(1)], [], []
    kd = base[10 + 2 * D:10 + 3 * D].copy()
    for i, (o, N, Q, kappa) in enumerate(gmrfs):
        gp[o:o + N] = np.arange(N) + 1024 * i
        gk[i] = kappa
        kd[o:o + N] = GMRF_KIND
        ip, ix, dt = csr(Q)
        start.append(start[-1][-1] + ip[1:])
        col.append(ix.astype(float))
        val.append(dt)
    start, col, val = np.concatenate(start), np.concatenate(col + [np.zeros(0)]), np.concatenate(val + [np.zeros(0)])
    tail = n * Dx + np.asarray(Y).size
    head = base[:base.size - tail].copy()
    head[10 + 2 * D:10 + 3 * D] = kd
    return np.concatenate([head[:10], [float(len(gmrfs)), float(start.size - 1), float(val.size)], head[10:], gp, gk, start, col, val,
                           base[base.size - tail:]])


def numpy_density_gmrf(family, Xe, Y, q, grp, local, S, kind, nu, pairs, eta, structs, seta, gmrfs, mu=None, tau=None):
    """test_glm_struct_cpu.numpy_density_struct with no prior on the members (tau = 0 there), then -1/2 u'Qu - 1/2 kappa (1'u)^2 and its
    gradient -(Qu + kappa (1'u) 1) per GMRF term: (l, grad, magnitude of l's terms, per-coordinate magnitude of the gradient's)"""
    D = q.size
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,)).copy()
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,)).copy()
    for o, N, Q, kappa in gmrfs:
        tau[o:o + N], mu[o:o + N] = 0.0, 0.0
    l, g, ls, gs = ST.numpy_density_struct(family, Xe, Y, q, grp, local, S, kind, nu, pairs, eta, structs, seta, mu, tau)
    g, gs = g.copy(), gs.copy()
    for o, N, Q, kappa in gmrfs:
        u, Q = q[o:o + N], np.asarray(Q, float)
        l += -0.5 * u @ Q @ u - 0.5 * kappa * u.sum() ** 2
        ls += 0.5 * np.abs(u) @ np.abs(Q) @ np.abs(u) + 0.5 * kappa * np.abs(u).sum() ** 2
        g[o:o + N] += -(Q @ u) - kappa * u.sum()
        gs[o:o + N] += np.abs(Q) @ np.abs(u) + kappa * np.abs(u).sum()
    return l, g, ls, gs


def grid_edges(rows, cols):
    """the rook neighbourhoods of a rows x cols grid, region r * cols + c"""
    e = []
    for r in range(rows):
        for c in range(cols):
            if c + 1 < cols:
                e.append((r * cols + c, r * cols + c + 1))
            if r + 1 < rows:
                e.append((r * cols + c, (r + 1) * cols + c))
    return e


# ---- glm.gmrf, the builders and the constructor ---------------------------------------------------------------------------------------
REGION = np.array([0, 4, 1, 2, 3, 0, 2])           # 5 regions
MAP5 = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4)]     # a triangle with a tail


def test_icar_precision_is_d_minus_w(idhmc):
    g = idhmc.glm
    W = np.zeros((5, 5))
    for i, j in MAP5:
        W[i, j] = W[j, i] = 1.0
    Q = g.icar_precision(MAP5, 5)
    assert np.array_equal(Q, np.diag(W.sum(1)) - W) and np.array_equal(np.diag(Q), [2.0, 2.0, 3.0, 2.0, 1.0])
    assert np.array_equal(Q @ np.ones(5), np.zeros(5)) and np.linalg.matrix_rank(Q) == 4
    assert np.array_equal(g.icar_precision([(1, 0)], 3), [[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])      # an island: iid
    for bad in ([(0, 5)], [(2, 2)], [(-1, 0)]):
        with pytest.raises(ValueError, match="two different regions"):
            g.icar_precision(bad, 5)
    assert np.array_equal(g.rw1_precision(4), g.icar_precision([(0, 1), (1, 2), (2, 3)], 4))


def test_walk_and_seasonal_precisions_are_their_difference_operators(idhmc):
    g = idhmc.glm
    for N in (3, 7, 150):
        D2 = np.zeros((N - 2, N))
        for r in range(N - 2):
            D2[r, r:r + 3] = [1.0, -2.0, 1.0]
        assert np.array_equal(g.rw2_precision(N), D2.T @ D2)
        k = np.arange(N, dtype=float)
        assert np.array_equal(g.rw2_precision(N) @ np.c_[np.ones(N), k], np.zeros((N, 2)))          # the level and the slope are free
    assert np.array_equal(np.diag(g.rw2_precision(7)), [1.0, 5.0, 6.0, 6.0, 6.0, 5.0, 1.0])
    for N, m in ((9, 4), (12, 12), (5, 2)):
        Sm = np.zeros((N - m + 1, N))
        for r in range(N - m + 1):
            Sm[r, r:r + m] = 1.0
        assert np.array_equal(g.seasonal_precision(N, m), Sm.T @ Sm) and np.linalg.matrix_rank(g.seasonal_precision(N, m)) == N - m + 1
    for fn, args in ((g.rw2_precision, (2,)), (g.rw1_precision, (1,)), (g.seasonal_precision, (3, 4)), (g.seasonal_precision, (9, 1))):
        with pytest.raises(ValueError):
            fn(*args)


def test_scaled_precisions_have_unit_geometric_mean_variance(idhmc):
    g = idhmc.glm
    for Q in (g.icar_precision(grid_edges(6, 5), 30), g.rw2_precision(40), g.seasonal_precision(24, 4), g.icar_precision(MAP5, 5),
              3.0 * np.eye(4)):
        Qs = g.scale_precision(Q)
        var = np.diag(np.linalg.pinv(Qs, hermitian=True))
        assert abs(np.exp(np.mean(np.log(var))) - 1.0) <= 1e-10
        ratio = Qs[Q != 0.0] / Q[Q != 0.0]
        assert np.allclose(ratio, ratio[0], rtol=1e-15) and np.array_equal(Qs, Qs.T) and np.array_equal(Qs != 0.0, Q != 0.0)
    for bad in (np.ones((2, 3)), np.array([[1.0, 2.0], [0.0, 1.0]]), -np.eye(3)):
        with pytest.raises(ValueError):
            g.scale_precision(bad)


def test_gmrf_is_a_small_named_tuple_and_checks_its_table(idhmc):
    g = idhmc.glm
    Q = g.icar_precision(MAP5, 5)
    e = g.gmrf(0, Q, sum_to_zero=0.5)
    assert isinstance(e, tuple) and e._fields == ("term", "indptr", "indices", "data", "kappa") and e.term == 0 and e.kappa == 0.5
    ip, ix, dt = csr(Q)
    assert np.array_equal(e.indptr, ip) and np.array_equal(e.indices, ix) and np.array_equal(e.data, dt) and g.gmrf(1, Q).kappa == 0.0
    t = g.gmrf(0, (ip, ix, dt))
    assert np.array_equal(t.indptr, ip) and t.indptr.dtype == np.int64 and t.indices.dtype == np.int32 and np.array_equal(t.data, dt)
    g.gmrf(0, np.eye(3))                                                    # proper
    g.gmrf(0, g.rw2_precision(150))                                         # semi-definite and kappa = 0: allowed, improper
    g.gmrf(0, np.ones((128, 128)) + 128.0 * np.eye(128))                    # a row of the full 128 entries
    for k in (-1.0, np.inf, np.nan, "1", True):
        with pytest.raises(ValueError, match="sum_to_zero"):
            g.gmrf(0, Q, k)
    bad = [("square matrix", np.ones((2, 3))), ("symmetric", np.array([[1.0, 0.5], [0.25, 1.0]])), ("diagonal must be present and > 0", np.zeros((2, 2))),
           ("diagonal must be present and > 0", np.array([[1.0, 0.0], [0.0, -1.0]])), ("non-finite", np.array([[1.0, np.nan], [np.nan, 1.0]])),
           ("entries", np.ones((130, 130)) + 130.0 * np.eye(130)), ("not a precision", np.array([[1.0, 2.0], [2.0, 1.0]])),
           ("strictly ascending", (np.array([0, 2, 3]), np.array([1, 0, 1]), np.array([-1.0, 1.0, 1.0]))),
           ("strictly ascending", (np.array([0, 2, 3]), np.array([0, 2, 1]), np.array([1.0, 1.0, 1.0]))),
           ("symmetric", (np.array([0, 2, 3]), np.array([0, 1, 1]), np.array([1.0, -0.5, 1.0]))),
           ("diagonal must be present", (np.array([0, 1, 2]), np.array([1, 0]), np.array([0.5, 0.5]))),
           ("indptr must not decrease", (np.array([0, 2, 1]), np.array([0]), np.array([1.0]))),
           ("entries", (np.array([0, 0, 1]), np.array([1]), np.array([1.0])))]
    for what, q in bad:
        with pytest.raises(ValueError, match=what):
            g.gmrf(0, q)
    # the eigenvalue bound: an indefinite Q is refused, and kappa can pay for the constant direction only
    with pytest.raises(ValueError, match="not a precision"):
        g.gmrf(0, Q - 0.01 * np.ones((5, 5)))
    g.gmrf(0, Q - 0.01 * np.ones((5, 5)), sum_to_zero=0.02)
    with pytest.raises(ValueError, match="not a precision"):
        g.gmrf(0, np.array([[1.0, 2.0], [2.0, 1.0]]), sum_to_zero=100.0)          # (1, -1) has the eigenvalue -1 whatever kappa is


def _region_model(idhmc, gmrf=None, **kw):
    X, Y = _data()
    g = idhmc.glm
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[(REGION, 5), SUBJECT], gmrf=gmrf, **kw)


def test_constructor_keeps_the_gmrfs(idhmc):
    g = idhmc.glm
    Q = g.icar_precision(MAP5, 5)
    m = _region_model(idhmc, [g.gmrf(0, Q, 0.25)], groups=g.random_effects(2, [5, 4])["groups"])
    assert (m.Dx, m.H, m.G, m.D) == (11, 2, 1, 13) and list(m.gmrf_term) == [0] and list(m.gmrf_kappa) == [0.25]
    assert m.gmrf_term.dtype == m.gmrf_col.dtype == np.int32 and m.gmrf_start.dtype == np.int64 and m.gmrf_val.dtype == np.float64
    ip, ix, dt = csr(Q)
    assert np.array_equal(m.gmrf_start, ip) and np.array_equal(m.gmrf_col, ix) and np.array_equal(m.gmrf_val, dt)
    assert np.array_equal(g.gmrf_precision(m, 0), Q) and m.gmrfs[0].term == 0
    # two terms: the rows of slot 0, then those of slot 1, start cumulative
    Q4 = g.rw1_precision(4)
    m = _region_model(idhmc, [g.gmrf(1, Q4), g.gmrf(0, Q, 1.0)])
    ip4 = csr(Q4)[0]
    assert m.G == 2 and list(m.gmrf_term) == [1, 0] and np.array_equal(m.gmrf_start, np.r_[ip4, ip4[-1] + ip[1:]]) and m.gmrf_val.size == ip4[-1] + ip[-1]
    assert np.array_equal(g.gmrf_precision(m, 0), Q4) and np.array_equal(g.gmrf_precision(m, 1), Q)
    for kw in ({}, {"gmrf": None}, {"gmrf": []}):
        m = _region_model(idhmc, **kw)
        assert m.G == 0 and m.gmrfs is None and m.gmrf_term is None and m.D == 11
    assert idhmc.GLM(*_data(), g.POISSON_LOG).G == 0


def test_no_new_coordinate_so_the_reported_vector_is_unchanged(idhmc):
    """glm.coefficients and the other host helpers see a GMRF model as the model without the keyword: D, the layout and the values"""
    g = idhmc.glm
    kw = g.gmrf_effects(2, [5, 4], [g.gmrf(0, g.icar_precision(MAP5, 5), 1.0)])
    base = g.random_intercepts(2, [5, 4])
    assert sorted(kw) == sorted(list(base) + ["gmrf"]) and all(np.array_equal(kw[k], base[k]) for k in base)
    m, m0 = _region_model(idhmc, **kw), _region_model(idhmc, **base)
    assert (m.D, m.Dx, m.H, m.P, m.S, m.Sz) == (m0.D, m0.Dx, m0.H, m0.P, m0.S, m0.Sz) and m.G == 1 and m0.G == 0
    draws = np.random.default_rng(0).standard_normal((3, 4, m.D))
    assert np.array_equal(g.coefficients(m, draws), g.coefficients(m0, draws)) and np.array_equal(g.group_scales(m, draws), g.group_scales(m0, draws))
    # next to a pair and a structure
    kw = g.gmrf_effects(1, [5, 4, 4, 3], [g.gmrf(0, g.icar_precision(MAP5, 5))], structured=[g.ar1(3)], correlated=[(1, 2)])
    assert kw["structured"] == [g.ar1(3)] and kw["correlated"] == [g.Pair(1, 2, 2.0)] and kw["prior_mu"].size == 1 + 16 + 4 + 1 + 1
    for bad in (dict(gmrf=[g.gmrf(1, np.eye(4))], correlated=[(1, 2)]), dict(gmrf=[g.gmrf(3, np.eye(3))], structured=[g.rw1(3)]),
                dict(gmrf=[g.gmrf(0, np.eye(4))]), dict(gmrf=[g.gmrf(0, np.eye(5))] * 2), dict(gmrf=[(0, np.eye(5))])):
        with pytest.raises(ValueError):
            g.gmrf_effects(1, [5, 4, 4, 3], **bad)


def test_constructor_validates_gmrfs(idhmc):
    g = idhmc.glm
    X, Y = _data()
    fac = [(REGION, 5), SUBJECT, g.term(SUBJECT, values=DOSE), (np.zeros(7, int), 2)]
    Q5, Q4 = g.icar_precision(MAP5, 5), g.rw1_precision(4)

    def bad(what, gmrf, factors=fac, **kw):
        with pytest.raises(ValueError, match=what):
            idhmc.GLM(X, Y, g.POISSON_LOG, factors=factors, gmrf=gmrf, **kw)
    bad("gmrf must be a list of glm.gmrf", g.gmrf(0, Q5))
    bad("gmrf must be a list of glm.gmrf", 3)
    bad(r"gmrf\[0\] must be a glm.gmrf", [(0, Q5)])
    bad("at most 2 GMRF terms", [g.gmrf(0, Q5), g.gmrf(1, Q4), g.gmrf(2, Q4)])
    bad("GMRF terms need factor terms", [g.gmrf(0, Q5)], factors=None)
    for t in (4, -1, 0.5, True):
        bad(r"gmrf\[0\]: term = .* is outside 0..3", [g.gmrf(t, Q5)])
    bad(r"gmrf\[1\]: term 0 is listed twice", [g.gmrf(0, Q5), g.gmrf(0, Q5)])
    bad(r"gmrf\[0\]: Q has 4 rows and term 0 has 5 levels", [g.gmrf(0, Q4)])
    bad(r"gmrf\[0\]: term 2 is in correlated\[0\]", [g.gmrf(2, Q4)], correlated=[g.pair(1, 2)])
    bad(r"gmrf\[1\]: term 1 is structured\[0\]", [g.gmrf(0, Q5), g.gmrf(1, Q4)], structured=[g.rw1(1)])
    loc = np.zeros(2 + 5 + 4 + 4 + 2, np.int32)
    loc[4] = 1
    bad(r"gmrf\[0\]: local\[4\] is set on level 2 of term 0", [g.gmrf(0, Q5)], local=loc)
    idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, gmrf=[g.gmrf(1, Q4)], local=loc)                 # a local scale on another term's column
    D = 17
    for name, val in (("prior_mu", 0.1), ("prior_tau", 2.0)):
        arr = np.zeros(D) if name == "prior_mu" else np.ones(D)
        arr[3] = val
        bad(r"gmrf\[0\]: %s\[3\] must be the default" % name, [g.gmrf(0, Q5)], **{name: arr})
        idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, gmrf=[g.gmrf(1, Q4)], **{name: arr})
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[6], nu[6] = STUDENT_T, 3.0
    bad(r"gmrf\[0\]: prior_kind\[6\] must be the default", [g.gmrf(0, Q5)], prior_kind=kind, prior_nu=nu)
    idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, gmrf=[g.gmrf(1, Q4)], prior_kind=kind, prior_nu=nu)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def _gmrfs_struct(G, term, start, col, val, kappa):
    from inplacedhmc_jl_amd import _lib
    keep = [None if a is None else np.ascontiguousarray(a, dtype=t)
            for a, t in ((term, np.int32), (start, np.int64), (col, np.int32), (val, np.float64), (kappa, np.float64))]
    gm = _lib.GlmGmrfs(G=G)
    for name, a, ct in zip(("term", "start", "col", "val", "kappa"), keep, (C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_double)):
        if a is not None:
            setattr(gm, name, a.ctypes.data_as(C.POINTER(ct)))
    return gm, keep


def _create(idhmc, desc, factors, values, pairs, structs, gmrfs, priors=None, local=None, M=1, R=0, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.idhmc_create_glm_gmrf(C.byref(h), 0, nchains, 0, C.byref(desc), ref(priors), ref(local), ref(factors), ref(values), ref(pairs),
                                   ref(structs), ref(gmrfs), M, R, None, 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def _c_model(idhmc, gmrf="default", correlated=None, structured=None):
    g = idhmc.glm
    X, Y = _data()
    gm = [g.gmrf(0, g.icar_precision(MAP5, 5), 1.0)] if gmrf == "default" else gmrf
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[(REGION, 5), SUBJECT, g.term(SUBJECT, values=DOSE)], gmrf=gm, correlated=correlated,
                     structured=structured, groups=[-1, -1] + [0] * 5 + [1] * 4 + [-1] * 4)


def test_good_gmrfs_pass_every_check(idhmc):
    """a valid descriptor reaches the device (or its absence): with one and two GMRF terms, with gmrfs = NULL, with G = 0 and its arrays
    NULL, and next to a structure and a pair on other terms"""
    ok = (0, idhmc.ERR_NO_DEVICE)
    g = idhmc.glm
    m = _c_model(idhmc)
    fc, k1 = _factors_struct(3, m.levels, m.factor_index)
    fv, k2 = _values_struct(m.factor_values, m.factor_has)
    gm, k3 = _gmrfs_struct(1, m.gmrf_term, m.gmrf_start, m.gmrf_col, m.gmrf_val, m.gmrf_kappa)
    rc, msg = _create(idhmc, m.glm_desc(), fc, fv, None, None, gm)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    m0 = _c_model(idhmc, None)
    for gmrfs in (None, _gmrfs_struct(0, None, None, None, None, None)[0]):
        rc, msg = _create(idhmc, m0.glm_desc(), fc, fv, None, None, gmrfs)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    m2 = _c_model(idhmc, [g.gmrf(2, g.seasonal_precision(4, 2)), g.gmrf(0, g.rw2_precision(5), 0.5)])
    gm, k3 = _gmrfs_struct(2, m2.gmrf_term, m2.gmrf_start, m2.gmrf_col, m2.gmrf_val, m2.gmrf_kappa)
    rc, msg = _create(idhmc, m2.glm_desc(), fc, fv, None, None, gm)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    m3 = _c_model(idhmc, structured=[g.ar1(1)])
    st, k4 = _structs_struct(1, m3.struct_term, m3.struct_kind, m3.struct_eta)
    gm, k3 = _gmrfs_struct(1, m3.gmrf_term, m3.gmrf_start, m3.gmrf_col, m3.gmrf_val, m3.gmrf_kappa)
    rc, msg = _create(idhmc, m3.glm_desc(), fc, fv, None, st, gm)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)


def test_bad_gmrfs_are_refused_before_the_device(idhmc):
    g = idhmc.glm
    m = _c_model(idhmc)
    lib = idhmc.load_library()
    D = m.D                                                        # 2 + 13 + 2 = 17
    assert D == 17
    ip, ix, dt = csr(g.icar_precision(MAP5, 5))

    def refused(what, G=1, term=(0,), start=ip, col=ix, val=dt, kappa=(1.0,), F=3, levels=(5, 4, 4), factors=True, desc=None, priors=None,
                pairs=None, structs=None, **kw):
        fc, k1 = _factors_struct(F, levels, m.factor_index)
        fv, k2 = _values_struct(m.factor_values, m.factor_has)
        gm, k3 = _gmrfs_struct(G, term, start, col, val, kappa)
        pp, k5 = (None, None) if pairs is None else _pairs_struct(*pairs)
        st, k6 = (None, None) if structs is None else _structs_struct(*structs)
        pr, k4 = (None, None) if priors is None else _priors_struct(*priors)
        rc, msg = _create(idhmc, m.glm_desc() if desc is None else desc, fc if factors else None, fv if factors and F else None, pp, st, gm, pr, **kw)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    h = C.c_void_p()
    assert lib.idhmc_create_glm_gmrf(C.byref(h), 0, 4, 0, None, None, None, None, None, None, None, None, 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert b"idhmc_create_glm_gmrf: null argument" in lib.idhmc_last_error()
    assert lib.idhmc_create_glm_gmrf(None, 0, 4, 0, C.byref(m.glm_desc()), None, None, None, None, None, None, None, 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert lib.idhmc_glm_gmrfs_get(None, None, None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    for G in (-1, 3, 1 << 20):
        refused(b"G = %d GMRF terms must be an integer in 0..2" % G, G=G)
    for name in ("term", "start", "col", "val", "kappa"):
        refused(b"need term, start, col, val and kappa (%s is NULL)" % name.encode(), **{name: None})
    for t in (-1, 3):
        refused(b"GMRF 0: term = %d is outside 0..2" % t, term=(t,))
    refused(b"GMRF 1: term 0 is listed twice", G=2, term=(0, 0), start=np.r_[ip, ip[-1] + ip[1:]], col=np.r_[ix, ix], val=np.r_[dt, dt], kappa=(1.0, 0.0))
    for k in (-1.0, np.inf, np.nan):
        refused(b"GMRF 0: kappa = ", kappa=(k,))
    refused(b"GMRF 0: term 1 is in pair 0", term=(1,), pairs=(1, [1], [2], [0.0]), desc=_c_model(idhmc, None, [g.pair(1, 2, 0.0)]).glm_desc())
    refused(b"GMRF 0: term 0 is structure 0", structs=(1, [0], [RW1], [0.0]))
    loc = np.zeros(15, np.int32)
    loc[2 + 3] = 1
    lc, k7 = _local_struct(loc)
    refused(b"GMRF 0: local[5] is set on level 3 of term 0", local=lc)
    # a non-default prior entry on a member
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[4], nu[4] = STUDENT_T, 3.0
    refused(b"GMRF 0: the entry of coordinate 4 (level 2 of term 0) in the prior arrays must be the default", priors=(kind, nu))
    for name, val_ in (("mu", 0.5), ("tau", 2.0)):
        arr = np.zeros(D) if name == "mu" else np.ones(D)
        arr[6] = val_
        d = m.glm_desc()
        setattr(d, name, arr.ctypes.data_as(C.POINTER(C.c_double)))
        refused(b"GMRF 0: the entry of coordinate 6 (level 4 of term 0)", desc=d)
    # the table
    refused(b"GMRF start[0] = 1 must be 0", start=ip + 1)
    s2 = ip.copy()
    s2[2] = s2[1] - 1
    refused(b"start must not decrease", start=s2)
    s2 = ip.copy()
    s2[1] = 0
    refused(b"GMRF 0: row 0 has 0 entries", start=s2)
    N = 130
    big = csr(np.ones((N, N)) + N * np.eye(N))
    m130 = idhmc.GLM(*_data(), g.POISSON_LOG, factors=[(REGION, N)])
    fc130, k8 = _factors_struct(1, m130.levels, m130.factor_index)
    rc, msg = _create(idhmc, m130.glm_desc(), fc130, None, None, None, _gmrfs_struct(1, [0], *big, [0.0])[0])
    assert rc == idhmc.ERR_BAD_ARG and b"GMRF 0: row 0 has 130 entries" in msg, (rc, msg)
    c2 = ix.copy()
    c2[0], c2[1] = c2[1], c2[0]
    refused(b"columns strictly ascending", col=c2)
    for cbad in (5, -1):
        c2 = ix.copy()
        c2[ip[4]] = cbad
        refused(b"GMRF 0: row 4: col[%d] = %d is outside 0..4" % (ip[4], cbad), col=c2)
    # a missing diagonal (row 4 is [3, 4]: drop the 4), a non-positive one, a non-finite value
    refused(b"GMRF 0: row 4 has no diagonal entry", start=np.r_[ip[:-1], ip[-1] - 1], col=ix[:-1], val=dt[:-1])
    v2 = dt.copy()
    v2[0] = 0.0
    refused(b"GMRF 0: row 0: the diagonal val[0] = 0 must be > 0", val=v2)
    for x in (np.nan, np.inf):
        v2 = dt.copy()
        v2[1] = x
        refused(b"GMRF 0: row 0: val[1] = ", val=v2)
    # symmetry: Q_01 nudged by one ulp; Q_34 absent while Q_43 is given
    v2 = dt.copy()
    v2[1] = np.nextafter(v2[1], 0.0)
    refused(b"are not bit-equal (Q must be symmetric)", val=v2)
    drop = ip[3] + 2                                               # row 3 is [2, 3, 4]
    assert ix[drop] == 4
    refused(b"GMRF 0: Q[4][3] is given and Q[3][4] is absent", start=np.r_[ip[:4], ip[4:] - 1], col=np.delete(ix, drop), val=np.delete(dt, drop))
    # GMRFs without factors
    X, Y = _data()
    m0 = idhmc.GLM(X, Y, g.POISSON_LOG, groups=[0, -1])
    refused(b"GMRF terms need factor terms (factors is NULL)", factors=False, desc=m0.glm_desc())
    refused(b"GMRF terms need factor terms (factors is given with F = 0)", F=0, desc=m0.glm_desc())
    # everything idhmc_create_glm_struct refuses
    refused(b"F = 5 factors must be an integer in 0..4", F=5)
    refused(b"levels[1] = 0: at least one level", levels=(5, 0, 4))
    refused(b"P = 3 pairs must be an integer in 0..2", pairs=(3, [0], [1], [2.0]))
    refused(b"S = 3 structured terms must be an integer in 0..2", structs=(3, [1], [AR1], [2.0]))
    d = m.glm_desc()
    d.H = 3
    refused(b"group 2 has no column", desc=d)
    refused(b"chains_per_response = 0", M=2, R=0)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def gmrf_columns(structs_like, Qs):
    """[(off, N, Q, kappa)] from [(off, N, anything)] and [(Q, kappa)]"""
    return [(o, N, Q, k) for (o, N, _), (Q, k) in zip(structs_like, Qs)]


@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    work = {}

    def model(family, Xe, Y, grp, local, S, kind, nu, pairs, eta, structs, seta, gmrfs, mu=None, tau=None):
        if family not in work:
            work[family] = str(tmp_path_factory.mktemp("gmrf_" + family.lower()))
        A, H, J = SHAPE[family][2], int(np.max(grp)) + 1, 0 if local is None else int(np.sum(local))
        D = Xe.shape[1] + A + H + J + len(pairs) + sum(1 for s in structs if s[2] == AR1)
        return oracle.OracleModel.custom(D, c_source_gmrf(family), oracle_params_gmrf(Xe, Y, A, grp, local, S, kind, nu, pairs, eta, structs, seta,
                                                                                     gmrfs, consts(family), mu, tau), work[family])
    return model


def gmrf_priors(D, Z, etas, seed, gmrfs):
    """test_glm_struct_cpu.case_priors with the defaults on the members of the GMRF terms"""
    kind, nu, mu, tau = ST.case_priors(D, Z, etas, seed)
    for o, N, Q, k in gmrfs:
        kind[o:o + N], nu[o:o + N], mu[o:o + N], tau[o:o + N] = NORMAL, 0.0, 0.0, 1.0
    return kind, nu, mu, tau


def case_setup(idhmc, case):
    """(family, n, Dd, N, which Q, kappa, valued, second = (N2, Q2 name, kappa2) or None, AR(1) and a pair on further terms)"""
    family, n, Dd, N, qn, kappa, valued, second, rest = case
    g = idhmc.glm
    build = {"icar": lambda M: g.icar_precision(grid_edges(M // 5, 5), M), "rw2": g.rw2_precision, "seasonal": lambda M: g.seasonal_precision(M, 4),
             "complete": lambda M: M * np.eye(M) - np.ones((M, M)) + np.eye(M), "scaled": lambda M: g.scale_precision(g.rw1_precision(M)),
             "identity": np.eye}
    if rest:
        X, Y, factors, Xe, grp, pairs, structs = ST.small_problem(idhmc, family, n, Dd, N, AR1, valued, True, (6, AR1), True)
        gm = [(structs[0][0], N, build[qn](N), kappa)]             # the first term is the GMRF one, the second stays AR(1)
        structs = structs[1:]
    else:
        X, Y, factors, Xe, grp, pairs, structs = ST.small_problem(idhmc, family, n, Dd, N, RW1, valued, True, None if second is None else (second[0], RW1), False)
        gm = [(structs[0][0], N, build[qn](N), kappa)]
        if second is not None:
            gm.append((structs[1][0], second[0], build[second[1]](second[0]), second[2]))
        structs = []
    Dx, A, H, P = Xe.shape[1], SHAPE[family][2], int(grp.max()) + 1, len(pairs)
    seta, eta = [2.0] * len(structs), [2.0][:P]
    Z = P + len(structs)
    D = Dx + A + H + Z
    kind, nu, mu, tau = gmrf_priors(D, Z, eta + seta, n, gm)
    return family, X, Y, factors, Xe, grp, pairs, eta, structs, seta, gm, (Dx, A, H, P, len(structs), D), (kind, nu, mu, tau)


CASES = [("POISSON_LOG", 37, 1, 30, "icar", 0.0, False, None, False), ("POISSON_LOG", 37, 3, 150, "rw2", 0.0, False, None, False),
         ("POISSON_LOG", 40, 2, 12, "seasonal", 0.0, False, (10, "icar", 2.0), False),
         ("GAUSSIAN_IDENTITY_LOGSIGMA", 50, 4, 128, "complete", 0.5, True, None, False),
         ("POISSON_LOG", 60, 8, 15, "scaled", 1.5, True, None, True)]


@pytest.mark.parametrize("case", CASES, ids=["%s-n%d-Dd%d-N%d-%s" % c[:5] for c in CASES])
def test_restatement_matches_numpy(idhmc, restated, case):
    family, X, Y, factors, Xe, grp, pairs, eta, structs, seta, gm, (Dx, A, H, P, Sz, D), (kind, nu, mu, tau) = case_setup(idhmc, case)
    om = restated(family, Xe, Y, grp, None, None, kind, nu, pairs, eta, structs, seta, gm, mu, tau)
    for k in range(3):
        q = ST.start_struct(family, 1, Dx, H, 0, P, Sz, seed=k)[0]
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_gmrf(family, Xe, Y, q, grp, np.zeros(Dx, int), None, kind, nu, pairs, eta, structs, seta, gm, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), np.max(np.abs(g[:D] - g_ref) / gscale)


def test_numpy_gradient_is_mpmath_derivative_of_the_model(idhmc):
    """Poisson with a log link, Dd = 2, an ICAR effect over the 5-region map with values, a sampled scale and kappa = 0.75, and a seasonal
    effect of 6 levels (period 3, kappa = 0): the log density written in mpmath straight from -1/2 u'Qu - 1/2 kappa (1'u)^2,
    differentiated numerically at 40 digits; numpy's l and gradient within 1e-12 of their terms' magnitude"""
    import mpmath as mp
    mp.mp.dps = 40
    g_ = idhmc.glm
    rng = np.random.default_rng(4)
    n, Dd, N, N2, kappa = 14, 2, 5, 6, 0.75
    X = 0.5 * rng.standard_normal((n, Dd))
    t, w, t2 = rng.integers(0, N, n), rng.standard_normal(n), rng.integers(0, N2, n)
    Y = rng.poisson(1.5, n).astype(float)
    Dx = Dd + N + N2
    D = Dx + 2
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    mu[Dd:Dx], tau[Dd:Dx] = 0.0, 1.0
    Xe = np.zeros((n, Dx))
    Xe[:, :Dd] = X
    Xe[np.arange(n), Dd + t] = w
    Xe[np.arange(n), Dd + N + t2] = 1.0
    grp = np.r_[[-1] * Dd, [0] * N, [1] * N2]
    Q1, Q2 = g_.icar_precision(MAP5, N), g_.seasonal_precision(N2, 3)
    gm = [(Dd, N, Q1, kappa), (Dd + N, N2, Q2, 0.0)]

    def logp(*q):
        u, om = q[:Dx], q[Dx:Dx + 2]
        s0, s1 = mp.exp(om[0]), mp.exp(om[1])
        total = mp.mpf(0)
        for i in range(n):
            z = sum(mp.mpf(float(X[i, j])) * u[j] for j in range(Dd)) + mp.mpf(float(w[i])) * s0 * u[Dd + t[i]] + s1 * u[Dd + N + t2[i]]
            total += mp.mpf(float(Y[i])) * z - mp.exp(z)
        for j in list(range(Dd)) + [Dx, Dx + 1]:
            total -= mp.mpf(float(tau[j])) * (q[j] - mp.mpf(float(mu[j]))) ** 2 / 2
        for o, M, Q, k in gm:
            for a in range(M):
                for b in range(M):
                    total -= mp.mpf(float(Q[a, b])) * u[o + a] * u[o + b] / 2
            total -= mp.mpf(k) * sum(u[o:o + M]) ** 2 / 2
        return total

    for seed in range(2):
        q = np.r_[np.random.default_rng(seed).uniform(-0.8, 0.8, Dx), np.log(0.6) + rng.uniform(-0.3, 0.3, 2)]
        l, g, ls, gs = numpy_density_gmrf("POISSON_LOG", Xe, Y, q, grp, np.zeros(Dx, int), None, np.zeros(D, int), np.zeros(D), [], [], [], [], gm, mu, tau)
        qm = [mp.mpf(float(x)) for x in q]
        assert abs(float(logp(*qm) - mp.mpf(l))) <= 1e-12 * ls
        for j in range(D):
            order = tuple(1 if i == j else 0 for i in range(D))
            ref = mp.diff(logp, tuple(qm), order)
            assert abs(float(ref - mp.mpf(float(g[j])))) <= 1e-12 * gs[j] + 1e-300, (seed, j, float(ref), g[j])


@pytest.mark.parametrize("Dd,N,L", [(3, 20, 128), (100, 300, 512)], ids=["L128", "L512"])
def test_identity_precision_gives_the_bits_of_the_normal_row(idhmc, restated, oracle, tmp_path, Dd, N, L):
    """The anchor: Q = I and kappa = 0 on a term, for random starts without a zero among them, give l and every component of the gradient
    of test_glm_struct_cpu's restatement of the same model without the feature (kind 0, mu 0, tau 1 on those columns), bit for bit"""
    family = "POISSON_LOG"
    X, Y, factors, Xe, grp, pairs, structs = ST.small_problem(idhmc, family, 37, Dd, N, RW1)
    Dx, H = Xe.shape[1], 2
    D = Dx + H
    assert 128 * (1 << int(np.ceil(np.log2((D + 127) // 128)))) == L
    gm = [(structs[0][0], N, np.eye(N), 0.0)]
    kind, nu, mu, tau = gmrf_priors(D, 0, [], 3, gm)
    om = restated(family, Xe, Y, grp, None, None, kind, nu, [], [], [], [], gm, mu, tau)
    base = oracle.OracleModel.custom(D, ST.c_source_struct(family), ST.oracle_params_struct(Xe, Y, 0, grp, None, None, kind, nu, [], [], [], [],
                                                                                           consts(family), mu, tau), str(tmp_path))
    for k in range(3):
        q = ST.start_struct(family, 1, Dx, H, 0, 0, 0, seed=k)[0]
        assert (q != 0.0).all()
        l1, g1 = om.logdensity_and_gradient(q)
        l0, g0 = base.logdensity_and_gradient(q)
        assert l1 == l0 and np.array_equal(np.asarray(g1[:D]).view(np.uint64), np.asarray(g0[:D]).view(np.uint64)) and np.isfinite(l1)


def test_kappa_adds_exactly_its_own_term(idhmc, restated):
    """Q = eps I with kappa going from 0 to a power of two, on a problem whose every operation is exact (dyadic data, coordinates and
    constants; a Gaussian likelihood at log sigma = 0): l changes by exactly -1/2 kappa S^2 and the members' gradient by exactly
    -kappa S, S the members' sum -- kappa S enters each member's s ahead of the entries (s = kappa S, then the dfma chain), once per
    member through T = dfma(u, s, T), and nowhere else"""
    family = "GAUSSIAN_IDENTITY_LOGSIGMA"
    rng = np.random.default_rng(2)
    n, Dd, N = 20, 2, 9
    X = rng.integers(-4, 5, (n, Dd)) / 4.0
    t = rng.integers(0, N, n)
    Y = rng.integers(-8, 9, n) / 4.0
    factors = [(t, N)]
    Xe = idhmc.glm.expand_factors(X, factors)
    Dx = Dd + N
    D = Dx + 1
    grp = np.full(Dx, -1, np.int32)
    q = np.r_[rng.integers(-8, 9, Dx) / 8.0, 0.0]
    q[q == 0.0] = 0.125
    q[-1] = 0.0                                                    # log sigma = 0: w = 1 exactly
    eps = 0.25
    S = float(q[Dd:Dx].sum())
    assert S != 0.0
    out = {}
    for kappa in (0.0, 4.0):
        gm = [(Dd, N, eps * np.eye(N), kappa)]
        om = restated(family, Xe, Y, grp, None, None, np.zeros(D, int), np.zeros(D), [], [], [], [], gm, np.zeros(D), np.ones(D))
        out[kappa] = om.logdensity_and_gradient(q)
    (l0, g0), (l1, g1) = out[0.0], out[4.0]
    assert l1 - l0 == -0.5 * 4.0 * S * S and l1 != l0
    assert np.array_equal(np.asarray(g1[Dd:Dx]) - np.asarray(g0[Dd:Dx]), np.full(N, -4.0 * S))
    assert np.array_equal(np.r_[g1[:Dd], g1[Dx:D]], np.r_[g0[:Dd], g0[Dx:D]])
    ref = numpy_density_gmrf(family, Xe, Y, q, grp, np.zeros(Dx, int), None, np.zeros(D, int), np.zeros(D), [], [], [], [], gm)
    assert l1 == ref[0] and np.array_equal(np.asarray(g1[:D]), ref[1])          # exact arithmetic: numpy's value too
