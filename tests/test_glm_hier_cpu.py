"""Hierarchical GLMs (GLM(..., groups=...), idhmc_create_glm) without a GPU: the constructor's validation and
packing, the C boundary's argument checks, and the C restatement of section 13's definition (section 12's with the non-centred
hierarchy: b = s * u in front of z = X b, the chain rule behind G, one canonical tree per group) against a numpy closed form,
central differences in every omega, every a and a spread of u, and the identity "omega held fixed is an ungrouped GLM on X diag(s)".

The restatement's params are [n, K, nc, A, H, mu (D), tau (D), c (nc), grp (Dx, as doubles), X row-major (n x Dx), Y row-major
(n x K)], D = Dx + A + H.  Its observation is the one of tests/test_glm_cpu.py (A = 0, behind a wrapper that ignores a and s) or of
tests/test_glm_aux_cpu.py (A > 0).  The GPU tests (tests/test_gpu_glm_hier.py) hand the same source to the oracle."""
import ctypes as C

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
import test_glm_cpu as FLAT

C_BODY_HIER = r"""
#include "orc_math.h"
%s
/* params: [n, K, nc, A, H, mu (D), tau (D), c (nc), grp (Dx, as doubles), X row-major (n x Dx), Y row-major (n x K)] */
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    const long n = (long)params[0];
    const int K = (int)params[1], nc = (int)params[2], A = (int)params[3], H = (int)params[4], Dx = D - A - H;
    const double *mu = params + 5, *tau = mu + D, *c = tau + D, *grp = c + nc, *X = grp + Dx, *Y = X + n * Dx;
    const double *a = q + Dx, *om = q + Dx + A;
    double e[4] = {0, 0, 0, 0}, b[1024], T[128], V[128], S[4][128], W[4][128];
    for (int g = 0; g < H; ++g) e[g] = orc_exp(om[g]);
    for (int j = 0; j < Dx; ++j) b[j] = grp[j] >= 0.0 ? q[j] * e[(int)grp[j]] : q[j];
    for (int r = 0; r < 128; ++r) { T[r] = 0.0; V[r] = 0.0; for (int j = 0; j < 4; ++j) S[j][r] = W[j][r] = 0.0; }
    for (int j = 0; j < L; ++j) grad[j] = 0.0;
    for (long i = 0; i < n; ++i) {
        const double *xi = X + i * Dx;
        double z = 0.0;
        for (int j = 0; j < Dx; ++j) z = fma(xi[j], b[j], z);
        double y[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < K; ++k) y[k] = Y[i * K + k];
        double r, v, s[4] = {0.0, 0.0, 0.0, 0.0};
        glm_observation(z, y, c, a, &r, &v, s);
        V[i & 127] = V[i & 127] + v;
        for (int j = 0; j < A; ++j) S[j][i & 127] = S[j][i & 127] + s[j];
        for (int j = 0; j < Dx; ++j) grad[j] = fma(xi[j], r, grad[j]);
    }
    for (int j = 0; j < A; ++j) grad[Dx + j] = orc_tree128(S[j]);
    for (int j = 0; j < Dx; ++j)
        if (grp[j] >= 0.0) {
            const int g = (int)grp[j];
            W[g][j & 127] = W[g][j & 127] + grad[j] * b[j];
            grad[j] = grad[j] * e[g];
        }
    for (int g = 0; g < H; ++g) grad[Dx + A + g] = orc_tree128(W[g]);
    for (int j = 0; j < D; ++j) {
        const double d = q[j] - mu[j];
        T[j & 127] = fma(tau[j] * d, d, T[j & 127]);
        grad[j] = fma(-tau[j], d, grad[j]);
    }
    for (int r = 0; r < 128; ++r) T[r] = fma(2.0, V[r], T[r]);
    return -0.5 * orc_tree128(T);
}
"""
# an observation without auxiliary coordinates behind the seven-argument call: a and s unused
WRAP_A0 = r"""
static void glm_observation(double z, const double *y, const double *c, const double *a, double *r, double *v, double *s)
{
    (void)a; (void)s;
    glm_observation0(z, y, c, r, v);
}"""
# Gaussian with KNOWN sigma = c[0] (test-only, section 11's form): the statistical test's likelihood
GAUSSIAN_KNOWN_SOURCE = r"""
__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)
{
    const double u = (o.y[0] - z) / o.c[0];
    v = 0.5 * (u * u);
    r = u / o.c[0];
}
"""
GAUSSIAN_KNOWN_C = r"""
static void glm_observation0(double z, const double *y, const double *c, double *r, double *v)
{
    const double u = (y[0] - z) / c[0];
    *v = 0.5 * (u * u);
    *r = u / c[0];
}"""
FAMILIES = ["BERNOULLI_LOGIT", "POISSON_LOG", "GAUSSIAN_IDENTITY_LOGSIGMA"]
SHAPE = {"BERNOULLI_LOGIT": (1, 0, 0), "POISSON_LOG": (1, 0, 0), "GAUSSIAN_IDENTITY_LOGSIGMA": (1, 0, 1), "TEST_A4": (2, 0, 4),
         "GAUSSIAN_KNOWN": (1, 1, 0)}                  # K, nc, A
OMEGA0 = np.log(0.6)


def source(idhmc, family):
    if family == "GAUSSIAN_KNOWN":
        return GAUSSIAN_KNOWN_SOURCE
    return AUX.TEST_A4_SOURCE if family == "TEST_A4" else getattr(idhmc.glm, family)


def c_source_hier(family):
    if family == "GAUSSIAN_KNOWN":
        return C_BODY_HIER % (GAUSSIAN_KNOWN_C + WRAP_A0)
    if SHAPE[family][2] == 0:
        return C_BODY_HIER % (FLAT.OBS_C[family].replace("glm_observation(", "glm_observation0(") + WRAP_A0)
    return C_BODY_HIER % AUX.OBS_C_AUX[family]


def interleaved(Dx, H):
    """grp[c] = c % (H + 1) - 1: neighbouring columns, and the two coordinates of a lane, in different groups"""
    return (np.arange(Dx) % (H + 1) - 1).astype(np.int32)


def blocks(Dx, H, levels):
    """the last H * levels columns are H contiguous blocks; the columns in front are in no group"""
    g = np.full(Dx, -1, np.int32)
    for k in range(H):
        g[Dx - (H - k) * levels:Dx - (H - k - 1) * levels] = k
    return g


def oracle_params_hier(X, Y, A, grp, c=None, mu=None, tau=None):
    n, Dx = X.shape
    grp = np.full(Dx, -1) if grp is None else np.asarray(grp)
    H = int(grp.max()) + 1
    D = Dx + A + H
    Y = np.asarray(Y, float).reshape(n, -1)
    c = np.zeros(0) if c is None else np.asarray(c, float)
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    return np.concatenate([[float(n), float(Y.shape[1]), float(c.size), float(A), float(H)], mu, tau, c, grp.astype(float),
                           np.asarray(X, float).ravel(), Y.ravel()])


def design(n, Dx, grp, one_hot, rng, scale=0.5):
    """a first column of ones, dense columns, and for one_hot a one-hot block per group (every observation has one level of each)"""
    X = rng.standard_normal((n, Dx)) * scale
    X[:, 0] = 1.0
    if one_hot:
        for g in range(int(grp.max()) + 1):
            cols = np.flatnonzero(grp == g)
            X[:, cols] = 0.0
            X[np.arange(n), cols[rng.integers(0, cols.size, n)]] = 1.0
    return X


def problem_hier(family, n, Dx, grp, one_hot, seed=3):
    """data from the family's own model: u ~ N(0, 1) in the groups (scale 0.6), N(0, 1 / Dx) elsewhere"""
    rng = np.random.default_rng(seed)
    X = design(n, Dx, grp, one_hot, rng)
    beta = np.where(grp >= 0, 0.6 * rng.standard_normal(Dx) / (1.0 if one_hot else np.sqrt(Dx)), rng.standard_normal(Dx) / np.sqrt(Dx))
    z = X @ beta
    if family == "BERNOULLI_LOGIT":
        Y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-z))).astype(float)
    elif family == "POISSON_LOG":
        Y = rng.poisson(np.exp(z)).astype(float)
    elif family == "GAUSSIAN_IDENTITY_LOGSIGMA":
        Y = z + np.exp(AUX.TRUE_A[family][0]) * rng.standard_normal(n)
    elif family == "GAUSSIAN_KNOWN":
        Y = z + 0.5 * rng.standard_normal(n)
    else:
        a = AUX.TRUE_A["TEST_A4"]
        y1 = rng.uniform(-1.0, 1.0, n)
        Y = np.stack([z + a[1] * y1 + a[2] + np.exp(a[0] + a[3] * y1) * rng.standard_normal(n), y1], 1)
    return X, Y


def consts(family):
    return np.array([0.5]) if family == "GAUSSIAN_KNOWN" else None


def start_hier(family, C, Dx, H, seed=0, scale=0.3):
    """u ~ U(-scale, scale), a around the data's own, omega ~ log 0.6 + U(-0.3, 0.3)"""
    rng = np.random.default_rng(seed + Dx)
    A = SHAPE[family][2]
    a = np.asarray(AUX.TRUE_A[family]) if A else np.zeros(0)
    return np.concatenate([rng.uniform(-scale, scale, (C, Dx)), a + rng.uniform(-0.2, 0.2, (C, A)),
                           OMEGA0 + rng.uniform(-0.3, 0.3, (C, H))], 1)


def numpy_density_hier(family, X, Y, q, grp, mu=None, tau=None):
    """(l(q), grad l(q), magnitude of l's terms, per-coordinate magnitude of the terms summed into grad), q = [u | a | omega]"""
    n, Dx = X.shape
    A = SHAPE[family][2]
    H = int(np.max(grp)) + 1
    D = Dx + A + H
    assert q.size == D
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    u, a, om = q[:Dx], q[Dx:Dx + A], q[Dx + A:]
    s = np.where(grp >= 0, np.exp(om)[np.maximum(grp, 0)], 1.0)
    b = s * u
    z = X @ b
    if family == "GAUSSIAN_KNOWN":
        w = (np.asarray(Y, float).reshape(-1) - z) / 0.5
        lp, r, mag, sc, smag = -0.5 * w * w, w / 0.5, 0.5 * w * w, np.zeros((n, 0)), np.zeros((n, 0))
    elif A == 0:
        lp, r, mag = FLAT.numpy_terms(family, z, Y)
        sc, smag = np.zeros((n, 0)), np.zeros((n, 0))
    else:
        lp, r, sc, mag, smag = AUX.numpy_terms_aux(family, z, Y, a)
    G, Gmag = X.T @ r, np.abs(X).T @ np.abs(r)
    d = q - mu
    member = [grp == g for g in range(H)]
    g = np.concatenate([s * G, sc.sum(0), [np.sum(G[m] * b[m]) for m in member]]) - tau * d
    gscale = np.concatenate([s * Gmag, smag.sum(0), [np.sum(Gmag[m] * np.abs(b[m])) for m in member]]) + np.abs(tau * d)
    return np.sum(lp) - 0.5 * np.sum(tau * d * d), g, np.sum(mag) + 0.5 * np.sum(tau * d * d), gscale


def make(idhmc, family, X, Y, grp, mu=None, tau=None):
    return idhmc.GLM(X, Y, source(idhmc, family), consts(family), mu, tau, aux=SHAPE[family][2], groups=grp)


# ---- the constructor ---------------------------------------------------------------------------------------------------------------
def test_constructor_keeps_the_parts(idhmc):
    grp = np.array([-1, 0, 1, 0, -1, 1])
    X, Y = problem_hier("GAUSSIAN_IDENTITY_LOGSIGMA", 9, 6, grp, False)
    m = idhmc.GLM(X, Y, idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, prior_mu=0.5, prior_tau=np.arange(1.0, 10.0), aux=1, groups=list(grp))
    assert m.kind == idhmc.MODEL_GLM_AUX and m.D == 9 and (m.Dx, m.A, m.H, m.n, m.K, m.nc) == (6, 1, 2, 9, 1, 0)
    assert m.groups.dtype == np.int32 and np.array_equal(m.groups, grp)
    assert np.array_equal(m.mu, np.full(9, 0.5)) and np.array_equal(m.tau, np.arange(1.0, 10.0))
    d = m.glm_desc()
    assert (d.n, d.Dx, d.K, d.nc, d.A, d.H) == (9, 6, 1, 0, 1, 2) and d.source == idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA.encode()
    assert [d.groups[c] for c in range(6)] == list(grp) and d.X[7] == X[1, 1] and d.Y[8] == Y[8] and d.tau[8] == 9.0 and not d.constants
    m = idhmc.GLM(X, Y > 0, idhmc.glm.BERNOULLI_LOGIT, groups=np.zeros(6, np.int64))       # A = 0, one group of every column
    assert m.kind == idhmc.MODEL_GLM and m.D == 7 and (m.Dx, m.A, m.H) == (6, 0, 1) and m.mu is None and m.tau is None


def test_without_groups_the_model_is_the_parents(idhmc):
    """groups=None (and an all -1 sequence) packs what GLM() always packed, byte for byte"""
    X, Y = AUX.problem_aux("TEST_A4", 9, 4)
    c = [1.5, -2.0, 0.25]
    want = np.concatenate([[2.0, 3.0], c, X.ravel(), Y.ravel()])
    for kw in ({}, {"groups": None}, {"groups": [-1, -1, -1, -1]}):
        m = idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, c, 0.5, 2.0, **kw)
        assert m.kind == idhmc.MODEL_GLM == 5 and m.D == 4 and (m.Dx, m.A, m.H) == (4, 0, 0) and m.groups is None
        assert m.params.dtype == np.float64 and m.params.tobytes() == want.tobytes()
        assert m.mu.tobytes() == np.full(4, 0.5).tobytes() and m.tau.tobytes() == np.full(4, 2.0).tobytes()
        d = m.desc()
        assert d.kind == 5 and d.D == 4 and d.nparams == want.size
    want = np.concatenate([[2.0, 0.0, 4.0], X.ravel(), Y.ravel()])
    m = idhmc.GLM(X, Y, AUX.TEST_A4_SOURCE, aux=4, groups=None)
    assert m.kind == idhmc.MODEL_GLM_AUX == 6 and m.D == 8 and m.H == 0 and m.params.tobytes() == want.tobytes()


def test_constructor_validates_groups(idhmc):
    X, Y = AUX.problem_aux("GAUSSIAN_IDENTITY_LOGSIGMA", 20, 5)
    src = idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA
    for bad, what in (([0, 0, 0, 0], "one entry per column"), ([0] * 6, "one entry per column"), ([[0] * 5], "one entry per column"),
                      (0, "one entry per column"), ([0.0, 0, 0, 0, 0], "integers"), ([True] * 5, "integers"), (["0"] * 5, "integers"),
                      ([-2, 0, 0, 0, 0], "-1"), ([0, 1, 2, 3, 4], "at most 4"), ([0, 2, 2, 0, -1], "group 1 has no column"),
                      ([1, 1, -1, -1, -1], "group 0 has no column")):
        with pytest.raises(ValueError, match=what):
            idhmc.GLM(X, Y, src, aux=1, groups=bad)
    assert idhmc.GLM(X, Y, src, aux=1, groups=[0, 1, 2, 3, -1]).H == 4
    with pytest.raises(ValueError, match="D <= 1024"):
        idhmc.GLM(np.zeros((4, 1020)), np.zeros(4), src, aux=1, groups=[0, 1, 2, 3] * 255)          # Dx + A + H = 1025
    assert idhmc.GLM(np.zeros((4, 1019)), np.zeros(4), src, aux=1, groups=[0, 1, 2, 3] * 254 + [0, 1, 2]).D == 1024
    for kw in ({"prior_mu": np.zeros(6)}, {"prior_tau": np.ones(6)}, {"prior_tau": np.r_[np.ones(7), 0.0]}, {"prior_mu": np.r_[np.zeros(7), np.nan]}):
        with pytest.raises(ValueError):
            idhmc.GLM(X, Y, src, aux=1, groups=[0, 0, 1, 1, -1], **kw)     # the prior has length Dx + A + H
    m = idhmc.GLM(X, Y, src, prior_mu=np.arange(8.0), prior_tau=np.arange(1.0, 9.0), aux=1, groups=[0, 0, 1, 1, -1])
    assert m.mu[7] == 7.0 and m.tau[7] == 8.0


def test_coefficients_and_group_scales(idhmc):
    grp = np.array([-1, 0, 1, 0, -1, 1])
    X, Y = problem_hier("GAUSSIAN_IDENTITY_LOGSIGMA", 9, 6, grp, False)
    m = make(idhmc, "GAUSSIAN_IDENTITY_LOGSIGMA", X, Y, grp)
    rng = np.random.default_rng(0)
    draws = rng.standard_normal((5, 3, 9))
    sg = idhmc.glm.group_scales(m, draws)
    assert sg.shape == (5, 3, 2) and np.array_equal(sg, np.exp(draws[..., 7:]))
    beta = idhmc.glm.coefficients(m, draws)
    assert beta.shape == (5, 3, 6)
    for c in range(6):
        want = draws[..., c] * (np.exp(draws[..., 7 + grp[c]]) if grp[c] >= 0 else 1.0)
        assert np.array_equal(beta[..., c], want)
    assert idhmc.glm.coefficients(m, draws[0, 0]).shape == (6,) and idhmc.glm.group_scales(m, draws[0, 0]).shape == (2,)
    with pytest.raises(ValueError):
        idhmc.glm.coefficients(m, draws[..., :8])
    flat = idhmc.GLM(X, Y, idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1)
    assert np.array_equal(idhmc.glm.coefficients(flat, draws[..., :7]), draws[..., :6]) and idhmc.glm.group_scales(flat, draws[..., :7]).shape == (5, 3, 0)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def _create_glm(idhmc, desc, opt=None):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create_glm(C.byref(h), 0, 4, 0, C.byref(desc), None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def test_a_valid_descriptor_passes_the_argument_checks(idhmc):
    for family in FAMILIES + ["TEST_A4", "GAUSSIAN_KNOWN"]:
        for grp in (interleaved(7, 1), interleaved(7, 4), blocks(7, 2, 3)):
            X, Y = problem_hier(family, 50, 7, grp, False)
            m = make(idhmc, family, X, Y, grp, 0.1, 0.5)                   # kept alive: the descriptor points into its arrays
            rc, msg = _create_glm(idhmc, m.glm_desc())
            # a context where a device exists; otherwise the constructor stops at its device check, past every argument check
            assert rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg), (family, rc, msg)
    # H = 0: the descriptor of a model without groups
    X, Y = FLAT.problem("POISSON_LOG", 30, 5)
    from inplacedhmc_jl_amd import _lib
    d = _lib.GlmDesc(n=30, Dx=5, K=1, nc=0, A=0, H=0, X=X.ctypes.data_as(C.POINTER(C.c_double)), Y=Y.ctypes.data_as(C.POINTER(C.c_double)),
                     source=idhmc.glm.POISSON_LOG.encode())
    assert _create_glm(idhmc, d)[0] in (0, idhmc.ERR_NO_DEVICE)


def test_bad_descriptors_are_refused_before_the_device(idhmc):
    grp = np.array([-1, 0, 0, 1, 1, -1], np.int32)
    X, Y = AUX.problem_aux("WEIBULL_LOG_LOGSHAPE", 50, 6)
    m = idhmc.GLM(X, Y, idhmc.glm.WEIBULL_LOG_LOGSHAPE, constants=[1.0, 2.0], aux=1, groups=grp)      # D = 6 + 1 + 2

    def refused(what, opt=None, model=m, **fields):
        d = model.glm_desc()
        keep = []
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data_as(C.POINTER(C.c_int32 if v.dtype == np.int32 else C.c_double))
            setattr(d, k, v)
        rc, msg = _create_glm(idhmc, d, opt)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (fields.keys(), rc, msg)

    lib = idhmc.load_library()
    h = C.c_void_p()
    assert lib.idhmc_create_glm(C.byref(h), 0, 4, 0, None, None, 1) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    # the hierarchy's own
    for H in (-1, 5, 100):
        refused(b"H = ", H=H)
    refused(b"groups is NULL", groups=None)
    refused(b"groups must be NULL with H = 0", H=0)
    for bad in (-2, 2, 7):
        g = grp.copy()
        g[3] = bad
        refused(b"groups[3] = %d is outside -1..1" % bad, groups=g)
    refused(b"group 1 has no column", groups=np.array([-1, 0, 0, 0, 0, -1], np.int32))
    refused(b"group 0 has no column", groups=np.array([-1, 1, 1, 1, 1, -1], np.int32))
    refused(b"group 2 has no column", H=3)
    for Dx in (0, -3):
        refused(b"Dx = ", Dx=Dx)
    # what kinds 5 and 6 refuse
    for K in (0, 5, -1):
        refused(b"K = ", K=K)
    for nc in (-1, 17):
        refused(b"nc = ", nc=nc)
    for A in (-1, 5):
        refused(b"A = ", A=A)
    refused(b"n = 0", n=0)
    refused(b"X and Y are needed", X=None)
    refused(b"X and Y are needed", Y=None)
    refused(b"constants are needed", constants=None)
    refused(b"c[1] is not finite", constants=np.array([1.0, np.nan]))
    bad = X.copy()
    bad[2, 5] = np.inf
    refused(b"X[2, 5] is not finite", X=bad)
    bad = np.ascontiguousarray(Y).copy()
    bad[3, 1] = -np.inf
    refused(b"Y[3, 1] is not finite", Y=bad)
    refused(b"needs HIP source", source=None)
    refused(b"needs HIP source", source=b"")
    tau = np.ones(9)
    tau[8] = 0.0                                                    # a log scale's precision
    refused(b"tau[8]", tau=tau)
    mu = np.zeros(9)
    mu[7] = np.nan
    refused(b"mu[7]", mu=mu)
    # the limits are on the total D: D > 512 needs a shared metric; D > 1024 is not supported; n_pad L <= 2^27
    big = idhmc.GLM(np.ones((2, 510)), [0.0, 1.0], idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=[0, 1] * 255)
    refused(b"SHARED", model=big)
    assert _create_glm(idhmc, big.glm_desc(), idhmc.default_options(metric_mode=idhmc.METRIC_SHARED))[0] in (0, idhmc.ERR_NO_DEVICE)
    refused(b"D <= 1024", model=big, Dx=1022)
    refused(b"2^27", n=(1 << 27) // 128 + 1)                        # refused before X is read


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    """each family's C restatement, compiled once per family; model() points it at a problem"""
    class R:
        def __init__(self):
            self.work = {}

        def model(self, family, X, Y, grp, mu=None, tau=None):
            if family not in self.work:
                self.work[family] = str(tmp_path_factory.mktemp(family.lower()))
            A, H = SHAPE[family][2], int(np.max(grp)) + 1
            return oracle.OracleModel.custom(X.shape[1] + A + H, c_source_hier(family), oracle_params_hier(X, Y, A, grp, consts(family), mu, tau),
                                             self.work[family])

        def flat(self, family, X, Y, mu, tau):
            """the ungrouped model of tests/test_glm_cpu.py or tests/test_glm_aux_cpu.py on the same data"""
            key, A = "flat_" + family, SHAPE[family][2]
            if key not in self.work:
                self.work[key] = str(tmp_path_factory.mktemp(key.lower()))
            if A == 0:
                return oracle.OracleModel.custom(X.shape[1], FLAT.c_source(family), FLAT.oracle_params(X, Y, None, mu, tau), self.work[key])
            return oracle.OracleModel.custom(X.shape[1] + A, AUX.c_source_aux(family), AUX.oracle_params_aux(X, Y, A, None, mu, tau), self.work[key])
    return R()


def layouts(Dx, H):
    out = [("interleaved", interleaved(Dx, H), False)]
    levels = (Dx - 1) // (H + 1)
    if levels >= 1:
        out.append(("blocks", blocks(Dx, H, levels), True))
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("n,Dx", [(1, 5), (37, 25), (128, 100), (1000, 127), (300, 300)])
def test_restatement_matches_the_closed_form(restated, family, H, n, Dx):
    A = SHAPE[family][2]
    D = Dx + A + H
    rng = np.random.default_rng(n * Dx + H)
    mu, tau = rng.standard_normal(D) * 0.3, rng.uniform(0.5, 2.0, D)
    for name, grp, one_hot in layouts(Dx, H):
        X, Y = problem_hier(family, n, Dx, grp, one_hot, seed=n + Dx)
        om = restated.model(family, X, Y, grp, mu, tau)
        for k in range(3):
            q = start_hier(family, 1, Dx, H, seed=k, scale=0.3 + 0.3 * k)[0]
            lq, g = om.logdensity_and_gradient(q)
            l_ref, g_ref, lscale, gscale = numpy_density_hier(family, X, Y, q, grp, mu, tau)
            assert abs(lq - l_ref) <= 1e-12 * lscale, (name, lq, l_ref)
            assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), (name, np.abs(g[:D] - g_ref) / gscale)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("H", [1, 2, 4])
def test_restatement_gradient_is_the_derivative(restated, family, H):
    """central differences in every omega, every a and a spread of u (the first columns, one of each group, the last)"""
    n, Dx = 200, 23
    A = SHAPE[family][2]
    D = Dx + A + H
    for name, grp, one_hot in layouts(Dx, H):
        X, Y = problem_hier(family, n, Dx, grp, one_hot, seed=11)
        om = restated.model(family, X, Y, grp, 0.1, 0.5)
        q = start_hier(family, 1, Dx, H, seed=5)[0]
        _, g = om.logdensity_and_gradient(q)
        coords = sorted(set(range(6)) | {int(np.flatnonzero(grp == k)[-1]) for k in range(H)} | {Dx - 1} | set(range(Dx, D)))
        h = 1e-5
        for c in coords:
            e = np.zeros(D)
            e[c] = h
            fd = (om.logdensity_and_gradient(q + e)[0] - om.logdensity_and_gradient(q - e)[0]) / (2 * h)
            assert fd == pytest.approx(g[c], rel=1e-6, abs=1e-6), (name, c)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("H", [1, 2, 4])
def test_fixed_scales_are_an_ungrouped_glm(restated, family, H):
    """omega held fixed is an ungrouped GLM on X diag(s): lq minus omega's prior term, and the gradient in u and a"""
    n, Dx = 150, 40
    A = SHAPE[family][2]
    D = Dx + A + H
    rng = np.random.default_rng(H)
    mu, tau = rng.standard_normal(D) * 0.3, rng.uniform(0.5, 2.0, D)
    for name, grp, one_hot in layouts(Dx, H):
        X, Y = problem_hier(family, n, Dx, grp, one_hot, seed=7)
        om = restated.model(family, X, Y, grp, mu, tau)
        for k in range(2):
            q = start_hier(family, 1, Dx, H, seed=k)[0]
            s = np.where(grp >= 0, np.exp(q[Dx + A:])[np.maximum(grp, 0)], 1.0)
            flat = restated.flat(family, X * s, Y, mu[:Dx + A], tau[:Dx + A])
            lq, g = om.logdensity_and_gradient(q)
            lf, gf = flat.logdensity_and_gradient(q[:Dx + A])
            d = q[Dx + A:] - mu[Dx + A:]
            prior = -0.5 * np.sum(tau[Dx + A:] * d * d)
            _, _, lscale, gscale = numpy_density_hier(family, X, Y, q, grp, mu, tau)
            assert abs((lq - prior) - lf) <= 1e-12 * lscale, (name, lq - prior, lf)
            assert np.all(np.abs(g[:Dx + A] - gf[:Dx + A]) <= 1e-12 * gscale[:Dx + A] + 1e-300), name


def test_a_scale_past_the_range_of_dexp(restated, oracle):
    """omega = -800: e = 0, the group's coefficients vanish and everything stays finite; omega = +800: e = inf, b = +-inf, z and v
    are inf or NaN (0 * inf in the one-hot columns), which a chain reads as l = -inf: the rejected point"""
    n, Dx, H, levels = 300, 40, 2, 12
    grp = blocks(Dx, H, levels)
    X, Y = problem_hier("BERNOULLI_LOGIT", n, Dx, grp, True, seed=1)
    om = restated.model("BERNOULLI_LOGIT", X, Y, grp)
    q = np.r_[np.full(Dx, 0.1), OMEGA0, OMEGA0]
    q[Dx] = -800.0
    lq, g = om.logdensity_and_gradient(q)
    l_ref, g_ref, lscale, gscale = numpy_density_hier("BERNOULLI_LOGIT", X, Y, q, grp)
    assert np.isfinite(lq) and np.isfinite(g).all() and abs(lq - l_ref) <= 1e-12 * lscale
    assert np.all(g[:Dx][grp == 0] == -0.1)                          # G e = 0: the prior alone
    q[Dx] = 800.0
    assert not np.isfinite(om.logdensity_and_gradient(q)[0])
    ch = oracle.OracleChain(om, None, seed=1, chain_id=0)
    ch.set_q(q)
    assert ch.lq == -np.inf
