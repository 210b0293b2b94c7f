"""GLM likelihoods with sampled auxiliary parameters (IDHMC_MODEL_GLM_AUX, GLM(..., aux=A)) without a GPU: the constructor's
validation and packing, the C boundary's argument checks, and the C restatement of DESIGN section 12's definition (section 11's
with the auxiliary coordinates: z over the Dx columns of X, the scores S_j summed per residue of 128 like v, their canonical tree
as the gradient) with the shipped observations, against numpy closed forms, central differences in every coordinate and a sweep
over |z| up to 700 and the a0 each source's docstring promises.

Per source: OBS_C_AUX holds the observation of the restatement the GPU tests hand the oracle (tests/test_gpu_glm_aux.py),
problem_aux() a data generator, numpy_density_aux() the closed form.  TEST_A4 is a test-only source with the maximum A = 4 and
K = 2 (a Gaussian whose mean and log scale both move with a covariate), so every plane and owner-lane position has a user.
The restatement's params are [n, K, nc, A, mu (D), tau (D), c (nc), X row-major (n x Dx), Y row-major (n x K)], D = Dx + A."""
import ctypes as C

import numpy as np
import pytest

C_BODY_AUX = r"""
#include "orc_math.h"
%s
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    const long n = (long)params[0];
    const int K = (int)params[1], nc = (int)params[2], A = (int)params[3], Dx = D - A;
    const double *mu = params + 4, *tau = mu + D, *c = tau + D, *X = c + nc, *Y = X + n * Dx;
    const double *a = q + Dx;
    double T[128], V[128], S[4][128];
    for (int r = 0; r < 128; ++r) { T[r] = 0.0; V[r] = 0.0; S[0][r] = S[1][r] = S[2][r] = S[3][r] = 0.0; }
    for (int j = 0; j < L; ++j) grad[j] = 0.0;
    for (long i = 0; i < n; ++i) {
        const double *xi = X + i * Dx;
        double z = 0.0;
        for (int j = 0; j < Dx; ++j) z = fma(xi[j], q[j], z);          /* columns of X ascending: a is in no product */
        double y[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < K; ++k) y[k] = Y[i * K + k];
        double r, v, s[4] = {0.0, 0.0, 0.0, 0.0};
        glm_observation(z, y, c, a, &r, &v, s);
        V[i & 127] = V[i & 127] + v;                                   /* observation blocks ascending, from +0 */
        for (int j = 0; j < A; ++j) S[j][i & 127] = S[j][i & 127] + s[j];
        for (int j = 0; j < Dx; ++j) grad[j] = fma(xi[j], r, grad[j]); /* observations ascending */
    }
    for (int j = 0; j < A; ++j) grad[Dx + j] = orc_tree128(S[j]);      /* the canonical 128-residue tree */
    for (int j = 0; j < D; ++j) {
        const double d = q[j] - mu[j];
        T[j & 127] = fma(tau[j] * d, d, T[j & 127]);
        grad[j] = fma(-tau[j], d, grad[j]);
    }
    for (int r = 0; r < 128; ++r) T[r] = fma(2.0, V[r], T[r]);
    return -0.5 * orc_tree128(T);
}
"""

# the shipped observations (inplacedhmc_jl_amd.glm) and the test-only one, restated in C with the oracle's orc_* functions
OBS_C_AUX = {
    "GAUSSIAN_IDENTITY_LOGSIGMA": r"""
static void glm_observation(double z, const double *y, const double *c, const double *a, double *r, double *v, double *s)
{
    const double w = orc_exp(-a[0]);
    const double u = (y[0] - z) * w;
    *v = 0.5 * (u * u) + a[0];
    *r = u * w;
    s[0] = u * u - 1.0;
}""",
    "STUDENT_T_IDENTITY_LOGSIGMA": r"""
static void glm_observation(double z, const double *y, const double *c, const double *a, double *r, double *v, double *s)
{
    const double nu = c[0], sg = orc_exp(a[0]);
    const double u = (y[0] - z) / sg;
    const double h = 0.5 * (nu + 1.0);
    if (fabs(u) < 1e100) {
        *v = h * orc_log1p(u * u / nu) + a[0];
        *r = (nu + 1.0) * u / (sg * (nu + u * u));
        s[0] = (nu + 1.0) * (u * u) / (nu + u * u) - 1.0;
    } else {
        const double iu = 1.0 / u;
        *v = h * (2.0 * orc_log(fabs(u)) - orc_log(nu) + orc_log1p(nu * iu * iu)) + a[0];
        *r = (nu + 1.0) * iu / (sg * (nu * iu * iu + 1.0));
        s[0] = (nu + 1.0) / (nu * iu * iu + 1.0) - 1.0;
    }
}""",
    "WEIBULL_LOG_LOGSHAPE": r"""
static void glm_observation(double z, const double *y, const double *c, const double *a, double *r, double *v, double *s)
{
    const double lt = y[0], dl = y[1];
    const double k = orc_exp(a[0]);
    const double w = k * (lt - z);
    const double H = orc_exp(w);
    *v = H - dl * (a[0] - lt + w);
    *r = k * (H - dl);
    s[0] = dl + w * (dl - H);
}""",
    "TEST_A4": r"""
static void glm_observation(double z, const double *y, const double *c, const double *a, double *r, double *v, double *s)
{
    const double ls = a[0] + a[3] * y[1];
    const double w = orc_exp(-ls);
    const double u = (y[0] - z - a[1] * y[1] - a[2]) * w;
    *v = 0.5 * (u * u) + ls;
    *r = u * w;
    s[0] = u * u - 1.0;
    s[1] = *r * y[1];
    s[2] = *r;
    s[3] = s[0] * y[1];
}""",
}
# y0 ~ N(z + a1 y1 + a2, exp(a0 + a3 y1)^2), y1 a covariate: K = 2, A = 4
TEST_A4_SOURCE = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double ls = a[0] + a[3] * o.y[1];
    const double w = dexp(-ls);
    const double u = (o.y[0] - z - a[1] * o.y[1] - a[2]) * w;
    v = 0.5 * (u * u) + ls;
    r = u * w;
    s[0] = u * u - 1.0;
    s[1] = r * o.y[1];
    s[2] = r;
    s[3] = s[0] * o.y[1];
}
"""
SHIPPED_AUX = ["GAUSSIAN_IDENTITY_LOGSIGMA", "STUDENT_T_IDENTITY_LOGSIGMA", "WEIBULL_LOG_LOGSHAPE"]
FAMILIES = SHIPPED_AUX + ["TEST_A4"]
SHAPE = {"GAUSSIAN_IDENTITY_LOGSIGMA": (1, 0, 1), "STUDENT_T_IDENTITY_LOGSIGMA": (1, 1, 1), "WEIBULL_LOG_LOGSHAPE": (2, 0, 1),
         "TEST_A4": (2, 0, 4)}                         # K, nc, A
NU = 4.0
TRUE_A = {"GAUSSIAN_IDENTITY_LOGSIGMA": [np.log(0.7)], "STUDENT_T_IDENTITY_LOGSIGMA": [np.log(0.7)],
          "WEIBULL_LOG_LOGSHAPE": [np.log(1.5)], "TEST_A4": [np.log(0.7), 0.3, -0.2, 0.25]}


def source(idhmc, family):
    return TEST_A4_SOURCE if family == "TEST_A4" else getattr(idhmc.glm, family)


def consts(family):
    return np.array([NU]) if family == "STUDENT_T_IDENTITY_LOGSIGMA" else None


def c_source_aux(family):
    return C_BODY_AUX % OBS_C_AUX[family]


def oracle_params_aux(X, Y, A, c=None, mu=None, tau=None):
    n, Dx = X.shape
    D = Dx + A
    Y = np.asarray(Y, float).reshape(n, -1)
    c = np.zeros(0) if c is None else np.asarray(c, float)
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    return np.concatenate([[float(n), float(Y.shape[1]), float(c.size), float(A)], mu, tau, c, np.asarray(X, float).ravel(), Y.ravel()])


def problem_aux(family, n, Dx, seed=3, scale=0.5):
    """synthetic data from the family's own model at TRUE_A: design with a first column of ones, coefficients ~ N(0, 1/Dx)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, Dx)) * scale
    X[:, 0] = 1.0
    z = X @ (rng.standard_normal(Dx) / np.sqrt(Dx))
    a = TRUE_A[family]
    if family == "GAUSSIAN_IDENTITY_LOGSIGMA":
        Y = z + np.exp(a[0]) * rng.standard_normal(n)
    elif family == "STUDENT_T_IDENTITY_LOGSIGMA":
        Y = z + np.exp(a[0]) * rng.standard_t(NU, n)
    elif family == "WEIBULL_LOG_LOGSHAPE":
        t = np.exp(z) * rng.weibull(np.exp(a[0]), n)
        cens = np.exp(z) * rng.uniform(0.5, 2.5, n)                       # right-censoring times: about a third censored
        Y = np.stack([np.log(np.minimum(t, cens)), (t <= cens).astype(float)], 1)
    else:
        y1 = rng.uniform(-1.0, 1.0, n)
        Y = np.stack([z + a[1] * y1 + a[2] + np.exp(a[0] + a[3] * y1) * rng.standard_normal(n), y1], 1)
    return X, Y


def start_aux(family, C, Dx, seed=0, scale=0.3):
    """positions near the data's own parameters: small coefficients, a around TRUE_A"""
    rng = np.random.default_rng(seed + Dx)
    a = np.asarray(TRUE_A[family])
    return np.concatenate([rng.uniform(-scale, scale, (C, Dx)) / np.sqrt(Dx), a + rng.uniform(-0.2, 0.2, (C, a.size))], 1)


def numpy_terms_aux(family, z, Y, a):
    """closed form per observation: (log p, d log p / dz, d log p / da [n, A], magnitude of log p's terms, of the scores' terms)"""
    Y = np.asarray(Y, float).reshape(z.size, -1)
    if family == "GAUSSIAN_IDENTITY_LOGSIGMA":
        sg = np.exp(a[0])
        u = (Y[:, 0] - z) / sg
        return -0.5 * u * u - a[0], u / sg, (u * u - 1.0)[:, None], 0.5 * u * u + abs(a[0]), (u * u + 1.0)[:, None]
    if family == "STUDENT_T_IDENTITY_LOGSIGMA":
        sg = np.exp(a[0])
        u = (Y[:, 0] - z) / sg
        big = np.abs(u) >= 1e100                                            # u^2 overflows: the same quantities from 1 / u
        us, iu = np.where(big, 1.0, u), 1.0 / np.where(big, u, 1.0)
        l1p = np.where(big, 2.0 * np.log(np.abs(np.where(big, u, 1.0))) - np.log(NU) + np.log1p(NU * iu * iu), np.log1p(us * us / NU))
        lp = -0.5 * (NU + 1.0) * l1p - a[0]
        r = np.where(big, (NU + 1.0) * iu / (sg * (NU * iu * iu + 1.0)), (NU + 1.0) * us / (sg * (NU + us * us)))
        f = np.where(big, (NU + 1.0) / (NU * iu * iu + 1.0), (NU + 1.0) * us * us / (NU + us * us))
        return lp, r, (f - 1.0)[:, None], np.abs(0.5 * (NU + 1.0) * l1p) + abs(a[0]), (f + 1.0)[:, None]
    if family == "WEIBULL_LOG_LOGSHAPE":
        lt, dl = Y[:, 0], Y[:, 1]
        k = np.exp(a[0])
        w = k * (lt - z)
        H = np.exp(w)
        return (dl * (a[0] - lt + w) - H, k * (H - dl), (dl + w * (dl - H))[:, None],
                dl * (abs(a[0]) + np.abs(lt) + np.abs(w)) + H, (dl + np.abs(w) * (dl + H))[:, None])
    y1 = Y[:, 1]
    ls = a[0] + a[3] * y1
    u = (Y[:, 0] - z - a[1] * y1 - a[2]) * np.exp(-ls)
    r = u * np.exp(-ls)
    s = np.stack([u * u - 1.0, r * y1, r, (u * u - 1.0) * y1], 1)
    return -0.5 * u * u - ls, r, s, 0.5 * u * u + np.abs(ls), np.stack([u * u + 1.0, np.abs(r * y1), np.abs(r), (u * u + 1.0) * np.abs(y1)], 1)


def numpy_density_aux(family, X, Y, q, mu=None, tau=None):
    """(l(q), grad l(q), magnitude of l's terms, per-coordinate magnitude of the terms summed into grad), q = [beta | a]"""
    n, Dx = X.shape
    D = q.size
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    lp, r, s, mag, smag = numpy_terms_aux(family, X @ q[:Dx], Y, q[Dx:])
    d = q - mu
    g = np.concatenate([X.T @ r, s.sum(0)]) - tau * d
    gscale = np.concatenate([np.abs(X).T @ np.abs(r), smag.sum(0)]) + np.abs(tau * d)
    return np.sum(lp) - 0.5 * np.sum(tau * d * d), g, np.sum(mag) + 0.5 * np.sum(tau * d * d), gscale


def make(idhmc, family, X, Y, mu=None, tau=None):
    return idhmc.GLM(X, Y, source(idhmc, family), consts(family), mu, tau, aux=SHAPE[family][2])


# ---- the constructor ---------------------------------------------------------------------------------------------------------------
def test_constructor_packs_params(idhmc):
    X, Y = problem_aux("WEIBULL_LOG_LOGSHAPE", 7, 3)
    c = [2.0, 0.5]
    m = idhmc.GLM(X, Y, idhmc.glm.WEIBULL_LOG_LOGSHAPE, constants=c, prior_mu=0.5, prior_tau=np.r_[1.0, 2.0, 3.0, 4.0, 5.0], aux=2)
    assert m.kind == idhmc.MODEL_GLM_AUX == 6 and m.D == 5 and (m.Dx, m.A, m.n, m.K, m.nc) == (3, 2, 7, 2, 2)
    assert np.array_equal(m.params, np.concatenate([[2.0, 2.0, 2.0], c, X.ravel(), Y.ravel()]))
    assert (m.params.size - 3 - m.nc) // (m.Dx + m.K) == m.n and (m.params.size - 3 - m.nc) % (m.Dx + m.K) == 0
    assert np.array_equal(m.mu, np.full(5, 0.5)) and np.array_equal(m.tau, [1.0, 2.0, 3.0, 4.0, 5.0])
    d = m.desc()
    assert d.kind == 6 and d.D == 5 and d.nparams == m.params.size and d.params[2] == 2.0 and d.tau[4] == 5.0
    assert d.source == idhmc.glm.WEIBULL_LOG_LOGSHAPE.encode()
    m = idhmc.GLM(X[:, :1], Y[:, 0], idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1)      # one coefficient, a 1-D Y
    assert (m.D, m.Dx, m.A, m.K, m.nc) == (2, 1, 1, 1, 0) and m.mu is None and m.tau is None
    assert np.array_equal(m.params, np.concatenate([[1.0, 0.0, 1.0], X[:, 0], Y[:, 0]]))


def test_aux_zero_packs_what_it_always_did(idhmc):
    """aux = 0 (and no aux argument) is IDHMC_MODEL_GLM with [K, nc, c | X | Y], byte for byte"""
    X, Y = problem_aux("TEST_A4", 9, 4)
    c = [1.5, -2.0, 0.25]
    want = np.concatenate([[2.0, 3.0], c, X.ravel(), Y.ravel()])
    for m in (idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, c, 0.5, 2.0), idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, c, 0.5, 2.0, aux=0)):
        assert m.kind == idhmc.MODEL_GLM == 5 and m.D == 4 and (m.Dx, m.A) == (4, 0)
        assert m.params.dtype == np.float64 and m.params.tobytes() == want.tobytes()
        assert m.mu.tobytes() == np.full(4, 0.5).tobytes() and m.tau.tobytes() == np.full(4, 2.0).tobytes()
        d = m.desc()
        assert d.kind == 5 and d.D == 4 and d.nparams == want.size


def test_constructor_validates_aux(idhmc):
    X, Y = problem_aux("GAUSSIAN_IDENTITY_LOGSIGMA", 20, 5)
    src = idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA
    for bad in (-1, 5, 1.0, 1.5, "1", None, True):
        with pytest.raises(ValueError):
            idhmc.GLM(X, Y, src, aux=bad)
    with pytest.raises(ValueError):
        idhmc.GLM(np.zeros((4, 1021)), np.zeros(4), src, aux=4)            # Dx + A > 1024
    assert idhmc.GLM(np.zeros((4, 1020)), np.zeros(4), src, aux=4).D == 1024
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, prior_mu=np.zeros(5), aux=1)                  # the prior has length Dx + A
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, prior_tau=np.ones(5), aux=1)
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, prior_tau=np.r_[np.ones(5), 0.0], aux=1)      # the auxiliary coordinate's precision
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, prior_mu=np.r_[np.zeros(5), np.nan], aux=1)
    m = idhmc.GLM(X, Y, src, prior_mu=np.arange(6.0), prior_tau=np.arange(1.0, 7.0), aux=1)
    assert m.mu[5] == 5.0 and m.tau[5] == 6.0
    for a in ((X[0], Y, src), (X, Y[:-1], src), (X, np.zeros((20, 5)), src), (X, Y, ""), (X, np.where(Y > 0, np.nan, Y), src)):
        with pytest.raises(ValueError):
            idhmc.GLM(*a, aux=1)
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, constants=np.zeros(17), aux=1)


def test_shipped_sources_declare_their_shapes(idhmc):
    assert set(idhmc.glm.AUX_SHAPES) == set(SHIPPED_AUX)
    for name, (K, nc, A) in idhmc.glm.AUX_SHAPES.items():
        src = getattr(idhmc.glm, name)
        assert (K, nc, A) == SHAPE[name]
        assert "glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)" in src
        assert ("o.y[%d]" % (K - 1)) in src and ("o.y[%d]" % K) not in src
        assert ("o.c[%d]" % (nc - 1) in src) if nc else "o.c[" not in src
        assert ("a[%d]" % (A - 1)) in src and ("s[%d]" % (A - 1)) in src and ("a[%d]" % A) not in src and ("s[%d]" % A) not in src
    assert "dexp" in idhmc.glm.__doc__ and all(n in idhmc.glm.__doc__ for n in SHIPPED_AUX)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def _create(idhmc, desc, opt=None):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create(C.byref(h), 0, 4, 0, C.byref(desc), None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def test_a_valid_desc_passes_the_argument_checks(idhmc):
    for family in FAMILIES:
        X, Y = problem_aux(family, 50, 6)
        m = make(idhmc, family, X, Y)                                  # kept alive: desc() points into its arrays
        rc, msg = _create(idhmc, m.desc())
        # a context where a device exists; otherwise idhmc_create stops at its device check, past every argument check
        assert rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg), (family, rc, msg)
    m = make(idhmc, "GAUSSIAN_IDENTITY_LOGSIGMA", *problem_aux("GAUSSIAN_IDENTITY_LOGSIGMA", 50, 6), 1.0, 0.25)
    rc, msg = _create(idhmc, m.desc())
    assert rc == 0 or rc == idhmc.ERR_NO_DEVICE, (rc, msg)
    m = idhmc.GLM(np.ones((3, 1)), np.zeros(3), idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1)     # Dx = 1, the smallest
    assert _create(idhmc, m.desc())[0] in (0, idhmc.ERR_NO_DEVICE)


def test_glm_form_is_declared_and_null_safe(idhmc):
    lib = idhmc.load_library()
    assert lib.idhmc_glm_form(None) == -1


def test_bad_descs_are_refused_before_the_device(idhmc):
    X, Y = problem_aux("WEIBULL_LOG_LOGSHAPE", 50, 6)
    m = idhmc.GLM(X, Y, idhmc.glm.WEIBULL_LOG_LOGSHAPE, constants=[1.0, 2.0], aux=1)   # params = [2, 2, 1, c0, c1 | X (300) | Y (100)], D = 7

    def refused(desc, what, opt=None):
        rc, msg = _create(idhmc, desc, opt)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (rc, msg)

    def with_params(p, D=None):
        d = m.desc()
        d.params = p.ctypes.data_as(C.POINTER(C.c_double))
        d.nparams = p.size
        if D is not None:
            d.D = D
        return d

    for a in (0.0, 5.0, 1.5, -1.0, np.nan, np.inf):
        p = m.params.copy()
        p[2] = a
        refused(with_params(p), b"A = ")
    p = m.params.copy()
    p[2] = 4.0
    refused(with_params(p, D=4), b"Dx = D - A")                    # no coefficient left
    refused(with_params(p, D=3), b"Dx = D - A")
    for k in (0.0, 5.0, 1.5, -1.0, np.nan, np.inf):
        p = m.params.copy()
        p[0] = k
        refused(with_params(p), b"K = ")
    for nc in (-1.0, 17.0, 0.5, np.nan):
        p = m.params.copy()
        p[1] = nc
        refused(with_params(p), b"nc = ")
    d = m.desc()
    d.nparams = m.params.size - 1                                   # remainder not a multiple of Dx + K
    refused(d, b"multiple of Dx + K")
    d = m.desc()
    d.nparams = 5                                                   # no observations
    refused(d, b"multiple of Dx + K")
    d = m.desc()
    d.D = 8                                                         # Dx = 7: 400 is not a multiple of 9
    refused(d, b"multiple of Dx + K")
    d = m.desc()
    d.nparams = 2
    refused(d, b"begin with K, nc and A")
    d = m.desc()
    d.params = None
    refused(d, b"begin with K, nc and A")
    p = m.params.copy()
    p[4] = np.nan                                                   # c[1]
    refused(with_params(p), b"c[1] is not finite")
    p = m.params.copy()
    p[5 + 17] = np.inf                                              # X[2, 5] of the n x Dx matrix
    refused(with_params(p), b"X[2, 5] is not finite")
    p = m.params.copy()
    p[5 + 300 + 7] = -np.inf                                        # Y[3, 1]
    refused(with_params(p), b"Y[3, 1] is not finite")
    d = m.desc()
    d.source = None
    refused(d, b"needs HIP source")
    d = m.desc()
    d.source = b""
    refused(d, b"needs HIP source")
    tau = np.ones(7)
    tau[6] = 0.0                                                    # the auxiliary coordinate's precision
    d = m.desc()
    d.tau = tau.ctypes.data_as(C.POINTER(C.c_double))
    refused(d, b"tau[6]")
    mu = np.zeros(7)
    mu[6] = np.nan
    d = m.desc()
    d.mu = mu.ctypes.data_as(C.POINTER(C.c_double))
    refused(d, b"mu[6]")
    # the limits are on the total D: D > 512 needs a shared metric; D > 1024 is not supported; n_pad L <= 2^27
    big = idhmc.GLM(np.ones((2, 512)), [0.0, 1.0], idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1)
    refused(big.desc(), b"SHARED")
    assert _create(idhmc, big.desc(), idhmc.default_options(metric_mode=idhmc.METRIC_SHARED))[0] in (0, idhmc.ERR_NO_DEVICE)
    wide = idhmc.Model(idhmc.MODEL_GLM_AUX, 1100, source="x", params=np.r_[1.0, 0.0, 1.0, np.zeros(1100)])
    refused(wide.desc(), b"D <= 1024")
    d = m.desc()                                                    # n_pad = 2^27 / 128 + 128 at L = 128 (refused before X is read)
    d.nparams = 5 + ((1 << 27) // 128 + 1) * 8
    refused(d, b"2^27")
    d = m.desc()
    d.kind = 7
    refused(d, b"unknown model kind")


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    """each family's C restatement, compiled once per family; model() points it at a problem"""
    class R:
        def __init__(self):
            self.work = {}

        def model(self, family, X, Y, mu=None, tau=None):
            if family not in self.work:
                self.work[family] = str(tmp_path_factory.mktemp(family.lower()))
            A = SHAPE[family][2]
            return oracle.OracleModel.custom(X.shape[1] + A, c_source_aux(family), oracle_params_aux(X, Y, A, consts(family), mu, tau),
                                             self.work[family])
    return R()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,Dx", [(1, 1), (37, 25), (128, 100), (1000, 127), (300, 300)])
def test_restatement_matches_the_closed_form(restated, family, n, Dx):
    X, Y = problem_aux(family, n, Dx, seed=n + Dx)
    A = SHAPE[family][2]
    rng = np.random.default_rng(n * Dx)
    mu, tau = rng.standard_normal(Dx + A) * 0.3, rng.uniform(0.5, 2.0, Dx + A)
    om = restated.model(family, X, Y, mu, tau)
    for k in range(3):
        q = start_aux(family, 1, Dx, seed=k, scale=0.3 + 0.5 * k)[0]
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_aux(family, X, Y, q, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g - g_ref) <= 1e-12 * gscale + 1e-300), np.abs(g - g_ref) / gscale


@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_gradient_is_the_derivative(restated, family):
    """central differences in every coordinate, the auxiliary ones included"""
    X, Y = problem_aux(family, 200, 12, seed=11)
    D = 12 + SHAPE[family][2]
    om = restated.model(family, X, Y, 0.1, 0.5)
    q = start_aux(family, 1, 12, seed=5)[0]
    _, g = om.logdensity_and_gradient(q)
    h = 1e-5
    for c in range(D):
        e = np.zeros(D)
        e[c] = h
        fd = (om.logdensity_and_gradient(q + e)[0] - om.logdensity_and_gradient(q - e)[0]) / (2 * h)
        assert fd == pytest.approx(g[c], rel=1e-6, abs=1e-6), c


# (z, a0) the docstring of inplacedhmc_jl_amd.glm promises: |z| to 700 with every |a0| <= 300 (Gaussian) or 700 (Student-t); the
# Weibull's k (log t - z) < 709.78 bounds a0 by z: k = 1 at |z| = 700, up to exp(2.8) at |z| = 40 (log t is about 0)
SWEEP = {"GAUSSIAN_IDENTITY_LOGSIGMA": [(z, a) for z in (700.0, -700.0, 300.0, 40.0, 1e-3) for a in (-300.0, -40.0, 0.0, 40.0, 300.0, 700.0)],
         "STUDENT_T_IDENTITY_LOGSIGMA": [(z, a) for z in (700.0, -700.0, 300.0, 40.0, 1e-3) for a in (-700.0, -300.0, -40.0, 0.0, 40.0, 700.0)],
         "WEIBULL_LOG_LOGSHAPE": [(z, a) for z in (700.0, -700.0, 300.0) for a in (-700.0, -40.0, 0.0)] +
                                 [(z, a) for z in (40.0, -40.0, 1e-3) for a in (-300.0, 0.0, 2.8)] + [(1e-3, 40.0)]}


@pytest.mark.parametrize("family", SHIPPED_AUX)
def test_restatement_is_overflow_safe(restated, family):
    """z = +-x: l and grad l finite and equal to the closed form over the promised range (the Student-t also past |u| = 1e100: a0 = -300
    and below).  Tolerance 1e-12 of the terms' magnitude: exp(w) carries |w| <= 710 roundings of its argument."""
    X = np.array([[1.0], [-1.0], [1.0], [-1.0]])
    _, Y = problem_aux(family, 4, 1, seed=1)
    tau = np.array([1e-6, 1e-6])
    om = restated.model(family, X, Y, tau=tau)
    for z, a0 in SWEEP[family]:
        if family == "WEIBULL_LOG_LOGSHAPE" and np.exp(a0) * (np.abs(Y[:, 0]).max() + abs(z)) >= 709.0:
            continue                                                    # outside the promise (this problem's log t)
        q = np.array([z, a0])
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_aux(family, X, Y, q, tau=tau)
        assert np.isfinite(lq) and np.isfinite(g).all(), (q, lq, g)
        assert abs(lq - l_ref) <= 1e-12 * lscale and np.all(np.abs(g - g_ref) <= 1e-12 * gscale + 1e-300), (q, lq, l_ref, g, g_ref)


def test_past_the_promise_the_density_is_minus_infinity(restated):
    """a0 = -800 for the Gaussian source: exp(800) is +inf, v is +inf (or NaN where y = z): the engine's rejected point"""
    X, Y = problem_aux("GAUSSIAN_IDENTITY_LOGSIGMA", 40, 3, seed=2)
    om = restated.model("GAUSSIAN_IDENTITY_LOGSIGMA", X, Y)
    lq, _ = om.logdensity_and_gradient(np.array([0.1, 0.2, -0.1, -800.0]))
    assert lq == -np.inf
