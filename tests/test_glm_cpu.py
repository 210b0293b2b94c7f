"""User-defined GLM likelihoods (IDHMC_MODEL_GLM) without a GPU: the Python constructor's validation and packing, the C boundary's
argument checks, and the C restatements of the shipped observation sources (section 10's arithmetic with the
observation swapped) against numpy closed forms, finite differences, and |z| up to 700.

Per shipped source: OBS_C holds the observation of the restatement the GPU tests hand the oracle (tests/test_gpu_glm.py),
problem() a data generator and numpy_density() the closed form.  The restatement's params are [n, K, nc, mu (D), tau (D), c (nc), X row-major (n x D), Y row-major (n x K)]
-- see oracle_params()."""
import ctypes as C

import numpy as np
import pytest

C_BODY = r"""
#include "orc_math.h"
%s
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    const long n = (long)params[0];
    const int K = (int)params[1], nc = (int)params[2];
    const double *mu = params + 3, *tau = mu + D, *c = tau + D, *X = c + nc, *Y = X + n * D;
    double T[128], A[128];
    (void)nc;
    for (int r = 0; r < 128; ++r) { T[r] = 0.0; A[r] = 0.0; }
    for (int j = 0; j < L; ++j) grad[j] = 0.0;
    for (long i = 0; i < n; ++i) {
        const double *xi = X + i * D;
        double z = 0.0;
        for (int j = 0; j < D; ++j) z = fma(xi[j], q[j], z);          /* columns ascending */
        double y[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < K; ++k) y[k] = Y[i * K + k];
        double r, v;
        glm_observation(z, y, c, &r, &v);
        A[i & 127] = A[i & 127] + v;                                  /* observation blocks ascending */
        for (int j = 0; j < D; ++j) grad[j] = fma(xi[j], r, grad[j]); /* observations ascending */
    }
    for (int j = 0; j < D; ++j) {
        const double d = q[j] - mu[j];
        T[j & 127] = fma(tau[j] * d, d, T[j & 127]);
        grad[j] = fma(-tau[j], d, grad[j]);
    }
    for (int r = 0; r < 128; ++r) T[r] = fma(2.0, A[r], T[r]);
    return -0.5 * orc_tree128(T);
}
"""

# the observation of each shipped source (inplacedhmc_jl_amd.glm), restated in C with the oracle's orc_* functions
OBS_C = {
    "POISSON_LOG": r"""
static void glm_observation(double z, const double *y, const double *c, double *r, double *v)
{
    const double e = orc_exp(z);
    *v = e - y[0] * z;
    *r = y[0] - e;
}""",
    "POISSON_LOG_OFFSET": r"""
static void glm_observation(double z, const double *y, const double *c, double *r, double *v)
{
    const double eta = z + y[1];
    const double e = orc_exp(eta);
    *v = e - y[0] * eta;
    *r = y[0] - e;
}""",
    "BINOMIAL_LOGIT": r"""
static void glm_observation(double z, const double *y, const double *c, double *r, double *v)
{
    const double s = y[0], f = y[1] - y[0];
    const double e = orc_exp(-fabs(z));
    const double l = orc_log1p(e);
    const double a = z > 0.0 ? z : 0.0, b = z > 0.0 ? 0.0 : -z;
    *v = s * (b + l) + f * (a + l);
    const double d = 1.0 + e;
    const double sp = (z >= 0.0 ? 1.0 : e) / d, sn = (z >= 0.0 ? e : 1.0) / d;
    *r = s * sn - f * sp;
}""",
    "BERNOULLI_LOGIT": r"""
static void glm_observation(double z, const double *y, const double *c, double *r, double *v)
{
    const double s = y[0] != 0.0 ? -z : z;
    const double e = orc_exp(-fabs(s));
    *v = (s > 0.0 ? s : 0.0) + orc_log1p(e);
    const double sg = (s >= 0.0 ? 1.0 : e) / (1.0 + e);
    *r = y[0] != 0.0 ? sg : -sg;
}""",
    "STUDENT_T_IDENTITY": r"""
static void glm_observation(double z, const double *y, const double *c, double *r, double *v)
{
    const double nu = c[0], sg = c[1];
    const double u = (y[0] - z) / sg;
    const double h = 0.5 * (nu + 1.0);
    if (fabs(u) < 1e100) {
        *v = h * orc_log1p(u * u / nu);
        *r = (nu + 1.0) * u / (sg * (nu + u * u));
    } else {
        const double iu = 1.0 / u;
        *v = h * (2.0 * orc_log(fabs(u)) - orc_log(nu) + orc_log1p(nu * iu * iu));
        *r = (nu + 1.0) * iu / (sg * (nu * iu * iu + 1.0));
    }
}""",
}
SHIPPED = ["POISSON_LOG", "POISSON_LOG_OFFSET", "BINOMIAL_LOGIT", "STUDENT_T_IDENTITY"]
STUDENT_C = np.array([4.0, 0.7])      # nu, sigma


def c_source(family):
    return C_BODY % OBS_C[family]


def constants(family):
    return STUDENT_C if family == "STUDENT_T_IDENTITY" else None


def oracle_params(X, Y, c=None, mu=None, tau=None):
    n, D = X.shape
    Y = np.asarray(Y, float).reshape(n, -1)
    c = np.zeros(0) if c is None else np.asarray(c, float)
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    return np.concatenate([[float(n), float(Y.shape[1]), float(c.size)], mu, tau, c, np.asarray(X, float).ravel(), Y.ravel()])


def problem(family, n, D, seed=3, scale=0.5):
    """synthetic data from the family's own model: design with a first column of ones, coefficients ~ N(0, 1/D)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) * scale
    X[:, 0] = 1.0
    z = X @ (rng.standard_normal(D) / np.sqrt(D))
    if family == "POISSON_LOG":
        Y = rng.poisson(np.exp(z)).astype(float)
    elif family == "POISSON_LOG_OFFSET":
        off = rng.uniform(-1.0, 1.0, n)
        Y = np.stack([rng.poisson(np.exp(z + off)).astype(float), off], 1)
    elif family == "BINOMIAL_LOGIT":
        m = rng.integers(1, 20, n)
        Y = np.stack([rng.binomial(m, 1.0 / (1.0 + np.exp(-z))).astype(float), m.astype(float)], 1)
    elif family == "BERNOULLI_LOGIT":
        Y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-z))).astype(float)
    else:
        Y = z + STUDENT_C[1] * rng.standard_t(STUDENT_C[0], n)
    return X, Y


def numpy_terms(family, z, Y):
    """closed form per observation: (log p up to data-only terms, d log p / dz, magnitude of the terms summed into log p)"""
    Y = np.asarray(Y, float).reshape(z.size, -1)
    if family in ("POISSON_LOG", "POISSON_LOG_OFFSET"):
        eta = z + (Y[:, 1] if family == "POISSON_LOG_OFFSET" else 0.0)
        e = np.exp(eta)
        return Y[:, 0] * eta - e, Y[:, 0] - e, np.abs(Y[:, 0] * eta) + e
    if family in ("BINOMIAL_LOGIT", "BERNOULLI_LOGIT"):
        s, m = Y[:, 0], (Y[:, 1] if family == "BINOMIAL_LOGIT" else np.ones(z.size))
        lp = -(s * np.logaddexp(0.0, -z) + (m - s) * np.logaddexp(0.0, z))
        return lp, s - m * (0.5 * (1.0 + np.tanh(0.5 * z))), np.abs(lp)
    nu, sg = STUDENT_C
    u = (Y[:, 0] - z) / sg
    lp = -0.5 * (nu + 1.0) * np.log1p(u * u / nu)
    return lp, (nu + 1.0) * u / (sg * (nu + u * u)), np.abs(lp)


def numpy_density(family, X, Y, q, mu=None, tau=None):
    """(l(q), grad l(q), magnitude of l's terms, per-coordinate magnitude of the terms summed into grad)"""
    n, D = X.shape
    mu = np.zeros(D) if mu is None else np.asarray(mu, float)
    tau = np.ones(D) if tau is None else np.asarray(tau, float)
    z = X @ q
    lp, r, mag = numpy_terms(family, z, Y)
    d = q - mu
    return (np.sum(lp) - 0.5 * np.sum(tau * d * d), X.T @ r - tau * d, np.sum(mag) + 0.5 * np.sum(tau * d * d),
            np.abs(X).T @ np.abs(r) + np.abs(tau * d))


def test_constructor_validates_shapes_and_values(idhmc):
    src = idhmc.glm.POISSON_LOG
    X, Y = problem("POISSON_LOG", 20, 5)
    bad = [
        (X[0], Y, src, None),                           # X not a matrix
        (np.zeros((0, 5)), np.zeros(0), src, None),     # no observations
        (np.zeros((4, 0)), np.zeros(4), src, None),     # no coefficients
        (np.zeros((4, 1025)), np.zeros(4), src, None),  # D > 1024
        (X, Y[:-1], src, None),                         # Y rows != n
        (X, np.zeros((20, 5)), src, None),              # K = 5
        (X, np.zeros((20, 0)), src, None),              # K = 0
        (X, np.zeros((20, 2, 2)), src, None),           # Y of three dimensions
        (X, np.where(Y > 1, np.nan, Y), src, None),     # Y not finite
        (X, Y, src, np.zeros(17)),                      # nc = 17
        (X, Y, src, [1.0, np.inf]),                     # constant not finite
        (X, Y, "", None),                               # no source
        (X, Y, "   ", None),
        (X, Y, None, None),
    ]
    for a in bad:
        with pytest.raises(ValueError):
            idhmc.GLM(*a)
    Xn = X.copy()
    Xn[3, 2] = np.nan
    with pytest.raises(ValueError):
        idhmc.GLM(Xn, Y, src)
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, prior_tau=np.r_[1.0, 1.0, 0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, prior_tau=-1.0)
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, prior_mu=np.ones(6))
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y, src, prior_mu=np.r_[0.0, np.inf, 0.0, 0.0, 0.0])


def test_constructor_packs_params(idhmc):
    X, Y = problem("BINOMIAL_LOGIT", 7, 3)
    c = [2.0, 0.5, -1.0]
    m = idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, constants=c, prior_mu=0.5, prior_tau=np.r_[1.0, 2.0, 3.0])
    assert m.kind == idhmc.MODEL_GLM == 5 and m.D == 3 and (m.n, m.K, m.nc) == (7, 2, 3)
    assert np.array_equal(m.params, np.concatenate([[2.0, 3.0], c, X.ravel(), Y.ravel()]))
    assert m.params.size == 2 + 3 + 7 * (3 + 2) and (m.params.size - 2 - m.nc) // (m.D + m.K) == m.n
    assert np.array_equal(m.mu, [0.5, 0.5, 0.5]) and np.array_equal(m.tau, [1.0, 2.0, 3.0])
    d = m.desc()
    assert d.kind == 5 and d.D == 3 and d.nparams == m.params.size and d.params[m.params.size - 1] == Y[-1, 1] and d.tau[2] == 3.0
    assert d.source == idhmc.glm.BINOMIAL_LOGIT.encode()
    y1 = np.arange(7.0)                                 # a 1-D Y is K = 1
    m = idhmc.GLM(X, y1, idhmc.glm.POISSON_LOG)
    assert (m.K, m.nc) == (1, 0) and np.array_equal(m.params, np.concatenate([[1.0, 0.0], X.ravel(), y1]))
    assert m.mu is None and m.tau is None
    d = m.desc()
    assert not d.mu and not d.tau


def test_shipped_sources_declare_their_shapes(idhmc):
    for name, (K, nc) in idhmc.glm.SHAPES.items():
        src = getattr(idhmc.glm, name)
        assert "glm_observation(double z, const GlmObs &o, double &r, double &v)" in src
        assert ("o.y[%d]" % (K - 1)) in src and ("o.y[%d]" % K) not in src
        assert ("o.c[%d]" % (nc - 1) in src) if nc else "o.c[" not in src
    assert set(SHIPPED) | {"BERNOULLI_LOGIT"} == set(idhmc.glm.SHAPES)


def _create(idhmc, desc, opt=None):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create(C.byref(h), 0, 4, 0, C.byref(desc), None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def test_a_valid_desc_passes_the_argument_checks(idhmc):
    X, Y = problem("STUDENT_T_IDENTITY", 50, 6)
    m = idhmc.GLM(X, Y, idhmc.glm.STUDENT_T_IDENTITY, STUDENT_C)      # kept alive: desc() points into its arrays
    rc, msg = _create(idhmc, m.desc())
    # a context where a device exists; otherwise idhmc_create stops at its device check, past every argument check
    assert rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg), (rc, msg)
    m = idhmc.GLM(X, Y, idhmc.glm.STUDENT_T_IDENTITY, STUDENT_C, prior_mu=1.0, prior_tau=0.25)
    rc, msg = _create(idhmc, m.desc())
    assert rc == 0 or rc == idhmc.ERR_NO_DEVICE, (rc, msg)


def test_bad_descs_are_refused_before_the_device(idhmc):
    X, Y = problem("POISSON_LOG_OFFSET", 50, 6)
    m = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG_OFFSET, constants=[1.0, 2.0])   # params = [2, 2, c0, c1 | X (300) | Y (100)]

    def refused(desc, what, opt=None):
        rc, msg = _create(idhmc, desc, opt)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (rc, msg)

    def with_params(p):
        d = m.desc()
        d.params = p.ctypes.data_as(C.POINTER(C.c_double))
        d.nparams = p.size
        return d

    for k in (0.0, 5.0, 1.5, -1.0, np.nan, np.inf):
        p = m.params.copy()
        p[0] = k
        refused(with_params(p), b"K = ")
    for nc in (-1.0, 17.0, 0.5, np.nan):
        p = m.params.copy()
        p[1] = nc
        refused(with_params(p), b"nc = ")
    d = m.desc()
    d.nparams = m.params.size - 1                                   # remainder not a multiple of D + K
    refused(d, b"multiple of D + K")
    d = m.desc()
    d.nparams = 4                                                   # no observations
    refused(d, b"multiple of D + K")
    d = m.desc()
    d.nparams = 1
    refused(d, b"begin with K and nc")
    d = m.desc()
    d.params = None
    refused(d, b"begin with K and nc")
    p = m.params.copy()
    p[3] = np.nan                                                   # c[1]
    refused(with_params(p), b"c[1] is not finite")
    p = m.params.copy()
    p[4 + 17] = np.inf                                              # X[2, 5]
    refused(with_params(p), b"X[2, 5] is not finite")
    p = m.params.copy()
    p[4 + 300 + 7] = -np.inf                                        # Y[3, 1]
    refused(with_params(p), b"Y[3, 1] is not finite")
    d = m.desc()
    d.source = None
    refused(d, b"needs HIP source")
    d = m.desc()
    d.source = b""
    refused(d, b"needs HIP source")
    tau = np.ones(6)
    tau[4] = 0.0
    d = m.desc()
    d.tau = tau.ctypes.data_as(C.POINTER(C.c_double))
    refused(d, b"tau[4]")
    mu = np.zeros(6)
    mu[1] = np.nan
    d = m.desc()
    d.mu = mu.ctypes.data_as(C.POINTER(C.c_double))
    refused(d, b"mu[1]")
    # D > 512 needs a shared metric; D > 1024 is not supported; n_pad L <= 2^27
    big = idhmc.GLM(np.ones((2, 600)), [0.0, 1.0], idhmc.glm.POISSON_LOG)
    refused(big.desc(), b"SHARED")
    assert _create(idhmc, big.desc(), idhmc.default_options(metric_mode=idhmc.METRIC_SHARED))[0] in (0, idhmc.ERR_NO_DEVICE)
    wide = idhmc.Model(idhmc.MODEL_GLM, 1100, source="x", params=np.r_[1.0, 0.0, np.zeros(1101)])
    refused(wide.desc(), b"D <= 1024")
    d = m.desc()                                                    # n_pad = 2^27 / 128 + 128 at L = 128 (refused before X is read)
    d.nparams = 4 + ((1 << 27) // 128 + 1) * 8
    refused(d, b"2^27")


@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    """each family's C restatement, compiled once per family; model() points it at a problem"""
    class R:
        def __init__(self):
            self.work = {}

        def model(self, family, X, Y, mu=None, tau=None):
            if family not in self.work:
                self.work[family] = str(tmp_path_factory.mktemp(family.lower()))
            return oracle.OracleModel.custom(X.shape[1], c_source(family), oracle_params(X, Y, constants(family), mu, tau),
                                             self.work[family])
    return R()


@pytest.mark.parametrize("family", SHIPPED + ["BERNOULLI_LOGIT"])
@pytest.mark.parametrize("n,D", [(1, 1), (37, 25), (128, 100), (1000, 100), (300, 300)])
def test_restatement_matches_the_closed_form(restated, family, n, D):
    X, Y = problem(family, n, D, seed=n + D)
    rng = np.random.default_rng(n * D)
    mu, tau = rng.standard_normal(D) * 0.3, rng.uniform(0.5, 2.0, D)
    om = restated.model(family, X, Y, mu, tau)
    for k in range(3):
        q = rng.standard_normal(D) * (0.3 + 0.5 * k) / np.sqrt(D)
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density(family, X, Y, q, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g - g_ref) <= 1e-12 * gscale + 1e-300)


@pytest.mark.parametrize("family", SHIPPED)
def test_restatement_gradient_is_the_derivative(restated, family):
    X, Y = problem(family, 200, 12, seed=11)
    om = restated.model(family, X, Y, 0.1, 0.5)
    q = np.random.default_rng(5).standard_normal(12) * 0.2
    _, g = om.logdensity_and_gradient(q)
    h = 1e-5
    for c in range(12):
        e = np.zeros(12)
        e[c] = h
        fd = (om.logdensity_and_gradient(q + e)[0] - om.logdensity_and_gradient(q - e)[0]) / (2 * h)
        assert fd == pytest.approx(g[c], rel=1e-6, abs=1e-6)


@pytest.mark.parametrize("family", SHIPPED + ["BERNOULLI_LOGIT"])
def test_restatement_is_overflow_safe(restated, family):
    """z = +-x for |x| up to 700: l and grad l finite and equal to the closed form (the Student-t also past |u| = 1e100)"""
    X = np.array([[1.0], [-1.0], [1.0], [-1.0]])
    _, Y = problem(family, 4, 1, seed=1)
    om = restated.model(family, X, Y, tau=1e-6)
    for q in (700.0, -700.0, 300.0, 40.0, 1e-3):
        lq, g = om.logdensity_and_gradient(np.array([q]))
        l_ref, g_ref, lscale, gscale = numpy_density(family, X, Y, np.array([q]), tau=np.array([1e-6]))
        assert np.isfinite(lq) and np.isfinite(g).all(), (q, lq, g)
        assert abs(lq - l_ref) <= 1e-13 * lscale and abs(g[0] - g_ref[0]) <= 1e-13 * gscale[0], (q, lq, l_ref, g, g_ref)
    if family == "STUDENT_T_IDENTITY":                  # |u| = 7e101 / sigma: the 1 / u branch
        lq, g = om.logdensity_and_gradient(np.array([7e101]))
        l_ref, g_ref, lscale, gscale = numpy_density(family, X, Y, np.array([7e101]), tau=np.array([1e-6]))
        assert np.isfinite(lq) and abs(lq - l_ref) <= 1e-13 * lscale and abs(g[0] - g_ref[0]) <= 1e-13 * gscale[0]
