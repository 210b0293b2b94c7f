"""Bayesian logistic regression (IDHMC_MODEL_LOGISTIC_REGRESSION) without a GPU: the Python constructor's validation and
packing, the C boundary's argument checks, and the density's C restatement (the arithmetic both device
forms follow bit for bit) against a numpy closed form and finite differences.

C_SRC is the restatement the GPU tests hand the oracle (tests/test_gpu_logistic.py).  Its params are
[n, mu (D), tau (D), X row-major (n x D), y (n)] -- see oracle_params()."""
import ctypes as C

import numpy as np
import pytest

C_SRC = r"""
#include "orc_math.h"
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    const long n = (long)params[0];
    const double *mu = params + 1, *tau = mu + D, *X = tau + D, *y = X + n * D;
    double T[128], A[128];
    for (int r = 0; r < 128; ++r) { T[r] = 0.0; A[r] = 0.0; }
    for (int c = 0; c < L; ++c) grad[c] = 0.0;
    for (long i = 0; i < n; ++i) {
        const double *xi = X + i * D;
        double z = 0.0;
        for (int c = 0; c < D; ++c) z = fma(xi[c], q[c], z);          /* columns ascending */
        const double s = y[i] != 0.0 ? -z : z;
        const double e = orc_exp(-fabs(s));
        const double v = (s > 0.0 ? s : 0.0) + orc_log1p(e);          /* softplus(z) - y z */
        const double sg = (s >= 0.0 ? 1.0 : e) / (1.0 + e);
        const double r = y[i] != 0.0 ? sg : -sg;                      /* y - sigma(z) */
        A[i & 127] = A[i & 127] + v;                                  /* observation blocks ascending */
        for (int c = 0; c < D; ++c) grad[c] = fma(xi[c], r, grad[c]); /* observations ascending */
    }
    for (int c = 0; c < D; ++c) {
        const double d = q[c] - mu[c];
        T[c & 127] = fma(tau[c] * d, d, T[c & 127]);
        grad[c] = fma(-tau[c], d, grad[c]);
    }
    for (int r = 0; r < 128; ++r) T[r] = fma(2.0, A[r], T[r]);
    return -0.5 * orc_tree128(T);
}
"""


def oracle_params(X, y, mu=None, tau=None):
    n, D = X.shape
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    return np.concatenate([[float(n)], mu, tau, np.asarray(X, float).ravel(), np.asarray(y, float)])


def numpy_density(X, y, q, mu=None, tau=None):
    """closed form: (l(q), grad l(q), per-coordinate magnitude of the terms summed into grad)"""
    n, D = X.shape
    mu = np.zeros(D) if mu is None else np.asarray(mu, float)
    tau = np.ones(D) if tau is None else np.asarray(tau, float)
    z = X @ q
    d = q - mu
    l = np.sum(y * z - np.logaddexp(0.0, z)) - 0.5 * np.sum(tau * d * d)
    r = y - 1.0 / (1.0 + np.exp(-z))
    g = X.T @ r - tau * d
    return l, g, np.abs(X).T @ np.abs(r) + np.abs(tau * d)


def problem(n, D, seed=3, scale=0.5):
    """synthetic data: standard normal design (first column 1), labels drawn from a logistic model"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) * scale
    X[:, 0] = 1.0
    beta = rng.standard_normal(D) / np.sqrt(D)
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    return X, y


def test_constructor_validates_shapes_and_values(idhmc):
    X, y = problem(20, 5)
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X[0], y)                         # X not a matrix
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(np.zeros((0, 5)), np.zeros(0))   # no observations
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(np.zeros((4, 0)), np.zeros(4))   # no coefficients
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(np.zeros((4, 1025)), np.zeros(4))
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X, y[:-1])
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X, np.where(y == 1, 2.0, 0.0))
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X, y - 0.5)
    Xn = X.copy()
    Xn[3, 2] = np.nan
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(Xn, y)
    Xn[3, 2] = np.inf
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(Xn, y)
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X, y, prior_tau=np.r_[1.0, 1.0, 0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X, y, prior_tau=-1.0)
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X, y, prior_tau=np.ones(4))
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X, y, prior_mu=np.ones(6))
    with pytest.raises(ValueError):
        idhmc.LogisticRegression(X, y, prior_mu=np.r_[0.0, np.inf, 0.0, 0.0, 0.0])


def test_constructor_packs_params(idhmc):
    X, y = problem(7, 3)
    m = idhmc.LogisticRegression(X, y.astype(bool), prior_mu=0.5, prior_tau=np.r_[1.0, 2.0, 3.0])
    assert m.kind == idhmc.MODEL_LOGISTIC_REGRESSION == 4 and m.D == 3 and m.n == 7
    assert np.array_equal(m.params, np.concatenate([X.ravel(), y]))
    assert m.params.size == 7 * (3 + 1)
    assert np.array_equal(m.mu, [0.5, 0.5, 0.5]) and np.array_equal(m.tau, [1.0, 2.0, 3.0])
    d = m.desc()
    assert d.kind == 4 and d.D == 3 and d.nparams == 28 and d.params[27] == y[-1] and d.tau[2] == 3.0
    m = idhmc.LogisticRegression(X, y)
    assert m.mu is None and m.tau is None
    d = m.desc()
    assert not d.mu and not d.tau


def _create(idhmc, desc, opt=None):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create(C.byref(h), 0, 4, 0, C.byref(desc), None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def test_a_valid_desc_passes_the_argument_checks(idhmc):
    X, y = problem(50, 6)
    rc, msg = _create(idhmc, idhmc.LogisticRegression(X, y).desc())
    # a context where a device exists; otherwise idhmc_create stops at its device check, past every argument check
    assert rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg), (rc, msg)
    rc, msg = _create(idhmc, idhmc.LogisticRegression(X, y, prior_mu=1.0, prior_tau=0.25).desc())
    assert rc == 0 or rc == idhmc.ERR_NO_DEVICE, (rc, msg)


def test_bad_descs_are_refused_before_the_device(idhmc):
    X, y = problem(50, 6)
    m = idhmc.LogisticRegression(X, y)

    def refused(desc, what, opt=None):
        rc, msg = _create(idhmc, desc, opt)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (rc, msg)

    d = m.desc()
    d.nparams = 50 * 7 - 1                                          # not a multiple of D + 1
    refused(d, b"multiple of D + 1")
    d = m.desc()
    d.nparams = 0
    refused(d, b"multiple of D + 1")
    d = m.desc()
    d.params = None
    refused(d, b"multiple of D + 1")
    bad = m.params.copy()
    bad[50 * 6 + 3] = 0.5                                           # y_3
    d = m.desc()
    d.params = bad.ctypes.data_as(C.POINTER(C.c_double))
    refused(d, b"neither 0 nor 1")
    bad = m.params.copy()
    bad[17] = np.inf                                                # X[2, 5]
    d = m.desc()
    d.params = bad.ctypes.data_as(C.POINTER(C.c_double))
    refused(d, b"X[2, 5] is not finite")
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
    big = idhmc.LogisticRegression(np.ones((2, 600)), [0, 1])
    refused(big.desc(), b"SHARED")
    assert _create(idhmc, big.desc(), idhmc.default_options(metric_mode=idhmc.METRIC_SHARED))[0] in (0, idhmc.ERR_NO_DEVICE)
    wide = idhmc.Model(idhmc.MODEL_LOGISTIC_REGRESSION, 1100, params=np.zeros(1101))
    refused(wide.desc(), b"D <= 1024")
    d = m.desc()                                                    # n_pad = 2^27 / 128 + 128 at L = 128 (refused before X is read)
    d.nparams = ((1 << 27) // 128 + 1) * 7
    refused(d, b"2^27")


@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    """the C restatement compiled once; set_data() points it at a problem"""
    class R:
        def __init__(self):
            self.work = str(tmp_path_factory.mktemp("logistic"))

        def model(self, X, y, mu=None, tau=None):
            return oracle.OracleModel.custom(X.shape[1], C_SRC, oracle_params(X, y, mu, tau), self.work)
    return R()


@pytest.mark.parametrize("n,D", [(1, 1), (37, 25), (128, 100), (1000, 100), (300, 300)])
def test_restatement_matches_the_closed_form(restated, n, D):
    X, y = problem(n, D, seed=n + D)
    rng = np.random.default_rng(n * D)
    mu, tau = rng.standard_normal(D) * 0.3, rng.uniform(0.5, 2.0, D)
    om = restated.model(X, y, mu, tau)
    for k in range(3):
        q = rng.standard_normal(D) * (0.5 + k)
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, scale = numpy_density(X, y, q, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * abs(l_ref)
        assert np.all(np.abs(g - g_ref) <= 1e-12 * scale + 1e-300)


def test_restatement_is_overflow_safe(restated):
    X = np.array([[1.0], [-1.0], [1.0], [-1.0]])
    y = np.array([1.0, 1.0, 0.0, 0.0])
    om = restated.model(X, y)
    for q in (800.0, -800.0, 40.0):                               # |z| past exp's overflow: softplus and sigma stay finite
        lq, g = om.logdensity_and_gradient(np.array([q]))
        l_ref = np.sum(y * X[:, 0] * q - np.logaddexp(0.0, X[:, 0] * q)) - 0.5 * q * q
        g_ref = X[:, 0] @ (y - 0.5 * (1.0 + np.tanh(0.5 * X[:, 0] * q))) - q
        assert np.isfinite(lq) and lq == pytest.approx(l_ref, rel=1e-14) and g[0] == pytest.approx(g_ref, rel=1e-14)


def test_restatement_gradient_is_the_derivative(restated):
    X, y = problem(200, 12, seed=11)
    om = restated.model(X, y, 0.1, 0.5)
    q = np.random.default_rng(5).standard_normal(12) * 0.7
    _, g = om.logdensity_and_gradient(q)
    h = 1e-5
    for c in range(12):
        e = np.zeros(12)
        e[c] = h
        fd = (om.logdensity_and_gradient(q + e)[0] - om.logdensity_and_gradient(q - e)[0]) / (2 * h)
        assert fd == pytest.approx(g[c], rel=1e-6, abs=1e-7)
