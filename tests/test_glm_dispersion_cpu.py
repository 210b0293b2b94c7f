"""Negative-binomial, gamma and beta regression (inplacedhmc_jl_amd.glm's NEG_BINOMIAL_LOG_LOGPHI, GAMMA_LOG_LOGSHAPE and
BETA_LOGIT_LOGPHI) without a GPU.  TWIN_C is the C twin of the device's dlgamma_psi (idhmc_math.hpp): section
14's definition restated operation for operation with orc_log and fma.  It lives here because oracle/orc_math.h has no gamma
function; every restatement that needs it carries it as a static function in the source handed to oracle.OracleModel.custom.

  the twin      against mpmath at 40 digits to 5e-14 (1 + |f|) over 1e-300 .. 1e300, its special values, and the recurrence
                ln Gamma(x + 1) - ln Gamma(x) = log x across the w = 8 switch;
  the sources   restated in C (OBS_C_DISP, inside test_glm_aux_cpu.C_BODY_AUX) against numpy + scipy closed forms to 1e-12 of the
                terms' magnitude, central differences in every coordinate, and a sweep over |z| <= 700 and the a0 the docstring
                of inplacedhmc_jl_amd.glm promises;
  the package   DISPERSION_SHAPES, the two response helpers, GLM(...) packing.

The GPU tests (tests/test_gpu_glm_dispersion.py) hand the same sources to the oracle."""
import numpy as np
import pytest
from scipy import special

import test_glm_aux_cpu as AUX
import test_glm_hier_cpu as HIER

TWIN_C = r"""
static void orc_lgamma_psi(double x, double *lg, double *psi)
{
    if (x != x) { *lg = x; *psi = x; return; }
    if (!(x > 0.0)) { *lg = INFINITY; *psi = NAN; return; }
    if (x == INFINITY) { *lg = x; *psi = x; return; }
    double w = x, p = 1.0, h = 0.0;
    while (w < 8.0) {
        p = p * w;
        h = h + 1.0 / w;
        w = w + 1.0;
    }
    const double lw = orc_log(w);
    const double iw = 1.0 / w;
    const double z = iw * iw;
    double S = 1.0 / 156.0;
    S = fma(S, z, -691.0 / 360360.0);
    S = fma(S, z, 1.0 / 1188.0);
    S = fma(S, z, -1.0 / 1680.0);
    S = fma(S, z, 1.0 / 1260.0);
    S = fma(S, z, -1.0 / 360.0);
    S = fma(S, z, 1.0 / 12.0);
    double T = 1.0 / 12.0;
    T = fma(T, z, -691.0 / 32760.0);
    T = fma(T, z, 1.0 / 132.0);
    T = fma(T, z, -1.0 / 240.0);
    T = fma(T, z, 1.0 / 252.0);
    T = fma(T, z, -1.0 / 120.0);
    T = fma(T, z, 1.0 / 12.0);
    *lg = w > 0x1p1000 ? w * (lw - 1.0) : (((w - 0.5) * lw - w) + 9.18938533204672741780e-01) + iw * S;
    if (x < 8.0) *lg = *lg - orc_log(p);
    *psi = ((lw - 0.5 * iw) - z * T) - h;
}
"""

# the twin by itself behind the oracle's density interface: q holds 256 arguments, grad returns ln Gamma in [0, 256) and psi in [256, 512)
TWIN_TABLE_C = r"""
#include "orc_math.h"
%s
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    for (int j = 0; j < 256; ++j) orc_lgamma_psi(q[j], &grad[j], &grad[256 + j]);
    return 0.0;
}
""" % TWIN_C

# the shipped observations and the test-only one that returns the function itself, restated in C
OBS_C_DISP = {
    "NEG_BINOMIAL_LOG_LOGPHI": TWIN_C + r"""
static void glm_observation(double z, const double *yy, const double *c, const double *a, double *r, double *v, double *s)
{
    const double y = yy[0];
    const double ph = orc_exp(a[0]);
    const double t = z - a[0];
    const double e = orc_exp(-fabs(t));
    const double sp = (t > 0.0 ? t : 0.0) + orc_log1p(e);
    const double sg = (t >= 0.0 ? 1.0 : e) / (1.0 + e);
    const double yp = y + ph;
    double l1, p1, l0, p0;
    orc_lgamma_psi(yp, &l1, &p1);
    orc_lgamma_psi(ph, &l0, &p0);
    *v = (yp * sp - y * t) - (l1 - l0);
    *r = y - yp * sg;
    s[0] = ph * ((p1 - p0) - sp) - *r;
}""",
    "GAMMA_LOG_LOGSHAPE": TWIN_C + r"""
static void glm_observation(double z, const double *y, const double *c, const double *a, double *r, double *v, double *s)
{
    const double k = orc_exp(a[0]);
    const double w = y[0] - z;
    const double E = orc_exp(w);
    const double u = (a[0] + w) - E;
    double lg, ps;
    orc_lgamma_psi(k, &lg, &ps);
    *v = lg - k * u;
    *r = k * (E - 1.0);
    s[0] = k * ((u + 1.0) - ps);
}""",
    "BETA_LOGIT_LOGPHI": TWIN_C + r"""
static void glm_observation(double z, const double *y, const double *c, const double *a, double *r, double *v, double *s)
{
    const double y0 = y[0], y1 = y[1];
    const double ph = orc_exp(a[0]);
    const double e = orc_exp(-fabs(z));
    const double d = 1.0 + e;
    const double sz = (z >= 0.0 ? 1.0 : e) / d, sn = (z >= 0.0 ? e : 1.0) / d;
    const double p = ph * sz, q = ph * sn;
    const double m = p * sn;
    double lp, pp, lq, pq, lf, pf;
    orc_lgamma_psi(p, &lp, &pp);
    orc_lgamma_psi(q, &lq, &pq);
    orc_lgamma_psi(ph, &lf, &pf);
    *v = (((lp + lq) - lf) - p * y0) - q * y1;
    *r = m * (((y0 - y1) - pp) + pq);
    s[0] = (((ph * pf - p * pp) - q * pq) + p * y0) + q * y1;
}""",
    "TEST_LGAMMA_PSI": TWIN_C + r"""
static void glm_observation(double z, const double *y, const double *c, const double *a, double *r, double *v, double *s)
{
    const double x = y[0] * orc_exp(a[0]);
    double lg, ps;
    orc_lgamma_psi(x, &lg, &ps);
    *v = lg;
    *r = 0.0;
    s[0] = -ps * x;
}""",
}
# v = ln Gamma(x), x = y exp(a0): -log p is the function itself and the score its derivative, over whatever a0 a chain holds
TEST_LGAMMA_PSI_SOURCE = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double x = o.y[0] * dexp(a[0]);
    double lg, ps;
    dlgamma_psi(x, lg, ps);
    v = lg;
    r = 0.0;
    s[0] = -ps * x;
}
"""
SHIPPED = ["NEG_BINOMIAL_LOG_LOGPHI", "GAMMA_LOG_LOGSHAPE", "BETA_LOGIT_LOGPHI"]
SHAPE = {"NEG_BINOMIAL_LOG_LOGPHI": (1, 0, 1), "GAMMA_LOG_LOGSHAPE": (1, 0, 1), "BETA_LOGIT_LOGPHI": (2, 0, 1),
         "TEST_LGAMMA_PSI": (1, 0, 1)}                 # K, nc, A
TRUE_A = {"NEG_BINOMIAL_LOG_LOGPHI": np.log(3.0), "GAMMA_LOG_LOGSHAPE": np.log(2.0), "BETA_LOGIT_LOGPHI": np.log(8.0)}


def source(idhmc, family):
    return TEST_LGAMMA_PSI_SOURCE if family == "TEST_LGAMMA_PSI" else getattr(idhmc.glm, family)


def c_source_disp(family):
    return AUX.C_BODY_AUX % OBS_C_DISP[family]


def c_source_disp_hier(family):
    return HIER.C_BODY_HIER % OBS_C_DISP[family]


def make(idhmc, family, X, Y, mu=None, tau=None, groups=None):
    return idhmc.GLM(X, Y, source(idhmc, family), None, mu, tau, aux=1, groups=groups)


def response(family, z, rng):
    """Y from the family's own model at TRUE_A with linear predictor z"""
    d = np.exp(TRUE_A[family])
    if family == "NEG_BINOMIAL_LOG_LOGPHI":
        return rng.negative_binomial(d, d / (d + np.exp(z))).astype(float)
    if family == "GAMMA_LOG_LOGSHAPE":
        return np.log(rng.gamma(d, np.exp(z) / d))
    m = special.expit(z)
    y = np.clip(rng.beta(d * m, d * (1.0 - m)), 1e-12, 1.0 - 1e-12)
    return np.stack([np.log(y), np.log1p(-y)], 1)


def problem_disp(family, n, Dx, seed=3, scale=0.5):
    """design with a first column of ones, coefficients ~ N(0, 1 / Dx)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, Dx)) * scale
    X[:, 0] = 1.0
    return X, response(family, X @ (rng.standard_normal(Dx) / np.sqrt(Dx)), rng)


def start_disp(family, C, Dx, seed=0, scale=0.3):
    """small coefficients, a0 around TRUE_A"""
    rng = np.random.default_rng(seed + Dx)
    return np.concatenate([rng.uniform(-scale, scale, (C, Dx)) / np.sqrt(Dx), TRUE_A[family] + rng.uniform(-0.2, 0.2, (C, 1))], 1)


def numpy_terms_disp(family, z, Y, a0):
    """closed form per observation: (log p, d log p / dz, d log p / da0, magnitude of log p's terms, of r's terms, of the score's),
    each magnitude the sum of the absolute values of the terms the source adds, the |ln Gamma| and phi |psi| ones included"""
    Y = np.asarray(Y, float).reshape(z.size, -1)
    gl, dg = special.gammaln, special.digamma
    if family == "NEG_BINOMIAL_LOG_LOGPHI":
        y, ph, t = Y[:, 0], np.exp(a0), z - a0
        sp, sg = np.logaddexp(0.0, t), special.expit(t)
        lp = gl(y + ph) - gl(ph) - (y + ph) * sp + y * t
        r = y - (y + ph) * sg
        return (lp, r, ph * (dg(y + ph) - dg(ph) - sp) - r, np.abs(gl(y + ph)) + np.abs(gl(ph)) + (y + ph) * sp + y * np.abs(t),
                y + (y + ph) * sg, ph * (np.abs(dg(y + ph)) + np.abs(dg(ph)) + sp) + y + (y + ph) * sg)
    if family == "GAMMA_LOG_LOGSHAPE":
        k, w = np.exp(a0), Y[:, 0] - z
        E = np.exp(w)
        return (k * (a0 + w - E) - gl(k), k * (E - 1.0), k * (a0 + w - E + 1.0 - dg(k)), k * (abs(a0) + np.abs(w) + E) + abs(gl(k)),
                k * (E + 1.0), k * (abs(a0) + np.abs(w) + E + 1.0 + abs(dg(k))))
    if family == "BETA_LOGIT_LOGPHI":
        y0, y1, ph = Y[:, 0], Y[:, 1], np.exp(a0)
        sz, sn = special.expit(z), special.expit(-z)
        p, q = ph * sz, ph * sn
        m = p * sn
        return (gl(ph) - gl(p) - gl(q) + p * y0 + q * y1, m * (y0 - y1 - dg(p) + dg(q)), ph * dg(ph) - p * dg(p) - q * dg(q) + p * y0 + q * y1,
                abs(gl(ph)) + np.abs(gl(p)) + np.abs(gl(q)) + p * np.abs(y0) + q * np.abs(y1),
                m * (np.abs(y0) + np.abs(y1) + np.abs(dg(p)) + np.abs(dg(q))),
                ph * abs(dg(ph)) + p * np.abs(dg(p)) + q * np.abs(dg(q)) + p * np.abs(y0) + q * np.abs(y1))
    x = Y[:, 0] * np.exp(a0)
    return -gl(x), 0.0 * x, -dg(x) * x, np.abs(gl(x)), 0.0 * x, np.abs(dg(x) * x)


def numpy_density_disp(family, X, Y, q, mu=None, tau=None, grp=None):
    """(l(q), grad l(q), magnitude of l's terms, per-coordinate magnitude of the terms summed into grad); q = [beta | a0], or
    [u | a0 | omega] with coefficient groups grp"""
    n, Dx = X.shape
    D = q.size
    H = D - Dx - 1
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    s = np.where(grp >= 0, np.exp(q[Dx + 1:])[np.maximum(grp, 0)], 1.0) if H else np.ones(Dx)
    b = s * q[:Dx]
    lp, r, sc, mag, rmag, smag = numpy_terms_disp(family, X @ b, Y, q[Dx])
    G, Gmag = X.T @ r, np.abs(X).T @ rmag
    d = q - mu
    g = np.concatenate([s * G, [sc.sum()], [np.sum((G * b)[grp == k]) for k in range(H)]]) - tau * d
    gscale = np.concatenate([s * Gmag, [smag.sum()], [np.sum((Gmag * np.abs(b))[grp == k]) for k in range(H)]]) + np.abs(tau * d)
    return np.sum(lp) - 0.5 * np.sum(tau * d * d), g, np.sum(mag) + 0.5 * np.sum(tau * d * d), gscale


# ---- the twin ------------------------------------------------------------------------------------------------------------------------
def twin_points():
    """log-uniform over 1e-300 .. 1e300, dense in (0.01, 12), and the points where something changes: 1, 2 (the zeros of ln Gamma),
    the zero of psi, every integer up to 9 (a shift count each), both sides of the w = 8 switch, the ends"""
    rng = np.random.default_rng(14)
    special_points = [1.0, 2.0, 1.4616321449683623, np.nextafter(8.0, 0.0), 8.0, np.nextafter(8.0, 9.0), 1e-300, 1e300, 3.0, 4.0, 5.0,
                      6.0, 7.0, 9.0, np.nextafter(1.0, 0.0), np.nextafter(7.0, 0.0), 0.5]
    return np.concatenate([special_points, 10.0 ** rng.uniform(-300.0, 300.0, 10000), rng.uniform(0.01, 12.0, 12000),
                           10.0 ** rng.uniform(-3.0, 3.0, 2000)])


@pytest.fixture(scope="module")
def twin(oracle, tmp_path_factory):
    om = oracle.OracleModel.custom(512, TWIN_TABLE_C, np.zeros(1), str(tmp_path_factory.mktemp("twin")))

    def evaluate(x):
        x = np.asarray(x, float)
        lg, ps = np.empty(x.size), np.empty(x.size)
        for k in range(0, x.size, 256):
            q = np.ones(512)
            m = min(256, x.size - k)
            q[:m] = x[k:k + m]
            g = om.logdensity_and_gradient(q)[1]
            lg[k:k + m], ps[k:k + m] = g[:m], g[256:256 + m]
        return lg, ps
    return evaluate


def test_twin_accuracy(twin):
    """5e-14 (1 + |f|) against mpmath at 40 digits: about 9 times what the same shape gives with libm's log (worst
    5.6e-15 for ln Gamma, 1.7e-15 for psi), the room for orc_log differing from libm in the last place"""
    import mpmath                                        # here, so that the GPU tests' import of this module does not need it
    x = twin_points()
    assert x.size >= 20000
    lg, ps = twin(x)
    mpmath.mp.dps = 40
    worst = [0.0, 0.0]
    for xi, l, p in zip(x, lg, ps):
        X = mpmath.mpf(float(xi))
        for k, (got, ref) in enumerate(((l, mpmath.loggamma(X)), (p, mpmath.digamma(X)))):
            worst[k] = max(worst[k], float(abs(mpmath.mpf(float(got)) - ref) / (1 + abs(ref))))
    print("worst |error| / (1 + |f|): ln Gamma %.3g, psi %.3g over %d points" % (worst[0], worst[1], x.size))
    assert worst[0] <= 5e-14 and worst[1] <= 5e-14, worst


def test_twin_special_values(twin):
    lg, ps = twin([np.nan, 0.0, -0.0, -1.5, -np.inf, np.inf, 1.0, 2.0])
    assert np.isnan(lg[0]) and np.isnan(ps[0])
    assert np.all(lg[1:5] == np.inf) and np.isnan(ps[1:5]).all()
    assert lg[5] == np.inf and ps[5] == np.inf
    assert abs(lg[6]) <= 5e-14 and abs(lg[7]) <= 5e-14
    assert abs(ps[6] + 0.5772156649015329) <= 5e-14 * 1.6 and abs(ps[7] - 0.42278433509846713) <= 5e-14 * 1.5


def test_twin_recurrence_across_the_switch(twin):
    """ln Gamma(x + 1) - ln Gamma(x) = log x and psi(x + 1) - psi(x) = 1 / x with x below and x + 1 above the w = 8 switch (and both
    below, both above): each side is within 5e-14 (1 + |f|), so is the difference of the two"""
    x = np.concatenate([np.linspace(6.0, 9.0, 193), [np.nextafter(7.0, 0.0), 7.0, np.nextafter(8.0, 0.0), 8.0]])
    l0, p0 = twin(x)
    l1, p1 = twin(x + 1.0)
    assert np.all(np.abs((l1 - l0) - np.log(x)) <= 5e-14 * (2.0 + np.abs(l0) + np.abs(l1)))
    assert np.all(np.abs((p1 - p0) - 1.0 / x) <= 5e-14 * (2.0 + np.abs(p0) + np.abs(p1)))


# ---- the package ---------------------------------------------------------------------------------------------------------------------
def test_shipped_sources_declare_their_shapes(idhmc):
    assert set(idhmc.glm.DISPERSION_SHAPES) == set(SHIPPED)
    for name, (K, nc, A) in idhmc.glm.DISPERSION_SHAPES.items():
        src = getattr(idhmc.glm, name)
        assert (K, nc, A) == SHAPE[name] and A == 1 and nc == 0
        assert "glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)" in src
        assert ("o.y[%d]" % (K - 1)) in src and ("o.y[%d]" % K) not in src and "o.c[" not in src
        assert "a[0]" in src and "s[0]" in src and "a[1]" not in src and "s[1]" not in src and "dlgamma_psi(" in src
    doc = idhmc.glm.__doc__
    assert all(n in doc for n in SHIPPED) and all(w in doc for w in ("dlgamma_psi", "dlgamma", "ddigamma", "Poisson limit"))
    assert set(idhmc.glm.SHAPES).isdisjoint(SHIPPED) and set(idhmc.glm.AUX_SHAPES).isdisjoint(SHIPPED)


def test_response_helpers(idhmc):
    y = np.array([0.25, 1.0, 7.5, 1e-300, 1e300])
    assert np.array_equal(idhmc.glm.gamma_response(y), np.log(y)) and idhmc.glm.gamma_response(list(y)).shape == (5,)
    u = np.array([0.25, 0.5, 1e-300, 1.0 - 2.0 ** -53])
    Y = idhmc.glm.beta_response(u)
    assert Y.shape == (4, 2) and np.array_equal(Y[:, 0], np.log(u)) and np.array_equal(Y[:, 1], np.log1p(-u)) and np.isfinite(Y).all()
    for bad in ([1.0, 0.0], [1.0, -2.0], [1.0, np.nan], [1.0, np.inf], [], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="gamma_response"):
            idhmc.glm.gamma_response(bad)
    for bad in ([0.5, 0.0], [0.5, 1.0], [0.5, -0.1], [0.5, 1.5], [0.5, np.nan], [0.5, np.inf], [], [[0.5, 0.5]]):
        with pytest.raises(ValueError, match="beta_response"):
            idhmc.glm.beta_response(bad)
    with pytest.raises(ValueError, match="finite and > 0"):
        idhmc.glm.gamma_response([0.0])
    with pytest.raises(ValueError, match="strictly between 0 and 1"):
        idhmc.glm.beta_response([1.0])


@pytest.mark.parametrize("family", SHIPPED)
def test_constructor_packs_each_family(idhmc, family):
    X, Y = problem_disp(family, 9, 4)
    K = SHAPE[family][0]
    m = make(idhmc, family, X, Y, 0.5, np.arange(1.0, 6.0))
    assert m.kind == idhmc.MODEL_GLM_AUX and m.D == 5 and (m.Dx, m.A, m.n, m.K, m.nc) == (4, 1, 9, K, 0)
    assert np.array_equal(m.params, np.concatenate([[float(K), 0.0, 1.0], X.ravel(), np.asarray(Y).ravel()]))
    assert (m.params.size - 3) // (m.Dx + m.K) == 9 and m.tau[4] == 5.0
    g = make(idhmc, family, X, Y, groups=[-1, 0, 0, 0])
    assert (g.D, g.Dx, g.A, g.H, g.n) == (6, 4, 1, 1, 9)
    if family == "GAMMA_LOG_LOGSHAPE":
        assert np.array_equal(idhmc.GLM(X, idhmc.glm.gamma_response(np.exp(Y)), idhmc.glm.GAMMA_LOG_LOGSHAPE, aux=1).params[:3], [1.0, 0.0, 1.0])


# ---- the restatements ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    """each family's C restatement, compiled once per family; model() points it at a problem"""
    class R:
        def __init__(self):
            self.work = {}

        def model(self, family, X, Y, mu=None, tau=None):
            if family not in self.work:
                self.work[family] = str(tmp_path_factory.mktemp(family.lower()))
            return oracle.OracleModel.custom(X.shape[1] + 1, c_source_disp(family), AUX.oracle_params_aux(X, Y, 1, None, mu, tau), self.work[family])
    return R()


@pytest.mark.parametrize("family", SHIPPED)
@pytest.mark.parametrize("n,Dx", [(1, 1), (37, 25), (130, 100), (1000, 127), (300, 300)])
def test_restatement_matches_the_closed_form(restated, family, n, Dx):
    """a0 = TRUE_A +- 0.2 and -5, 0, 5: within |a0| <= 5 scipy's own error stays below 1e-12 of the ln Gamma and phi psi terms"""
    X, Y = problem_disp(family, n, Dx, seed=n + Dx)
    rng = np.random.default_rng(n * Dx)
    mu, tau = rng.standard_normal(Dx + 1) * 0.3, rng.uniform(0.5, 2.0, Dx + 1)
    om = restated.model(family, X, Y, mu, tau)
    qs = [start_disp(family, 1, Dx, seed=k, scale=0.3 + 0.5 * k)[0] for k in range(3)]
    for a0 in (-5.0, 0.0, 5.0):
        qs.append(np.r_[qs[0][:Dx], a0])
    for q in qs:
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_disp(family, X, Y, q, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (q[Dx], lq, l_ref)
        assert np.all(np.abs(g - g_ref) <= 1e-12 * gscale + 1e-300), (q[Dx], np.abs(g - g_ref) / gscale)


@pytest.mark.parametrize("family", SHIPPED)
def test_restatement_gradient_is_the_derivative(restated, family):
    """central differences in every coordinate, the log dispersion included"""
    X, Y = problem_disp(family, 200, 12, seed=11)
    om = restated.model(family, X, Y, 0.1, 0.5)
    q = start_disp(family, 1, 12, seed=5)[0]
    _, g = om.logdensity_and_gradient(q)
    h = 1e-5
    for c in range(13):
        e = np.zeros(13)
        e[c] = h
        fd = (om.logdensity_and_gradient(q + e)[0] - om.logdensity_and_gradient(q - e)[0]) / (2 * h)
        assert fd == pytest.approx(g[c], rel=1e-6, abs=1e-6), c


# (z, a0) inside what the docstring of inplacedhmc_jl_amd.glm promises.  Negative binomial: every |z|, |a0| <= 700.  Gamma: w = log y - z
# and a0 + w below 709.78, so a0 is bounded by z where z is very negative (the filter in the test applies this problem's log y).
# Beta: -|z| + a0 > -708 keeps p and q normal numbers.
_Z = (700.0, -700.0, 300.0, -300.0, 40.0, 1e-3)
SWEEP = {"NEG_BINOMIAL_LOG_LOGPHI": [(z, a) for z in _Z for a in (-700.0, -300.0, -40.0, -5.0, 0.0, 5.0, 40.0, 300.0, 700.0)],
         "GAMMA_LOG_LOGSHAPE": [(z, a) for z in _Z for a in (-700.0, -300.0, -40.0, -5.0, 0.0, 5.0, 40.0, 300.0, 700.0)],
         "BETA_LOGIT_LOGPHI": [(z, a) for z in (700.0, -700.0) for a in (-5.0, 0.0, 5.0, 300.0, 700.0)] +
                              [(z, a) for z in (300.0, -300.0) for a in (-400.0, -5.0, 0.0, 5.0, 700.0)] +
                              [(z, a) for z in (40.0, 1e-3) for a in (-650.0, -40.0, -5.0, 0.0, 5.0, 40.0, 650.0)]}


@pytest.mark.parametrize("family", SHIPPED)
def test_restatement_is_finite_wherever_the_density_is(restated, family):
    """z = +-x: l and grad l finite over the promised range, and equal to the closed form (1e-12 of the terms' magnitude) where
    |a0| <= 5; past that scipy's ln Gamma and psi are no reference at that precision"""
    X = np.array([[1.0], [-1.0], [1.0], [-1.0]])
    _, Y = problem_disp(family, 4, 1, seed=1)
    tau = np.array([1e-6, 1e-6])
    om = restated.model(family, X, Y, tau=tau)
    checked = compared = 0
    for z, a0 in SWEEP[family]:
        if family == "GAMMA_LOG_LOGSHAPE":
            w = np.asarray(Y).reshape(-1).max() + abs(z)
            if w >= 709.0 or a0 + w >= 709.0:
                continue                                                # outside the promise (this problem's log y)
        q = np.array([z, a0])
        lq, g = om.logdensity_and_gradient(q)
        assert np.isfinite(lq) and np.isfinite(g).all(), (q, lq, g)
        checked += 1
        if abs(a0) <= 5.0:
            l_ref, g_ref, lscale, gscale = numpy_density_disp(family, X, Y, q, tau=tau)
            assert abs(lq - l_ref) <= 1e-12 * lscale and np.all(np.abs(g - g_ref) <= 1e-12 * gscale + 1e-300), (q, lq, l_ref, g, g_ref)
            compared += 1
    assert checked >= 25 and compared >= 6


@pytest.mark.parametrize("family", SHIPPED)
def test_past_the_promise_the_density_is_minus_infinity(oracle, restated, family):
    """a0 = -800: the dispersion exp(a0) is 0, ln Gamma(0) = +inf, v is +inf or NaN (inf - inf where the other ln Gamma is +inf too),
    which a chain reads as l(q) = -inf: the rejected point.  The same at a0 = 720, where exp(a0) is +inf."""
    X, Y = problem_disp(family, 40, 3, seed=2)
    om = restated.model(family, X, Y)
    ch = oracle.OracleChain(om, seed=1, chain_id=0)
    for a0 in (-800.0, 720.0):
        q = np.array([0.1, 0.2, -0.1, a0])
        assert not np.isfinite(om.logdensity_and_gradient(q)[0])
        ch.set_q(q)
        assert ch.lq == -np.inf


def test_negative_binomial_with_groups_matches_the_closed_form(oracle, tmp_path):
    """the twin inside test_glm_hier_cpu.C_BODY_HIER: a random-intercept block of 8 one-hot columns beside 4 ungrouped ones"""
    family, n, Dx = "NEG_BINOMIAL_LOG_LOGPHI", 130, 12
    grp = HIER.blocks(Dx, 1, 8)
    X, Y, mu, tau = problem_grouped(n, Dx, grp)
    om = oracle.OracleModel.custom(Dx + 2, c_source_disp_hier(family), HIER.oracle_params_hier(X, Y, 1, grp, None, mu, tau), str(tmp_path))
    for q in start_grouped(3, Dx):
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_disp(family, X, Y, q, mu, tau, grp)
        assert abs(lq - l_ref) <= 1e-12 * lscale and np.all(np.abs(g - g_ref) <= 1e-12 * gscale + 1e-300)


def problem_grouped(n, Dx, grp, seed=4):
    """negative-binomial counts from a design with one one-hot block (HIER.design), effects of scale 0.6; a prior over u, a0, omega"""
    rng = np.random.default_rng(seed)
    X = HIER.design(n, Dx, grp, True, rng)
    beta = np.where(grp >= 0, 0.6 * rng.standard_normal(Dx), rng.standard_normal(Dx) / np.sqrt(Dx))
    Y = response("NEG_BINOMIAL_LOG_LOGPHI", X @ beta, rng)
    return X, Y, rng.standard_normal(Dx + 2) * 0.2, rng.uniform(0.5, 2.0, Dx + 2)


def start_grouped(C, Dx, seed=0):
    rng = np.random.default_rng(seed + Dx)
    return np.concatenate([rng.uniform(-0.3, 0.3, (C, Dx)), TRUE_A["NEG_BINOMIAL_LOG_LOGPHI"] + rng.uniform(-0.2, 0.2, (C, 1)),
                           HIER.OMEGA0 + rng.uniform(-0.3, 0.3, (C, 1))], 1)
