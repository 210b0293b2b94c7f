"""Priors beyond the Gaussian (GLM(..., prior_kind=, prior_nu=), idhmc_create_glm_priors) without a GPU: the
constructor's validation, glm.priors and its specs, the C boundary's argument checks through both forms of the entry point (one
response: M = 1, chains_per_response = 0; several), and the C restatement of section 18's table against closed-form log densities from
scipy.stats, central differences in every non-Gaussian coordinate, and, with every kind 0, the bits of section 13's restatement.

The restatement is C_BODY_HIER of tests/test_glm_hier_cpu.py with kind (D) and nu (D) added to its params and the table in its last
loop: params are [n, K, nc, A, H, mu (D), tau (D), kind (D, as doubles), nu (D), c (nc), grp (Dx, as doubles), X row-major (n x Dx),
Y row-major (n x K)], D = Dx + A + H.  The GPU tests (tests/test_gpu_glm_priors.py) hand the same source to the oracle."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import test_glm_hier_cpu as HIER
from test_glm_hier_cpu import SHAPE, consts, numpy_density_hier, source

NORMAL, STUDENT_T, LOG_HALF_NORMAL, LOG_HALF_STUDENT_T, LOG_EXPONENTIAL = range(5)

C_BODY_PRIORS = r"""
#include "orc_math.h"
%s
/* params: [n, K, nc, A, H, mu (D), tau (D), kind (D), nu (D), c (nc), grp (Dx, as doubles), X row-major (n x Dx), Y row-major (n x K)] */
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    const long n = (long)params[0];
    const int K = (int)params[1], nc = (int)params[2], A = (int)params[3], H = (int)params[4], Dx = D - A - H;
    const double *mu = params + 5, *tau = mu + D, *kind = tau + D, *nu = kind + D, *c = nu + D, *grp = c + nc, *X = grp + Dx, *Y = X + n * Dx;
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
        const double d = q[j] - mu[j], G = grad[j], t = tau[j], f = nu[j];
        const int k = (int)kind[j], r = j & 127;
        if (k == 0) {
            T[r] = fma(t * d, d, T[r]);
            grad[j] = fma(-t, d, G);
        } else if (k == 1) {
            const double w = t * d, s = w * d;
            T[r] = T[r] + (f + 1.0) * orc_log1p(s / f);
            grad[j] = G + (-((f + 1.0) * w) / (f + s));
        } else if (k == 2) {
            const double x = orc_exp(2.0 * d);
            T[r] = T[r] + (x - 2.0 * d);
            grad[j] = G + (1.0 - x);
        } else if (k == 3) {
            const double x = orc_exp(2.0 * d);
            T[r] = T[r] + ((f + 1.0) * orc_log1p(x / f) - 2.0 * d);
            grad[j] = G + (1.0 - ((f + 1.0) * x) / (f + x));
        } else {
            const double x = orc_exp(d);
            T[r] = T[r] + 2.0 * (x - d);
            grad[j] = G + (1.0 - x);
        }
    }
    for (int r = 0; r < 128; ++r) T[r] = fma(2.0, V[r], T[r]);
    return -0.5 * orc_tree128(T);
}
"""


def c_source_priors(family):
    """C_BODY_PRIORS around the family's observation, as HIER.c_source_hier builds C_BODY_HIER"""
    body = HIER.c_source_hier(family)
    head, tail = HIER.C_BODY_HIER.split("%s")
    assert body.startswith(head) and body.endswith(tail)
    return C_BODY_PRIORS % body[len(head):len(body) - len(tail)]


def oracle_params_priors(X, Y, A, grp, kind, nu, c=None, mu=None, tau=None):
    n, Dx = X.shape
    grp = np.full(Dx, -1) if grp is None else np.asarray(grp)
    H = int(grp.max()) + 1
    D = Dx + A + H
    Y = np.asarray(Y, float).reshape(n, -1)
    c = np.zeros(0) if c is None else np.asarray(c, float)
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    kind = np.broadcast_to(np.asarray(kind, float), (D,))
    nu = np.broadcast_to(np.asarray(nu, float), (D,))
    return np.concatenate([[float(n), float(Y.shape[1]), float(c.size), float(A), float(H)], mu, tau, kind, nu, c, grp.astype(float),
                           np.asarray(X, float).ravel(), Y.ravel()])


def numpy_prior(kind, nu, mu, tau, q):
    """per coordinate: log prior up to a constant, its derivative, and the magnitude of the terms of each"""
    d = q - mu
    nu1 = np.where(nu > 0, nu, 1.0)
    e2, e1 = np.exp(2.0 * d), np.exp(d)
    s = tau * d * d
    lp = [-0.5 * s, -0.5 * (nu1 + 1.0) * np.log1p(s / nu1), -0.5 * e2 + d, -0.5 * (nu1 + 1.0) * np.log1p(e2 / nu1) + d, -e1 + d]
    lmag = [0.5 * s, 0.5 * (nu1 + 1.0) * np.log1p(s / nu1), 0.5 * e2 + np.abs(d), 0.5 * (nu1 + 1.0) * np.log1p(e2 / nu1) + np.abs(d),
            e1 + np.abs(d)]
    g = [-tau * d, -(nu1 + 1.0) * tau * d / (nu1 + s), 1.0 - e2, 1.0 - (nu1 + 1.0) * e2 / (nu1 + e2), 1.0 - e1]
    gmag = [np.abs(tau * d), np.abs(g[1]), 1.0 + e2, 1.0 + np.abs(g[3] - 1.0), 1.0 + e1]
    k = np.asarray(kind, int)
    pick = lambda rows: np.choose(k, rows)
    return pick(lp), pick(g), pick(lmag), pick(gmag)


def numpy_density_priors(family, X, Y, q, grp, kind, nu, mu=None, tau=None):
    """numpy_density_hier with the table's priors in the place of the Gaussian one: (l, grad, magnitude of l's terms, per-coordinate
    magnitude of the gradient's terms)"""
    D = q.size
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    l0, g0, ls0, gs0 = numpy_density_hier(family, X, Y, q, grp, mu, tau)
    d = q - mu
    # take the Gaussian prior out again, term by term (it was added in exactly this form)
    like_l, like_g = l0 + 0.5 * np.sum(tau * d * d), g0 + tau * d
    like_ls, like_gs = ls0 - 0.5 * np.sum(tau * d * d), gs0 - np.abs(tau * d)
    lp, gp, lmag, gmag = numpy_prior(np.broadcast_to(kind, (D,)), np.broadcast_to(np.asarray(nu, float), (D,)), mu, tau, q)
    return like_l + lp.sum(), like_g + gp, like_ls + lmag.sum() + 0.5 * np.sum(tau * d * d), like_gs + gmag + np.abs(tau * d)


def mixed_priors(Dx, A, H, rng=None):
    """(kind, nu, mu, tau) with coefficients alternating NORMAL and STUDENT_T and the log coordinates cycling through the log kinds"""
    D = Dx + A + H
    rng = np.random.default_rng(Dx + 7 * A + 13 * H) if rng is None else rng
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:Dx:2] = STUDENT_T
    for k, c in enumerate(range(Dx, D)):
        kind[c] = (LOG_HALF_STUDENT_T, LOG_EXPONENTIAL, LOG_HALF_NORMAL, NORMAL)[k % 4]
    takes = (kind == STUDENT_T) | (kind == LOG_HALF_STUDENT_T)
    nu[takes] = rng.choice([1.0, 3.0, 4.5, 30.0], int(takes.sum()))
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[kind >= LOG_HALF_NORMAL] = 1.0
    return kind, nu, mu, tau


def make(idhmc, family, X, Y, grp, kind, nu, mu=None, tau=None, **kw):
    return idhmc.GLM(X, Y, source(idhmc, family), consts(family), mu, tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu, **kw)


# ---- the constructor ---------------------------------------------------------------------------------------------------------------
def _data(family="GAUSSIAN_IDENTITY_LOGSIGMA", n=9, Dx=6):
    grp = np.array([-1, 0, 1, 0, -1, 1][:Dx])
    return HIER.problem_hier(family, n, Dx, grp, False) + (grp,)


def test_constructor_keeps_the_priors(idhmc):
    X, Y, grp = _data()
    g = idhmc.glm
    assert (g.PRIOR_NORMAL, g.PRIOR_STUDENT_T, g.PRIOR_LOG_HALF_NORMAL, g.PRIOR_LOG_HALF_STUDENT_T, g.PRIOR_LOG_EXPONENTIAL) == (0, 1, 2, 3, 4)
    kind = [0, 1, "STUDENT_T", 0, "PRIOR_NORMAL", 1, g.PRIOR_LOG_HALF_STUDENT_T, "LOG_EXPONENTIAL", np.int64(2)]
    nu = [0, 3, 1, 0, 0, 2.5, 4, 0, 0]
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=grp, prior_kind=kind, prior_nu=nu)
    assert m.prior_kind.dtype == np.int32 and list(m.prior_kind) == [0, 1, 1, 0, 0, 1, 3, 4, 2]
    assert m.prior_nu.dtype == np.float64 and list(m.prior_nu) == [0, 3, 1, 0, 0, 2.5, 4, 0, 0]
    assert m.D == 9 and (m.Dx, m.A, m.H) == (6, 1, 2) and m.kind == idhmc.MODEL_GLM_AUX
    # scalars: one kind and one nu for every coordinate (a model without log coordinates)
    X5, Y5 = X[:, :5], (Y > 0).astype(float)
    m = idhmc.GLM(X5, Y5, g.BERNOULLI_LOGIT, prior_kind="STUDENT_T", prior_nu=3)
    assert list(m.prior_kind) == [1] * 5 and list(m.prior_nu) == [3.0] * 5 and m.kind == idhmc.MODEL_GLM
    d = m.glm_desc()                                    # handed over in parts: idhmc_create_glm_priors takes a descriptor
    assert (d.n, d.Dx, d.K, d.nc, d.A, d.H) == (9, 5, 1, 0, 0, 0) and not d.groups
    # without the keywords the attributes are None
    m = idhmc.GLM(X5, Y5, g.BERNOULLI_LOGIT)
    assert m.prior_kind is None and m.prior_nu is None


def test_all_normal_kinds_are_the_model_without_them(idhmc):
    """every kind 0 packs what GLM() always packed, byte for byte, and keeps what was given"""
    X, Y, _ = _data("POISSON_LOG")
    plain = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, prior_mu=0.5, prior_tau=2.0)
    for kw in ({"prior_kind": 0}, {"prior_kind": [0] * 6, "prior_nu": 0.0}, {"prior_kind": "NORMAL", "prior_nu": np.zeros(6)}):
        m = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, prior_mu=0.5, prior_tau=2.0, **kw)
        assert m.kind == plain.kind and m.params.tobytes() == plain.params.tobytes() and m.mu.tobytes() == plain.mu.tobytes()
        assert list(m.prior_kind) == [0] * 6 and list(m.prior_nu) == [0.0] * 6


def test_constructor_validates_priors(idhmc):
    X, Y, grp = _data()
    src = idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA            # D = 6 + 1 + 2; coordinates 6, 7, 8 are logarithms
    ok = [0, 1, 0, 1, 0, 0, 3, 4, 2]
    oknu = [0, 3, 0, 1, 0, 0, 4, 0, 0]

    def bad(what, kind=ok, nu=oknu, **kw):
        with pytest.raises(ValueError, match=what):
            idhmc.GLM(X, Y, src, aux=1, groups=grp, prior_kind=kind, prior_nu=nu, **kw)

    def at(seq, c, v):
        out = list(seq)
        out[c] = v
        return out
    assert idhmc.GLM(X, Y, src, aux=1, groups=grp, prior_kind=ok, prior_nu=oknu).D == 9
    bad("prior_nu needs prior_kind", kind=None)
    for shape in ([0] * 8, [0] * 10, [[0] * 9]):
        bad("prior_kind must be a scalar or have one entry per sampled coordinate", kind=shape, nu=None)
    for shape in ([0.0] * 8, [[0.0] * 9]):
        bad("prior_nu must be a scalar or have one entry per sampled coordinate", nu=shape)
    for k in (-1, 5, 100, 1.0, True, None, "CAUCHY", "student_t"):
        bad(r"prior_kind\[3\]", kind=at(ok, 3, k))
    for v in (0.0, -1.0, np.inf, np.nan):
        bad(r"prior_nu\[1\] = .* must be finite and > 0 \(PRIOR_STUDENT_T\)", nu=at(oknu, 1, v))
        bad(r"prior_nu\[6\] = .* must be finite and > 0 \(PRIOR_LOG_HALF_STUDENT_T\)", nu=at(oknu, 6, v))
    bad(r"prior_nu\[1\]", nu=None)                      # a t kind without any nu
    for c, name in ((0, "NORMAL"), (8, "LOG_HALF_NORMAL"), (7, "LOG_EXPONENTIAL")):
        bad(r"prior_nu\[%d\] = .* must be 0 \(PRIOR_%s takes no nu\)" % (c, name), nu=at(oknu, c, 2.0))
    for k in (2, 3, 4):
        bad(r"prior_kind\[5\] = PRIOR_.* coordinate 5 is a coefficient, not a logarithm", kind=at(ok, 5, k), nu=at(oknu, 5, 3.0 if k == 3 else 0.0))
    for c in (6, 7, 8):
        bad(r"prior_tau\[%d\] = .* must be 1" % c, prior_tau=at([1.0] * 9, c, 2.0))
    idhmc.GLM(X, Y, src, aux=1, groups=grp, prior_kind=ok, prior_nu=oknu, prior_tau=at([1.0] * 9, 1, 2.0))      # a t kind takes any tau
    bad("prior_tau must be finite and > 0", prior_tau=at([1.0] * 9, 1, 0.0))                                      # what GLM() always refused


def test_prior_specs_and_the_builder(idhmc):
    g = idhmc.glm
    assert tuple(g.normal()) == (0, 0.0, 1.0, 0.0) and tuple(g.normal(1.5, 0.5)) == (0, 1.5, 4.0, 0.0)
    assert tuple(g.student_t(3)) == (1, 0.0, 1.0, 3.0) and tuple(g.student_t(1, -2.0, 4.0)) == (1, -2.0, 0.0625, 1.0)
    assert tuple(g.half_normal()) == (2, 0.0, 1.0, 0.0) and tuple(g.half_normal(2.0)) == (2, np.log(2.0), 1.0, 0.0)
    assert tuple(g.half_student_t(4)) == (3, 0.0, 1.0, 4.0) and tuple(g.half_student_t(1, 0.5)) == (3, np.log(0.5), 1.0, 1.0)
    assert tuple(g.exponential()) == (4, 0.0, 1.0, 0.0) and tuple(g.exponential(3.0)) == (4, np.log(3.0), 1.0, 0.0)
    for f, args in ((g.normal, (0, 0)), (g.normal, (np.nan, 1)), (g.student_t, (0,)), (g.student_t, (3, 0, -1)), (g.student_t, (np.inf,)),
                    (g.half_normal, (0,)), (g.half_student_t, (-2,)), (g.half_student_t, (3, np.inf)), (g.exponential, (0,))):
        with pytest.raises(ValueError):
            f(*args)
    # the defaults reproduce today's prior
    kw = g.priors(5, 1, 2)
    assert sorted(kw) == ["prior_kind", "prior_mu", "prior_nu", "prior_tau"]
    assert kw["prior_kind"].dtype == np.int32 and not kw["prior_kind"].any() and not kw["prior_nu"].any()
    assert np.array_equal(kw["prior_mu"], np.zeros(8)) and np.array_equal(kw["prior_tau"], np.ones(8))
    # one spec per role, or one per coordinate
    kw = g.priors(3, 1, 2, coefficients=[g.normal(), g.student_t(3, 0.5, 2.0), g.normal(1, 0.5)], aux=g.half_student_t(4, 2.0),
                  scales=[g.exponential(2.0), g.half_normal()])
    assert list(kw["prior_kind"]) == [0, 1, 0, 3, 4, 2] and list(kw["prior_nu"]) == [0, 3, 0, 4, 0, 0]
    assert np.array_equal(kw["prior_mu"], [0, 0.5, 1, np.log(2.0), np.log(2.0), 0]) and list(kw["prior_tau"]) == [1, 0.25, 4, 1, 1, 1]
    kw = g.priors(4, coefficients=g.student_t(1))
    assert list(kw["prior_kind"]) == [1] * 4 and list(kw["prior_nu"]) == [1.0] * 4
    for bad in (dict(coefficients=g.half_normal()), dict(coefficients=[g.normal()] * 2), dict(aux=[g.normal()] * 2), dict(scales=(0, 1.0)),
                dict(coefficients=[g.normal(), g.normal(), g.exponential()])):
        with pytest.raises(ValueError):
            g.priors(3, 1, 2, **bad)
    # GLM() takes them as they are
    X, Y, grp = _data()
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=grp,
                  **g.priors(6, 1, 2, coefficients=g.student_t(3, scale=2.5), aux=g.half_student_t(4), scales=g.exponential(0.5)))
    assert list(m.prior_kind) == [1] * 6 + [3, 4, 4] and m.tau[0] == 0.16 and m.mu[8] == np.log(0.5)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def _priors_struct(kind, nu):
    from inplacedhmc_jl_amd import _lib
    keep = [None if kind is None else np.ascontiguousarray(kind, np.int32), None if nu is None else np.ascontiguousarray(nu, np.float64)]
    p = _lib.GlmPriors()
    if keep[0] is not None:
        p.kind = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
    if keep[1] is not None:
        p.nu = keep[1].ctypes.data_as(C.POINTER(C.c_double))
    return p, keep


def _create_priors(idhmc, desc, priors, M, R, opt=None, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create_glm_priors(C.byref(h), 0, nchains, 0, C.byref(desc), None if priors is None else C.byref(priors), M, R,
                                     None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


FORMS = [(1, 0), (3, 2)]            # (M, chains_per_response): the context of idhmc_create_glm, of idhmc_create_glm_responses


def _model(idhmc, M, R):
    """D = 6 + 1 + 2, tau given (all 1 on the logarithms), one response or M of them"""
    grp = np.array([-1, 0, 0, 1, 1, -1], np.int32)
    X, Y = HIER.problem_hier("GAUSSIAN_IDENTITY_LOGSIGMA", 20, 6, grp, False)
    kw = {}
    if R:
        Y, kw = np.stack([Y + k for k in range(M)])[:, :, None], {"chains_per_response": R}
    tau = np.r_[np.full(6, 0.5), np.ones(3)]
    return idhmc.GLM(X, Y, idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, prior_mu=0.1, prior_tau=tau, aux=1, groups=grp, **kw)


@pytest.mark.parametrize("M,R", FORMS)
def test_valid_priors_pass_the_argument_checks(idhmc, M, R):
    m = _model(idhmc, M, R)
    ok = (0, idhmc.ERR_NO_DEVICE)
    for kind, nu in (([0, 1, 0, 1, 0, 0, 3, 4, 2], [0, 3, 0, 1, 0, 0, 4, 0, 0]), ([1] * 6 + [0, 0, 0], [2.0] * 6 + [0, 0, 0]),
                     ([0] * 6 + [2, 4, 2], None), ([0] * 9, None), ([0] * 9, [0.0] * 9), (None, None)):
        p, keep = _priors_struct(kind, nu)
        rc, msg = _create_priors(idhmc, m.glm_desc(), p, M, R)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (kind, rc, msg)
    assert _create_priors(idhmc, m.glm_desc(), None, M, R)[0] in ok


@pytest.mark.parametrize("M,R", FORMS)
def test_bad_priors_are_refused_before_the_device(idhmc, M, R):
    m = _model(idhmc, M, R)
    ok, oknu = [0, 1, 0, 1, 0, 0, 3, 4, 2], [0, 3, 0, 1, 0, 0, 4, 0, 0]

    def at(seq, c, v):
        out = list(seq)
        out[c] = v
        return out

    def refused(what, kind=ok, nu=oknu, opt=None, **fields):
        d = m.glm_desc()
        keep = []
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data_as(C.POINTER(C.c_int32 if v.dtype == np.int32 else C.c_double))
            setattr(d, k, v)
        p, keep2 = _priors_struct(kind, nu)
        rc, msg = _create_priors(idhmc, d, p, M, R, opt)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    lib = idhmc.load_library()
    h = C.c_void_p()
    p, keep = _priors_struct(ok, oknu)
    assert lib.idhmc_create_glm_priors(C.byref(h), 0, 4, 0, None, C.byref(p), M, R, None, 1) == idhmc.ERR_BAD_ARG
    assert b"null argument" in lib.idhmc_last_error()
    # the priors' own
    for k in (-1, 5, 1 << 20):
        refused(b"kind[4] = %d is outside 0..4" % k, kind=at(ok, 4, k))
    for v in (0.0, -2.0, np.inf, -np.inf, np.nan):
        refused(b"nu[1] = ", nu=at(oknu, 1, v))
        refused(b"nu[6] = ", nu=at(oknu, 6, v))
    refused(b"needs nu", nu=None)
    refused(b"nu without", kind=None)
    for c in (0, 7, 8):
        refused(b"nu[%d] = 2 must be 0" % c, nu=at(oknu, c, 2.0))
    for k in (2, 3, 4):
        refused(b"kind[5] = %d is a prior on exp(q)" % k, kind=at(ok, 5, k), nu=at(oknu, 5, 3.0 if k == 3 else 0.0))
        refused(b"kind[0] = %d is a prior on exp(q)" % k, kind=at(ok, 0, k), nu=at(oknu, 0, 3.0 if k == 3 else 0.0))
    for c in (6, 7, 8):
        tau = np.r_[np.full(6, 0.5), np.ones(3)]
        tau[c] = 2.0
        refused(b"tau[%d] = 2 must be 1" % c, tau=tau)
    # what the existing creation functions refuse
    for H in (-1, 5):
        refused(b"H = ", H=H)
    refused(b"groups is NULL", groups=None)
    refused(b"groups[3] = 7 is outside -1..1", groups=np.array([-1, 0, 0, 7, 1, -1], np.int32))
    refused(b"Dx = ", Dx=0)
    refused(b"K = ", K=0)
    refused(b"nc = ", nc=17)
    refused(b"A = ", A=5)
    refused(b"n = 0", n=0)
    refused(b"X and Y are needed", X=None)
    refused(b"needs HIP source", source=None)
    bad = np.ascontiguousarray(m.X).copy()
    bad[2, 5] = np.inf
    refused(b"X[2, 5] is not finite", X=bad)
    tau = np.r_[np.full(6, 0.5), np.ones(3)]
    tau[1] = 0.0
    refused(b"tau[1]", tau=tau)
    mu = np.zeros(9)
    mu[7] = np.nan
    refused(b"mu[7]", mu=mu)
    refused(b"max_depth", opt=idhmc.default_options(max_depth=40))
    if R:
        p, keep = _priors_struct(ok, oknu)
        for bad_m, bad_r, what in ((0, R, b"M = 0"), (M, -1, b"chains_per_response = -1"), (1, 1, b"first_chain_id + nchains")):
            rc, msg = _create_priors(idhmc, m.glm_desc(), p, bad_m, bad_r)
            assert rc == idhmc.ERR_BAD_ARG and what in msg, (rc, msg)
        refused(b"eps_mode = GLOBAL", opt=idhmc.default_options(eps_mode=idhmc.EPS_GLOBAL))
    else:
        refused(b"PER_RESPONSE", opt=idhmc.default_options(eps_mode=idhmc.EPS_PER_RESPONSE))


def test_priors_get_refuses_null(idhmc):
    lib = idhmc.load_library()
    assert lib.idhmc_glm_priors_get(None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    """each family's C restatement with priors, compiled once per family; model() points it at a problem"""
    class R:
        def __init__(self):
            self.work = {}

        def _dir(self, key):
            if key not in self.work:
                self.work[key] = str(tmp_path_factory.mktemp(key.lower()))
            return self.work[key]

        def model(self, family, X, Y, grp, kind, nu, mu=None, tau=None):
            A, H = SHAPE[family][2], int(np.max(grp)) + 1
            return oracle.OracleModel.custom(X.shape[1] + A + H, c_source_priors(family),
                                             oracle_params_priors(X, Y, A, grp, kind, nu, consts(family), mu, tau), self._dir(family))

        def hier(self, family, X, Y, grp, mu=None, tau=None):
            A, H = SHAPE[family][2], int(np.max(grp)) + 1
            return oracle.OracleModel.custom(X.shape[1] + A + H, HIER.c_source_hier(family),
                                             HIER.oracle_params_hier(X, Y, A, grp, consts(family), mu, tau), self._dir("hier_" + family))
    return R()


def scipy_log_prior(kind, nu, mu, tau, q):
    """the log density of coordinate q under its prior, from scipy.stats: the density of sigma = exp(q) plus the Jacobian q for the log kinds"""
    if kind == NORMAL:
        return stats.norm(mu, 1.0 / np.sqrt(tau)).logpdf(q)
    if kind == STUDENT_T:
        return stats.t(nu, mu, 1.0 / np.sqrt(tau)).logpdf(q)
    if kind == LOG_HALF_NORMAL:
        return stats.halfnorm(scale=np.exp(mu)).logpdf(np.exp(q)) + q
    if kind == LOG_HALF_STUDENT_T:
        return np.log(2.0) + stats.t(nu, 0.0, np.exp(mu)).logpdf(np.exp(q)) + q
    return stats.expon(scale=np.exp(mu)).logpdf(np.exp(q)) + q


@pytest.mark.parametrize("Dx,H", [(5, 2), (126, 2), (140, 4)])
def test_restatement_matches_scipy(restated, Dx, H):
    """X = 0, so the likelihood is a constant and l(q1) - l(q2) is the difference of the log priors: against scipy.stats' t, halfnorm,
    2 t on the positive axis and expon, each plus the Jacobian, within 1e-12 of the magnitude of the terms summed"""
    family, n = "POISSON_LOG", 3
    grp = HIER.interleaved(Dx, H)
    D = Dx + H
    rng = np.random.default_rng(Dx)
    X, Y = np.zeros((n, Dx)), rng.poisson(2.0, n).astype(float)
    kind, nu, mu, tau = mixed_priors(Dx, 0, H)
    kind[Dx:] = [LOG_HALF_NORMAL, LOG_HALF_STUDENT_T, LOG_EXPONENTIAL, LOG_HALF_STUDENT_T][:H]
    nu[Dx:] = [0.0, 4.0, 0.0, 1.0][:H]
    om = restated.model(family, X, Y, grp, kind, nu, mu, tau)
    for k in range(4):
        q1, q2 = (mu + rng.standard_normal(D) * (0.5 + k) for _ in range(2))
        l1, l2 = om.logdensity_and_gradient(q1)[0], om.logdensity_and_gradient(q2)[0]
        s1 = np.array([scipy_log_prior(kind[c], nu[c], mu[c], tau[c], q1[c]) for c in range(D)])
        s2 = np.array([scipy_log_prior(kind[c], nu[c], mu[c], tau[c], q2[c]) for c in range(D)])
        scale = np.abs(s1).sum() + np.abs(s2).sum() + 2.0 * n
        assert abs((l1 - l2) - (s1.sum() - s2.sum())) <= 1e-12 * scale, ((l1 - l2), s1.sum() - s2.sum(), scale)
    # one coordinate at a time, so that no kind hides behind another
    q0 = mu + 0.3
    l0 = om.logdensity_and_gradient(q0)[0]
    for c in list(range(min(Dx, 8))) + list(range(Dx, D)):
        q1 = q0.copy()
        q1[c] += 1.7
        want = scipy_log_prior(kind[c], nu[c], mu[c], tau[c], q1[c]) - scipy_log_prior(kind[c], nu[c], mu[c], tau[c], q0[c])
        _, _, lscale, _ = numpy_density_priors(family, X, Y, q1, grp, kind, nu, mu, tau)
        assert abs((om.logdensity_and_gradient(q1)[0] - l0) - want) <= 1e-12 * 2.0 * lscale, (c, kind[c])


@pytest.mark.parametrize("family", ["POISSON_LOG", "GAUSSIAN_IDENTITY_LOGSIGMA"])
@pytest.mark.parametrize("n,Dx,H", [(1, 5, 1), (37, 25, 2), (130, 127, 1), (200, 300, 4)])
def test_restatement_matches_the_closed_form(restated, family, n, Dx, H):
    A = SHAPE[family][2]
    D = Dx + A + H
    grp = HIER.interleaved(Dx, H)
    X, Y = HIER.problem_hier(family, n, Dx, grp, False, seed=n + Dx)
    kind, nu, mu, tau = mixed_priors(Dx, A, H)
    om = restated.model(family, X, Y, grp, kind, nu, mu, tau)
    for k in range(3):
        q = HIER.start_hier(family, 1, Dx, H, seed=k, scale=0.3 + 0.3 * k)[0]
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_priors(family, X, Y, q, grp, kind, nu, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), np.max(np.abs(g[:D] - g_ref) / gscale)


@pytest.mark.parametrize("family", ["POISSON_LOG", "GAUSSIAN_IDENTITY_LOGSIGMA"])
def test_restatement_gradient_is_the_derivative(restated, family):
    """central differences in every non-Gaussian coordinate"""
    n, Dx, H = 60, 23, 4
    A = SHAPE[family][2]
    D = Dx + A + H
    grp = HIER.interleaved(Dx, H)
    X, Y = HIER.problem_hier(family, n, Dx, grp, False, seed=11)
    kind, nu, mu, tau = mixed_priors(Dx, A, H)
    kind[D - 1], nu[D - 1] = LOG_HALF_STUDENT_T, 1.0            # (the cycle's fourth log coordinate is NORMAL: every kind, twice)
    om = restated.model(family, X, Y, grp, kind, nu, mu, tau)
    q = HIER.start_hier(family, 1, Dx, H, seed=5)[0]
    _, g = om.logdensity_and_gradient(q)
    coords = np.flatnonzero(kind != NORMAL)
    assert set(kind[coords]) == {1, 2, 3, 4}
    h = 1e-5
    for c in coords:
        e = np.zeros(D)
        e[c] = h
        fd = (om.logdensity_and_gradient(q + e)[0] - om.logdensity_and_gradient(q - e)[0]) / (2 * h)
        assert fd == pytest.approx(g[c], rel=1e-6, abs=1e-6), (c, kind[c])


@pytest.mark.parametrize("family", ["POISSON_LOG", "GAUSSIAN_IDENTITY_LOGSIGMA"])
def test_all_normal_kinds_give_the_bits_of_the_hierarchical_restatement(restated, family):
    n, Dx, H = 130, 140, 2
    A = SHAPE[family][2]
    D = Dx + A + H
    grp = HIER.interleaved(Dx, H)
    X, Y = HIER.problem_hier(family, n, Dx, grp, False, seed=2)
    rng = np.random.default_rng(1)
    mu, tau = rng.standard_normal(D) * 0.3, rng.uniform(0.5, 2.0, D)
    a, b = restated.model(family, X, Y, grp, 0, 0.0, mu, tau), restated.hier(family, X, Y, grp, mu, tau)
    for k in range(4):
        q = HIER.start_hier(family, 1, Dx, H, seed=k, scale=0.2 + 0.4 * k)[0]
        (la, ga), (lb, gb) = a.logdensity_and_gradient(q), b.logdensity_and_gradient(q)
        assert np.float64(la).tobytes() == np.float64(lb).tobytes() and ga.tobytes() == gb.tobytes()


def test_past_the_range_of_dexp(restated, oracle):
    """the end of each log kind's finite range: exp overflows, T is +inf and a chain reads l = -inf; far below the scale everything is
    finite (e = 0: -2 log p is linear in d)"""
    family, n, Dx, H = "POISSON_LOG", 5, 6, 3
    grp = HIER.interleaved(Dx, H)
    X, Y = HIER.problem_hier(family, n, Dx, grp, False, seed=1)
    kind, nu = np.r_[np.zeros(Dx), [2, 3, 4]], np.r_[np.zeros(Dx), [0, 4.0, 0]]
    om = restated.model(family, X, Y, grp, kind, nu)
    q0 = np.r_[np.full(Dx, 0.1), np.zeros(H)]
    for c, d_bad, d_ok in ((Dx, 354.9, 354.88), (Dx + 1, 354.9, 354.88), (Dx + 2, 709.1, 709.07)):
        X0 = np.zeros_like(X)                            # (a group scale of e^355 times u would overflow z on its own)
        om0 = restated.model(family, X0, Y, grp, kind, nu)
        q = q0.copy()
        q[c] = d_bad
        assert not np.isfinite(om0.logdensity_and_gradient(q)[0])
        ch = oracle.OracleChain(om0, None, seed=1, chain_id=0)
        ch.set_q(q)
        assert ch.lq == -np.inf
        q[c] = d_ok
        assert np.isfinite(om0.logdensity_and_gradient(q)[0])
        q[c] = -800.0
        lq, g = om.logdensity_and_gradient(q)
        assert np.isfinite(lq) and np.isfinite(g).all() and g[c] == pytest.approx(1.0, abs=1e-9)
