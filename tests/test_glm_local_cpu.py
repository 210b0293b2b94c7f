"""Per-coefficient local scales (GLM(..., local=, slab_scale=), idhmc_create_glm_local) without a GPU: the
constructor's validation, glm.priors' fourth role, glm.horseshoe, the host helpers on hand-made draws, the C boundary's argument checks
through both forms of the entry point, and the C restatement of section 19's definition against a numpy restatement, central
differences in every lambda, the omega of a flagged group and flagged u, the closed forms of st and h at the ends of s, and, with no
column flagged, the bits of section 18's restatement.

The restatement is C_BODY_PRIORS of tests/test_glm_priors_cpu.py with J, inv2 and local (Dx) added to its params and section 19 in its
body: params are [n, K, nc, A, H, J, inv2, mu (D), tau (D), kind (D, as doubles), nu (D), c (nc), grp (Dx, as doubles), local (Dx, as
doubles), X row-major (n x Dx), Y row-major (n x K)], D = Dx + A + H + J.  The GPU tests (tests/test_gpu_glm_local.py) hand the same
source to the oracle."""
import ctypes as C

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
import test_glm_cpu as FLAT
import test_glm_hier_cpu as HIER
import test_glm_priors_cpu as PRI
from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_priors_cpu import LOG_HALF_STUDENT_T, NORMAL, mixed_priors, numpy_prior

C_BODY_LOCAL = r"""
#include <math.h>
#include "orc_math.h"
%s
/* params: [n, K, nc, A, H, J, inv2, mu (D), tau (D), kind (D), nu (D), c (nc), grp (Dx, as doubles), local (Dx, as doubles),
            X row-major (n x Dx), Y row-major (n x K)] */
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    const long n = (long)params[0];
    const int K = (int)params[1], nc = (int)params[2], A = (int)params[3], H = (int)params[4], J = (int)params[5], Dx = D - A - H - J;
    const double inv2 = params[6];
    const double *mu = params + 7, *tau = mu + D, *kind = tau + D, *nu = kind + D, *c = nu + D, *grp = c + nc, *loc = grp + Dx, *X = loc + Dx,
                 *Y = X + n * Dx;
    const double *a = q + Dx, *om = q + Dx + A, *lam = q + Dx + A + H;
    double b[1024], st[1024], hh[1024];
    int kk[1024];
    double e[4] = {0, 0, 0, 0}, T[128], V[128], S[4][128], W[4][128];
    for (int g = 0; g < H; ++g) e[g] = orc_exp(om[g]);
    for (int j = 0, k = 0; j < Dx; ++j) {
        if (loc[j] != 0.0) {
            const double f = orc_exp(lam[k]);
            const double s = grp[j] >= 0.0 ? e[(int)grp[j]] * f : f;
            st[j] = s;
            hh[j] = 1.0;
            if (inv2 != 0.0) {
                const double i = 1.0 / s;
                const double nn = fma(i, i, inv2);
                st[j] = 1.0 / sqrt(nn);
                hh[j] = 1.0 - inv2 / nn;
            }
            b[j] = q[j] * st[j];
            kk[j] = k++;
        } else {
            b[j] = grp[j] >= 0.0 ? q[j] * e[(int)grp[j]] : q[j];
            kk[j] = -1;
        }
    }
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
    for (int j = 0; j < Dx; ++j) {
        if (kk[j] >= 0) {
            const double w = grad[j] * b[j];
            const double wl = inv2 != 0.0 ? w * hh[j] : w;
            grad[Dx + A + H + kk[j]] = wl;
            if (grp[j] >= 0.0) W[(int)grp[j]][j & 127] = W[(int)grp[j]][j & 127] + wl;
            grad[j] = grad[j] * st[j];
        } else if (grp[j] >= 0.0) {
            const int g = (int)grp[j];
            W[g][j & 127] = W[g][j & 127] + grad[j] * b[j];
            grad[j] = grad[j] * e[g];
        }
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


def c_source_local(family):
    """C_BODY_LOCAL around the family's observation, as PRI.c_source_priors builds on HIER.c_source_hier"""
    body = HIER.c_source_hier(family)
    head, tail = HIER.C_BODY_HIER.split("%s")
    assert body.startswith(head) and body.endswith(tail)
    return C_BODY_LOCAL % body[len(head):len(body) - len(tail)]


def inv2_of(S):
    return 1.0 / (S * S) if S else 0.0


def oracle_params_local(X, Y, A, grp, local, S, kind, nu, c=None, mu=None, tau=None):
    n, Dx = X.shape
    grp = np.full(Dx, -1) if grp is None else np.asarray(grp)
    local = np.zeros(Dx) if local is None else np.asarray(local, float)
    H, J = int(grp.max()) + 1, int(local.sum())
    D = Dx + A + H + J
    Y = np.asarray(Y, float).reshape(n, -1)
    c = np.zeros(0) if c is None else np.asarray(c, float)
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    kind = np.broadcast_to(np.asarray(kind, float), (D,))
    nu = np.broadcast_to(np.asarray(nu, float), (D,))
    return np.concatenate([[float(n), float(Y.shape[1]), float(c.size), float(A), float(H), float(J), inv2_of(S)], mu, tau, kind, nu, c,
                           grp.astype(float), local, np.asarray(X, float).ravel(), Y.ravel()])


def numpy_density_local(family, X, Y, q, grp, local, S, kind, nu, mu=None, tau=None):
    """(l(q), grad l(q), magnitude of l's terms, per-coordinate magnitude of the terms summed into grad), q = [u | a | omega | lambda],
    from the closed forms st = s / sqrt(1 + s^2 / S^2), h = 1 / (1 + s^2 / S^2)"""
    n, Dx = X.shape
    A, H = SHAPE[family][2], int(np.max(grp)) + 1
    cols = np.flatnonzero(local)
    J = cols.size
    D = Dx + A + H + J
    assert q.size == D
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    u, a, om, lam = q[:Dx], q[Dx:Dx + A], q[Dx + A:Dx + A + H], q[Dx + A + H:]
    scale = np.where(grp >= 0, np.exp(om)[np.maximum(grp, 0)], 1.0) if H else np.ones(Dx)
    h = np.ones(Dx)
    sl = scale[cols] * np.exp(lam)
    if S:
        h[cols] = 1.0 / (1.0 + sl * sl / (S * S))
        sl = sl / np.sqrt(1.0 + sl * sl / (S * S))
    scale[cols] = sl
    b = scale * u
    z = X @ b
    if A == 0:
        lp, r, mag = FLAT.numpy_terms(family, z, Y)
        sc, smag = np.zeros((n, 0)), np.zeros((n, 0))
    else:
        lp, r, sc, mag, smag = AUX.numpy_terms_aux(family, z, Y, a)
    G, Gmag = X.T @ r, np.abs(X).T @ np.abs(r)
    wl, wmag = G * b * h, Gmag * np.abs(b) * h
    member = [grp == g for g in range(H)]
    plp, pg, plmag, pgmag = numpy_prior(np.broadcast_to(kind, (D,)), np.broadcast_to(np.asarray(nu, float), (D,)), mu, tau, q)
    g = np.concatenate([scale * G, sc.sum(0), [np.sum(wl[m]) for m in member], wl[cols]]) + pg
    gscale = np.concatenate([scale * Gmag, smag.sum(0), [np.sum(wmag[m]) for m in member], wmag[cols]]) + pgmag
    return np.sum(lp) + plp.sum(), g, np.sum(mag) + plmag.sum(), gscale


def local_priors(Dx, A, H, J):
    """mixed_priors on [u | a | omega]; the lambdas cycle LOG_HALF_STUDENT_T (nu = 1) and NORMAL"""
    kind, nu, mu, tau = mixed_priors(Dx, A, H)
    lk = np.where(np.arange(J) % 2 == 0, LOG_HALF_STUDENT_T, NORMAL).astype(np.int32)
    rng = np.random.default_rng(J)
    return (np.r_[kind, lk].astype(np.int32), np.r_[nu, np.where(lk == LOG_HALF_STUDENT_T, 1.0, 0.0)], np.r_[mu, rng.standard_normal(J) * 0.2],
            np.r_[tau, np.where(lk == NORMAL, rng.uniform(0.5, 2.0, J), 1.0)])


def start_local(family, C_, Dx, H, J, seed=0, scale=0.3):
    """HIER.start_hier, then lambda ~ U(-0.7, 0.7)"""
    rng = np.random.default_rng(seed + Dx + 1000)
    return np.concatenate([HIER.start_hier(family, C_, Dx, H, seed, scale), rng.uniform(-0.7, 0.7, (C_, J))], 1)


def make(idhmc, family, X, Y, grp, local, S, kind, nu, mu=None, tau=None, **kw):
    return idhmc.GLM(X, Y, source(idhmc, family), consts(family), mu, tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu,
                     local=local, slab_scale=S, **kw)


# ---- the constructor and the host helpers ---------------------------------------------------------------------------------------------
def _data(family="GAUSSIAN_IDENTITY_LOGSIGMA", n=9, Dx=6):
    grp = np.array([-1, 0, 1, 0, -1, 1][:Dx])
    return HIER.problem_hier(family, n, Dx, grp, False) + (grp,)


def test_constructor_keeps_the_local_scales(idhmc):
    X, Y, grp = _data()
    g = idhmc.glm
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=grp, local=[0, 1, 1, 0, True, 0], slab_scale=2.5)
    assert m.D == 12 and (m.Dx, m.A, m.H, m.J) == (6, 1, 2, 3) and m.slab_scale == 2.5
    assert m.local.dtype == np.int32 and list(m.local) == [0, 1, 1, 0, 1, 0]
    assert m.glm_desc().Dx == 6                          # handed over in parts
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, local=True)
    assert m.J == 6 and m.D == 13 and m.H == 0 and list(m.local) == [1] * 6 and m.slab_scale is None
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, local=np.array([True, False] * 3), slab_scale=0)
    assert m.J == 3 and m.slab_scale is None
    # the priors cover the lambdas, and the log kinds apply to them
    kind, nu = [0] * 6 + [3, 0, 0] + [3, 2, 4], [0] * 6 + [4.0, 0, 0] + [1.0, 0, 0]
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=grp, local=[0, 1, 1, 0, 1, 0], prior_kind=kind, prior_nu=nu)
    assert list(m.prior_kind) == kind and m.prior_kind.size == m.D
    with pytest.raises(ValueError, match="one entry per sampled coordinate"):
        idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=grp, local=[0, 1, 1, 0, 1, 0], prior_kind=kind[:9])
    # without a flagged column: the model without the keywords, byte for byte
    X5, Y5 = X[:, :5], (Y > 0).astype(float)
    plain = idhmc.GLM(X5, Y5, g.BERNOULLI_LOGIT)
    for kw in ({"local": None}, {"local": np.zeros(5)}, {"local": [False] * 5, "slab_scale": None}, {"local": [0] * 5, "slab_scale": 0.0}):
        m = idhmc.GLM(X5, Y5, g.BERNOULLI_LOGIT, **kw)
        assert m.J == 0 and m.local is None and m.slab_scale is None and m.D == 5 and m.params.tobytes() == plain.params.tobytes()
    assert plain.J == 0 and plain.local is None and plain.slab_scale is None


def test_constructor_validates_local(idhmc):
    X, Y, grp = _data()
    src = idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA

    def bad(what, **kw):
        with pytest.raises(ValueError, match=what):
            idhmc.GLM(X, Y, src, aux=1, groups=grp, **kw)
    for shape in ([1] * 5, [1] * 7, [[1] * 6], 1, False):
        bad("local must be True or have one entry per column", local=shape)
    for v in (2, -1, 0.5, np.nan):
        bad("every entry of local must be 0 or 1", local=[0, 1, v, 0, 0, 0])
    bad("every entry of local must be 0 or 1", local=["a"] * 6)
    for v in (-1.0, np.inf, np.nan):
        bad("slab_scale = .* must be finite and >= 0", local=True, slab_scale=v)
    for v in ("2", True, [2.0]):
        bad("slab_scale must be a number", local=True, slab_scale=v)
    bad("slab_scale = 2.0 needs a column with a local scale", slab_scale=2.0)
    bad("slab_scale = 2.0 needs a column with a local scale", slab_scale=2.0, local=[0] * 6)
    Xw = np.ones((2, 600))
    with pytest.raises(ValueError, match=r"limited to D <= 1024 \(D = 1200\)"):
        idhmc.GLM(Xw, np.zeros(2), idhmc.glm.POISSON_LOG, local=True)
    assert idhmc.GLM(np.ones((2, 512)), np.zeros(2), idhmc.glm.POISSON_LOG, local=True).D == 1024


def test_priors_builder_takes_the_local_scales(idhmc):
    g = idhmc.glm
    kw = g.priors(3, 1, 2, 2, scales=g.exponential(2.0), local_scales=g.half_student_t(1))
    assert list(kw["prior_kind"]) == [0, 0, 0, 0, 4, 4, 3, 3] and list(kw["prior_nu"]) == [0] * 6 + [1.0, 1.0]
    kw = g.priors(2, J=2, local_scales=[g.half_normal(2.0), g.normal(0.5, 2.0)])
    assert list(kw["prior_kind"]) == [0, 0, 2, 0] and np.array_equal(kw["prior_mu"], [0, 0, np.log(2.0), 0.5]) and list(kw["prior_tau"]) == [1, 1, 1, 0.25]
    assert g.priors(5, 1, 2)["prior_kind"].size == 8 and g.priors(5, 1, 2, 0)["prior_kind"].size == 8
    for bad in (dict(local_scales=[g.normal()]), dict(local_scales=(0, 1.0))):
        with pytest.raises(ValueError):
            g.priors(3, 1, 2, 2, **bad)
    with pytest.raises(ValueError):
        g.priors(3, 1, 2, -1)


def test_horseshoe_assembles_the_model(idhmc):
    g = idhmc.glm
    kw = g.horseshoe(6, [1, 2, 4], 0.1, A=1, slab_scale=2.0)
    assert sorted(kw) == ["groups", "local", "prior_kind", "prior_mu", "prior_nu", "prior_tau", "slab_scale"]
    assert list(kw["groups"]) == [-1, 0, 0, -1, 0, -1] and list(kw["local"]) == [0, 1, 1, 0, 1, 0] and kw["slab_scale"] == 2.0
    assert list(kw["prior_kind"]) == [0] * 7 + [3] + [3] * 3 and list(kw["prior_nu"]) == [0] * 7 + [1.0] * 4
    assert np.array_equal(kw["prior_mu"], [0] * 7 + [np.log(0.1)] + [0] * 3) and list(kw["prior_tau"]) == [1.0] * 11
    X, Y, _ = _data()
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, **kw)
    assert (m.Dx, m.A, m.H, m.J, m.D) == (6, 1, 1, 3, 11) and m.slab_scale == 2.0
    kw = g.horseshoe(4, np.array([True, False, True, True]), 1.0, nu_local=3.0, nu_global=2.0, aux=None)
    assert list(kw["local"]) == [1, 0, 1, 1] and kw["slab_scale"] is None and list(kw["prior_nu"]) == [0] * 4 + [2.0] + [3.0] * 3
    for bad in (dict(columns=[]), dict(columns=[0, 0]), dict(columns=[6]), dict(columns=[-1]), dict(columns=[0.5]), dict(columns=[True] * 5),
                dict(columns=[False] * 6), dict(global_scale=0.0), dict(slab_scale=0.0), dict(slab_scale=-1.0), dict(nu_local=0.0)):
        args = dict(columns=[1, 2], global_scale=0.1)
        args.update(bad)
        with pytest.raises(ValueError):
            g.horseshoe(6, **args)


def test_host_helpers_on_hand_made_draws(idhmc):
    g = idhmc.glm
    X, Y, grp = _data()                                  # grp = [-1, 0, 1, 0, -1, 1]
    local = [0, 1, 0, 1, 1, 0]                           # column 1 and 3 (group 0) and column 4 (no group)
    draws = np.zeros((2, 3, 12))
    draws[..., :6] = [1.0, 2.0, 3.0, -1.0, 0.5, 4.0]
    draws[..., 6] = 0.3
    draws[..., 7:9] = np.log([2.0, 0.5])
    draws[..., 9:] = np.log([3.0, 0.25, 4.0])
    draws[1, 2, 9] = np.log(5.0)
    for S in (None, 2.0):
        m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=grp, local=local, slab_scale=S)
        sig, lam, beta = g.group_scales(m, draws), g.local_scales(m, draws), g.coefficients(m, draws)
        assert sig.shape == (2, 3, 2) and np.allclose(sig, [2.0, 0.5], rtol=1e-15)
        assert lam.shape == (2, 3, 3) and np.allclose(lam[0, 0], [3.0, 0.25, 4.0], rtol=1e-15) and np.isclose(lam[1, 2, 0], 5.0, rtol=1e-15)
        s = np.array([6.0, 0.5, 4.0])
        st = s if S is None else s / np.sqrt(1.0 + s * s / (S * S))
        want = np.array([1.0, 2.0 * st[0], 3.0 * 0.5, -1.0 * st[1], 0.5 * st[2], 4.0 * 0.5])
        assert beta.shape == (2, 3, 6) and np.allclose(beta[0, 0], want, rtol=1e-14)
        s10 = 10.0
        assert np.isclose(beta[1, 2, 1], 2.0 * (s10 if S is None else s10 / np.sqrt(1.0 + s10 * s10 / (S * S))), rtol=1e-14)
        for f in (g.group_scales, g.local_scales, g.coefficients):
            with pytest.raises(ValueError, match="12 coordinates"):
                f(m, draws[..., :9])
    # no groups at all, and the ends of s with a slab: s = inf gives S, s = 0 gives 0
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, local=[0, 0, 1, 0, 0, 0], slab_scale=3.0)
    d = np.zeros((3, 8))
    d[:, 2], d[:, 7] = 2.0, [800.0, -800.0, 0.0]
    assert g.group_scales(m, d).shape == (3, 0) and g.local_scales(m, d).shape == (3, 1)
    assert np.allclose(g.coefficients(m, d)[:, 2], [6.0, 0.0, 2.0 / np.sqrt(1.0 + 1.0 / 9.0)], rtol=1e-15)
    # a model without local scales: as before, and an empty last axis
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=grp)
    assert g.local_scales(m, np.zeros((4, 9))).shape == (4, 0) and g.coefficients(m, np.ones((4, 9))).shape == (4, 6)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
FORMS = PRI.FORMS


def _local_struct(local, slab):
    from inplacedhmc_jl_amd import _lib
    keep = None if local is None else np.ascontiguousarray(local, np.int32)
    s = _lib.GlmLocal(slab_scale=slab)
    if keep is not None:
        s.local = keep.ctypes.data_as(C.POINTER(C.c_int32))
    return s, keep


def _create_local(idhmc, desc, priors, local, M, R, opt=None, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create_glm_local(C.byref(h), 0, nchains, 0, C.byref(desc), None if priors is None else C.byref(priors),
                                    None if local is None else C.byref(local), M, R, None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def _model(idhmc, M, R, J=3):
    """Dx = 6, A = 1, H = 2 and J lambdas: mu and tau given over all D (tau 1 on the logarithms), one response or M of them"""
    grp = np.array([-1, 0, 0, 1, 1, -1], np.int32)
    X, Y = HIER.problem_hier("GAUSSIAN_IDENTITY_LOGSIGMA", 20, 6, grp, False)
    kw = {}
    if R:
        Y, kw = np.stack([Y + k for k in range(M)])[:, :, None], {"chains_per_response": R}
    tau = np.r_[np.full(6, 0.5), np.ones(3 + J)]
    local = np.r_[np.ones(J, np.int32), np.zeros(6 - J, np.int32)] if J else None
    return idhmc.GLM(X, Y, idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, prior_mu=0.1, prior_tau=tau, aux=1, groups=grp, local=local, **kw)


OK_KIND, OK_NU = [0, 1, 0, 1, 0, 0, 3, 4, 2, 3, 0, 2], [0, 3, 0, 1, 0, 0, 4, 0, 0, 1, 0, 0]


@pytest.mark.parametrize("M,R", FORMS)
def test_valid_local_scales_pass_the_argument_checks(idhmc, M, R):
    ok = (0, idhmc.ERR_NO_DEVICE)
    m = _model(idhmc, M, R)
    p, keep = PRI._priors_struct(OK_KIND, OK_NU)
    for S in (0.0, 2.5):
        lc, keep2 = _local_struct([1, 1, 1, 0, 0, 0], S)
        for pr in (p, None):
            rc, msg = _create_local(idhmc, m.glm_desc(), pr, lc, M, R)
            assert rc in ok and (rc == 0 or b"no HIP device" in msg), (S, rc, msg)
    # no local scales: the context of idhmc_create_glm_priors, whose arrays have Dx + A + H entries
    m0 = _model(idhmc, M, R, J=0)
    p0, keep0 = PRI._priors_struct(OK_KIND[:9], OK_NU[:9])
    for lc in (None, _local_struct(None, 0.0)[0], _local_struct([0] * 6, 0.0)[0]):
        rc, msg = _create_local(idhmc, m0.glm_desc(), p0, lc, M, R)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)


@pytest.mark.parametrize("M,R", FORMS)
def test_bad_local_scales_are_refused_before_the_device(idhmc, M, R):
    m = _model(idhmc, M, R)

    def at(seq, c, v):
        out = list(seq)
        out[c] = v
        return out

    def refused(what, local=(1, 1, 1, 0, 0, 0), slab=0.0, kind=OK_KIND, nu=OK_NU, opt=None, model=m, **fields):
        d = model.glm_desc()
        keep = []
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data_as(C.POINTER(C.c_int32 if v.dtype == np.int32 else C.c_double))
            setattr(d, k, v)
        p, keep2 = PRI._priors_struct(kind, nu)
        lc, keep3 = _local_struct(local, slab)
        rc, msg = _create_local(idhmc, d, p, lc, M, R, opt)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    lib = idhmc.load_library()
    h = C.c_void_p()
    lc, keep = _local_struct([1, 1, 1, 0, 0, 0], 0.0)
    assert lib.idhmc_create_glm_local(C.byref(h), 0, 4, 0, None, None, C.byref(lc), M, R, None, 1) == idhmc.ERR_BAD_ARG
    assert b"null argument" in lib.idhmc_last_error()
    assert lib.idhmc_glm_local_get(None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    # the local scales' own
    for v in (2, -1, 1 << 20):
        refused(b"local[1] = %d is neither 0 nor 1" % v, local=at([1, 1, 1, 0, 0, 0], 1, v))
    for v in (-1.0, np.inf, -np.inf, np.nan):
        refused(b"slab_scale = ", slab=v)
    m0 = _model(idhmc, M, R, J=0)
    refused(b"slab_scale = 2 without a column", local=None, slab=2.0, kind=OK_KIND[:9], nu=OK_NU[:9], model=m0)
    refused(b"slab_scale = 2 without a column", local=[0] * 6, slab=2.0, kind=OK_KIND[:9], nu=OK_NU[:9], model=m0)
    # D = Dx + A + H + J > 1024, though Dx + A + H is not
    Xw = np.ones((2, 600))
    Yw = np.zeros((M, 2, 1)) if R else np.zeros(2)
    wide = idhmc.GLM(Xw, Yw, idhmc.glm.POISSON_LOG, groups=[0] * 600, **({"chains_per_response": R} if R else {}))
    refused(b"D = Dx + A + H + J = 1201: a GLM is limited to D <= 1024", local=[1] * 600, kind=None, nu=None, model=wide)
    # the priors cover the lambdas: a kind outside the table behind the group scales, a log kind's tau there
    refused(b"kind[10] = 7 is outside 0..4", kind=at(OK_KIND, 10, 7))
    refused(b"nu[9] = ", nu=at(OK_NU, 9, 0.0))
    tau = np.r_[np.full(6, 0.5), np.ones(6)]
    tau[11] = 2.0
    refused(b"tau[11] = 2 must be 1", tau=tau)
    refused(b"kind[2] = 3 is a prior on exp(q)", kind=at(OK_KIND, 2, 3), nu=at(OK_NU, 2, 1.0))
    # what the other creation functions refuse
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
    mu = np.zeros(12)
    mu[10] = np.nan
    refused(b"mu[10]", mu=mu)
    refused(b"max_depth", opt=idhmc.default_options(max_depth=40))
    if R:
        p, keep = PRI._priors_struct(OK_KIND, OK_NU)
        for bad_m, bad_r, what in ((0, R, b"M = 0"), (M, -1, b"chains_per_response = -1"), (1, 1, b"first_chain_id + nchains")):
            rc, msg = _create_local(idhmc, m.glm_desc(), p, lc, bad_m, bad_r)
            assert rc == idhmc.ERR_BAD_ARG and what in msg, (rc, msg)
        refused(b"eps_mode = GLOBAL", opt=idhmc.default_options(eps_mode=idhmc.EPS_GLOBAL))
        # the per-response metric keeps its D <= 512, D counting the lambdas
        Xm = np.ones((2, 300))
        mid = idhmc.GLM(Xm, np.zeros((M, 2, 1)), idhmc.glm.POISSON_LOG, chains_per_response=R)
        refused(b"D = 600 > 512 and metric_mode = PER_RESPONSE", local=[1] * 300, kind=None, nu=None, model=mid,
                opt=idhmc.default_options(metric_mode=idhmc.METRIC_PER_RESPONSE, eps_mode=idhmc.EPS_PER_CHAIN))
    else:
        refused(b"PER_RESPONSE", opt=idhmc.default_options(eps_mode=idhmc.EPS_PER_RESPONSE))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    """each family's C restatement with local scales, compiled once per family; model() points it at a problem"""
    class R:
        def __init__(self):
            self.work = {}

        def _dir(self, key):
            if key not in self.work:
                self.work[key] = str(tmp_path_factory.mktemp(key.lower()))
            return self.work[key]

        def model(self, family, X, Y, grp, local, S, kind, nu, mu=None, tau=None):
            A, H, J = SHAPE[family][2], int(np.max(grp)) + 1, int(np.sum(local))
            return oracle.OracleModel.custom(X.shape[1] + A + H + J, c_source_local(family),
                                             oracle_params_local(X, Y, A, grp, local, S, kind, nu, consts(family), mu, tau), self._dir(family))

        def priors(self, family, X, Y, grp, kind, nu, mu=None, tau=None):
            A, H = SHAPE[family][2], int(np.max(grp)) + 1
            return oracle.OracleModel.custom(X.shape[1] + A + H, PRI.c_source_priors(family),
                                             PRI.oracle_params_priors(X, Y, A, grp, kind, nu, consts(family), mu, tau), self._dir("pri_" + family))
    return R()


def flags(Dx, which):
    if which == "all":
        return np.ones(Dx, np.int32)
    if which == "thirds":
        return (np.arange(Dx) % 3 != 0).astype(np.int32)
    if which == "fourths":
        return (np.arange(Dx) % 4 != 0).astype(np.int32)
    return (np.arange(Dx) == Dx // 2).astype(np.int32)   # "one"


@pytest.mark.parametrize("family", ["POISSON_LOG", "GAUSSIAN_IDENTITY_LOGSIGMA"])
@pytest.mark.parametrize("S", [None, 2.5])
@pytest.mark.parametrize("n,Dx,H,which", [(1, 5, 0, "one"), (37, 25, 2, "thirds"), (130, 63, 1, "all"), (200, 300, 4, "fourths")])
def test_restatement_matches_numpy(restated, family, S, n, Dx, H, which):
    A = SHAPE[family][2]
    grp = HIER.interleaved(Dx, H) if H else np.full(Dx, -1, np.int32)
    local = flags(Dx, which)
    J = int(local.sum())
    D = Dx + A + H + J
    X, Y = HIER.problem_hier(family, n, Dx, grp, False, seed=n + Dx)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    om = restated.model(family, X, Y, grp, local, S, kind, nu, mu, tau)
    for k in range(3):
        q = start_local(family, 1, Dx, H, J, seed=k, scale=0.3 + 0.3 * k)[0]
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_local(family, X, Y, q, grp, local, S, kind, nu, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), np.max(np.abs(g[:D] - g_ref) / gscale)


@pytest.mark.parametrize("family", ["POISSON_LOG", "GAUSSIAN_IDENTITY_LOGSIGMA"])
@pytest.mark.parametrize("S", [None, 1.5])
def test_restatement_gradient_is_the_derivative(restated, family, S):
    """central differences in every lambda, the omega of every group (each holds flagged columns) and the flagged u"""
    n, Dx, H = 60, 23, 2
    A = SHAPE[family][2]
    grp = HIER.interleaved(Dx, H)
    local = flags(Dx, "fourths")
    J = int(local.sum())
    D = Dx + A + H + J
    assert all(local[grp == g].any() for g in range(H)) and local[grp < 0].any()
    X, Y = HIER.problem_hier(family, n, Dx, grp, False, seed=11)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    om = restated.model(family, X, Y, grp, local, S, kind, nu, mu, tau)
    q = start_local(family, 1, Dx, H, J, seed=5)[0]
    _, g = om.logdensity_and_gradient(q)
    h = 1e-5
    for c in list(np.flatnonzero(local)) + list(range(Dx + A, D)):
        e = np.zeros(D)
        e[c] = h
        fd = (om.logdensity_and_gradient(q + e)[0] - om.logdensity_and_gradient(q - e)[0]) / (2 * h)
        assert fd == pytest.approx(g[c], rel=1e-6, abs=1e-6), c


def test_closed_forms_of_st_and_h(restated, oracle, idhmc):
    """One observation y = 0 of a Gaussian with known sigma = 0.5 on one flagged column x = 1 with u = 1, priors centred on q: G = -4 st,
    so grad_u = G st = -4 st^2 and grad_lambda = G b h = -4 st^2 h.  At s = exp(lambda) in {0, 1e-200, 1, S, 1e200, inf}."""
    family, S = "GAUSSIAN_KNOWN", 3.0
    X, Y, grp, local = np.ones((1, 1)), np.zeros(1), np.array([-1]), np.array([1])
    for slab in (S, None):
        for s, lam in ((0.0, -800.0), (1e-200, np.log(1e-200)), (1.0, 0.0), (S, np.log(S)), (1e200, np.log(1e200)), (np.inf, 800.0)):
            q = np.array([1.0, lam])
            om = restated.model(family, X, Y, grp, local, slab, 0, 0.0, mu=q, tau=1.0)
            lq, g = om.logdensity_and_gradient(q)
            if slab is None:
                st, h = s, 1.0
            elif s == 0.0 or s == 1e-200:
                st, h = 0.0, 1.0                          # (1e-200: 1 / s^2 overflows; st is 0 where it should be 1e-200, as stated)
            elif s >= 1e200:
                st, h = S, 0.0                            # (1e200: 1 / s^2 underflows against 1 / S^2; S (1 - 4.5e-400) and h = 9e-400 round to these)
            else:
                st, h = s / np.sqrt(1.0 + s * s / (S * S)), 1.0 / (1.0 + s * s / (S * S))
            if slab is None and s >= 1e200:
                assert not np.isfinite(lq)               # without a slab (4 st^2 overflows): the rejected point
                ch = oracle.OracleChain(om, None, seed=1, chain_id=0)
                ch.set_q(q)
                assert ch.lq == -np.inf
                continue
            assert np.isfinite(lq) and np.isfinite(g[:2]).all(), (slab, s)
            assert g[0] == pytest.approx(-4.0 * st * st, rel=1e-12, abs=0.0), (slab, s)
            assert g[1] == pytest.approx(-4.0 * st * st * h, rel=1e-12, abs=0.0), (slab, s)
            assert lq == pytest.approx(-2.0 * st * st, rel=1e-12, abs=0.0)
            m = idhmc.GLM(X, Y, HIER.GAUSSIAN_KNOWN_SOURCE, [0.5], local=[1], slab_scale=slab)
            assert idhmc.glm.coefficients(m, q)[0] == pytest.approx(st, rel=1e-12, abs=0.0)


@pytest.mark.parametrize("family", ["POISSON_LOG", "GAUSSIAN_IDENTITY_LOGSIGMA"])
def test_no_flagged_column_gives_the_bits_of_the_priors_restatement(restated, family):
    n, Dx, H = 130, 140, 2
    A = SHAPE[family][2]
    grp = HIER.interleaved(Dx, H)
    X, Y = HIER.problem_hier(family, n, Dx, grp, False, seed=2)
    kind, nu, mu, tau = mixed_priors(Dx, A, H)
    a, b = restated.model(family, X, Y, grp, np.zeros(Dx), None, kind, nu, mu, tau), restated.priors(family, X, Y, grp, kind, nu, mu, tau)
    for k in range(4):
        q = HIER.start_hier(family, 1, Dx, H, seed=k, scale=0.2 + 0.4 * k)[0]
        (la, ga), (lb, gb) = a.logdensity_and_gradient(q), b.logdensity_and_gradient(q)
        assert np.float64(la).tobytes() == np.float64(lb).tobytes() and ga.tobytes() == gb.tobytes()
