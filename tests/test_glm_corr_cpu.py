"""Correlated random effects (GLM(..., correlated=[glm.pair(..)]), idhmc_create_glm_corr) without a GPU: glm.pair and
the constructor's validation, glm.priors' fifth role, glm.correlated_effects, the host helpers on hand-made draws, the C boundary's
argument checks, and the C restatement of section 22's definition against a numpy restatement, whose gradient is held against mpmath's
differentiation (40 digits) of the log density written straight from the model, b = sigma .* (L u), L = [[1, 0], [rho, sqrt(1 - rho^2)]],
rho = tanh zeta.

The restatement is C_BODY_LOCAL of tests/test_glm_local_cpu.py with P and the partner table of the paired columns added to its params and
section 22 in its body: params are [n, K, nc, A, H, J, P, inv2, mu (D), tau (D), kind (D, as doubles; 5 marks a zeta with eta > 0, whose nu
entry holds eta), nu (D), c (nc), grp (Dx, as doubles), local (Dx, as doubles), cpart (Dx, as doubles: -1 or partner + 1024 pair +
2048 for the second column of its pair), X row-major (n x Dx, the expanded matrix of glm.expand_factors), Y row-major (n x K)],
D = Dx + A + H + J + P.  The GPU tests (tests/test_gpu_glm_corr.py) hand the same source to the oracle.

One sentence of the issue does not follow from its normative definition: "with eta > 0, l is -inf at zeta = 800".  By the definition
s = dexp(-800) = 0, t = 0, rho = 1, c = 0 and T takes 4 eta (800 - ln 2): every term is finite, and l is the finite value the exact
log density eta log(1 - rho^2) = -2 eta log cosh(zeta) has there.  (-inf is what log(1 - tanh(800)^2) gives when tanh is rounded to 1
first.)  test_the_ends_of_zeta asserts the definition's value, against -2 eta (|zeta| - ln 2)."""
import ctypes as C
import math

import numpy as np
import pytest

import test_glm_hier_cpu as HIER
from test_glm_factors_cpu import ITEM, SUBJECT, _data, _factors_struct
from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_local_cpu import C_BODY_LOCAL, inv2_of, numpy_density_local
from test_glm_priors_cpu import NORMAL, STUDENT_T, numpy_prior
from test_glm_slopes_cpu import DOSE, _values_struct

LKJ = 5            # the device table's (and the restatement's) mark of a zeta with eta > 0; never a public kind

_HEAD_OLD = """    const int K = (int)params[1], nc = (int)params[2], A = (int)params[3], H = (int)params[4], J = (int)params[5], Dx = D - A - H - J;
    const double inv2 = params[6];
    const double *mu = params + 7, *tau = mu + D, *kind = tau + D, *nu = kind + D, *c = nu + D, *grp = c + nc, *loc = grp + Dx, *X = loc + Dx,
                 *Y = X + n * Dx;
    const double *a = q + Dx, *om = q + Dx + A, *lam = q + Dx + A + H;
    double b[1024], st[1024], hh[1024];
"""
_HEAD_NEW = """    const int K = (int)params[1], nc = (int)params[2], A = (int)params[3], H = (int)params[4], J = (int)params[5], P = (int)params[6],
              Dx = D - A - H - J - P;
    const double inv2 = params[7];
    const double *mu = params + 8, *tau = mu + D, *kind = tau + D, *nu = kind + D, *c = nu + D, *grp = c + nc, *loc = grp + Dx, *cp = loc + Dx,
                 *X = cp + Dx, *Y = X + n * Dx;
    const double *a = q + Dx, *om = q + Dx + A, *lam = q + Dx + A + H, *zeta = q + D - P;
    double b[1024], st[1024], hh[1024], ut[1024];
    double rho[2] = {0.0, 0.0}, cc[2] = {1.0, 1.0}, M[2][128];
    for (int p = 0; p < P; ++p) {
        const double s = orc_exp(-fabs(zeta[p]));
        const double t = s * s, d = 1.0 + t;
        rho[p] = copysign((1.0 - t) / d, zeta[p]);
        cc[p] = (2.0 * s) / d;
    }
    for (int j = 0; j < Dx; ++j) {
        ut[j] = q[j];
        if (cp[j] >= 0.0 && ((int)cp[j] & 2048)) {
            const int e = (int)cp[j], p = (e >> 10) & 1;
            ut[j] = fma(rho[p], q[e & 1023], cc[p] * q[j]);
        }
    }
"""
_TAIL_OLD = """    for (int g = 0; g < H; ++g) grad[Dx + A + g] = orc_tree128(W[g]);
"""
_TAIL_NEW = """    for (int g = 0; g < H; ++g) grad[Dx + A + g] = orc_tree128(W[g]);
    for (int r = 0; r < 128; ++r) M[0][r] = M[1][r] = 0.0;
    for (int j = 0; j < Dx; ++j)
        if (cp[j] >= 0.0 && ((int)cp[j] & 2048)) {
            const int e = (int)cp[j], p = (e >> 10) & 1, c1 = e & 1023;
            M[p][j & 127] = M[p][j & 127] + grad[j] * (cc[p] * fma(cc[p], q[c1], -(rho[p] * q[j])));
        }
    for (int j = 0; j < Dx; ++j)
        if (cp[j] >= 0.0 && ((int)cp[j] & 2048)) {
            const int e = (int)cp[j], p = (e >> 10) & 1, c1 = e & 1023;
            const double gh = grad[j];
            grad[c1] = fma(rho[p], gh, grad[c1]);
            grad[j] = cc[p] * gh;
        }
    for (int p = 0; p < P; ++p) grad[D - P + p] = orc_tree128(M[p]);
"""
_LKJ_OLD = """        } else if (k == 2) {"""
_LKJ_NEW = """        } else if (k == 5) {
            const double z = fabs(d);
            const double s = orc_exp(-z);
            const double x = s * s;
            const double rh = copysign((1.0 - x) / (1.0 + x), d);
            T[r] = T[r] + (4.0 * f) * ((z + orc_log1p(x)) - 0.69314718055994530942);
            grad[j] = fma(-2.0 * f, rh, G);
        } else if (k == 2) {"""


def _body():
    s = C_BODY_LOCAL
    for old, new in ((_HEAD_OLD, _HEAD_NEW), (_TAIL_OLD, _TAIL_NEW), (_LKJ_OLD, _LKJ_NEW)):
        assert s.count(old) == 1
        s = s.replace(old, new)
    # everything between the head and the chain rules runs on ut where it ran on q: the two products that make b
    for old in ("b[j] = q[j] * st[j];", "b[j] = grp[j] >= 0.0 ? q[j] * e[(int)grp[j]] : q[j];"):
        assert s.count(old) == 1
        s = s.replace(old, old.replace("q[j]", "ut[j]"))
    return s


C_BODY_CORR = _body()


def c_source_corr(family):
    """C_BODY_CORR around the family's observation, as test_glm_local_cpu.c_source_local builds on HIER.c_source_hier"""
    body = HIER.c_source_hier(family)
    head, tail = HIER.C_BODY_HIER.split("%s")
    assert body.startswith(head) and body.endswith(tail)
    return C_BODY_CORR % body[len(head):len(body) - len(tail)]


def partner_table(Dx, pairs):
    """pairs: (off_first, off_second, N) per pair -> the table of the params (and of DevState::lr_cpart)"""
    cp = np.full(Dx, -1.0)
    for p, (o1, o2, N) in enumerate(pairs):
        for k in range(N):
            cp[o1 + k] = (o2 + k) + 1024 * p
            cp[o2 + k] = (o1 + k) + 1024 * p + 2048
    return cp


def twin_priors(kind, nu, eta):
    """the public kind and nu (D entries, the zetas last) with the internal mark where eta > 0"""
    kind, nu = np.array(kind, float), np.array(nu, float)
    P = len(eta)
    for p, e in enumerate(eta):
        if e > 0.0:
            kind[kind.size - P + p], nu[nu.size - P + p] = LKJ, e
    return kind, nu


def oracle_params_corr(Xe, Y, A, grp, local, S, kind, nu, pairs, eta, c=None, mu=None, tau=None):
    n, Dx = Xe.shape
    grp = np.full(Dx, -1) if grp is None else np.asarray(grp)
    local = np.zeros(Dx) if local is None else np.asarray(local, float)
    H, J, P = int(grp.max()) + 1, int(local.sum()), len(pairs)
    D = Dx + A + H + J + P
    Y = np.asarray(Y, float).reshape(n, -1)
    c = np.zeros(0) if c is None else np.asarray(c, float)
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    kind, nu = twin_priors(np.broadcast_to(np.asarray(kind, float), (D,)), np.broadcast_to(np.asarray(nu, float), (D,)), eta)
    return np.concatenate([[float(n), float(Y.shape[1]), float(c.size), float(A), float(H), float(J), float(P), inv2_of(S)], mu, tau, kind, nu, c,
                           grp.astype(float), local, partner_table(Dx, pairs), np.asarray(Xe, float).ravel(), Y.ravel()])


def numpy_density_corr(family, Xe, Y, q, grp, local, S, kind, nu, pairs, eta, mu=None, tau=None):
    """(l(q), grad l(q), magnitude of l's terms, per-coordinate magnitude of the terms summed into grad), q = [u | a | omega | lambda | zeta],
    from rho = tanh zeta, c = 1 / cosh zeta: section 19's closed form at ut, its prior moved so that it sees q - mu, then the chain rule"""
    P = len(pairs)
    D, D0 = q.size, q.size - P
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    kind, nu = np.broadcast_to(np.asarray(kind), (D,)), np.broadcast_to(np.asarray(nu, float), (D,))
    zeta = q[D0:]
    rho, c = np.tanh(zeta), 2.0 * np.exp(-np.abs(zeta)) / (1.0 + np.exp(-2.0 * np.abs(zeta)))      # 1 / cosh, without its overflow
    qt = q[:D0].copy()
    for p, (o1, o2, N) in enumerate(pairs):
        qt[o2:o2 + N] = rho[p] * q[o1:o1 + N] + c[p] * q[o2:o2 + N]
    mu0 = mu[:D0] + (qt - q[:D0])                          # d = qt - mu0 = q - mu: the prior of u is on u
    l0, g0, ls0, gs0 = numpy_density_local(family, Xe, Y, qt, grp, local, S, kind[:D0], nu[:D0], mu0, tau[:D0])
    _, pg, _, pgmag = numpy_prior(kind[:D0], nu[:D0], mu0, tau[:D0], qt)
    Gh, Ghmag = g0 - pg, gs0 - pgmag                       # the likelihood's part, dl / dut
    g, gs = np.r_[g0, np.zeros(P)], np.r_[gs0, np.zeros(P)]
    l, ls = l0, ls0
    for p, (o1, o2, N) in enumerate(pairs):
        a, b = slice(o1, o1 + N), slice(o2, o2 + N)
        g[a] += rho[p] * Gh[b]
        gs[a] += abs(rho[p]) * Ghmag[b]
        g[b] = c[p] * Gh[b] + pg[b]
        gs[b] = c[p] * Ghmag[b] + pgmag[b]
        m = Gh[b] * c[p] * (c[p] * q[a] - rho[p] * q[b])
        mmag = Ghmag[b] * c[p] * (c[p] * np.abs(q[a]) + abs(rho[p]) * np.abs(q[b]))
        cz = D0 + p
        if eta[p] > 0.0:
            z = abs(zeta[p])
            lp = -2.0 * eta[p] * ((z + np.log1p(np.exp(-2.0 * z))) - math.log(2.0))
            pgz, lmag, gmag = -2.0 * eta[p] * rho[p], 2.0 * eta[p] * (z + math.log(2.0)), 2.0 * eta[p] * abs(rho[p])
        else:
            lp, pgz, lmag, gmag = (x[0] for x in numpy_prior(kind[cz:cz + 1], nu[cz:cz + 1], mu[cz:cz + 1], tau[cz:cz + 1], q[cz:cz + 1]))
        g[cz], gs[cz] = m.sum() + pgz, mmag.sum() + gmag
        l, ls = l + lp, ls + lmag
    return l, g, ls, gs


def make_corr(idhmc, family, X, Y, factors, grp, local, S, kind, nu, mu, tau, correlated, **kw):
    return idhmc.GLM(X, Y, source(idhmc, family), consts(family), mu, tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu,
                     local=local, slab_scale=S, factors=factors, correlated=correlated, **kw)


# ---- glm.pair, the constructor and the host helpers -----------------------------------------------------------------------------------
def _slope_model(idhmc, correlated=None, **kw):
    X, Y = _data()
    g = idhmc.glm
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[SUBJECT, g.term(SUBJECT, values=DOSE)], correlated=correlated, **kw)


def test_pair_is_a_small_named_tuple(idhmc):
    g = idhmc.glm
    p = g.pair(0, 1)
    assert isinstance(p, tuple) and p._fields == ("first", "second", "eta") and p == (0, 1, 2.0) and g.pair(1, 0, eta=0.5).eta == 0.5


def test_constructor_keeps_the_pairs(idhmc):
    g = idhmc.glm
    m = _slope_model(idhmc, [g.pair(0, 1, eta=2.0)], groups=g.random_effects(2, [4, 4])["groups"])
    assert (m.Dx, m.A, m.H, m.J, m.P, m.D) == (10, 0, 2, 0, 1, 13) and m.pairs == [g.Pair(0, 1, 2.0)]
    assert m.pair_first.dtype == np.int32 and list(m.pair_first) == [0] and list(m.pair_second) == [1] and list(m.pair_eta) == [2.0]
    assert m.mu is None and m.glm_desc().Dx == 10         # the defaults: what an LKJ zeta needs
    # second before first, two plain terms, and two pairs
    X, Y = _data()
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[(ITEM, 3), SUBJECT, (ITEM, 4), (SUBJECT % 3, 3)], correlated=[g.pair(2, 1, 0.0), g.pair(0, 3, 1)])
    assert (m.P, m.D) == (2, 2 + 14 + 2) and m.pairs == [g.Pair(2, 1, 0.0), g.Pair(0, 3, 1.0)]
    # without pairs: the model without the keyword
    for kw in ({}, {"correlated": None}, {"correlated": []}):
        m = _slope_model(idhmc, **kw)
        assert m.P == 0 and m.pairs is None and m.pair_first is None and m.pair_eta is None and m.D == 10
    assert idhmc.GLM(X, Y, g.POISSON_LOG).P == 0
    # eta = 0: the entry of the prior arrays applies, normal or Student-t
    kw = g.priors(10, 0, 2, P=1, correlations=g.student_t(4, 0.0, 1.5))
    m = _slope_model(idhmc, [g.pair(0, 1, eta=0)], groups=g.random_effects(2, [4, 4])["groups"], **kw)
    assert m.prior_kind[12] == STUDENT_T and m.prior_nu[12] == 4.0 and m.tau[12] == pytest.approx(1.0 / 1.5 ** 2)


def test_constructor_validates_pairs(idhmc):
    g = idhmc.glm
    X, Y = _data()
    fac = [SUBJECT, g.term(SUBJECT, values=DOSE), (ITEM, 3)]

    def bad(what, correlated, factors=fac, **kw):
        with pytest.raises(ValueError, match=what):
            idhmc.GLM(X, Y, g.POISSON_LOG, factors=factors, correlated=correlated, **kw)
    bad("correlated must be a list of glm.pair", g.pair(0, 1))
    bad("correlated must be a list of glm.pair", 3)
    bad(r"correlated\[0\] must be a glm.pair", [(0, 1)])
    bad("at most 2 correlated pairs", [g.pair(0, 1)] * 3)
    bad("correlated pairs need factor terms", [g.pair(0, 1)], factors=None)
    bad("correlated pairs need factor terms", [g.pair(0, 1)], factors=[])
    for t in (3, -1, 0.5, True):
        bad(r"correlated\[0\]: first = .* is outside 0..2", [g.pair(t, 1)])
        bad(r"correlated\[0\]: second = .* is outside 0..2", [g.pair(0, t)])
    bad(r"correlated\[0\]: first = second = 1", [g.pair(1, 1)])
    bad(r"correlated\[1\]: term 0 is in two pairs", [g.pair(0, 1), g.pair(2, 0)], factors=[SUBJECT, (SUBJECT, 4), (ITEM, 4)])
    bad(r"correlated\[0\]: terms 0 and 2 have 4 and 3 levels", [g.pair(0, 2)])
    for e in (-1.0, np.inf, np.nan, "2", True):
        bad(r"correlated\[0\]: eta = .* must be finite and >= 0", [g.pair(0, 1, e)])
    # the prior arrays on a zeta: D = 2 + 11 + 1 = 14, zeta is coordinate 13
    D = 14
    for name, val in (("prior_mu", 0.1), ("prior_tau", 2.0)):
        arr = np.zeros(D) if name == "prior_mu" else np.ones(D)
        arr[13] = val
        bad(r"correlated\[0\]: eta = 2.0 is the LKJ prior of zeta: the entry of coordinate 13", [g.pair(0, 1)], **{name: arr})
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[13], nu[13] = STUDENT_T, 3.0
    bad(r"correlated\[0\]: eta = 2.0 is the LKJ prior of zeta", [g.pair(0, 1)], prior_kind=kind, prior_nu=nu)
    idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, correlated=[g.pair(0, 1, 0.0)], prior_kind=kind, prior_nu=nu)       # eta = 0: it applies
    for k in (2, 3, 4):
        kind[13], nu[13] = k, 3.0 if k == 3 else 0.0
        for e in (0.0, 2.0):
            bad(r"correlated\[0\]: prior_kind\[13\] = PRIOR_LOG_.* is a prior on exp\(q\): coordinate 13 is zeta", [g.pair(0, 1, e)],
                prior_kind=kind, prior_nu=nu)
    kind[13] = 5
    bad(r"prior_kind\[13\] = 5 must be an integer in 0..4", [g.pair(0, 1)], prior_kind=kind)
    with pytest.raises(ValueError, match=r"limited to D <= 1024 \(D = 1025\)"):
        idhmc.GLM(np.ones((2, 2)), np.zeros(2), g.POISSON_LOG, factors=[(np.zeros(2, int), 511), (np.zeros(2, int), 511)], correlated=[g.pair(0, 1)])
    assert idhmc.GLM(np.ones((2, 1)), np.zeros(2), g.POISSON_LOG, factors=[(np.zeros(2, int), 511), (np.zeros(2, int), 511)],
                     correlated=[g.pair(0, 1)]).D == 1024


def test_priors_builder_takes_the_correlations(idhmc):
    g = idhmc.glm
    kw = g.priors(3, 1, 2, 2, scales=g.exponential(2.0), P=2, correlations=[g.normal(0.0, 0.5), g.student_t(3)])
    assert list(kw["prior_kind"]) == [0, 0, 0, 0, 4, 4, 0, 0, 0, 1] and list(kw["prior_nu"]) == [0] * 9 + [3.0]
    assert kw["prior_tau"][8] == 4.0 and kw["prior_mu"].size == 10
    assert g.priors(3, 1, 2, 2)["prior_kind"].size == 8 and g.priors(3, 1, 2, 2, P=1)["prior_kind"].size == 9     # positional calls keep their meaning
    with pytest.raises(TypeError):
        g.priors(3, 1, 2, 2, None, None, None, None, 1)          # P is keyword-only
    for bad in (dict(P=1, correlations=g.half_normal()), dict(P=1, correlations=[g.exponential()]), dict(P=2, correlations=[g.normal()]),
                dict(P=-1)):
        with pytest.raises(ValueError):
            g.priors(3, **bad)


def test_correlated_effects_assembles_the_model(idhmc):
    g = idhmc.glm
    kw = g.correlated_effects(2, [4, 4], [(0, 1)], eta=1.5, scale=g.half_student_t(3))
    assert sorted(kw) == ["correlated", "groups", "prior_kind", "prior_mu", "prior_nu", "prior_tau"]
    base = g.random_intercepts(2, [4, 4], scale=g.half_student_t(3))
    assert kw["correlated"] == [g.Pair(0, 1, 1.5)] and np.array_equal(kw["groups"], base["groups"])
    for k in ("prior_kind", "prior_mu", "prior_nu", "prior_tau"):
        assert np.array_equal(kw[k][:-1], base[k]) and kw[k].size == 13
    assert (kw["prior_kind"][-1], kw["prior_mu"][-1], kw["prior_tau"][-1], kw["prior_nu"][-1]) == (0, 0.0, 1.0, 0.0)
    m = _slope_model(idhmc, **kw)
    assert (m.H, m.P, m.D) == (2, 1, 13)
    kw = g.correlated_effects(1, [3, 3, 5, 5], [(0, 1), (3, 2)], eta=[1.0, 4.0], A=1)
    assert kw["correlated"] == [g.Pair(0, 1, 1.0), g.Pair(3, 2, 4.0)] and kw["prior_mu"].size == 1 + 16 + 1 + 4 + 2
    for bad in (dict(pairs=[(0, 1)] * 3), dict(pairs=[(0, 0)]), dict(pairs=[(0, 2)]), dict(pairs=[(0, 1)], eta=0.0), dict(pairs=[(0, 1)], eta=[1.0, 2.0]),
                dict(pairs=[0, 1]), dict(pairs=[(0, 1)], eta=-1.0)):
        args = dict(Dd=2, levels=[4, 4, 3], pairs=[(0, 1)])
        args.update(bad)
        with pytest.raises(ValueError):
            g.correlated_effects(**args)


def test_host_helpers_on_hand_made_draws(idhmc):
    g = idhmc.glm
    m = _slope_model(idhmc, **g.correlated_effects(2, [4, 4], [(0, 1)]))
    draws = np.zeros((2, 3, 13))
    draws[..., :2] = [1.0, -2.0]
    draws[..., 2:6] = [1.0, 2.0, 3.0, 4.0]
    draws[..., 6:10] = [0.5, -0.5, 0.25, 0.0]
    draws[..., 10:12] = np.log([2.0, 0.5])
    draws[..., 12] = np.arctanh(0.6)
    draws[1, 2, 12] = -np.arctanh(0.8)
    rho = g.correlations(m, draws)
    assert rho.shape == (2, 3, 1) and np.allclose(rho[0, 0], 0.6, rtol=1e-15) and np.isclose(rho[1, 2, 0], -0.8, rtol=1e-15)
    beta = g.coefficients(m, draws)
    u1, u2 = np.array([1.0, 2.0, 3.0, 4.0]), np.array([0.5, -0.5, 0.25, 0.0])
    assert beta.shape == (2, 3, 10) and np.allclose(beta[0, 0], np.r_[1.0, -2.0, 2.0 * u1, 0.5 * (0.6 * u1 + 0.8 * u2)], rtol=1e-14)
    assert np.allclose(beta[1, 2, 6:], 0.5 * (-0.8 * u1 + 0.6 * u2), rtol=1e-14)
    assert np.allclose(g.group_scales(m, draws), [2.0, 0.5], rtol=1e-15) and g.local_scales(m, draws).shape == (2, 3, 0)
    for f in (g.correlations, g.coefficients, g.group_scales, g.local_scales):
        with pytest.raises(ValueError, match="13 coordinates"):
            f(m, draws[..., :12])
    # the ends: rho is exactly +-1 and every coefficient finite
    d = np.zeros((3, 13))
    d[:, 2:10], d[:, 12] = 1.0, [800.0, -800.0, 0.0]
    assert list(g.correlations(m, d)[:, 0]) == [1.0, -1.0, 0.0] and np.isfinite(g.coefficients(m, d)).all()
    assert np.array_equal(g.coefficients(m, d)[:, 6:], [[1.0] * 4, [-1.0] * 4, [1.0] * 4])
    # local scales next to pairs: the lambdas end where the zetas begin
    kw = g.correlated_effects(2, [4, 4], [(0, 1)])
    kw = {k: (np.r_[v[:12], np.zeros(4) if k != "prior_tau" else np.ones(4), v[12:]].astype(v.dtype) if k.startswith("prior_") else v)
          for k, v in kw.items()}
    m = _slope_model(idhmc, local=[0] * 6 + [1] * 4, **kw)
    d = np.zeros((2, 17))
    d[:, 12:16] = np.log([1.0, 2.0, 3.0, 4.0])
    assert (m.J, m.P, m.D) == (4, 1, 17) and np.allclose(g.local_scales(m, d), [1.0, 2.0, 3.0, 4.0]) and g.correlations(m, d).shape == (2, 1)
    # a model without pairs: an empty last axis
    m = _slope_model(idhmc)
    assert g.correlations(m, np.zeros((4, 10))).shape == (4, 0)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def _pairs_struct(P, first, second, eta):
    from inplacedhmc_jl_amd import _lib
    keep = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((first, np.int32), (second, np.int32), (eta, np.float64))]
    pp = _lib.GlmPairs(P=P)
    if keep[0] is not None:
        pp.first = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
    if keep[1] is not None:
        pp.second = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
    if keep[2] is not None:
        pp.eta = keep[2].ctypes.data_as(C.POINTER(C.c_double))
    return pp, keep


def _priors_struct(kind, nu):
    from inplacedhmc_jl_amd import _lib
    keep = [np.ascontiguousarray(kind, dtype=np.int32), np.ascontiguousarray(nu, dtype=np.float64)]
    return _lib.GlmPriors(kind=keep[0].ctypes.data_as(C.POINTER(C.c_int32)), nu=keep[1].ctypes.data_as(C.POINTER(C.c_double))), keep


def _create(idhmc, desc, factors, values, pairs, priors=None, M=1, R=0, opt=None, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create_glm_corr(C.byref(h), 0, nchains, 0, C.byref(desc), None if priors is None else C.byref(priors), None,
                                   None if factors is None else C.byref(factors), None if values is None else C.byref(values),
                                   None if pairs is None else C.byref(pairs), M, R, None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def _c_model(idhmc, correlated="default"):
    g = idhmc.glm
    X, Y = _data()
    corr = [g.pair(0, 1)] if correlated == "default" else correlated
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[SUBJECT, g.term(SUBJECT, values=DOSE), (ITEM, 3)], correlated=corr,
                     groups=[-1, -1] + [0] * 4 + [1] * 4 + [-1] * 3)


def test_good_pairs_pass_every_check(idhmc):
    """a valid descriptor reaches the device (or its absence): with a pair, with pairs = NULL, with P = 0 and its arrays NULL"""
    ok = (0, idhmc.ERR_NO_DEVICE)
    m = _c_model(idhmc)
    fc, k1 = _factors_struct(3, m.levels, m.factor_index)
    fv, k2 = _values_struct(m.factor_values, m.factor_has)
    pp, k3 = _pairs_struct(1, m.pair_first, m.pair_second, m.pair_eta)
    rc, msg = _create(idhmc, m.glm_desc(), fc, fv, pp)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    m0 = _c_model(idhmc, None)
    for pairs in (None, _pairs_struct(0, None, None, None)[0]):
        rc, msg = _create(idhmc, m0.glm_desc(), fc, fv, pairs)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    # eta = 0 with a Student-t entry on zeta
    m1 = _c_model(idhmc, [idhmc.glm.pair(1, 0, 0.0)])
    kind, nu = np.zeros(m1.D, np.int32), np.zeros(m1.D)
    kind[-1], nu[-1] = STUDENT_T, 3.0
    pr, k4 = _priors_struct(kind, nu)
    pp, k3 = _pairs_struct(1, [1], [0], [0.0])
    rc, msg = _create(idhmc, m1.glm_desc(), fc, fv, pp, pr)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)


def test_bad_pairs_are_refused_before_the_device(idhmc):
    m = _c_model(idhmc)
    lib = idhmc.load_library()
    D = m.D                                                        # 2 + 11 + 2 + 1 = 16, zeta is coordinate 15

    def refused(what, P=1, first=(0,), second=(1,), eta=(2.0,), F=3, levels=(4, 4, 3), factors=True, desc=None, priors=None, **kw):
        fc, k1 = _factors_struct(F, levels, m.factor_index)
        fv, k2 = _values_struct(m.factor_values, m.factor_has)
        pp, k3 = _pairs_struct(P, first, second, eta)
        pr, k4 = (None, None) if priors is None else _priors_struct(*priors)
        rc, msg = _create(idhmc, m.glm_desc() if desc is None else desc, fc if factors else None, fv if factors and F else None, pp, pr, **kw)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    h = C.c_void_p()
    assert lib.idhmc_create_glm_corr(C.byref(h), 0, 4, 0, None, None, None, None, None, None, 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert b"idhmc_create_glm_corr: null argument" in lib.idhmc_last_error()
    assert lib.idhmc_create_glm_corr(None, 0, 4, 0, C.byref(m.glm_desc()), None, None, None, None, None, 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert lib.idhmc_glm_pairs_get(None, None, None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    for P in (-1, 3, 1 << 20):
        refused(b"P = %d pairs must be an integer in 0..2" % P, P=P)
    refused(b"need first, second and eta (first is NULL)", first=None)
    refused(b"need first, second and eta (second is NULL)", second=None)
    refused(b"need first, second and eta (eta is NULL)", eta=None)
    for t in (-1, 3):
        refused(b"pair 0: first = %d is outside 0..2" % t, first=(t,))
        refused(b"pair 0: second = %d is outside 0..2" % t, second=(t,))
    refused(b"pair 0: first = second = 1", first=(1,))
    refused(b"pair 1: term 0 is in two pairs", P=2, first=(0, 2), second=(1, 0), eta=(2.0, 2.0), levels=(4, 4, 4))
    refused(b"pair 0: terms 0 and 2 have 4 and 3 levels", second=(2,))
    for e in (-1.0, np.inf, np.nan):
        refused(b"must be finite and >= 0", eta=(e,))
    # the prior arrays on zeta
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[15], nu[15] = STUDENT_T, 3.0
    refused(b"pair 0: eta = 2 is the LKJ prior of zeta: the entry of coordinate 15", priors=(kind, nu))
    for name, val in (("mu", 0.5), ("tau", 2.0)):
        arr = np.zeros(D) if name == "mu" else np.ones(D)
        arr[15] = val
        d = m.glm_desc()
        setattr(d, name, arr.ctypes.data_as(C.POINTER(C.c_double)))
        refused(b"pair 0: eta = 2 is the LKJ prior of zeta", desc=d)
    for k in (2, 3, 4):
        kind[15], nu[15] = k, 3.0 if k == 3 else 0.0
        for e in (0.0, 2.0):
            refused(b"pair 0: prior kind[15] = %d is a prior on exp(q): coordinate 15 is zeta" % k, eta=(e,), priors=(kind, nu))
    kind[15], nu[15] = 5, 0.0
    refused(b"prior kind[15] = 5 is outside 0..4", eta=(0.0,), priors=(kind, nu))
    # pairs without factors
    X, Y = _data()
    m0 = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, groups=[0, -1])
    refused(b"pairs need factor terms (factors is NULL)", factors=False, desc=m0.glm_desc())
    refused(b"pairs need factor terms (factors is given with F = 0)", F=0, desc=m0.glm_desc())
    # D counts P
    d = m.glm_desc()
    d.Dx = 1022
    refused(b"D = Dx + A + H + J + P = 1025: a GLM is limited to D <= 1024 (P = 1 pairs)", desc=d)
    # everything idhmc_create_glm_slopes refuses
    refused(b"F = 5 factors must be an integer in 0..4", F=5)
    refused(b"levels[1] = 0: at least one level", levels=(4, 0, 3))
    d = m.glm_desc()
    d.H = 3
    refused(b"group 2 has no column", desc=d)
    refused(b"chains_per_response = 0", M=2, R=0)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def small_problem(idhmc, family, n, Dd, N, valued=True, seed=0, two=False):
    """(X dense, Y, factors, Xe, grp, pairs as (off_first, off_second, N)): a plain and a valued (or plain) term of N levels on one index,
    each a group; two: two more terms of N + 1 levels on another index, the second pair (3, 2) with its second term in front"""
    g = idhmc.glm
    rng = np.random.default_rng(seed + n + N)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    s = rng.integers(0, N, n)
    w = 0.5 * rng.standard_normal(n)
    factors = [(s, N), g.term(s, values=w, levels=N) if valued else (rng.integers(0, N, n), N)]
    pairs = [(Dd, Dd + N, N)]
    if two:
        t = rng.integers(0, N + 1, n)
        factors += [g.term(t, values=0.5 * rng.standard_normal(n), levels=N + 1), (t, N + 1)]
        pairs.append((Dd + 3 * N + 1, Dd + 2 * N, N + 1))
    Xe = g.expand_factors(X, factors)
    Dx = Xe.shape[1]
    grp = np.full(Dx, -1, np.int32)
    grp[Dd:Dd + N], grp[Dd + N:Dd + 2 * N] = 0, 1
    if two:
        grp[Dd + 2 * N:] = 2
    z = Xe @ (0.4 * rng.standard_normal(Dx))
    Y = rng.poisson(np.exp(z)).astype(float) if family == "POISSON_LOG" else z + 0.5 * rng.standard_normal(n)
    return X, Y, factors, Xe, grp, pairs


def start_corr(family, C_, Dx, H, J, P, seed=0, zeta=None):
    from test_glm_local_cpu import start_local
    rng = np.random.default_rng(seed + 77)
    z = rng.uniform(-0.8, 0.8, (C_, P)) if zeta is None else np.broadcast_to(np.asarray(zeta, float), (C_, P))
    return np.concatenate([start_local(family, C_, Dx, H, J, seed), z], 1)


@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    work = {}

    def model(family, Xe, Y, grp, local, S, kind, nu, pairs, eta, mu=None, tau=None):
        if family not in work:
            work[family] = str(tmp_path_factory.mktemp("corr_" + family.lower()))
        A, H, J = SHAPE[family][2], int(np.max(grp)) + 1, 0 if local is None else int(np.sum(local))
        D = Xe.shape[1] + A + H + J + len(pairs)
        return oracle.OracleModel.custom(D, c_source_corr(family), oracle_params_corr(Xe, Y, A, grp, local, S, kind, nu, pairs, eta, consts(family), mu, tau),
                                         work[family])
    return model


CASES = [("POISSON_LOG", 1, 3, 4, False, None), ("POISSON_LOG", 37, 20, 15, False, None), ("GAUSSIAN_IDENTITY_LOGSIGMA", 130, 100, 20, False, 2.0),
         ("GAUSSIAN_IDENTITY_LOGSIGMA", 60, 8, 6, True, None), ("POISSON_LOG", 200, 10, 12, True, 1.5)]


def case_priors(D, P, eta, seed):
    """normal and Student-t on the coordinates in front, the defaults on a zeta with eta > 0 and a Student-t entry on one with eta = 0"""
    rng = np.random.default_rng(seed)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:D - P:2] = STUDENT_T
    nu[kind == STUDENT_T] = 4.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    for p in range(P):
        cz = D - P + p
        if eta[p] > 0.0:
            kind[cz], nu[cz], mu[cz], tau[cz] = NORMAL, 0.0, 0.0, 1.0
        else:
            kind[cz], nu[cz] = STUDENT_T, 3.0
    return kind, nu, mu, tau


@pytest.mark.parametrize("family,n,Dd,N,two,S", CASES, ids=["%s-n%d-Dd%d-N%d%s%s" % (c[0][:4], c[1], c[2], c[3], "-two" if c[4] else "", "-slab" if c[5] else "")
                                                          for c in CASES])
def test_restatement_matches_numpy(idhmc, restated, family, n, Dd, N, two, S):
    X, Y, factors, Xe, grp, pairs = small_problem(idhmc, family, n, Dd, N, two=two)
    Dx, A, H, P = Xe.shape[1], SHAPE[family][2], int(grp.max()) + 1, len(pairs)
    local = None
    if S:
        local = np.zeros(Dx, np.int32)
        local[Dd + N::2] = 1                               # on the second term's columns (and beyond)
    J = 0 if local is None else int(local.sum())
    D = Dx + A + H + J + P
    eta = [2.0, 0.0][:P]
    kind, nu, mu, tau = case_priors(D, P, eta, n)
    om = restated(family, Xe, Y, grp, local, S, kind, nu, pairs, eta, mu, tau)
    for k in range(3):
        q = start_corr(family, 1, Dx, H, J, P, seed=k)[0]
        if k == 2:
            q[D - P:] = -q[D - P:] - 1.0
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_corr(family, Xe, Y, q, grp, np.zeros(Dx, int) if local is None else local, S, kind, nu, pairs,
                                                          eta, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), np.max(np.abs(g[:D] - g_ref) / gscale)


def test_numpy_gradient_is_mpmath_derivative_of_the_model():
    """Poisson with a log link, Dd = 2, (1 + x | s) with 3 subjects, a group per term, LKJ(2): the log density written in mpmath straight
    from b = sigma .* (L u), differentiated numerically at 40 digits; numpy's l and gradient within 1e-12 of their terms' magnitude"""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(4)
    n, Dd, N, eta = 14, 2, 3, 2.0
    X = 0.5 * rng.standard_normal((n, Dd))
    s, w = rng.integers(0, N, n), rng.standard_normal(n)
    Y = rng.poisson(1.5, n).astype(float)
    Dx, D = Dd + 2 * N, Dd + 2 * N + 2 + 1
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    mu[-1], tau[-1] = 0.0, 1.0
    Xe = np.zeros((n, Dx))
    Xe[:, :Dd] = X
    Xe[np.arange(n), Dd + s] = 1.0
    Xe[np.arange(n), Dd + N + s] = w
    grp = np.r_[[-1] * Dd, [0] * N, [1] * N]

    def logp(*q):
        u, om, zeta = q[:Dx], q[Dx:Dx + 2], q[Dx + 2]
        rho = mp.tanh(zeta)
        L = [[mp.mpf(1), mp.mpf(0)], [rho, mp.sqrt(1 - rho * rho)]]
        sig = [mp.exp(om[0]), mp.exp(om[1])]
        b = list(u[:Dd])
        eff = [[sig[r] * (L[r][0] * u[Dd + k] + L[r][1] * u[Dd + N + k]) for k in range(N)] for r in range(2)]
        total = mp.mpf(0)
        for i in range(n):
            z = sum(mp.mpf(float(X[i, c])) * b[c] for c in range(Dd)) + eff[0][s[i]] + mp.mpf(float(w[i])) * eff[1][s[i]]
            total += mp.mpf(float(Y[i])) * z - mp.exp(z)
        for c in range(D - 1):
            total -= mp.mpf(float(tau[c])) * (q[c] - mp.mpf(float(mu[c]))) ** 2 / 2
        return total + eta * mp.log(1 - rho * rho)

    for k, zeta in enumerate((0.7, -1.3, 0.0)):
        q = np.r_[rng.uniform(-0.8, 0.8, Dx), np.log(0.6) + rng.uniform(-0.3, 0.3, 2), zeta]
        l, g, ls, gs = numpy_density_corr("POISSON_LOG", Xe, Y, q, grp, np.zeros(Dx, int), None, np.zeros(D, int), np.zeros(D), [(Dd, Dd + N, N)],
                                          [eta], mu, tau)
        qm = [mp.mpf(float(x)) for x in q]
        assert abs(float(logp(*qm) - mp.mpf(l))) <= 1e-12 * ls
        for c in range(D):
            order = tuple(1 if j == c else 0 for j in range(D))
            ref = mp.diff(logp, tuple(qm), order)
            assert abs(float(ref - mp.mpf(float(g[c])))) <= 1e-12 * gs[c] + 1e-300, (zeta, c, float(ref), g[c])


def test_lkj_makes_rho_a_symmetric_beta():
    """exp(eta log(1 - rho^2)) d zeta is Beta(eta, eta) in (rho + 1) / 2: the density of zeta integrates to the Beta's CDF"""
    from scipy import integrate, stats
    for eta in (0.5, 1.0, 2.0, 5.0):
        f = lambda z: np.cosh(z) ** (-2.0 * eta)               # 1 - tanh^2 = 1 / cosh^2
        quad = lambda a, b: integrate.quad(f, a, b, epsabs=1e-13, epsrel=1e-13, limit=400)[0]
        Z = quad(-60, 0) + quad(0, 60)
        for z in (-1.0, 0.3, 2.0):
            assert (quad(-60, -1.0) + quad(-1.0, z)) / Z == pytest.approx(stats.beta(eta, eta).cdf((np.tanh(z) + 1.0) / 2.0), abs=1e-9)


def test_zeta_zero_and_no_pairs_give_the_bits_of_section_19(idhmc, restated, oracle, tmp_path):
    """at zeta = +0 with eta = 0 and a normal entry the first D - P coordinates of the gradient and (with zeta's mu = 0) l are bit for bit
    those of test_glm_local_cpu's restatement on the model without the pair; with P = 0 the two restatements agree on everything"""
    from test_glm_local_cpu import c_source_local, oracle_params_local
    family = "GAUSSIAN_IDENTITY_LOGSIGMA"
    X, Y, factors, Xe, grp, pairs = small_problem(idhmc, family, 50, 5, 7)
    Dx, A, H = Xe.shape[1], 1, 2
    D = Dx + A + H + 1
    kind, nu, mu, tau = case_priors(D, 1, [0.0], 3)
    kind[-1], nu[-1], mu[-1] = NORMAL, 0.0, 0.0
    om = restated(family, Xe, Y, grp, None, None, kind, nu, pairs, [0.0], mu, tau)
    base = oracle.OracleModel.custom(D - 1, c_source_local(family), oracle_params_local(Xe, Y, A, grp, None, None, kind[:-1], nu[:-1], None, mu[:-1], tau[:-1]),
                                     str(tmp_path))
    none = restated(family, Xe, Y, grp, None, None, kind[:-1], nu[:-1], [], [], mu[:-1], tau[:-1])
    for k in range(3):
        q = start_corr(family, 1, Dx, H, 0, 1, seed=k, zeta=0.0)[0]
        l1, g1 = om.logdensity_and_gradient(q)
        l0, g0 = base.logdensity_and_gradient(q[:-1])
        l2, g2 = none.logdensity_and_gradient(q[:-1])
        assert l1 == l0 == l2 and np.array_equal(g1[:-1], g0) and np.array_equal(g2, g0) and np.isfinite(g1[-1]) and g1[-1] != 0.0


def test_the_ends_of_zeta(idhmc, restated):
    """zeta = +-40 and 800: with eta = 0 every output is finite; with eta > 0 l is finite at 40 -- and at 800 too, where the definition
    gives rho = 1, c = 0 and T = 4 eta (800 - ln 2), the exact -2 eta log cosh (see the module docstring on the issue's "-inf")"""
    family = "POISSON_LOG"
    X, Y, factors, Xe, grp, pairs = small_problem(idhmc, family, 30, 3, 5)
    Dx, H = Xe.shape[1], 2
    D = Dx + H + 1
    for eta in (0.0, 2.0):
        kind, nu, mu, tau = case_priors(D, 1, [eta], 5)
        if eta == 0.0:
            kind[-1], nu[-1], mu[-1], tau[-1] = STUDENT_T, 3.0, 0.0, 1.0
        om = restated(family, Xe, Y, grp, None, None, kind, nu, pairs, [eta], mu, tau)
        q0 = start_corr(family, 1, Dx, H, 0, 1, zeta=0.0)[0]
        l0, _ = om.logdensity_and_gradient(q0)
        for zeta in (40.0, -40.0, 800.0, -800.0):
            q = q0.copy()
            q[-1] = zeta
            lq, g = om.logdensity_and_gradient(q)
            assert np.isfinite(lq) and np.isfinite(g[:D]).all(), (eta, zeta)
            if abs(zeta) == 800.0:
                # rho = +-1, c = 0: the second term's columns see their prior only, and zeta's likelihood term is exactly 0
                cols = np.array([c for c in range(pairs[0][1], pairs[0][1] + 5) if kind[c] == NORMAL])
                assert cols.size and np.array_equal(g[cols], -tau[cols] * (q - mu)[cols])
                if eta > 0.0:
                    assert g[D - 1] == -2.0 * eta * np.sign(zeta)
            if eta > 0.0:
                # the prior's part of l is -2 eta (|zeta| - ln 2) to rounding at both sizes: a finite number, -3197.2 at 800
                l_like, *_ = numpy_density_corr(family, Xe, Y, q, grp, np.zeros(Dx, int), None, kind, nu, pairs, [eta], mu, tau)
                assert lq == pytest.approx(l_like, rel=1e-12)
                other = numpy_density_corr(family, Xe, Y, q, grp, np.zeros(Dx, int), None, kind, nu, pairs, [1e-300], mu, tau)[0]
                assert l_like - other == pytest.approx(-2.0 * eta * (abs(zeta) - math.log(2.0)), rel=1e-9)
