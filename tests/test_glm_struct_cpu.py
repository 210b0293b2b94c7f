"""Structured factor terms (GLM(..., structured=[glm.ar1(..) / glm.rw1(..)]), idhmc_create_glm_struct) without a GPU:
glm.ar1 / glm.rw1 and the constructor's validation, glm.priors' sixth role, glm.structured_effects, the host helpers on hand-made draws
(the scan against exact-rational fma), the C boundary's argument checks, and the C restatement of section 23's definition against a
numpy restatement, whose gradient is held against mpmath's differentiation (40 digits) of the log density written straight from the
model -- the sequential recurrence ut_0 = u_0, ut_k = phi ut_{k-1} + sqrt(1 - phi^2) u_k, phi = tanh zeta.

The restatement is C_BODY_CORR of tests/test_glm_corr_cpu.py with S, Sz, the level table of the structured columns and the slots' levels
and kinds added to its params and section 23 in its body: params are [n, K, nc, A, H, J, P, S, Sz, inv2, mu (D), tau (D), kind (D, as
doubles; 5 marks a zeta with eta > 0, whose nu entry holds eta), nu (D), c (nc), grp (Dx), local (Dx), cpart (Dx), spart (Dx, as doubles:
-1 or k + 1024 slot), N of the two slots, kind of the two slots, X row-major (n x Dx, the expanded matrix of glm.expand_factors),
Y row-major (n x K)], D = Dx + A + H + J + P + Sz.  The scan is the Kogge-Stone one of include/idhmc.h, stage by stage from a copy of
the values before the stage.  The GPU tests (tests/test_gpu_glm_struct.py) hand the same source to the oracle."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import test_glm_corr_cpu as CORR
import test_glm_hier_cpu as HIER
from test_glm_corr_cpu import LKJ, _pairs_struct, _priors_struct, partner_table
from test_glm_factors_cpu import SUBJECT, _data, _factors_struct
from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_local_cpu import inv2_of, numpy_density_local, start_local
from test_glm_priors_cpu import NORMAL, STUDENT_T, numpy_prior
from test_glm_slopes_cpu import DOSE, _values_struct

AR1, RW1 = 1, 2

_HEAD_SCAN = """    double s_phi[2] = {1.0, 1.0}, s_c[2] = {1.0, 1.0}, s_M[128], s_x[1024];
    int s_o[2] = {0, 0}, s_cz[2] = {-1, -1};
    for (int i = 0, z = 0; i < NS; ++i)
        if ((int)sk[i] == 1) {
            const double s = orc_exp(-fabs(zs[z]));
            const double t = s * s, d = 1.0 + t;
            s_phi[i] = copysign((1.0 - t) / d, zs[z]);
            s_c[i] = (2.0 * s) / d;
            s_cz[i] = D - Sz + z++;
        }
    for (int i = 0; i < NS; ++i) {
        const int N = (int)sn[i];
        for (int j = 0; j < Dx; ++j)
            if (sp[j] >= 0.0 && ((int)sp[j] >> 10) == i && ((int)sp[j] & 1023) == 0) s_o[i] = j;
        const int o = s_o[i];
        for (int k = 1; k < N; ++k) ut[o + k] = s_c[i] * q[o + k];
        double p = s_phi[i];
        for (int h = 1; h < N; h *= 2) {
            for (int k = 0; k < N; ++k) s_x[k] = ut[o + k];
            for (int k = h; k < N; ++k) ut[o + k] = fma(p, s_x[k - h], s_x[k]);
            p = p * p;
        }
    }
"""
_TAIL_SCAN = """    for (int i = 0; i < NS; ++i) {
        const int o = s_o[i], N = (int)sn[i];
        double p = s_phi[i];
        for (int h = 1; h < N; h *= 2) {
            for (int k = 0; k < N; ++k) s_x[k] = grad[o + k];
            for (int k = 0; k + h < N; ++k) grad[o + k] = fma(p, s_x[k + h], s_x[k]);
            p = p * p;
        }
        for (int r = 0; r < 128; ++r) s_M[r] = 0.0;
        for (int k = 1; k < N; ++k) {
            const int j = o + k;
            s_M[j & 127] = s_M[j & 127] + grad[j] * (s_c[i] * fma(s_c[i], ut[j - 1], -(s_phi[i] * q[j])));
            grad[j] = s_c[i] * grad[j];
        }
        if (s_cz[i] >= 0) grad[s_cz[i]] = orc_tree128(s_M);
    }
"""


def _body():
    s = CORR.C_BODY_CORR
    head = CORR._HEAD_NEW
    assert s.count(head) == 1
    new = head
    for old, rep in (("P = (int)params[6],\n              Dx = D - A - H - J - P;",
                      "P = (int)params[6], NS = (int)params[7], Sz = (int)params[8],\n              Dx = D - A - H - J - P - Sz;"),
                     ("const double inv2 = params[7];", "const double inv2 = params[9];"),
                     ("*mu = params + 8,", "*mu = params + 10,"),
                     ("*cp = loc + Dx,\n                 *X = cp + Dx,", "*cp = loc + Dx, *sp = cp + Dx, *sn = sp + Dx, *sk = sn + 2,\n                 *X = sk + 2,"),
                     ("*zeta = q + D - P;", "*zeta = q + D - Sz - P, *zs = q + D - Sz;")):
        assert new.count(old) == 1, old
        new = new.replace(old, rep)
    s = s.replace(head, new + _HEAD_SCAN)
    old = "    for (int p = 0; p < P; ++p) grad[D - P + p] = orc_tree128(M[p]);\n"
    assert s.count(old) == 1
    return s.replace(old, "    for (int p = 0; p < P; ++p) grad[D - Sz - P + p] = orc_tree128(M[p]);\n" + _TAIL_SCAN)


C_BODY_STRUCT = _body()


def c_source_struct(family):
    """C_BODY_STRUCT around the family's observation, as test_glm_corr_cpu.c_source_corr builds on HIER.c_source_hier"""
    body = HIER.c_source_hier(family)
    head, tail = HIER.C_BODY_HIER.split("%s")
    assert body.startswith(head) and body.endswith(tail)
    return C_BODY_STRUCT % body[len(head):len(body) - len(tail)]


def struct_table(Dx, structs):
    """structs: (off, N, kind) per slot -> the level table of the params (and of DevState::lr_spart)"""
    sp = np.full(Dx, -1.0)
    for i, (o, N, kd) in enumerate(structs):
        sp[o:o + N] = np.arange(N) + 1024 * i
    return sp


def twin_priors_struct(kind, nu, eta, structs, seta):
    """the public kind and nu (D entries) with the internal mark on every zeta with eta > 0: the pairs', then the AR(1) terms'"""
    kind, nu = np.array(kind, float), np.array(nu, float)
    ar = [e for (o, N, kd), e in zip(structs, seta) if kd == AR1]
    P, Sz = len(eta), len(ar)
    for p, e in enumerate(list(eta) + ar):
        if e > 0.0:
            kind[kind.size - Sz - P + p], nu[nu.size - Sz - P + p] = LKJ, e
    return kind, nu


def oracle_params_struct(Xe, Y, A, grp, local, S, kind, nu, pairs, eta, structs, seta, c=None, mu=None, tau=None):
    n, Dx = Xe.shape
    grp = np.full(Dx, -1) if grp is None else np.asarray(grp)
    local = np.zeros(Dx) if local is None else np.asarray(local, float)
    H, J, P, Sz = int(grp.max()) + 1, int(local.sum()), len(pairs), sum(1 for s in structs if s[2] == AR1)
    D = Dx + A + H + J + P + Sz
    Y = np.asarray(Y, float).reshape(n, -1)
    c = np.zeros(0) if c is None else np.asarray(c, float)
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    kind, nu = twin_priors_struct(np.broadcast_to(np.asarray(kind, float), (D,)), np.broadcast_to(np.asarray(nu, float), (D,)), eta, structs, seta)
    sn, sk = np.zeros(2), np.zeros(2)
    for i, (o, N, kd) in enumerate(structs):
        sn[i], sk[i] = N, kd
    return np.concatenate([[float(n), float(Y.shape[1]), float(c.size), float(A), float(H), float(J), float(P), float(len(structs)), float(Sz),
                            inv2_of(S)], mu, tau, kind, nu, c, grp.astype(float), local, partner_table(Dx, pairs), struct_table(Dx, structs),
                           sn, sk, np.asarray(Xe, float).ravel(), Y.ravel()])


def scan_matrices(N, zeta, kd):
    """L with ut = L u by the sequential recurrence, dL / dzeta, and the entrywise magnitudes of the terms of each"""
    if kd == AR1:
        phi, c = np.tanh(zeta), 2.0 * np.exp(-abs(zeta)) / (1.0 + np.exp(-2.0 * abs(zeta)))
    else:
        phi, c = 1.0, 1.0
    dphi, dc = c * c, -phi * c
    L, dL, aL, adL = (np.zeros((N, N)) for _ in range(4))
    for k in range(N):
        for j in range(k + 1):
            m = k - j
            pw, pw1 = phi ** m, (phi ** (m - 1) if m >= 1 else 0.0)
            if j == 0:
                L[k, j], dL[k, j] = pw, m * pw1 * dphi
                aL[k, j], adL[k, j] = abs(pw), abs(m * pw1 * dphi)
            else:
                L[k, j], dL[k, j] = c * pw, dc * pw + c * m * pw1 * dphi
                aL[k, j], adL[k, j] = abs(c * pw), abs(dc * pw) + abs(c * m * pw1 * dphi)
    return L, dL, aL, adL


def _zeta_prior(e, cz, kind, nu, mu, tau, q):
    """(log prior, its derivative, the magnitudes of the two) of the zeta at coordinate cz: Beta(e, e) on (tanh + 1) / 2, or its entry"""
    if e > 0.0:
        z = abs(q[cz])
        return (-2.0 * e * ((z + np.log1p(np.exp(-2.0 * z))) - math.log(2.0)), -2.0 * e * np.tanh(q[cz]), 2.0 * e * (z + math.log(2.0)),
                2.0 * e * abs(np.tanh(q[cz])))
    return tuple(x[0] for x in numpy_prior(kind[cz:cz + 1], nu[cz:cz + 1], mu[cz:cz + 1], tau[cz:cz + 1], q[cz:cz + 1]))


def numpy_density_struct(family, Xe, Y, q, grp, local, S, kind, nu, pairs, eta, structs, seta, mu=None, tau=None):
    """(l(q), grad l(q), magnitude of l's terms, per-coordinate magnitude of the terms summed into grad),
    q = [u | a | omega | lambda | zeta_pairs | zeta_ar]: section 19's closed form at ut = (mix, L(phi) u), its prior moved so that it
    sees q - mu, then the chain rule through the mix and through L and dL / dzeta"""
    P, Sz = len(pairs), sum(1 for s in structs if s[2] == AR1)
    D, D0 = q.size, q.size - P - Sz
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    kind, nu = np.broadcast_to(np.asarray(kind), (D,)), np.broadcast_to(np.asarray(nu, float), (D,))
    zeta = q[D0:D0 + P]
    rho, c = np.tanh(zeta), 2.0 * np.exp(-np.abs(zeta)) / (1.0 + np.exp(-2.0 * np.abs(zeta)))
    qt = q[:D0].copy()
    for p, (o1, o2, N) in enumerate(pairs):
        qt[o2:o2 + N] = rho[p] * q[o1:o1 + N] + c[p] * q[o2:o2 + N]
    mats, z = [], 0
    for o, N, kd in structs:
        cz = -1
        if kd == AR1:
            cz, z = D0 + P + z, z + 1
        mats.append(scan_matrices(N, q[cz] if cz >= 0 else 0.0, kd) + (cz,))
        qt[o:o + N] = mats[-1][0] @ q[o:o + N]
    mu0 = mu[:D0] + (qt - q[:D0])                          # d = qt - mu0 = q - mu: the prior of u is on u
    l0, g0, ls0, gs0 = numpy_density_local(family, Xe, Y, qt, grp, local, S, kind[:D0], nu[:D0], mu0, tau[:D0])
    _, pg, _, pgmag = numpy_prior(kind[:D0], nu[:D0], mu0, tau[:D0], qt)
    Gh, Ghmag = g0 - pg, gs0 - pgmag                       # the likelihood's part, dl / dut
    g, gs = np.r_[g0, np.zeros(P + Sz)], np.r_[gs0, np.zeros(P + Sz)]
    l, ls = l0, ls0
    for p, (o1, o2, N) in enumerate(pairs):
        a, b = slice(o1, o1 + N), slice(o2, o2 + N)
        g[a] += rho[p] * Gh[b]
        gs[a] += abs(rho[p]) * Ghmag[b]
        g[b] = c[p] * Gh[b] + pg[b]
        gs[b] = c[p] * Ghmag[b] + pgmag[b]
        m = Gh[b] * c[p] * (c[p] * q[a] - rho[p] * q[b])
        mmag = Ghmag[b] * c[p] * (c[p] * np.abs(q[a]) + abs(rho[p]) * np.abs(q[b]))
        lp, pgz, lmag, gmag = _zeta_prior(eta[p], D0 + p, kind, nu, mu, tau, q)
        g[D0 + p], gs[D0 + p] = m.sum() + pgz, mmag.sum() + gmag
        l, ls = l + lp, ls + lmag
    for (o, N, kd), e, (L, dL, aL, adL, cz) in zip(structs, seta, mats):
        sl = slice(o, o + N)
        g[sl] = L.T @ Gh[sl] + pg[sl]
        gs[sl] = aL.T @ Ghmag[sl] + pgmag[sl]
        if cz >= 0:
            lp, pgz, lmag, gmag = _zeta_prior(e, cz, kind, nu, mu, tau, q)
            g[cz], gs[cz] = Gh[sl] @ (dL @ q[sl]) + pgz, Ghmag[sl] @ (adL @ np.abs(q[sl])) + gmag
            l, ls = l + lp, ls + lmag
    return l, g, ls, gs


def make_struct(idhmc, family, X, Y, factors, grp, local, S, kind, nu, mu, tau, correlated, structured, **kw):
    return idhmc.GLM(X, Y, source(idhmc, family), consts(family), mu, tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu,
                     local=local, slab_scale=S, factors=factors, correlated=correlated, structured=structured, **kw)


def start_struct(family, C_, Dx, H, J, P, Sz, seed=0, zeta=None):
    """start_local, then the pairs' zetas and the AR(1) terms' ~ U(-0.8, 0.8) (or `zeta` in all of them)"""
    rng = np.random.default_rng(seed + 77)
    z = rng.uniform(-0.8, 0.8, (C_, P + Sz)) if zeta is None else np.broadcast_to(np.asarray(zeta, float), (C_, P + Sz))
    return np.concatenate([start_local(family, C_, Dx, H, J, seed), z], 1)


def fma_twin(a, b, c):
    """fma(a, b, c) rounded once, through exact rationals (finite arguments)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def scan_twin(u, phi, c):
    """section 23's forward scan of one term with exact-rational fma"""
    x = [float(u[0])] + [float(c) * float(v) for v in u[1:]]
    N, p, h = len(x), float(phi), 1
    while h < N:
        x = [fma_twin(p, x[k - h], x[k]) if k >= h else x[k] for k in range(N)]
        p, h = p * p, 2 * h
    return np.array(x)


# ---- glm.ar1 / glm.rw1, the constructor and the host helpers --------------------------------------------------------------------------
WEEK = np.array([0, 4, 1, 2, 3, 0, 2])            # 5 levels


def _week_model(idhmc, structured=None, **kw):
    X, Y = _data()
    g = idhmc.glm
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[(WEEK, 5), SUBJECT], structured=structured, **kw)


def test_structure_is_a_small_named_tuple(idhmc):
    g = idhmc.glm
    s = g.ar1(0)
    assert isinstance(s, tuple) and s._fields == ("term", "kind", "eta") and s == (0, 1, 2.0) and g.ar1(1, eta=0.5).eta == 0.5
    assert g.rw1(2) == (2, 2, 0.0) and (g.STRUCT_AR1, g.STRUCT_RW1) == (1, 2) and g.Term._fields == ("index", "values", "levels")


def test_constructor_keeps_the_structures(idhmc):
    g = idhmc.glm
    m = _week_model(idhmc, [g.ar1(0, eta=2.0)], groups=g.random_effects(2, [5, 4])["groups"])
    assert (m.Dx, m.A, m.H, m.J, m.P, m.S, m.Sz, m.D) == (11, 0, 2, 0, 0, 1, 1, 14) and m.structs == [g.Structure(0, 1, 2.0)]
    assert m.struct_term.dtype == m.struct_kind.dtype == np.int32 and list(m.struct_term) == [0] and list(m.struct_kind) == [1]
    assert list(m.struct_eta) == [2.0] and m.mu is None
    m = _week_model(idhmc, [g.rw1(1), g.ar1(0, 0)])
    assert (m.S, m.Sz, m.D) == (2, 1, 12) and m.structs == [g.Structure(1, 2, 0.0), g.Structure(0, 1, 0.0)]
    m = _week_model(idhmc, [g.rw1(0)])
    assert (m.S, m.Sz, m.D) == (1, 0, 11)
    for kw in ({}, {"structured": None}, {"structured": []}):
        m = _week_model(idhmc, **kw)
        assert m.S == 0 and m.Sz == 0 and m.structs is None and m.struct_term is None and m.D == 11
    X, Y = _data()
    assert idhmc.GLM(X, Y, g.POISSON_LOG).S == 0
    # next to a pair: the pair's zeta first, the term's last
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[(WEEK, 5), SUBJECT, g.term(SUBJECT, values=DOSE)], correlated=[g.pair(1, 2)], structured=[g.ar1(0, 0.0)],
                  **g.priors(15, P=1, S=1, autocorrelations=g.student_t(4, 0.0, 1.5)))
    assert (m.P, m.Sz, m.D) == (1, 1, 17) and m.prior_kind[16] == STUDENT_T and m.prior_kind[15] == NORMAL and m.tau[16] == pytest.approx(1 / 2.25)


def test_constructor_validates_structures(idhmc):
    g = idhmc.glm
    X, Y = _data()
    fac = [(WEEK, 5), SUBJECT, g.term(SUBJECT, values=DOSE), (np.zeros(7, int), 1)]

    def bad(what, structured, factors=fac, **kw):
        with pytest.raises(ValueError, match=what):
            idhmc.GLM(X, Y, g.POISSON_LOG, factors=factors, structured=structured, **kw)
    bad("structured must be a list of glm.ar1", g.ar1(0))
    bad("structured must be a list of glm.ar1", 3)
    bad(r"structured\[0\] must be a glm.ar1", [(0, 1, 2.0)])
    bad("at most 2 structured terms", [g.ar1(0), g.rw1(1), g.rw1(2)])
    bad("structured terms need factor terms", [g.ar1(0)], factors=None)
    bad("structured terms need factor terms", [g.ar1(0)], factors=[])
    for t in (4, -1, 0.5, True):
        bad(r"structured\[0\]: term = .* is outside 0..3", [g.ar1(t)])
    bad(r"structured\[1\]: term 0 is listed twice", [g.ar1(0), g.rw1(0)])
    for k in (0, 3, 1.0, True):
        bad(r"structured\[0\]: kind = .* must be glm.STRUCT_AR1", [g.Structure(0, k, 0.0)])
    for e in (-1.0, np.inf, np.nan, "2", True):
        bad(r"structured\[0\]: eta = .* must be finite and >= 0", [g.ar1(0, e)])
    bad(r"structured\[0\]: eta = 2.0 on a random walk", [g.Structure(0, g.STRUCT_RW1, 2.0)])
    bad(r"structured\[0\]: term 3 has 1 level", [g.rw1(3)])
    bad(r"structured\[1\]: term 2 is in correlated\[0\]", [g.ar1(0), g.rw1(2)], correlated=[g.pair(1, 2)])
    loc = np.zeros(2 + 5 + 4 + 4 + 1, np.int32)
    loc[4] = 1
    bad(r"structured\[0\]: local\[4\] is set on level 2 of term 0", [g.ar1(0)], local=loc)
    idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, structured=[g.ar1(1)], local=loc)              # a local scale on another term's column
    # the prior arrays on a zeta: D = 16 + 1 = 17, zeta is coordinate 16
    D = 17
    for name, val in (("prior_mu", 0.1), ("prior_tau", 2.0)):
        arr = np.zeros(D) if name == "prior_mu" else np.ones(D)
        arr[16] = val
        bad(r"structured\[0\]: eta = 2.0 is the Beta\(eta, eta\) prior of zeta: the entry of coordinate 16", [g.ar1(0)], **{name: arr})
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[16], nu[16] = STUDENT_T, 3.0
    bad(r"structured\[0\]: eta = 2.0 is the Beta", [g.ar1(0)], prior_kind=kind, prior_nu=nu)
    idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, structured=[g.ar1(0, 0.0)], prior_kind=kind, prior_nu=nu)         # eta = 0: it applies
    for k in (2, 3, 4):
        kind[16], nu[16] = k, 3.0 if k == 3 else 0.0
        for e in (0.0, 2.0):
            bad(r"structured\[0\]: prior_kind\[16\] = PRIOR_LOG_.* is a prior on exp\(q\): coordinate 16 is zeta", [g.ar1(0, e)],
                prior_kind=kind, prior_nu=nu)
    with pytest.raises(ValueError, match=r"limited to D <= 1024 \(D = 1025\)"):
        idhmc.GLM(np.ones((2, 2)), np.zeros(2), g.POISSON_LOG, factors=[(np.zeros(2, int), 1022)], structured=[g.ar1(0)])
    assert idhmc.GLM(np.ones((2, 2)), np.zeros(2), g.POISSON_LOG, factors=[(np.zeros(2, int), 1022)], structured=[g.rw1(0)]).D == 1024


def test_priors_builder_takes_the_autocorrelations(idhmc):
    g = idhmc.glm
    kw = g.priors(3, 1, 2, 2, scales=g.exponential(2.0), P=1, correlations=g.normal(0.0, 0.5), S=2, autocorrelations=[g.normal(0.0, 0.5), g.student_t(3)])
    assert list(kw["prior_kind"]) == [0, 0, 0, 0, 4, 4, 0, 0, 0, 0, 1] and list(kw["prior_nu"]) == [0] * 10 + [3.0]
    assert kw["prior_tau"][9] == 4.0 and kw["prior_mu"].size == 11
    assert g.priors(3, 1, 2, 2, P=1)["prior_kind"].size == 9 and g.priors(3, 1, 2, 2, S=1)["prior_kind"].size == 9
    with pytest.raises(TypeError):
        g.priors(3, 1, 2, 2, None, None, None, None, 0, None, 1)          # S is keyword-only
    for bad in (dict(S=1, autocorrelations=g.half_normal()), dict(S=1, autocorrelations=[g.exponential()]), dict(S=2, autocorrelations=[g.normal()]),
                dict(S=-1)):
        with pytest.raises(ValueError):
            g.priors(3, **bad)


def test_structured_effects_assembles_the_model(idhmc):
    g = idhmc.glm
    kw = g.structured_effects(2, [5, 4], [g.ar1(0, eta=1.5)], scale=g.half_student_t(3))
    assert sorted(kw) == ["groups", "prior_kind", "prior_mu", "prior_nu", "prior_tau", "structured"]
    base = g.random_intercepts(2, [5, 4], scale=g.half_student_t(3))
    assert kw["structured"] == [g.Structure(0, 1, 1.5)] and np.array_equal(kw["groups"], base["groups"])
    for k in ("prior_kind", "prior_mu", "prior_nu", "prior_tau"):
        assert np.array_equal(kw[k][:-1], base[k]) and kw[k].size == 14
    assert (kw["prior_kind"][-1], kw["prior_mu"][-1], kw["prior_tau"][-1], kw["prior_nu"][-1]) == (0, 0.0, 1.0, 0.0)
    m = _week_model(idhmc, **kw)
    assert (m.H, m.S, m.Sz, m.D) == (2, 1, 1, 14)
    # a random walk adds nothing to the prior arrays; pairs go through correlated_effects
    kw = g.structured_effects(2, [5, 4], [g.rw1(1)])
    assert kw["prior_mu"].size == 13 and "correlated" not in kw
    kw = g.structured_effects(1, [5, 4, 4], [g.ar1(0), g.rw1(0)][:1], correlated=[(1, 2)], eta=1.0, A=1)
    assert kw["correlated"] == [g.Pair(1, 2, 1.0)] and kw["prior_mu"].size == 1 + 13 + 1 + 3 + 1 + 1
    for bad in (dict(structured=[g.ar1(0)] * 2), dict(structured=[g.ar1(2)]), dict(structured=[g.ar1(1)], correlated=[(0, 1)], levels=[4, 4]),
                dict(structured=[g.rw1(0), g.ar1(1), g.rw1(1)]), dict(structured=[(0, 1)])):
        args = dict(Dd=2, levels=[5, 4], structured=[g.ar1(0)])
        args.update(bad)
        with pytest.raises((ValueError, AttributeError)):
            g.structured_effects(**args)


def test_host_helpers_on_hand_made_draws(idhmc):
    g = idhmc.glm
    m = _week_model(idhmc, **g.structured_effects(2, [5, 4], [g.ar1(0)]))
    draws = np.zeros((2, 3, 14))
    draws[..., :2] = [1.0, -2.0]
    draws[..., 2:7] = [1.0, 2.0, -3.0, 0.5, 0.25]
    draws[..., 7:11] = [0.5, -0.5, 0.25, 0.0]
    draws[..., 11:13] = np.log([2.0, 0.5])
    draws[..., 13] = np.arctanh(0.6)
    draws[1, 2, 13] = -np.arctanh(0.8)
    phi = g.autocorrelations(m, draws)
    assert phi.shape == (2, 3, 1) and np.allclose(phi[0, 0], 0.6, rtol=1e-15) and np.isclose(phi[1, 2, 0], -0.8, rtol=1e-15)
    assert g.correlations(m, draws).shape == (2, 3, 0)
    beta = g.coefficients(m, draws)
    u = draws[0, 0, 2:7]
    for (i, j), (f, c) in (((0, 0), g._rho_c(draws[0, 0, 13])), ((1, 2), g._rho_c(draws[1, 2, 13]))):
        ut = scan_twin(u, f, c)
        seq = [u[0]]
        for k in range(1, 5):
            seq.append(f * seq[-1] + c * u[k])
        assert np.allclose(ut, seq, rtol=1e-14)                                 # the scan is the recurrence
        assert beta.shape == (2, 3, 11) and np.allclose(beta[i, j], np.r_[1.0, -2.0, 2.0 * ut, 0.5 * draws[0, 0, 7:11]], rtol=1e-14)
        assert np.allclose(g.struct_scan(u, f, c), ut, rtol=1e-15)
    for fn in (g.autocorrelations, g.coefficients, g.group_scales, g.correlations):
        with pytest.raises(ValueError, match="14 coordinates"):
            fn(m, draws[..., :13])
    # the ends: phi is exactly +-1, every level is +-u_0 and finite
    d = np.zeros((3, 14))
    d[:, 2:7], d[:, 13] = [1.0, 2.0, 3.0, 4.0, 5.0], [800.0, -800.0, 0.0]
    assert list(g.autocorrelations(m, d)[:, 0]) == [1.0, -1.0, 0.0] and np.isfinite(g.coefficients(m, d)).all()
    assert np.array_equal(g.coefficients(m, d)[:, 2:7], [[1.0] * 5, [1.0, -1.0, 1.0, -1.0, 1.0], [1.0, 2.0, 3.0, 4.0, 5.0]])
    # a random walk: the cumulative sum, and no phi
    m = _week_model(idhmc, [g.rw1(0)])
    d = np.zeros((2, 11))
    d[:, 2:7] = [1.0, 2.0, -3.0, 0.5, 0.25]
    assert np.array_equal(g.coefficients(m, d)[:, 2:7], np.cumsum(d[:, 2:7], -1)) and g.autocorrelations(m, d).shape == (2, 0)
    assert g.autocorrelations(_week_model(idhmc), np.zeros((4, 11))).shape == (4, 0)


def test_scan_identities(idhmc):
    """the scan of the identity gives L(phi) with L L' = phi^|i - j| (the stationary unit-variance AR(1)); the random walk's is cumsum"""
    g = idhmc.glm
    rng = np.random.default_rng(1)
    for N in (7, 130):
        for zeta in (0.9, -1.7, 0.0):
            phi, c = g._rho_c(np.float64(zeta))
            L = g.struct_scan(np.eye(N), phi, c).T
            assert np.array_equal(L, np.tril(L)) and L[0, 0] == 1.0
            i = np.arange(N)
            assert np.max(np.abs(L @ L.T - phi ** np.abs(i[:, None] - i[None, :])) ) <= 1e-13
            u = rng.standard_normal(N)
            assert np.allclose(scan_twin(u, phi, c), L @ u, rtol=0, atol=1e-13)
        u = rng.integers(-8, 9, N).astype(float)
        assert np.array_equal(scan_twin(u, 1.0, 1.0), np.cumsum(u)) and np.array_equal(g.struct_scan(u, 1.0, 1.0), np.cumsum(u))


def test_beta_prior_on_the_autocorrelation():
    """exp(eta log(1 - phi^2)) d zeta is Beta(eta, eta) in (phi + 1) / 2 (section 22's prior row, used for phi)"""
    from scipy import integrate, stats
    for eta in (0.5, 2.0, 5.0):
        f = lambda z: np.cosh(z) ** (-2.0 * eta)
        quad = lambda a, b: integrate.quad(f, a, b, epsabs=1e-13, epsrel=1e-13, limit=400)[0]
        Z = quad(-60, 0) + quad(0, 60)
        for z in (-1.0, 0.3, 2.0):
            assert (quad(-60, -1.0) + quad(-1.0, z)) / Z == pytest.approx(stats.beta(eta, eta).cdf((np.tanh(z) + 1.0) / 2.0), abs=1e-9)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def _structs_struct(S, term, kind, eta):
    from inplacedhmc_jl_amd import _lib
    keep = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((term, np.int32), (kind, np.int32), (eta, np.float64))]
    st = _lib.GlmStructs(S=S)
    if keep[0] is not None:
        st.term = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
    if keep[1] is not None:
        st.kind = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
    if keep[2] is not None:
        st.eta = keep[2].ctypes.data_as(C.POINTER(C.c_double))
    return st, keep


def _local_struct(local, slab=0.0):
    from inplacedhmc_jl_amd import _lib
    keep = np.ascontiguousarray(local, dtype=np.int32)
    lc = _lib.GlmLocal()
    lc.local = keep.ctypes.data_as(C.POINTER(C.c_int32))
    lc.slab_scale = slab
    return lc, keep


def _create(idhmc, desc, factors, values, pairs, structs, priors=None, local=None, M=1, R=0, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create_glm_struct(C.byref(h), 0, nchains, 0, C.byref(desc), None if priors is None else C.byref(priors),
                                     None if local is None else C.byref(local), None if factors is None else C.byref(factors),
                                     None if values is None else C.byref(values), None if pairs is None else C.byref(pairs),
                                     None if structs is None else C.byref(structs), M, R, None, 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def _c_model(idhmc, structured="default", correlated=None):
    g = idhmc.glm
    X, Y = _data()
    st = [g.ar1(0)] if structured == "default" else structured
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[(WEEK, 5), SUBJECT, g.term(SUBJECT, values=DOSE)], structured=st, correlated=correlated,
                     groups=[-1, -1] + [0] * 5 + [1] * 4 + [-1] * 4)


def test_good_structures_pass_every_check(idhmc):
    """a valid descriptor reaches the device (or its absence): with a structure, with structs = NULL, with S = 0 and its arrays NULL"""
    ok = (0, idhmc.ERR_NO_DEVICE)
    m = _c_model(idhmc)
    fc, k1 = _factors_struct(3, m.levels, m.factor_index)
    fv, k2 = _values_struct(m.factor_values, m.factor_has)
    st, k3 = _structs_struct(1, m.struct_term, m.struct_kind, m.struct_eta)
    rc, msg = _create(idhmc, m.glm_desc(), fc, fv, None, st)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    m0 = _c_model(idhmc, None)
    for structs in (None, _structs_struct(0, None, None, None)[0]):
        rc, msg = _create(idhmc, m0.glm_desc(), fc, fv, None, structs)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    # a random walk on the valued term next to a pair-free AR(1) with eta = 0 and a Student-t entry on its zeta
    m1 = _c_model(idhmc, [idhmc.glm.rw1(2), idhmc.glm.ar1(0, 0.0)])
    kind, nu = np.zeros(m1.D, np.int32), np.zeros(m1.D)
    kind[-1], nu[-1] = STUDENT_T, 3.0
    pr, k4 = _priors_struct(kind, nu)
    st, k3 = _structs_struct(2, [2, 0], [RW1, AR1], [0.0, 0.0])
    rc, msg = _create(idhmc, m1.glm_desc(), fc, fv, None, st, pr)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)


def test_bad_structures_are_refused_before_the_device(idhmc):
    m = _c_model(idhmc)
    lib = idhmc.load_library()
    D = m.D                                                        # 2 + 13 + 2 + 1 = 18, zeta is coordinate 17
    assert D == 18

    def refused(what, S=1, term=(0,), kind=(AR1,), eta=(2.0,), F=3, levels=(5, 4, 4), factors=True, desc=None, priors=None, pairs=None, **kw):
        fc, k1 = _factors_struct(F, levels, m.factor_index)
        fv, k2 = _values_struct(m.factor_values, m.factor_has)
        st, k3 = _structs_struct(S, term, kind, eta)
        pp, k5 = (None, None) if pairs is None else _pairs_struct(*pairs)
        pr, k4 = (None, None) if priors is None else _priors_struct(*priors)
        rc, msg = _create(idhmc, m.glm_desc() if desc is None else desc, fc if factors else None, fv if factors and F else None, pp, st, pr, **kw)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    h = C.c_void_p()
    assert lib.idhmc_create_glm_struct(C.byref(h), 0, 4, 0, None, None, None, None, None, None, None, 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert b"idhmc_create_glm_struct: null argument" in lib.idhmc_last_error()
    assert lib.idhmc_create_glm_struct(None, 0, 4, 0, C.byref(m.glm_desc()), None, None, None, None, None, None, 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert lib.idhmc_glm_structs_get(None, None, None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    for S in (-1, 3, 1 << 20):
        refused(b"S = %d structured terms must be an integer in 0..2" % S, S=S)
    refused(b"need term, kind and eta (term is NULL)", term=None)
    refused(b"need term, kind and eta (kind is NULL)", kind=None)
    refused(b"need term, kind and eta (eta is NULL)", eta=None)
    for t in (-1, 3):
        refused(b"structure 0: term = %d is outside 0..2" % t, term=(t,))
    refused(b"structure 1: term 0 is listed twice", S=2, term=(0, 0), kind=(AR1, RW1), eta=(2.0, 0.0), desc=_c_model(idhmc, [idhmc.glm.ar1(0)]).glm_desc())
    for k in (0, 3, -1):
        refused(b"structure 0: kind = %d must be IDHMC_STRUCT_AR1 (1) or IDHMC_STRUCT_RW1 (2)" % k, kind=(k,))
    for e in (-1.0, np.inf, np.nan):
        refused(b"must be finite and >= 0", eta=(e,))
    refused(b"structure 0: eta = 2 on a random walk", kind=(RW1,), desc=_c_model(idhmc, [idhmc.glm.rw1(0)]).glm_desc())
    m1 = idhmc.GLM(*_data(), idhmc.glm.POISSON_LOG, factors=[(WEEK, 5), SUBJECT, (np.zeros(7, int), 1)])
    fc1, k7 = _factors_struct(3, m1.levels, m1.factor_index)
    rc, msg = _create(idhmc, m1.glm_desc(), fc1, None, None, _structs_struct(1, [2], [RW1], [0.0])[0])
    assert rc == idhmc.ERR_BAD_ARG and b"structure 0: term 2 has 1 level" in msg, (rc, msg)
    refused(b"structure 0: term 1 is in pair 0", term=(1,), pairs=(1, [1], [2], [0.0]), desc=_c_model(idhmc, None, [idhmc.glm.pair(1, 2, 0.0)]).glm_desc())
    # a local-scale flag on a level of the structured term: one more coordinate (J = 1) in front of zeta
    loc = np.zeros(15, np.int32)
    loc[2 + 3] = 1
    lc, k6 = _local_struct(loc)
    d = m.glm_desc()
    refused(b"structure 0: local[5] is set on level 3 of term 0", local=lc, desc=d)
    # the prior arrays on zeta
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[17], nu[17] = STUDENT_T, 3.0
    refused(b"structure 0: eta = 2 is the Beta(eta, eta) prior of zeta: the entry of coordinate 17", priors=(kind, nu))
    for name, val in (("mu", 0.5), ("tau", 2.0)):
        arr = np.zeros(D) if name == "mu" else np.ones(D)
        arr[17] = val
        d = m.glm_desc()
        setattr(d, name, arr.ctypes.data_as(C.POINTER(C.c_double)))
        refused(b"structure 0: eta = 2 is the Beta(eta, eta) prior of zeta", desc=d)
    for k in (2, 3, 4):
        kind[17], nu[17] = k, 3.0 if k == 3 else 0.0
        for e in (0.0, 2.0):
            refused(b"structure 0: prior kind[17] = %d is a prior on exp(q): coordinate 17 is zeta" % k, eta=(e,), priors=(kind, nu))
    # structures without factors
    X, Y = _data()
    m0 = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, groups=[0, -1])
    refused(b"structured terms need factor terms (factors is NULL)", factors=False, desc=m0.glm_desc())
    refused(b"structured terms need factor terms (factors is given with F = 0)", F=0, desc=m0.glm_desc())
    # D counts Sz
    d = m.glm_desc()
    d.Dx = 1022
    refused(b"D = Dx + A + H + J + P + Sz = 1025: a GLM is limited to D <= 1024 (Sz = 1 AR(1) terms)", desc=d)
    # everything idhmc_create_glm_corr refuses
    refused(b"F = 5 factors must be an integer in 0..4", F=5)
    refused(b"levels[1] = 0: at least one level", levels=(5, 0, 4))
    refused(b"P = 3 pairs must be an integer in 0..2", pairs=(3, [0], [1], [2.0]))
    d = m.glm_desc()
    d.H = 3
    refused(b"group 2 has no column", desc=d)
    refused(b"chains_per_response = 0", M=2, R=0)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def small_problem(idhmc, family, n, Dd, N, kd=AR1, valued=False, groups=True, second=None, pair=False, seed=0):
    """(X dense, Y, factors, Xe, grp, pairs, structs): a structured term of N levels (valued or plain) in group 0 and a plain term of 4
    levels in group 1 (left out when both of the following are asked for: a model has at most 4 terms); second = (N2, kind): a further
    structured term in group 2; pair: two further terms of 3 levels, paired"""
    g = idhmc.glm
    rng = np.random.default_rng(seed + n + N)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    t = rng.integers(0, N, n)
    N1 = 0 if second is not None and pair else 4
    factors = [g.term(t, values=0.5 * rng.standard_normal(n) + 1.0, levels=N) if valued else (t, N)] + ([(rng.integers(0, 4, n), 4)] if N1 else [])
    structs, pairs, off = [(Dd, N, kd)], [], Dd + N + N1
    if second is not None:
        factors.append((rng.integers(0, second[0], n), second[0]))
        structs.append((off, second[0], second[1]))
        off += second[0]
    if pair:
        s = rng.integers(0, 3, n)
        factors += [(s, 3), g.term(s, values=0.5 * rng.standard_normal(n), levels=3)]
        pairs.append((off, off + 3, 3))
    Xe = g.expand_factors(X, factors)
    Dx = Xe.shape[1]
    grp = np.full(Dx, -1, np.int32)
    if groups:
        grp[Dd:Dd + N], grp[Dd + N:Dd + N + N1] = 0, 1
        if second is not None:
            grp[Dd + N + N1:Dd + N + N1 + second[0]] = 2 if N1 else 1
    z = Xe @ (0.3 * rng.standard_normal(Dx))
    Y = rng.poisson(np.exp(z)).astype(float) if family == "POISSON_LOG" else z + 0.5 * rng.standard_normal(n)
    return X, Y, factors, Xe, grp, pairs, structs


@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    work = {}

    def model(family, Xe, Y, grp, local, S, kind, nu, pairs, eta, structs, seta, mu=None, tau=None):
        if family not in work:
            work[family] = str(tmp_path_factory.mktemp("struct_" + family.lower()))
        A, H, J = SHAPE[family][2], int(np.max(grp)) + 1, 0 if local is None else int(np.sum(local))
        D = Xe.shape[1] + A + H + J + len(pairs) + sum(1 for s in structs if s[2] == AR1)
        return oracle.OracleModel.custom(D, c_source_struct(family), oracle_params_struct(Xe, Y, A, grp, local, S, kind, nu, pairs, eta, structs, seta,
                                                                                         consts(family), mu, tau), work[family])
    return model


def case_priors(D, Z, etas, seed):
    """normal and Student-t on the coordinates in front, the defaults on a zeta with eta > 0 and a Student-t entry on one with eta = 0;
    Z zetas (the pairs', then the AR(1) terms') with etas"""
    rng = np.random.default_rng(seed)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:D - Z:2] = STUDENT_T
    nu[kind == STUDENT_T] = 4.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    for p in range(Z):
        cz = D - Z + p
        if etas[p] > 0.0:
            kind[cz], nu[cz], mu[cz], tau[cz] = NORMAL, 0.0, 0.0, 1.0
        else:
            kind[cz], nu[cz] = STUDENT_T, 3.0
    return kind, nu, mu, tau


# family, n, Dd, N, kind, valued, groups, second, pair, slab, eta of the first structure
CASES = [("POISSON_LOG", 1, 3, 5, AR1, False, True, None, False, None, 2.0), ("POISSON_LOG", 37, 4, 2, AR1, False, True, None, False, None, 0.0),
         ("GAUSSIAN_IDENTITY_LOGSIGMA", 130, 100, 60, AR1, True, True, None, False, None, 2.0),
         ("POISSON_LOG", 40, 1, 130, RW1, False, False, None, False, None, 0.0),
         ("POISSON_LOG", 60, 8, 9, AR1, True, True, (6, RW1), True, 1.5, 2.0),
         ("GAUSSIAN_IDENTITY_LOGSIGMA", 50, 5, 7, AR1, False, True, (3, AR1), False, None, 0.0)]


def case_setup(idhmc, case):
    family, n, Dd, N, kd, valued, groups, second, pair, S, e0 = case
    X, Y, factors, Xe, grp, pairs, structs = small_problem(idhmc, family, n, Dd, N, kd, valued, groups, second, pair)
    Dx, A, H, P = Xe.shape[1], SHAPE[family][2], int(grp.max()) + 1, len(pairs)
    local = None
    if S:
        local = np.zeros(Dx, np.int32)
        local[pairs[0][1]:pairs[0][1] + 3] = 1                 # on the pair's second term
        local[0] = 1
    J = 0 if local is None else int(local.sum())
    seta = [e0 if kd == AR1 else 0.0] + ([2.0 if second[1] == AR1 else 0.0] if second else [])
    eta = [2.0][:P]
    zetas = eta + [e for s, e in zip(structs, seta) if s[2] == AR1]
    D = Dx + A + H + J + len(zetas)
    kind, nu, mu, tau = case_priors(D, len(zetas), zetas, n)
    return family, X, Y, factors, Xe, grp, local, S, pairs, eta, structs, seta, (Dx, A, H, J, P, len(zetas) - P, D), (kind, nu, mu, tau)


@pytest.mark.parametrize("case", CASES, ids=["%s-n%d-Dd%d-N%d-k%d" % c[:5] for c in CASES])
def test_restatement_matches_numpy(idhmc, restated, case):
    family, X, Y, factors, Xe, grp, local, S, pairs, eta, structs, seta, (Dx, A, H, J, P, Sz, D), (kind, nu, mu, tau) = case_setup(idhmc, case)
    om = restated(family, Xe, Y, grp, local, S, kind, nu, pairs, eta, structs, seta, mu, tau)
    for k in range(3):
        q = start_struct(family, 1, Dx, H, J, P, Sz, seed=k)[0]
        if k == 2:
            q[D - P - Sz:] = -q[D - P - Sz:] - 1.0
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_struct(family, Xe, Y, q, grp, np.zeros(Dx, int) if local is None else local, S, kind, nu, pairs,
                                                            eta, structs, seta, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), np.max(np.abs(g[:D] - g_ref) / gscale)


def test_numpy_gradient_is_mpmath_derivative_of_the_model():
    """Poisson with a log link, Dd = 2, an AR(1) week effect of 5 levels with values and a sampled scale, Beta(2, 2) on (phi + 1) / 2, and
    a random walk of 4 levels: the log density written in mpmath straight from the sequential recurrence, differentiated numerically at
    40 digits; numpy's l and gradient within 1e-12 of their terms' magnitude"""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(4)
    n, Dd, N, N2, eta = 14, 2, 5, 4, 2.0
    X = 0.5 * rng.standard_normal((n, Dd))
    t, w, t2 = rng.integers(0, N, n), rng.standard_normal(n), rng.integers(0, N2, n)
    Y = rng.poisson(1.5, n).astype(float)
    Dx = Dd + N + N2
    D = Dx + 2 + 1
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    mu[-1], tau[-1] = 0.0, 1.0
    Xe = np.zeros((n, Dx))
    Xe[:, :Dd] = X
    Xe[np.arange(n), Dd + t] = w
    Xe[np.arange(n), Dd + N + t2] = 1.0
    grp = np.r_[[-1] * Dd, [0] * N, [1] * N2]
    structs = [(Dd, N, AR1), (Dd + N, N2, RW1)]

    def logp(*q):
        u, om, zeta = q[:Dx], q[Dx:Dx + 2], q[Dx + 2]
        phi = mp.tanh(zeta)
        c = mp.sqrt(1 - phi * phi)
        ar = [u[Dd]]
        for k in range(1, N):
            ar.append(phi * ar[-1] + c * u[Dd + k])
        rw = [u[Dd + N]]
        for k in range(1, N2):
            rw.append(rw[-1] + u[Dd + N + k])
        s0, s1 = mp.exp(om[0]), mp.exp(om[1])
        total = mp.mpf(0)
        for i in range(n):
            z = sum(mp.mpf(float(X[i, j])) * u[j] for j in range(Dd)) + mp.mpf(float(w[i])) * s0 * ar[t[i]] + s1 * rw[t2[i]]
            total += mp.mpf(float(Y[i])) * z - mp.exp(z)
        for j in range(D - 1):
            total -= mp.mpf(float(tau[j])) * (q[j] - mp.mpf(float(mu[j]))) ** 2 / 2
        return total + eta * mp.log(1 - phi * phi)

    for zeta in (0.7, -1.3, 0.0):
        q = np.r_[rng.uniform(-0.8, 0.8, Dx), np.log(0.6) + rng.uniform(-0.3, 0.3, 2), zeta]
        l, g, ls, gs = numpy_density_struct("POISSON_LOG", Xe, Y, q, grp, np.zeros(Dx, int), None, np.zeros(D, int), np.zeros(D), [], [], structs,
                                            [eta, 0.0], mu, tau)
        qm = [mp.mpf(float(x)) for x in q]
        assert abs(float(logp(*qm) - mp.mpf(l))) <= 1e-12 * ls
        for j in range(D):
            order = tuple(1 if i == j else 0 for i in range(D))
            ref = mp.diff(logp, tuple(qm), order)
            assert abs(float(ref - mp.mpf(float(g[j])))) <= 1e-12 * gs[j] + 1e-300, (zeta, j, float(ref), g[j])


def test_zeta_zero_and_no_structure_give_the_bits_of_section_22(idhmc, restated, oracle, tmp_path):
    """at zeta = +0 with eta = 0 and a normal entry, for starts without a -0: the first D - Sz coordinates of the gradient and (with
    zeta's mu = 0) l are bit for bit those of test_glm_corr_cpu's restatement on the model without the structure; with S = 0 the two
    restatements agree on everything"""
    family = "GAUSSIAN_IDENTITY_LOGSIGMA"
    X, Y, factors, Xe, grp, pairs, structs = small_problem(idhmc, family, 50, 5, 7, pair=True)
    Dx, A, H, P = Xe.shape[1], 1, 2, 1
    D = Dx + A + H + P + 1
    kind, nu, mu, tau = case_priors(D, 2, [2.0, 0.0], 3)
    kind[-1], nu[-1], mu[-1] = NORMAL, 0.0, 0.0
    om = restated(family, Xe, Y, grp, None, None, kind, nu, pairs, [2.0], structs, [0.0], mu, tau)
    base = oracle.OracleModel.custom(D - 1, CORR.c_source_corr(family), CORR.oracle_params_corr(Xe, Y, A, grp, None, None, kind[:-1], nu[:-1], pairs,
                                                                                                [2.0], consts(family), mu[:-1], tau[:-1]), str(tmp_path))
    none = restated(family, Xe, Y, grp, None, None, kind[:-1], nu[:-1], pairs, [2.0], [], [], mu[:-1], tau[:-1])
    for k in range(3):
        q = start_struct(family, 1, Dx, H, 0, 1, 1, seed=k)[0]
        q[-1] = 0.0
        assert not (np.signbit(q) & (q == 0.0)).any()
        l1, g1 = om.logdensity_and_gradient(q)
        l0, g0 = base.logdensity_and_gradient(q[:-1])
        l2, g2 = none.logdensity_and_gradient(q[:-1])
        assert l1 == l0 == l2 and np.array_equal(g1[:D - 1], g0[:D - 1]) and np.array_equal(g2[:D - 1], g0[:D - 1])
        assert np.isfinite(g1[D - 1]) and g1[D - 1] != 0.0


def test_the_ends_of_zeta(idhmc, restated):
    """zeta = +-0, +-40, +-800 on an AR(1) term of 7 levels: every output is finite, asserted at the restatement's own values -- at 800
    phi = +-1 and c = 0, so every ut_k is +-u_0, the levels k >= 1 see their prior only, the likelihood's part of G_zeta is exactly 0,
    and l's prior part is the finite -2 eta (|zeta| - ln 2)"""
    family = "POISSON_LOG"
    X, Y, factors, Xe, grp, pairs, structs = small_problem(idhmc, family, 30, 3, 7)
    Dx, H = Xe.shape[1], 2
    D = Dx + H + 1
    o, N = structs[0][:2]
    for eta in (0.0, 2.0):
        kind, nu, mu, tau = case_priors(D, 1, [eta], 5)
        if eta == 0.0:
            kind[-1], nu[-1], mu[-1], tau[-1] = STUDENT_T, 3.0, 0.0, 1.0
        om = restated(family, Xe, Y, grp, None, None, kind, nu, pairs, [], structs, [eta], mu, tau)
        q0 = start_struct(family, 1, Dx, H, 0, 0, 1, zeta=0.0)[0]
        for zeta in (0.0, -0.0, 40.0, -40.0, 800.0, -800.0):
            q = q0.copy()
            q[-1] = zeta
            lq, g = om.logdensity_and_gradient(q)
            assert np.isfinite(lq) and np.isfinite(g[:D]).all(), (eta, zeta)
            l_ref, g_ref, lscale, gscale = numpy_density_struct(family, Xe, Y, q, grp, np.zeros(Dx, int), None, kind, nu, pairs, [], structs, [eta], mu, tau)
            assert abs(lq - l_ref) <= 1e-12 * lscale and np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), (eta, zeta)
            if zeta == 0.0:
                l0, g0 = om.logdensity_and_gradient(np.r_[q[:-1], 0.0])
                assert lq == l0 and np.array_equal(g[:D - 1], g0[:D - 1])          # -0 is +0 to everything but zeta's own gradient
            if abs(zeta) == 800.0:
                cols = np.array([j for j in range(o + 1, o + N) if kind[j] == NORMAL])
                assert cols.size and np.array_equal(g[cols], -tau[cols] * (q - mu)[cols])
                if eta > 0.0:
                    assert g[D - 1] == -2.0 * eta * np.sign(zeta)
            if eta > 0.0 and abs(zeta) >= 40.0:
                other = numpy_density_struct(family, Xe, Y, q, grp, np.zeros(Dx, int), None, kind, nu, pairs, [], structs, [1e-300], mu, tau)[0]
                assert l_ref - other == pytest.approx(-2.0 * eta * (abs(zeta) - math.log(2.0)), rel=1e-9, abs=1e-12)
