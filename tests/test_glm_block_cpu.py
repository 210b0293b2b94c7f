"""A correlation block of three or four factor terms (GLM(..., correlated=[glm.block(..)]), idhmc_create_glm_block)
without a GPU: glm.block and the constructor's validation, glm.block_effects, the host helpers on hand-made draws, the C boundary's
argument checks, that the host's exponents make the prior LKJ, and the C restatement of section 26's definition against a numpy
restatement, whose gradient is held against mpmath's differentiation (40 digits) of the log density written straight from the model,
b = sigma .* (L u), L the Cholesky factor of a correlation matrix in canonical partial correlations z = tanh zeta.

The restatement is C_BODY_STRUCT of tests/test_glm_struct_cpu.py -- C_BODY_CORR with the structured terms, so that a block next to an
AR(1) term has a twin too -- with the block in the pairs' place: params are [n, K, nc, A, H, J, BK, NS, Sz, inv2, bo (4: the first column
of the term in row r), mu (D), tau (D), kind (D, as doubles; 5 marks a zeta with eta > 0, whose nu entry holds its exponent beta), nu (D),
c (nc), grp (Dx), local (Dx), bp (Dx: -1 or k + 1024 row), sp (Dx), sn (2), sk (2), X row-major (n x Dx, glm.expand_factors), Y row-major
(n x K)], D = Dx + A + H + J + BK (BK - 1) / 2 + Sz.  The GPU tests (tests/test_gpu_glm_block.py) hand the same source to the oracle."""
import ctypes as C
import math

import numpy as np
import pytest

import test_glm_corr_cpu as CORR
import test_glm_hier_cpu as HIER
import test_glm_struct_cpu as STRUCT
from test_glm_factors_cpu import ITEM, SUBJECT, _data, _factors_struct
from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_local_cpu import inv2_of, numpy_density_local, start_local
from test_glm_priors_cpu import NORMAL, STUDENT_T, numpy_prior
from test_glm_slopes_cpu import DOSE, _values_struct

LKJ = 5

_COEF = """/* coef(j, m, i) of section 26, m < i <= j (m = -1: L_ji): where s is still the initial 1 the other factor is taken itself */
static double blk_coef(const double *z, const double *c, int j, int m, int i)
{
    const int o = j * (j - 1) / 2;
    double s = 1.0;
    int one = 1;
    for (int t = m + 1; t < i; ++t) {
        s = one ? c[o + t] : s * c[o + t];
        one = 0;
    }
    if (i == j) return s;
    return one ? z[o + i] : z[o + i] * s;
}
double logdensity_and_gradient("""
_MIX_OLD = """        if (cp[j] >= 0.0 && ((int)cp[j] & 2048)) {
            const int e = (int)cp[j], p = (e >> 10) & 1;
            ut[j] = fma(rho[p], q[e & 1023], cc[p] * q[j]);
        }
"""
_MIX_NEW = """        if (cp[j] >= 1024.0) {
            const int e = (int)cp[j], r = e >> 10, k = e & 1023;
            double x = blk_coef(rho, cc, r, -1, r) * q[j];
            for (int i = 0; i < r; ++i) x = fma(blk_coef(rho, cc, r, -1, i), q[(int)bo[i] + k], x);
            ut[j] = x;
        }
"""
_CHAIN_NEW = """    for (int e = 0; e < 6; ++e)
        for (int r = 0; r < 128; ++r) M[e][r] = 0.0;
    for (int j = 0; j < Dx; ++j)
        if (cp[j] >= 1024.0) {
            const int e = (int)cp[j], r = e >> 10, k = e & 1023, o = r * (r - 1) / 2;
            for (int m = 0; m < r; ++m) {
                double w = r == m + 1 ? q[j] : blk_coef(rho, cc, r, m, r) * q[j];
                for (int i = m + 1; i < r; ++i) w = fma(blk_coef(rho, cc, r, m, i), q[(int)bo[i] + k], w);
                double ee = cc[o + m] * fma(cc[o + m], q[(int)bo[m] + k], -(rho[o + m] * w));
                if (m >= 1) {
                    double rr = cc[o];
                    for (int i = 1; i < m; ++i) rr = rr * cc[o + i];
                    ee = rr * ee;
                }
                M[o + m][j & 127] = M[o + m][j & 127] + grad[j] * ee;
            }
        }
    {
        double gh[1024];
        for (int j = 0; j < Dx; ++j) gh[j] = grad[j];
        for (int j = 0; j < Dx; ++j)
            if (cp[j] >= 0.0) {
                const int e = (int)cp[j], i = e >> 10, k = e & 1023;
                double x = i == 0 ? gh[j] : blk_coef(rho, cc, i, -1, i) * gh[j];
                for (int r = i + 1; r < BK; ++r) x = fma(blk_coef(rho, cc, r, -1, i), gh[(int)bo[r] + k], x);
                grad[j] = x;
            }
    }
"""


def _body():
    s = STRUCT.C_BODY_STRUCT
    for old, new in (("P = (int)params[6], NS = (int)params[7],", "BK = (int)params[6], P = BK * (BK - 1) / 2, NS = (int)params[7],"),
                     ("*mu = params + 10,", "*bo = params + 10, *mu = bo + 4,"),
                     ("double rho[2] = {0.0, 0.0}, cc[2] = {1.0, 1.0}, M[2][128];",
                      "double rho[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, cc[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, M[6][128];"),
                     (_MIX_OLD, _MIX_NEW), ("double logdensity_and_gradient(", _COEF)):
        assert s.count(old) == 1, old
        s = s.replace(old, new)
    # the pair's chain rule, from the zeroing of M to the line in front of the zetas' trees, becomes the block's
    a = s.index("    for (int r = 0; r < 128; ++r) M[0][r] = M[1][r] = 0.0;\n")
    b = s.index("    for (int p = 0; p < P; ++p) grad[D - Sz - P + p] = orc_tree128(M[p]);\n")
    assert 0 < a < b
    return s[:a] + _CHAIN_NEW + s[b:]


C_BODY_BLOCK = _body()


def c_source_block(family):
    body = HIER.c_source_hier(family)
    head, tail = HIER.C_BODY_HIER.split("%s")
    assert body.startswith(head) and body.endswith(tail)
    return C_BODY_BLOCK % body[len(head):len(body) - len(tail)]


def nz_of(K):
    return K * (K - 1) // 2


def betas(K, eta):
    """the exponent of every zeta, row-major: beta_ji = eta + (K - 2 - i) / 2, i the column"""
    return np.array([eta + 0.5 * (K - 2 - i) for j in range(1, K) for i in range(j)])


def block_table(Dx, offs, N):
    """offs: the first column of the term in row r -> the table of the params (and of DevState::lr_bpart)"""
    bp = np.full(Dx, -1.0)
    for r, o in enumerate(offs):
        bp[o:o + N] = np.arange(N) + 1024 * r
    return bp


def twin_priors(kind, nu, K, eta, Sz=0, seta=()):
    """the public kind and nu (D entries) with the internal mark on the block's zetas (eta > 0) and on the AR(1) zetas with eta > 0"""
    kind, nu = np.array(kind, float), np.array(nu, float)
    nz = nz_of(K)
    z0 = kind.size - Sz - nz
    if eta > 0.0:
        kind[z0:z0 + nz], nu[z0:z0 + nz] = LKJ, betas(K, eta)
    for i, e in enumerate(seta):
        if e > 0.0:
            kind[kind.size - Sz + i], nu[nu.size - Sz + i] = LKJ, e
    return kind, nu


def oracle_params_block(Xe, Y, A, grp, local, S, kind, nu, offs, N, eta, structs=(), seta=(), c=None, mu=None, tau=None):
    """structs: (off, N, kind) per structured slot, seta their eta (AR(1) slots only carry a zeta)"""
    n, Dx = Xe.shape
    K = len(offs)
    grp = np.full(Dx, -1) if grp is None else np.asarray(grp)
    local = np.zeros(Dx) if local is None else np.asarray(local, float)
    ar = [e for (o, Ns, kd), e in zip(structs, seta) if kd == STRUCT.AR1]
    H, J, Sz = int(grp.max()) + 1, int(local.sum()), len(ar)
    D = Dx + A + H + J + nz_of(K) + Sz
    Y = np.asarray(Y, float).reshape(n, -1)
    c = np.zeros(0) if c is None else np.asarray(c, float)
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    kind, nu = twin_priors(np.broadcast_to(np.asarray(kind, float), (D,)), np.broadcast_to(np.asarray(nu, float), (D,)), K, eta, Sz, ar)
    sn, sk = np.zeros(2), np.zeros(2)
    for i, (o, Ns, kd) in enumerate(structs):
        sn[i], sk[i] = Ns, kd
    bo = np.zeros(4)
    bo[:K] = offs
    return np.concatenate([[float(n), float(Y.shape[1]), float(c.size), float(A), float(H), float(J), float(K), float(len(structs)), float(Sz),
                            inv2_of(S)], bo, mu, tau, kind, nu, c, grp.astype(float), local, block_table(Dx, offs, N),
                           STRUCT.struct_table(Dx, structs), sn, sk, np.asarray(Xe, float).ravel(), Y.ravel()])


def numpy_factors(zeta, K):
    """L (K x K), dL / dzeta_e (nz x K x K) and the entrywise magnitudes of dL's terms, from z = tanh zeta, c = 1 / cosh zeta:
    L_ji = z_ji prod_{t<i} c_jt, L_jj = prod_t c_jt, dz = c^2, dc = -z c"""
    z, c = np.tanh(zeta), 2.0 * np.exp(-np.abs(zeta)) / (1.0 + np.exp(-2.0 * np.abs(zeta)))
    L, dL = np.zeros((K, K)), np.zeros((nz_of(K), K, K))
    L[0, 0] = 1.0
    for j in range(1, K):
        o = nz_of(j)
        for i in range(j + 1):
            pr = np.prod(c[o:o + i])
            L[j, i] = pr if i == j else z[o + i] * pr
            for m in range(min(i + 1, j)):
                if m < i:
                    dL[o + m, j, i] = -z[o + m] * L[j, i]
                else:
                    dL[o + m, j, i] = c[o + m] * c[o + m] * pr
    return L, dL


def numpy_density_block(family, Xe, Y, q, grp, local, S, kind, nu, offs, N, eta, mu=None, tau=None):
    """(l(q), grad l(q), magnitude of l's terms, per-coordinate magnitude of the terms summed into grad), q = [u | a | omega | lambda | zeta]:
    section 19's closed form at ut = L u, its prior moved so that it sees q - mu, then the chain rule through L(zeta)"""
    K = len(offs)
    nz = nz_of(K)
    D, D0 = q.size, q.size - nz
    mu = np.zeros(D) if mu is None else np.broadcast_to(np.asarray(mu, float), (D,))
    tau = np.ones(D) if tau is None else np.broadcast_to(np.asarray(tau, float), (D,))
    kind, nu = np.broadcast_to(np.asarray(kind), (D,)), np.broadcast_to(np.asarray(nu, float), (D,))
    zeta = q[D0:]
    L, dL = numpy_factors(zeta, K)
    rows = [slice(o, o + N) for o in offs]
    U = np.stack([q[r] for r in rows])                       # K x N
    qt = q[:D0].copy()
    for j in range(K):
        qt[rows[j]] = L[j] @ U
    mu0 = mu[:D0] + (qt - q[:D0])
    l0, g0, ls0, gs0 = numpy_density_local(family, Xe, Y, qt, grp, local, S, kind[:D0], nu[:D0], mu0, tau[:D0])
    _, pg, _, pgmag = numpy_prior(kind[:D0], nu[:D0], mu0, tau[:D0], qt)
    Gh, Ghmag = g0 - pg, gs0 - pgmag
    g, gs = np.r_[g0, np.zeros(nz)], np.r_[gs0, np.zeros(nz)]
    GH, GHmag = np.stack([Gh[r] for r in rows]), np.stack([Ghmag[r] for r in rows])
    for i in range(K):
        g[rows[i]] = L[:, i] @ GH + pg[rows[i]]
        gs[rows[i]] = np.abs(L[:, i]) @ GHmag + pgmag[rows[i]]
    l, ls = l0, ls0
    be = betas(K, eta)
    for e in range(nz):
        cz = D0 + e
        m = np.sum(GH * (dL[e] @ U))
        mmag = np.sum(GHmag * (np.abs(dL[e]) @ np.abs(U)))
        if eta > 0.0:
            z = abs(zeta[e])
            lp = -2.0 * be[e] * ((z + np.log1p(np.exp(-2.0 * z))) - math.log(2.0))
            pgz, lmag, gmag = -2.0 * be[e] * np.tanh(zeta[e]), 2.0 * be[e] * (z + math.log(2.0)), 2.0 * be[e] * abs(np.tanh(zeta[e]))
        else:
            lp, pgz, lmag, gmag = (x[0] for x in numpy_prior(kind[cz:cz + 1], nu[cz:cz + 1], mu[cz:cz + 1], tau[cz:cz + 1], q[cz:cz + 1]))
        g[cz], gs[cz] = m + pgz, mmag + gmag
        l, ls = l + lp, ls + lmag
    return l, g, ls, gs


def make_block(idhmc, family, X, Y, factors, grp, local, S, kind, nu, mu, tau, correlated, **kw):
    return idhmc.GLM(X, Y, source(idhmc, family), consts(family), mu, tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu,
                     local=local, slab_scale=S, factors=factors, correlated=correlated, **kw)


# ---- glm.block, the constructor and the host helpers ----------------------------------------------------------------------------------
DOSE2 = np.array([1.0, 0.25, -0.5, 0.0, 2.0, -1.0, 0.75])


def _slopes_model(idhmc, correlated=None, **kw):
    X, Y = _data()
    g = idhmc.glm
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[SUBJECT, g.term(SUBJECT, values=DOSE), g.term(SUBJECT, values=DOSE2)], correlated=correlated, **kw)


def test_block_is_a_small_named_tuple(idhmc):
    g = idhmc.glm
    b = g.block([0, 1, 2])
    assert isinstance(b, tuple) and b._fields == ("terms", "eta") and b == ((0, 1, 2), 2.0) and g.block((2, 0), eta=0.5).eta == 0.5


def test_constructor_keeps_the_block(idhmc):
    g = idhmc.glm
    m = _slopes_model(idhmc, [g.block((0, 1, 2))], groups=g.random_effects(2, [4, 4, 4])["groups"])
    assert (m.Dx, m.H, m.P, m.BK, m.Bz, m.D) == (14, 3, 0, 3, 3, 20) and m.block == g.Block((0, 1, 2), 2.0) and m.pairs is None
    assert m.block_term.dtype == np.int32 and list(m.block_term) == [0, 1, 2] and m.block_eta == 2.0
    # the order is the user's, K = 4 on two index arrays, K = 2
    X, Y = _data()
    fac = [(ITEM, 4), SUBJECT, (SUBJECT % 3, 4), g.term(SUBJECT, values=DOSE)]
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, correlated=[g.block((2, 0, 3, 1), eta=1)])
    assert (m.BK, m.Bz, m.D) == (4, 6, 2 + 16 + 6) and list(m.block_term) == [2, 0, 3, 1] and m.block_eta == 1.0
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, correlated=[g.block((3, 1), eta=0)])
    assert (m.BK, m.Bz, m.D) == (2, 1, 2 + 16 + 1)
    for kw in ({}, {"correlated": None}, {"correlated": []}, {"correlated": [g.pair(0, 1)]}):
        m = _slopes_model(idhmc, **kw)
        assert m.BK == 0 and m.Bz == 0 and m.block is None and m.block_term is None
    # eta = 0: the entries of the prior arrays apply
    kw = g.priors(14, 0, 3, P=3, correlations=g.student_t(4, 0.0, 1.5))
    m = _slopes_model(idhmc, [g.block((0, 1, 2), eta=0)], groups=g.random_effects(2, [4, 4, 4])["groups"], **kw)
    assert list(m.prior_kind[17:]) == [STUDENT_T] * 3 and m.tau[19] == pytest.approx(1.0 / 1.5 ** 2)
    # next to an AR(1) term: the block's zetas, then the AR(1) zeta
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, correlated=[g.block((0, 1, 2))], structured=[g.ar1(3)])
    assert (m.Bz, m.Sz, m.D) == (3, 1, 2 + 16 + 4)


def test_constructor_validates_the_block(idhmc):
    g = idhmc.glm
    X, Y = _data()
    fac = [SUBJECT, g.term(SUBJECT, values=DOSE), g.term(SUBJECT, values=DOSE2), (ITEM, 3)]

    def bad(what, correlated, factors=fac, **kw):
        with pytest.raises(ValueError, match=what):
            idhmc.GLM(X, Y, g.POISSON_LOG, factors=factors, correlated=correlated, **kw)
    bad("correlated must be a list of glm.pair", g.block((0, 1, 2)))
    bad("a glm.block is the single entry of correlated", [g.block((0, 1, 2)), g.pair(0, 1)])
    bad("a glm.block is the single entry of correlated", [g.block((0, 1)), g.block((2, 3))])
    bad("a correlation block needs factor terms", [g.block((0, 1, 2))], factors=None)
    for t in ((0,), (0, 1, 2, 3, 0), 3, ()):
        bad(r"correlated\[0\]: a block names K = 2, 3 or 4 terms", [g.block(t)])
    for t in (4, -1, 0.5, True):
        bad(r"correlated\[0\]: terms\[1\] = .* is outside 0..3", [g.block((0, t, 2))])
    bad(r"correlated\[0\]: term 1 is listed twice", [g.block((0, 1, 1))])
    bad(r"correlated\[0\]: terms 0 and 3 have 4 and 3 levels", [g.block((0, 1, 3))])
    for e in (-1.0, np.inf, np.nan, "2", True):
        bad(r"correlated\[0\]: eta = .* must be finite and >= 0", [g.block((0, 1, 2), e)])
    # the prior arrays on the zetas: D = 2 + 15 + 3 = 20, the zetas are coordinates 17 .. 19
    D = 20
    for name, val in (("prior_mu", 0.1), ("prior_tau", 2.0)):
        arr = np.zeros(D) if name == "prior_mu" else np.ones(D)
        arr[18] = val
        bad(r"correlated\[0\]: eta = 2.0 is the LKJ prior of the zetas: the entry of coordinate 18", [g.block((0, 1, 2))], **{name: arr})
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[19], nu[19] = STUDENT_T, 3.0
    bad(r"correlated\[0\]: eta = 2.0 is the LKJ prior of the zetas", [g.block((0, 1, 2))], prior_kind=kind, prior_nu=nu)
    idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, correlated=[g.block((0, 1, 2), 0.0)], prior_kind=kind, prior_nu=nu)
    for k in (2, 3, 4):
        kind[19], nu[19] = k, 3.0 if k == 3 else 0.0
        for e in (0.0, 2.0):
            bad(r"correlated\[0\]: prior_kind\[19\] = PRIOR_LOG_.* is a prior on exp\(q\): coordinate 19 is a zeta", [g.block((0, 1, 2), e)],
                prior_kind=kind, prior_nu=nu)
    # a block term is neither structured nor a GMRF term
    bad(r"structured\[0\]: term 1 is in correlated\[0\]", [g.block((0, 1, 2))], structured=[g.ar1(1)])
    bad(r"gmrf\[0\]: term 2 is in correlated\[0\]", [g.block((0, 1, 2))], gmrf=[g.gmrf(2, np.eye(4))])
    with pytest.raises(ValueError, match=r"limited to D <= 1024 \(D = 1025\)"):
        idhmc.GLM(np.ones((2, 2)), np.zeros(2), g.POISSON_LOG, factors=[(np.zeros(2, int), 340)] * 3, correlated=[g.block((0, 1, 2))])
    assert idhmc.GLM(np.ones((2, 1)), np.zeros(2), g.POISSON_LOG, factors=[(np.zeros(2, int), 340)] * 3, correlated=[g.block((0, 1, 2))]).D == 1024


def test_block_effects_assembles_the_model(idhmc):
    g = idhmc.glm
    kw = g.block_effects(2, [4, 4, 4], (0, 1, 2), eta=1.5, scale=g.half_student_t(3))
    assert sorted(kw) == ["correlated", "groups", "prior_kind", "prior_mu", "prior_nu", "prior_tau"]
    base = g.random_intercepts(2, [4, 4, 4], scale=g.half_student_t(3))
    assert kw["correlated"] == [g.Block((0, 1, 2), 1.5)] and np.array_equal(kw["groups"], base["groups"])
    for k in ("prior_kind", "prior_mu", "prior_nu", "prior_tau"):
        assert np.array_equal(kw[k][:-3], base[k]) and kw[k].size == 20
    assert list(kw["prior_kind"][-3:]) == [0] * 3 and list(kw["prior_tau"][-3:]) == [1.0] * 3
    m = _slopes_model(idhmc, **kw)
    assert (m.H, m.BK, m.D) == (3, 3, 20)
    kw = g.block_effects(1, [5, 5, 5, 5], [3, 1, 0, 2], A=1)
    assert kw["correlated"] == [g.Block((3, 1, 0, 2), 2.0)] and kw["prior_mu"].size == 1 + 20 + 1 + 4 + 6
    for bad in (dict(terms=(0, 0, 1)), dict(terms=(0, 1, 3)), dict(eta=0.0), dict(eta=-1.0), dict(terms=(0,)), dict(eta=[1.0, 2.0])):
        args = dict(Dd=2, levels=[4, 4, 4, 3], terms=(0, 1, 2))
        args.update(bad)
        with pytest.raises(ValueError):
            g.block_effects(**args)


def test_host_helpers_on_hand_made_draws(idhmc):
    g = idhmc.glm
    rng = np.random.default_rng(3)
    X, Y = _data()
    fac = [(ITEM, 4), SUBJECT, (SUBJECT % 3, 4), g.term(SUBJECT, values=DOSE)]
    for terms in ((0, 1, 2), (2, 0, 3, 1), (3, 1)):
        K = len(terms)
        nz = nz_of(K)
        m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=fac, **g.block_effects(2, [4, 4, 4, 4], terms))
        D = m.D
        assert D == 2 + 16 + 4 + nz
        draws = rng.standard_normal((2, 5, D))
        draws[..., D - nz:] = rng.uniform(-2.0, 2.0, (2, 5, nz))
        draws[1, 4, D - nz:] = [800.0, -800.0, 0.0, 30.0, -30.0, 1.0][:nz]
        L = g.cholesky_factors(m, draws)
        R = g.correlation_matrix(m, draws)
        assert L.shape == R.shape == (2, 5, K, K) and np.all(np.triu(L, 1) == 0.0) and np.all(L[..., 0, 0] == 1.0)
        LLt = L @ np.swapaxes(L, -1, -2)
        assert np.all(np.abs(np.diagonal(LLt, axis1=-2, axis2=-1) - 1.0) <= 1e-15)
        assert np.array_equal(R, np.swapaxes(R, -1, -2)) and np.all(np.diagonal(R, axis1=-2, axis2=-1) == 1.0)
        assert np.allclose(R, LLt, rtol=0, atol=1e-15) and np.isfinite(R).all() and np.all(np.abs(R) <= 1.0 + 1e-15)
        rho = g.correlations(m, draws)
        assert rho.shape == (2, 5, nz)
        assert np.array_equal(rho, np.stack([R[..., j, i] for j in range(1, K) for i in range(j)], -1))
        assert np.array_equal(rho[..., 0], np.tanh(draws[..., D - nz])) or np.allclose(rho[..., 0], np.tanh(draws[..., D - nz]), rtol=1e-15)
        # coefficients = sigma .* (L u)
        beta = g.coefficients(m, draws)
        sig = g.group_scales(m, draws)
        assert beta.shape == (2, 5, 18) and np.array_equal(beta[..., :2], draws[..., :2])
        U = np.stack([draws[..., 2 + 4 * t:6 + 4 * t] for t in terms], -2)            # (..., K, N)
        want = L @ U
        for r, t in enumerate(terms):
            assert np.allclose(beta[..., 2 + 4 * t:6 + 4 * t], sig[..., t:t + 1] * want[..., r, :], rtol=1e-14, atol=1e-300)
        for t in set(range(4)) - set(terms):
            assert np.array_equal(beta[..., 2 + 4 * t:6 + 4 * t], sig[..., t:t + 1] * draws[..., 2 + 4 * t:6 + 4 * t])
        for f in (g.correlations, g.coefficients, g.cholesky_factors, g.correlation_matrix, g.group_scales):
            with pytest.raises(ValueError, match="%d coordinates" % D):
                f(m, draws[..., :D - 1])
    m = _slopes_model(idhmc)
    with pytest.raises(ValueError, match="no correlation block"):
        g.cholesky_factors(m, np.zeros((2, m.D)))


# ---- the prior is LKJ ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_exponents_make_the_prior_lkj(K):
    """sum_ji beta_ji log(1 - z_ji^2), beta_ji = eta + (K - 2 - i) / 2, equals (eta - 1) log det R + log |det dR_lower / dzeta| with no
    constant left over: the Jacobian by mpmath's differentiation of the map zeta -> R_lower written straight from R = L L'"""
    import mpmath as mp
    mp.mp.dps = 40
    nz = nz_of(K)
    rng = np.random.default_rng(K)

    def r_lower(*zeta):
        z = [mp.tanh(x) for x in zeta]
        L = mp.zeros(K, K)
        L[0, 0] = mp.mpf(1)
        for j in range(1, K):
            rem = mp.mpf(1)
            for i in range(j):
                zz = z[nz_of(j) + i]
                L[j, i] = zz * mp.sqrt(rem)
                rem = rem * (1 - zz * zz)
            L[j, j] = mp.sqrt(rem)
        R = L * L.T
        return R, [R[j, i] for j in range(1, K) for i in range(j)]

    for eta in (0.5, 1.0, 2.0, 3.5):
        for _ in range(2):
            zeta = [mp.mpf(float(x)) for x in rng.uniform(-1.2, 1.2, nz)]
            R, _ = r_lower(*zeta)
            J = mp.zeros(nz, nz)
            for a in range(nz):
                for b in range(nz):
                    J[a, b] = mp.diff(lambda *x: r_lower(*x)[1][a], tuple(zeta), tuple(1 if t == b else 0 for t in range(nz)))
            want = (mp.mpf(eta) - 1) * mp.log(mp.det(R)) + mp.log(abs(mp.det(J)))
            got = sum(mp.mpf(float(be)) * mp.log(1 - mp.tanh(x) ** 2) for be, x in zip(betas(K, eta), zeta))
            assert abs(got - want) <= mp.mpf(10) ** -12, (K, eta, float(got), float(want))


# ---- the C boundary --------------------------------------------------------------------------------------------------------------------
def _block_struct(K, term, eta):
    from inplacedhmc_jl_amd import _lib
    keep = None if term is None else np.ascontiguousarray(term, dtype=np.int32)
    bk = _lib.GlmBlock(K=K, eta=eta)
    if keep is not None:
        bk.term = keep.ctypes.data_as(C.POINTER(C.c_int32))
    return bk, keep


def _create(idhmc, desc, factors, values, block, priors=None, pairs=None, structs=None, gmrfs=None, M=1, R=0, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.idhmc_create_glm_block(C.byref(h), 0, nchains, 0, C.byref(desc), ref(priors), None, ref(factors), ref(values), ref(pairs),
                                    ref(structs), ref(gmrfs), ref(block), M, R, None, 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def _c_model(idhmc, correlated="default", **kw):
    g = idhmc.glm
    X, Y = _data()
    corr = [g.block((0, 1, 2))] if correlated == "default" else correlated
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[SUBJECT, g.term(SUBJECT, values=DOSE), g.term(SUBJECT, values=DOSE2), (ITEM, 3)],
                     correlated=corr, groups=[-1, -1] + [0] * 4 + [1] * 4 + [2] * 4 + [-1] * 3, **kw)


def test_a_good_block_passes_every_check(idhmc):
    """a valid descriptor reaches the device (or its absence): with a block, with block = NULL, with K = 0 and term NULL"""
    ok = (0, idhmc.ERR_NO_DEVICE)
    m = _c_model(idhmc)
    fc, k1 = _factors_struct(4, m.levels, m.factor_index)
    fv, k2 = _values_struct(m.factor_values, m.factor_has)
    for K, term in ((3, (0, 1, 2)),):
        bk, k3 = _block_struct(K, term, 2.0)
        rc, msg = _create(idhmc, m.glm_desc(), fc, fv, bk)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    m0 = _c_model(idhmc, None)
    for bk in (None, _block_struct(0, None, 0.0)[0]):
        rc, msg = _create(idhmc, m0.glm_desc(), fc, fv, bk)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    # eta = 0 with Student-t entries on the zetas, rows not in term order
    m1 = _c_model(idhmc, [idhmc.glm.block((2, 0, 1), 0.0)])
    kind, nu = np.zeros(m1.D, np.int32), np.zeros(m1.D)
    kind[-3:], nu[-3:] = STUDENT_T, 3.0
    pr, k4 = CORR._priors_struct(kind, nu)
    bk, k3 = _block_struct(3, (2, 0, 1), 0.0)
    rc, msg = _create(idhmc, m1.glm_desc(), fc, fv, bk, pr)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    # next to an AR(1) term on the remaining term
    m2 = _c_model(idhmc, structured=[idhmc.glm.ar1(3)])
    st, k5 = STRUCT._structs_struct(1, [3], [1], [2.0])
    bk, k3 = _block_struct(3, (0, 1, 2), 2.0)
    rc, msg = _create(idhmc, m2.glm_desc(), fc, fv, bk, structs=st)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)


def test_a_bad_block_is_refused_before_the_device(idhmc):
    m = _c_model(idhmc)
    lib = idhmc.load_library()
    D = m.D                                                        # 2 + 15 + 3 + 3 = 23, the zetas are coordinates 20 .. 22
    assert D == 23

    def refused(what, K=3, term=(0, 1, 2), eta=2.0, F=4, levels=(4, 4, 4, 3), factors=True, desc=None, priors=None, **kw):
        fc, k1 = _factors_struct(F, levels, m.factor_index)
        fv, k2 = _values_struct(m.factor_values, m.factor_has)
        bk, k3 = _block_struct(K, term, eta)
        pr, k4 = (None, None) if priors is None else CORR._priors_struct(*priors)
        rc, msg = _create(idhmc, m.glm_desc() if desc is None else desc, fc if factors else None, fv if factors and F else None, bk, pr, **kw)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    h = C.c_void_p()
    assert lib.idhmc_create_glm_block(C.byref(h), 0, 4, 0, None, None, None, None, None, None, None, None, None, 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert b"idhmc_create_glm_block: null argument" in lib.idhmc_last_error()
    assert lib.idhmc_glm_block_get(None, None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    for K in (-1, 1, 5, 1 << 20):
        refused(b"a block of K = %d terms: K must be 0, 2, 3 or 4" % K, K=K)
    refused(b"needs term (term is NULL)", term=None)
    for t in (-1, 4):
        refused(b"block row 1: term = %d is outside 0..3" % t, term=(0, t, 2))
    refused(b"block row 2: term 0 is listed twice", term=(0, 1, 0))
    refused(b"block row 2: terms 0 and 3 have 4 and 3 levels", term=(0, 1, 3))
    for e in (-1.0, np.inf, np.nan):
        refused(b"must be finite and >= 0", eta=e)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[21], nu[21] = STUDENT_T, 3.0
    refused(b"block: eta = 2 is the LKJ prior of the zetas: the entry of coordinate 21", priors=(kind, nu))
    for name, val in (("mu", 0.5), ("tau", 2.0)):
        arr = np.zeros(D) if name == "mu" else np.ones(D)
        arr[22] = val
        d = m.glm_desc()
        setattr(d, name, arr.ctypes.data_as(C.POINTER(C.c_double)))
        refused(b"block: eta = 2 is the LKJ prior of the zetas: the entry of coordinate 22", desc=d)
    for k in (2, 3, 4):
        kind[:] = 0
        kind[20], nu[20] = k, 3.0 if k == 3 else 0.0
        for e in (0.0, 2.0):
            refused(b"block: prior kind[20] = %d is a prior on exp(q): coordinate 20 is a zeta" % k, eta=e, priors=(kind, nu))
    # a block together with pairs
    mp_ = _c_model(idhmc, [idhmc.glm.pair(0, 1)])
    pp, k5 = CORR._pairs_struct(1, [0], [1], [2.0])
    d = mp_.glm_desc()
    refused(b"a block next to P = 1 pairs", term=(2, 3), K=2, desc=d, pairs=pp)
    # a block term that is structured (a GMRF term: the next test)
    st, k6 = STRUCT._structs_struct(1, [2], [1], [2.0])
    refused(b"block row 2: term 2 is structure 0", desc=_c_model(idhmc, structured=[idhmc.glm.ar1(3)]).glm_desc(), structs=st)
    # a block without factors
    X, Y = _data()
    m0 = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, groups=[0, -1])
    refused(b"a block needs factor terms (factors is NULL)", factors=False, desc=m0.glm_desc())
    refused(b"a block needs factor terms (factors is given with F = 0)", F=0, desc=m0.glm_desc())
    # D counts the zetas
    d = m.glm_desc()
    d.Dx = 1019
    refused(b"a GLM is limited to D <= 1024 (a block of K = 3 terms)", desc=d)
    # everything idhmc_create_glm_gmrf refuses
    refused(b"F = 5 factors must be an integer in 0..4", F=5)
    refused(b"levels[1] = 0: at least one level", levels=(4, 0, 4, 3))
    refused(b"chains_per_response = 0", M=2, R=0)


def test_a_gmrf_term_in_the_block_is_refused(idhmc):
    from test_glm_gmrf_cpu import _gmrfs_struct
    m = _c_model(idhmc)
    g = idhmc.glm
    mg = _c_model(idhmc, None, gmrf=[g.gmrf(1, np.eye(4))])
    fc, k1 = _factors_struct(4, m.levels, m.factor_index)
    fv, k2 = _values_struct(m.factor_values, m.factor_has)
    gm, k3 = _gmrfs_struct(1, mg.gmrf_term, mg.gmrf_start, mg.gmrf_col, mg.gmrf_val, mg.gmrf_kappa)
    bk, k4 = _block_struct(3, (0, 1, 2), 2.0)
    rc, msg = _create(idhmc, m.glm_desc(), fc, fv, bk, gmrfs=gm)
    assert rc == idhmc.ERR_BAD_ARG and b"block row 1: term 1 is GMRF 0" in msg, (rc, msg)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def small_problem(idhmc, family, n, Dd, N, K=3, order=None, two_index=False, seed=0, extra=None):
    """(X dense, Y, factors, Xe, grp, offs): K terms of N levels -- the first plain, the others valued -- on one index array (two_index:
    the odd terms on a second one), each a group (K <= 3) or groups (0, 1, 2, 2) shared by the last two; order: the block's rows as term
    indices (default 0 .. K-1); extra: the levels of one more plain term behind them, in the last group; offs: the first column of the
    term in each ROW"""
    g = idhmc.glm
    rng = np.random.default_rng(seed + n + N + 10 * K)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    s, s2 = rng.integers(0, N, n), rng.integers(0, N, n)
    factors = []
    for t in range(K):
        idx = s2 if two_index and t % 2 else s
        factors.append((idx, N) if t == 0 else g.term(idx, values=0.5 * rng.standard_normal(n), levels=N))
    if extra:
        factors.append((rng.integers(0, extra, n), extra))
    Xe = g.expand_factors(X, factors)
    Dx = Xe.shape[1]
    grp = np.full(Dx, -1, np.int32)
    for t in range(K):
        grp[Dd + t * N:Dd + (t + 1) * N] = min(t, 2)
    if extra:
        grp[Dd + K * N:] = 3 if K == 3 else 2
    order = tuple(range(K)) if order is None else order
    offs = [Dd + t * N for t in order]
    z = Xe @ (0.4 * rng.standard_normal(Dx))
    Y = rng.poisson(np.exp(np.clip(z, -3, 3))).astype(float) if family == "POISSON_LOG" else z + 0.5 * rng.standard_normal(n)
    return X, Y, factors, Xe, grp, offs


def start_block(family, C_, Dx, H, J, nz, seed=0, zeta=None, Sz=0):
    rng = np.random.default_rng(seed + 77)
    z = rng.uniform(-0.8, 0.8, (C_, nz + Sz)) if zeta is None else np.broadcast_to(np.asarray(zeta, float), (C_, nz + Sz))
    return np.concatenate([start_local(family, C_, Dx, H, J, seed), z], 1)


@pytest.fixture(scope="module")
def restated(oracle, tmp_path_factory):
    work = {}

    def model(family, Xe, Y, grp, local, S, kind, nu, offs, N, eta, mu=None, tau=None, structs=(), seta=()):
        if family not in work:
            work[family] = str(tmp_path_factory.mktemp("block_" + family.lower()))
        A, H, J = SHAPE[family][2], int(np.max(grp)) + 1, 0 if local is None else int(np.sum(local))
        Sz = sum(1 for s in structs if s[2] == STRUCT.AR1)
        D = Xe.shape[1] + A + H + J + nz_of(len(offs)) + Sz
        return oracle.OracleModel.custom(D, c_source_block(family),
                                         oracle_params_block(Xe, Y, A, grp, local, S, kind, nu, offs, N, eta, structs, seta, consts(family), mu, tau),
                                         work[family])
    return model


def case_priors(D, nz, eta, seed):
    """normal and Student-t on the coordinates in front; the defaults on the zetas with eta > 0, Student-t(3) entries with eta = 0"""
    rng = np.random.default_rng(seed)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:D - nz:2] = STUDENT_T
    nu[kind == STUDENT_T] = 4.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    if eta > 0.0:
        kind[D - nz:], nu[D - nz:], mu[D - nz:], tau[D - nz:] = NORMAL, 0.0, 0.0, 1.0
    else:
        kind[D - nz:], nu[D - nz:] = STUDENT_T, 3.0
    return kind, nu, mu, tau


# family, n, Dd, N, K, order, two_index, eta, slab
CASES = [("POISSON_LOG", 1, 3, 4, 3, None, False, 2.0, None), ("POISSON_LOG", 37, 20, 15, 3, None, False, 2.0, None),
         ("GAUSSIAN_IDENTITY_LOGSIGMA", 130, 100, 20, 4, (2, 0, 3, 1), True, 1.0, None),
         ("GAUSSIAN_IDENTITY_LOGSIGMA", 60, 8, 6, 3, (1, 2, 0), False, 0.0, None), ("POISSON_LOG", 200, 10, 12, 3, None, True, 2.0, 1.5),
         ("POISSON_LOG", 50, 4, 7, 4, None, False, 0.0, 2.0), ("POISSON_LOG", 40, 5, 9, 2, (1, 0), False, 2.0, None)]


@pytest.mark.parametrize("case", CASES, ids=["%s-n%d-Dd%d-N%d-K%d%s%s" % (c[0][:4], c[1], c[2], c[3], c[4], "-eta%g" % c[7], "-slab" if c[8] else "")
                                             for c in CASES])
def test_restatement_matches_numpy(idhmc, restated, case):
    family, n, Dd, N, K, order, two_index, eta, S = case
    X, Y, factors, Xe, grp, offs = small_problem(idhmc, family, n, Dd, N, K, order, two_index)
    Dx, A, H, nz = Xe.shape[1], SHAPE[family][2], int(grp.max()) + 1, nz_of(K)
    local = None
    if S:
        local = np.zeros(Dx, np.int32)
        local[offs[1]:offs[1] + N] = 1                     # on row 1's columns
        local[1] = 1
    J = 0 if local is None else int(local.sum())
    D = Dx + A + H + J + nz
    kind, nu, mu, tau = case_priors(D, nz, eta, n)
    om = restated(family, Xe, Y, grp, local, S, kind, nu, offs, N, eta, mu, tau)
    for k in range(3):
        q = start_block(family, 1, Dx, H, J, nz, seed=k)[0]
        if k == 2:
            q[D - nz:] = -q[D - nz:] - 1.0
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_block(family, Xe, Y, q, grp, np.zeros(Dx, int) if local is None else local, S, kind, nu, offs, N,
                                                           eta, mu, tau)
        assert abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), np.max(np.abs(g[:D] - g_ref) / gscale)


@pytest.mark.parametrize("K", [3, 4])
def test_numpy_gradient_is_mpmath_derivative_of_the_model(K):
    """Poisson with a log link, Dd = 2, K terms on one index with 3 subjects, groups (0, 1, 2, 2), LKJ(1.5): the log density written in
    mpmath straight from b = sigma .* (L u), differentiated numerically at 40 digits; numpy's l and gradient within 1e-12 of their terms'
    magnitude.  The rows are not in term order."""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(4 + K)
    n, Dd, N, eta = 14, 2, 3, 1.5
    nz = nz_of(K)
    order = (1, 2, 0) if K == 3 else (2, 0, 3, 1)
    X = 0.5 * rng.standard_normal((n, Dd))
    s = rng.integers(0, N, n)
    W = rng.standard_normal((K, n))
    W[0] = 1.0
    Y = rng.poisson(1.5, n).astype(float)
    Dx, H = Dd + K * N, 3
    D = Dx + H + nz
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    mu[-nz:], tau[-nz:] = 0.0, 1.0
    Xe = np.zeros((n, Dx))
    Xe[:, :Dd] = X
    for t in range(K):
        Xe[np.arange(n), Dd + t * N + s] = W[t]
    grp = np.r_[[-1] * Dd, np.repeat([min(t, 2) for t in range(K)], N)]
    offs = [Dd + t * N for t in order]
    be = betas(K, eta)

    def logp(*q):
        om, zeta = q[Dx:Dx + H], q[Dx + H:]
        z = [mp.tanh(x) for x in zeta]
        L = [[mp.mpf(0)] * K for _ in range(K)]
        L[0][0] = mp.mpf(1)
        for j in range(1, K):
            rem = mp.mpf(1)
            for i in range(j):
                zz = z[nz_of(j) + i]
                L[j][i] = zz * mp.sqrt(rem)
                rem = rem * (1 - zz * zz)
            L[j][j] = mp.sqrt(rem)
        eff = {}
        for r, t in enumerate(order):
            sg = mp.exp(om[min(t, 2)])
            eff[t] = [sg * sum(L[r][i] * q[offs[i] + k] for i in range(r + 1)) for k in range(N)]
        total = mp.mpf(0)
        for i in range(n):
            zi = sum(mp.mpf(float(X[i, c])) * q[c] for c in range(Dd)) + sum(mp.mpf(float(W[t, i])) * eff[t][s[i]] for t in range(K))
            total += mp.mpf(float(Y[i])) * zi - mp.exp(zi)
        for c in range(D - nz):
            total -= mp.mpf(float(tau[c])) * (q[c] - mp.mpf(float(mu[c]))) ** 2 / 2
        return total + sum(mp.mpf(float(b)) * mp.log(1 - zz * zz) for b, zz in zip(be, z))

    for k in range(2):
        zeta = rng.uniform(-1.3, 1.3, nz)
        if k == 1:
            zeta[0] = 0.0
        q = np.r_[rng.uniform(-0.8, 0.8, Dx), np.log(0.6) + rng.uniform(-0.3, 0.3, H), zeta]
        l, g, ls, gs = numpy_density_block("POISSON_LOG", Xe, Y, q, grp, np.zeros(Dx, int), None, np.zeros(D, int), np.zeros(D), offs, N, eta, mu, tau)
        qm = [mp.mpf(float(x)) for x in q]
        assert abs(float(logp(*qm) - mp.mpf(l))) <= 1e-12 * ls
        for c in list(range(Dd, Dx, 2)) + list(range(Dx, D)):
            ref = mp.diff(logp, tuple(qm), tuple(1 if j == c else 0 for j in range(D)))
            assert abs(float(ref - mp.mpf(float(g[c])))) <= 1e-12 * gs[c] + 1e-300, (K, c, float(ref), g[c])


def test_a_block_of_two_gives_the_bits_of_the_pair(idhmc, restated, oracle, tmp_path):
    """the anchor: a K = 2 block's restatement gives the bits of C_BODY_CORR with the pair, in l and every gradient entry, with groups,
    local scales with a slab, LKJ and the prior arrays' path, the second term in front"""
    family = "GAUSSIAN_IDENTITY_LOGSIGMA"
    for order, eta, S in (((0, 1), 2.0, None), ((1, 0), 0.0, 1.5), ((1, 0), 0.7, None)):
        X, Y, factors, Xe, grp, offs = small_problem(idhmc, family, 50, 5, 7, 2, order)
        Dx, A, H, N = Xe.shape[1], 1, 2, 7
        local = None
        if S:
            local = np.zeros(Dx, np.int32)
            local[offs[1]:offs[1] + N:2] = 1
        J = 0 if local is None else int(local.sum())
        D = Dx + A + H + J + 1
        kind, nu, mu, tau = case_priors(D, 1, eta, 3)
        blk = restated(family, Xe, Y, grp, local, S, kind, nu, offs, N, eta, mu, tau)
        par = oracle.OracleModel.custom(D, CORR.c_source_corr(family),
                                        CORR.oracle_params_corr(Xe, Y, A, grp, local, S, kind, nu, [(offs[0], offs[1], N)], [eta], consts(family), mu, tau),
                                        str(tmp_path))
        for k in range(3):
            q = start_block(family, 1, Dx, H, J, 1, seed=k)[0]
            if k == 2:
                q[-1] = -3.0
            l1, g1 = blk.logdensity_and_gradient(q)
            l0, g0 = par.logdensity_and_gradient(q)
            assert l1 == l0 and np.array_equal(g1[:D], g0[:D]) and np.isfinite(g1[:D]).all()


def test_zeta_zero_gives_the_bits_of_the_model_without_a_block(idhmc, restated, oracle, tmp_path):
    """every zeta = +0 (eta = 0, normal entries with mu = 0): L = I, and l and the first D - nz gradient entries are bit for bit those of
    test_glm_local_cpu's restatement on the model without the block"""
    from test_glm_local_cpu import c_source_local, oracle_params_local
    family = "GAUSSIAN_IDENTITY_LOGSIGMA"
    for K in (3, 4):
        X, Y, factors, Xe, grp, offs = small_problem(idhmc, family, 50, 5, 7, K, (2, 0, 1) if K == 3 else (3, 1, 0, 2))
        Dx, A, H, nz = Xe.shape[1], 1, 3, nz_of(K)
        D = Dx + A + H + nz
        kind, nu, mu, tau = case_priors(D, nz, 0.0, 3)
        kind[-nz:], nu[-nz:], mu[-nz:] = NORMAL, 0.0, 0.0
        om = restated(family, Xe, Y, grp, None, None, kind, nu, offs, 7, 0.0, mu, tau)
        base = oracle.OracleModel.custom(D - nz, c_source_local(family),
                                         oracle_params_local(Xe, Y, A, grp, None, None, kind[:-nz], nu[:-nz], None, mu[:-nz], tau[:-nz]), str(tmp_path))
        for k in range(3):
            q = start_block(family, 1, Dx, H, 0, nz, seed=k, zeta=0.0)[0]
            l1, g1 = om.logdensity_and_gradient(q)
            l0, g0 = base.logdensity_and_gradient(q[:-nz])
            assert l1 == l0 and np.array_equal(g1[:D - nz], g0) and np.isfinite(g1[D - nz:D]).all() and np.all(g1[D - nz:D] != 0.0)


def test_the_ends_of_zeta(idhmc, restated):
    """every |zeta| = 800, all sign patterns of a K = 3 block and two of K = 4: l and every gradient entry are finite, with LKJ and with
    the prior arrays' entries"""
    family = "POISSON_LOG"
    for K in (3, 4):
        X, Y, factors, Xe, grp, offs = small_problem(idhmc, family, 30, 3, 5, K)
        Dx, H, nz = Xe.shape[1], 3, nz_of(K)
        D = Dx + H + nz
        for eta in (0.0, 2.0):
            kind, nu, mu, tau = case_priors(D, nz, eta, 5)
            if eta == 0.0:
                mu[-nz:], tau[-nz:] = 0.0, 1.0
            om = restated(family, Xe, Y, grp, None, None, kind, nu, offs, 5, eta, mu, tau)
            q0 = start_block(family, 1, Dx, H, 0, nz, zeta=0.0)[0]
            signs = [[(b >> e) & 1 for e in range(nz)] for b in (range(8) if K == 3 else (0, 0b101101))]
            for sg in signs:
                q = q0.copy()
                q[-nz:] = [800.0 if s else -800.0 for s in sg]
                lq, g = om.logdensity_and_gradient(q)
                assert np.isfinite(lq) and np.isfinite(g[:D]).all(), (K, eta, sg)
                if eta > 0.0:
                    assert np.array_equal(g[D - nz:D], -2.0 * betas(K, eta) * np.sign(q[-nz:]))
