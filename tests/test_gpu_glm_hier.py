"""Hierarchical GLMs (GLM(..., groups=...), idhmc_create_glm) on the device.  Grouped models are bit-identical to
the CPU oracle running the C restatement of section 13 (tests/test_glm_hier_cpu.py, through oracle.OracleModel.custom) and within
1e-12 of numpy, in both device forms: one chain per wavefront (evaluation, leapfrog, stepsize search; NUTS at L = 512) and the
matrix-core gradient of the NUTS kernel.  No tolerance on the device side.  Every context compiles its source with hipRTC, so
engines are shared across assertions."""
import ctypes as C

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
import test_glm_cpu as FLAT
from test_glm_hier_cpu import (OMEGA0, SHAPE, blocks, c_source_hier, consts, interleaved, make, numpy_density_hier, oracle_params_hier,
                               problem_hier, source, start_hier)

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def prior(D, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)


def setup(idhmc, oracle, tmp_path, family, n, Dx, grp, one_hot, C, seed, opt=None, oopt=None):
    A, H = SHAPE[family][2], int(grp.max()) + 1
    D = Dx + A + H
    X, Y = problem_hier(family, n, Dx, grp, one_hot, seed=n + Dx)
    mu, tau = prior(D)
    eng = idhmc.Engine(make(idhmc, family, X, Y, grp, mu, tau), C, opt, seed=seed)
    om = oracle.OracleModel.custom(D, c_source_hier(family), oracle_params_hier(X, Y, A, grp, consts(family), mu, tau), str(tmp_path))
    chains = [oracle.OracleChain(om, oopt, seed=seed, chain_id=c) for c in range(C)]
    return X, Y, mu, tau, eng, chains


def start(eng, chains, family, Dx, H, q=None):
    q = start_hier(family, len(chains), Dx, H) if q is None else q
    eng.set_q(q)
    for c, ch in enumerate(chains):
        ch.set_q(q[c])
    return q


def coop_expected(L, A, shared):
    """DESIGN section 12's table; groups move no row of it"""
    if L == 128:
        return True
    if L == 256:
        return A <= 1 or (A == 2 and shared)
    return False


def check_density(eng, chains, family, X, Y, grp, mu, tau, D, ends):
    q, g, lq = eng.q, eng.grad, eng.lq
    assert same_bits(lq, [c.lq for c in chains]) and same_bits(g, np.stack([c.grad[:D] for c in chains]))
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_hier(family, X, Y, q[c], grp, mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


def straddling(Dx):
    """group 0: columns 100..160 (across column 128, the chunk boundary); group 1: the columns behind"""
    g = np.full(Dx, -1, np.int32)
    g[100:161] = 0
    g[161:] = 1
    return g


# name: (family, Dx, grp, one-hot blocks, padded length, matrix cores)
SHAPES = {
    "one block, L = 128": ("BERNOULLI_LOGIT", 25, blocks(25, 1, 10), True, 128, 1),
    "omega is index 127": ("POISSON_LOG", 127, interleaved(127, 1), False, 128, 1),             # last lane, second residue
    "omega is index 128": ("BERNOULLI_LOGIT", 128, blocks(128, 1, 40), True, 256, 1),           # first of chunk 1
    "a group across column 128": ("POISSON_LOG", 200, straddling(200), False, 256, 1),
    "H = 4 interleaved, L = 128": ("BERNOULLI_LOGIT", 120, interleaved(120, 4), False, 128, 1),
    "H = 4 interleaved, A = 1, L = 256": ("GAUSSIAN_IDENTITY_LOGSIGMA", 250, interleaved(250, 4), False, 256, 1),
    "A = 1, two blocks": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, blocks(100, 2, 30), True, 128, 1),
    "A = 4, L = 128": ("TEST_A4", 100, interleaved(100, 2), False, 128, 1),
    "L = 512": ("BERNOULLI_LOGIT", 300, blocks(300, 2, 100), True, 512, 0),
    "L = 512, A = 1, H = 4": ("GAUSSIAN_IDENTITY_LOGSIGMA", 300, interleaved(300, 4), False, 512, 0),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1, 37, 128, 1000])
def test_density_both_forms(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l: the per-wave form (evaluation), and after one NUTS transition the form the NUTS kernel ran, each bit-identical to
    the oracle and within 1e-12 of numpy's closed form"""
    family, Dx, grp, one_hot, L, form = SHAPES[shape]
    A, H = SHAPE[family][2], int(grp.max()) + 1
    C_, D = 18, Dx + A + H
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, grp, one_hot, C_, seed=3, opt=idhmc.default_options(max_depth=4),
                                       oopt=oracle.default_options(max_depth=4))
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D
    start(eng, chains, family, Dx, H)
    check_density(eng, chains, family, X, Y, grp, mu, tau, D, (0, C_ - 1))
    eng.set_eps(0.02)
    eng.nuts_transition(1)
    for ch in chains:
        ch.sample_tree(0.02, 1)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    check_density(eng, chains, family, X, Y, grp, mu, tau, D, (0, C_ - 1))
    eng.close()


def _form_source(A):
    """a Gaussian with known scale (A = 0), or with log sigma = a[0] whose further auxiliary coordinates see only their prior"""
    if A == 0:
        return "__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)\n{\n    r = o.y[0] - z;\n    v = 0.5 * (r * r);\n}\n"
    return ("__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)\n{\n"
            "    const double w = dexp(-a[0]);\n    const double u = (o.y[0] - z) * w;\n    v = 0.5 * (u * u) + a[0];\n    r = u * w;\n"
            "    s[0] = u * u - 1.0;\n" + "".join("    s[%d] = 0.0;\n" % j for j in range(1, A)) + "}\n")


@pytest.mark.parametrize("H", [1, 4])
def test_groups_move_no_row_of_the_table(idhmc, H):
    """idhmc_glm_form per (L, A, metric) is DESIGN section 12's table with H = 1 and H = 4 groups, and each of those kernels launches
    (the hierarchy adds no LDS)"""
    rng = np.random.default_rng(0)
    for Dx, L in ((30, 128), (200, 256), (300, 512)):
        X = rng.standard_normal((40, Dx)) * 0.3
        Y = rng.standard_normal(40)
        grp = interleaved(Dx, H)
        for A in (0, 1, 2, 3, 4):
            for mode in (idhmc.METRIC_PER_CHAIN, idhmc.METRIC_SHARED, idhmc.METRIC_POOLED):
                if (L == 512 and A > 1) or (mode == idhmc.METRIC_POOLED and (L, A) != (128, 4)):
                    continue                                    # a pooled metric is a shared one to the kernel: one case of it
                eng = idhmc.Engine(idhmc.GLM(X, Y, _form_source(A), aux=A, groups=grp), 20, idhmc.default_options(max_depth=3, metric_mode=mode), seed=2)
                assert eng.padded_dim() == L
                assert eng.glm_form() == (1 if coop_expected(L, A, mode != idhmc.METRIC_PER_CHAIN) else 0), (L, A, mode)
                q = rng.uniform(-0.1, 0.1, (20, Dx + A + H))
                q[:, Dx + A:] += OMEGA0
                eng.set_q(q)
                eng.set_eps(0.01)
                eng.nuts_transition(1)
                assert np.isfinite(eng.lq).all() and (eng.tree_stats()["steps"] >= 1).all()
                eng.close()


LEAP = {"BERNOULLI_LOGIT": interleaved(100, 4), "POISSON_LOG": blocks(100, 1, 40), "GAUSSIAN_IDENTITY_LOGSIGMA": blocks(100, 2, 30),
        "TEST_A4": interleaved(100, 2)}


@pytest.mark.parametrize("family", list(LEAP))
def test_leapfrog_and_stepsize_search(idhmc, oracle, tmp_path, family):
    Dx, n, C_, grp = 100, 128, 6, LEAP[family]
    A, H = SHAPE[family][2], int(grp.max()) + 1
    D = Dx + A + H
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, grp, family != "BERNOULLI_LOGIT" and family != "TEST_A4", C_, seed=21)
    start(eng, chains, family, Dx, H)
    eng.refresh_momentum(1)
    eng.leapfrog(0.01, 3)
    eng.leapfrog(-0.01, 1)
    for ch in chains:
        ch.rand_p(1)
        for e in (0.01, 0.01, 0.01, -0.01):
            ch.leapfrog(e)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains])) and same_bits(eng.p, np.stack([c.p[:D] for c in chains]))
    assert same_bits(eng.grad, np.stack([c.grad[:D] for c in chains])) and same_bits(eng.logdensity(), [c.logdensity() for c in chains])
    eng.refresh_momentum(0)
    eng.find_initial_stepsize()
    ref = []
    for ch in chains:
        ch.rand_p(0)
        rc, e = ch.find_initial_stepsize()
        assert rc == 0
        ref.append(e)
    assert same_bits(eng.eps, ref)
    eng.close()


NUTS_CASES = {"BERNOULLI_LOGIT": blocks(25, 2, 8), "GAUSSIAN_IDENTITY_LOGSIGMA": interleaved(25, 4), "TEST_A4": blocks(25, 1, 12)}


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("family", list(NUTS_CASES))
def test_nuts_transitions(idhmc, oracle, tmp_path, family, shared):
    """single-transition launches, then several per launch (idhmc_nuts_transitions): a ragged last group of 16 (37 chains), per-chain
    and shared unit metric; then a small eps whose trees stop at max_depth"""
    Dx, n, C_, depth, T, grp = 25, 200, 37, 4, 2, NUTS_CASES[family]
    A, H = SHAPE[family][2], int(grp.max()) + 1
    D = Dx + A + H
    opt = idhmc.default_options(max_depth=depth, metric_mode=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, grp, family == "BERNOULLI_LOGIT", C_, seed=5, opt=opt,
                                       oopt=oracle.default_options(max_depth=depth))
    assert eng.glm_form() == 1
    start(eng, chains, family, Dx, H)
    it = 0
    for eps in (0.03, 0.0005):
        eng.set_eps(eps)
        reached = 0
        for _ in range(T):
            it += 1
            eng.nuts_transition(it)
            st = eng.tree_stats()
            ost = [ch.sample_tree(eps, it) for ch in chains]
            for f in ("depth", "steps", "term_left", "term_right"):
                np.testing.assert_array_equal(st[f], [getattr(s, f) for s in ost], err_msg="%s @%d" % (f, it))
            assert same_bits(st["pi"], [s.pi for s in ost]) and same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
            reached += int((st["depth"] == depth).sum())
        eng.nuts_transitions(it + 1, T)
        for k in range(T):
            for ch in chains:
                ch.sample_tree(eps, it + 1 + k)
        it += T
        assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        assert same_bits(eng.grad, np.stack([c.grad[:D] for c in chains])) and same_bits(eng.lq, [c.lq for c in chains])
        if eps < 0.001:
            assert reached >= T * C_ // 2                 # trees that ran to max_depth
    eng.close()


@pytest.mark.parametrize("family", ["BERNOULLI_LOGIT", "GAUSSIAN_IDENTITY_LOGSIGMA"])
def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path, family):
    Dx, n, C_, N = 25, 200, 5, 8
    grp = blocks(Dx, 2, 8)
    A, H = SHAPE[family][2], 2
    D = Dx + A + H
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    X, Y = problem_hier(family, n, Dx, grp, True, seed=9)
    eng = idhmc.Engine(make(idhmc, family, X, Y, grp), C_, idhmc.default_options(**short), seed=77)
    draws, stats = eng.mcmc_with_warmup(N)
    om = oracle.OracleModel.custom(D, c_source_hier(family), oracle_params_hier(X, Y, A, grp, consts(family)), str(tmp_path))
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, C_, oracle.default_options(**short), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps)
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats.T, ost[:, :N])
    eng.close()


@pytest.mark.parametrize("Dx,levels,form", [(40, 12, 1), (300, 100, 0)])
def test_scales_past_the_range_of_dexp(idhmc, oracle, tmp_path, Dx, levels, form):
    """one chain of 37 with omega_0 = -800 (e = 0: the group's coefficients vanish, lq finite) and one with omega_0 = +800 (e = inf:
    lq = -inf, a rejected start) report what the oracle reports, in the per-wave form (evaluation; NUTS at L = 512) and on the
    matrix cores (NUTS at L = 128), while the other chains of their workgroups keep their oracle bits; single launches; no device
    error.  Non-finite values are data here."""
    family, n, C_, H, lo, hi = "BERNOULLI_LOGIT", 300, 37, 2, 5, 20
    grp = blocks(Dx, H, levels)
    D = Dx + H
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, grp, True, C_, seed=6, opt=idhmc.default_options(max_depth=4),
                                       oopt=oracle.default_options(max_depth=4))
    assert eng.glm_form() == form
    q = start_hier(family, C_, Dx, H)
    q[lo, Dx] = -800.0
    q[hi, Dx] = 800.0
    start(eng, chains, family, Dx, H, q)
    ok = np.arange(C_) != hi
    lq = eng.lq
    assert lq[hi] == -np.inf and chains[hi].lq == -np.inf and np.isfinite(lq[ok]).all()
    assert same_bits(lq, [c.lq for c in chains]) and same_bits(eng.grad[ok], np.stack([c.grad[:D] for c in chains])[ok])
    assert np.isfinite(eng.grad[lo]).all()
    eng.set_eps(0.02)
    for it in (1, 2):
        eng.nuts_transition(it)
        for ch in chains:
            ch.sample_tree(0.02, it)
        lq = eng.lq
        assert lq[hi] == -np.inf and np.isfinite(lq[ok]).all() and same_bits(lq, [c.lq for c in chains])
        assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        assert same_bits(eng.grad[ok], np.stack([c.grad[:D] for c in chains])[ok])
    assert eng.poll_abort() == 0
    eng.close()


def _engine_from_glm_desc(idhmc, model, desc, nchains, opt, seed):
    """an Engine over a context made by idhmc_create_glm (Engine itself takes that road only for a model with groups)"""
    eng = idhmc.Engine.__new__(idhmc.Engine)
    eng.lib, eng.model, eng.opt, eng.C, eng.D, eng._hook = idhmc.load_library(), model, opt, nchains, model.D, None
    h = C.c_void_p()
    rc = eng.lib.idhmc_create_glm(C.byref(h), 0, nchains, 0, C.byref(desc), C.byref(opt), seed)
    assert rc == 0, eng.lib.idhmc_last_error()
    eng.h = h
    return eng


@pytest.mark.parametrize("family", ["POISSON_LOG", "GAUSSIAN_IDENTITY_LOGSIGMA"])
def test_without_groups_the_context_is_the_one_of_kinds_5_and_6(idhmc, family):
    """idhmc_create_glm with H = 0 against idhmc_create (IDHMC_MODEL_GLM, IDHMC_MODEL_GLM_AUX) on the same data: the same form, the
    same bits after evaluation and three fused transitions, the same device bytes"""
    from inplacedhmc_jl_amd import _lib
    n, Dx, C_ = 300, 100, 37
    A = SHAPE[family][2]
    X, Y = (FLAT.problem(family, n, Dx, seed=4) if A == 0 else AUX.problem_aux(family, n, Dx, seed=4))
    mu, tau = prior(Dx + A)
    opt = idhmc.default_options(max_depth=6)
    m = idhmc.GLM(X, Y, getattr(idhmc.glm, family), prior_mu=mu, prior_tau=tau, aux=A)
    assert m.kind == (idhmc.MODEL_GLM_AUX if A else idhmc.MODEL_GLM)
    a = idhmc.Engine(m, C_, opt, seed=9)
    Xc, Yc = np.ascontiguousarray(X), np.ascontiguousarray(Y, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    d = _lib.GlmDesc(n=n, Dx=Dx, K=1, nc=0, A=A, H=0, X=Xc.ctypes.data_as(dp), Y=Yc.ctypes.data_as(dp), mu=mu.ctypes.data_as(dp),
                     tau=tau.ctypes.data_as(dp), source=getattr(idhmc.glm, family).encode())
    b = _engine_from_glm_desc(idhmc, m, d, C_, opt, 9)
    assert a.glm_form() == b.glm_form() == 1 and a.padded_dim() == b.padded_dim() and a.device_bytes() == b.device_bytes()

    def same():
        return same_bits(a.q, b.q) and same_bits(a.lq, b.lq) and same_bits(a.grad, b.grad)
    q = np.random.default_rng(2).uniform(-0.2, 0.2, (C_, Dx + A))
    a.set_q(q)
    b.set_q(q)
    assert same()
    a.set_eps(0.03)
    b.set_eps(0.03)
    a.nuts_transitions(1, 3)
    b.nuts_transitions(1, 3)
    assert same() and np.array_equal(a.tree_stats(), b.tree_stats())
    a.close()
    b.close()


def test_posterior_mean_of_the_log_scale_against_quadrature(idhmc):
    """An independent answer.  Gaussian likelihood with KNOWN sigma (a test-only source), an ungrouped intercept and one group of 10
    one-hot levels, n = 60: given omega the coefficients integrate out, p(omega | y) is proportional to
    N(omega; mu, 1 / tau) N(y; 0, sigma^2 I + X diag(s_c^2 / tau_c) X'), one-dimensional, and quadrature (5601 points on [-8, 6])
    gives E[omega | y].  The mean over 64 chains of their means of omega (default warm-up, 200 draws each) must lie within 5
    standard errors, the standard error being the standard deviation of the 64 chain means over sqrt(64): chains are independent,
    so 5 is a false-alarm rate near 6e-7 -- a condition, not a tuned number.  The oracle's own threaded_mcmc on this problem gave
    -0.62838, -0.63568, -0.63431 (seeds 1, 2, 3; standard errors about 0.005) against the quadrature's -0.63658, with no
    divergent transition and every draw finite, so no share of non-finite draws is allowed."""
    n, levels, sigma, C_, N = 60, 10, 0.5, 64, 200
    rng = np.random.default_rng(5)
    lab = rng.integers(0, levels, n)
    eff = rng.standard_normal(levels) * 0.7
    noise = rng.standard_normal(n) * sigma
    X = np.zeros((n, 1 + levels))
    X[:, 0] = 1.0
    X[np.arange(n), 1 + lab] = 1.0
    y = 0.3 + eff[lab] + noise
    grp = np.r_[-1, np.zeros(levels, int)]
    om = np.linspace(-8.0, 6.0, 5601)
    logp = np.empty(om.size)
    for k, w in enumerate(om):
        S = sigma ** 2 * np.eye(n) + X @ np.diag(np.r_[1.0, np.full(levels, np.exp(2.0 * w))]) @ X.T
        logp[k] = -0.5 * w * w - 0.5 * np.linalg.slogdet(S)[1] - 0.5 * y @ np.linalg.solve(S, y)
    p = np.exp(logp - logp.max())
    want = np.sum(om * p) / np.sum(p)
    model = idhmc.GLM(X, y, source(idhmc, "GAUSSIAN_KNOWN"), constants=[sigma], groups=grp)
    assert (model.Dx, model.A, model.H, model.D) == (11, 0, 1, 12)
    chains, stats = idhmc.threaded_mcmc(model, N, nchains=C_, seed=1)
    # a chain has NS = max(N, longest warm-up stage) rows, the reference's layout: the first N are the draws
    assert len(chains) == C_ and all(ch.shape == (400, 12) for ch in chains) and stats.shape == (C_, 400)
    draws = np.stack(chains)[:, :N]
    assert draws.shape == (C_, N, 12) and np.isfinite(draws).all()
    beta = idhmc.glm.coefficients(model, draws)
    assert beta.shape == (C_, N, 11) and np.isfinite(beta).all() and idhmc.glm.group_scales(model, draws).shape == (C_, N, 1)
    means = draws[:, :, 11].mean(1)
    se = means.std(ddof=1) / np.sqrt(C_)
    print("E[omega | y]: quadrature %.5f, chains %.5f, standard error %.5f" % (want, means.mean(), se))
    assert abs(means.mean() - want) <= 5.0 * se, (means.mean(), want, se)
