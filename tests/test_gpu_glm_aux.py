"""GLM likelihoods with sampled auxiliary parameters (IDHMC_MODEL_GLM_AUX) on the device.  Each shipped source, and a test-only
one with the maximum A = 4, is bit-identical to the CPU oracle running the C restatement of DESIGN section 12
(tests/test_glm_aux_cpu.py, through oracle.OracleModel.custom) and within 1e-12 of numpy, in both device forms: one chain per
wavefront (evaluation, leapfrog, stepsize search, local optimum; NUTS where the tiles do not fit) and the matrix-core gradient of
the NUTS kernel.  No tolerance on the device side.  Every context compiles its source with hipRTC (about a second), so engines
are shared across assertions."""
import numpy as np
import pytest

from test_glm_aux_cpu import (FAMILIES, SHAPE, SHIPPED_AUX, TRUE_A, c_source_aux, consts, make, numpy_density_aux, oracle_params_aux,
                              problem_aux, start_aux)
from test_glm_cpu import problem

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def prior(D, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)


def setup(idhmc, oracle, tmp_path, family, n, Dx, C, seed, opt=None, oopt=None):
    A = SHAPE[family][2]
    D = Dx + A
    X, Y = problem_aux(family, n, Dx, seed=n + Dx)
    mu, tau = prior(D)
    eng = idhmc.Engine(make(idhmc, family, X, Y, mu, tau), C, opt, seed=seed)
    om = oracle.OracleModel.custom(D, c_source_aux(family), oracle_params_aux(X, Y, A, consts(family), mu, tau), str(tmp_path))
    chains = [oracle.OracleChain(om, oopt, seed=seed, chain_id=c) for c in range(C)]
    return X, Y, mu, tau, eng, chains


def start(eng, chains, family, Dx, q=None):
    q = start_aux(family, len(chains), Dx) if q is None else q
    eng.set_q(q)
    for c, ch in enumerate(chains):
        ch.set_q(q[c])
    return q


def coop_expected(L, A, shared):
    """DESIGN section 12's table: the matrix-core form where the A further planes fit a CU's LDS next to the NUTS kernel's vectors"""
    if L == 128:
        return True
    if L == 256:
        return A <= 1 or (A == 2 and shared)
    return False


def check_density(eng, chains, family, X, Y, mu, tau, D, ends):
    q, g, lq = eng.q, eng.grad, eng.lq
    assert same_bits(lq, [c.lq for c in chains]) and same_bits(g, np.stack([c.grad[:D] for c in chains]))
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_aux(family, X, Y, q[c], mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


@pytest.mark.parametrize("family", SHIPPED_AUX)
@pytest.mark.parametrize("Dx", [25, 127, 128, 200, 300])
@pytest.mark.parametrize("n", [1, 37, 128, 1000])
def test_density_both_forms(idhmc, oracle, tmp_path, family, Dx, n):
    """lq and grad l: the per-wave form (evaluation), and after one NUTS transition the form the NUTS kernel ran -- the matrix cores
    up to Dx = 200 (Dx = 127: the auxiliary coordinate is index 127, the last lane's second residue; Dx = 128: index 128, L = 256),
    the per-wave form at Dx = 300 -- each bit-identical to the oracle and within 1e-12 of numpy's closed form"""
    C, D = 18, Dx + 1
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, C, seed=3, opt=idhmc.default_options(max_depth=4),
                                       oopt=oracle.default_options(max_depth=4))
    assert eng.glm_form() == (1 if Dx <= 200 else 0) and eng.padded_dim() == (128 if Dx <= 127 else 256 if Dx <= 200 else 512)
    start(eng, chains, family, Dx)
    check_density(eng, chains, family, X, Y, mu, tau, D, (0, C - 1))
    eng.set_eps(0.02)
    eng.nuts_transition(1)
    for ch in chains:
        ch.sample_tree(0.02, 1)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    check_density(eng, chains, family, X, Y, mu, tau, D, (0, C - 1))
    eng.close()


@pytest.mark.parametrize("Dx,n,shared", [(20, 300, True), (20, 300, False), (124, 37, True), (126, 200, True), (126, 200, False), (300, 128, True)])
def test_four_auxiliary_coordinates(idhmc, oracle, tmp_path, Dx, n, shared):
    """A = 4, K = 2: every plane and owner-lane position.  L = 128 is the matrix-core form with either metric (with a per-chain one
    the tightest row of the LDS table); Dx = 124 puts the four coordinates in the last two lanes; Dx = 126 splits them across the
    chunks of L = 256, where four planes do not fit and NUTS runs the per-wave form, as it does at L = 512.  The evaluation before
    the first transition is the per-wave form at every shape."""
    family, C = "TEST_A4", 37
    D = Dx + 4
    mode = idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, C, seed=8, opt=idhmc.default_options(max_depth=4, metric_mode=mode),
                                       oopt=oracle.default_options(max_depth=4))
    assert eng.glm_form() == (1 if coop_expected(eng.padded_dim(), 4, shared) else 0) == (1 if Dx <= 124 else 0)
    start(eng, chains, family, Dx)
    check_density(eng, chains, family, X, Y, mu, tau, D, (0, 17, C - 1))
    for it, eps in ((1, 0.02), (2, 0.002)):
        eng.set_eps(eps)
        eng.nuts_transition(it)
        st = eng.tree_stats()
        ost = [ch.sample_tree(eps, it) for ch in chains]
        np.testing.assert_array_equal(st["depth"], [s.depth for s in ost])
        np.testing.assert_array_equal(st["steps"], [s.steps for s in ost])
        assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        check_density(eng, chains, family, X, Y, mu, tau, D, (0, C - 1))
    eng.close()


def _form_source(A):
    """a Gaussian with log sigma = a[0] whose further auxiliary coordinates see only their prior"""
    return ("__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)\n{\n"
            "    const double w = dexp(-a[0]);\n    const double u = (o.y[0] - z) * w;\n    v = 0.5 * (u * u) + a[0];\n    r = u * w;\n"
            "    s[0] = u * u - 1.0;\n" + "".join("    s[%d] = 0.0;\n" % j for j in range(1, A)) + "}\n")


def test_the_form_in_use_matches_the_table(idhmc):
    """idhmc_glm_form per (L, A, metric) is DESIGN section 12's table, and each of those kernels launches (its LDS fits)"""
    rng = np.random.default_rng(0)
    for Dx, L in ((30, 128), (200, 256), (300, 512)):
        X = rng.standard_normal((40, Dx)) * 0.3
        Y = rng.standard_normal(40)
        for A in (1, 2, 3, 4):
            for mode in (idhmc.METRIC_PER_CHAIN, idhmc.METRIC_SHARED, idhmc.METRIC_POOLED):
                if (L == 512 and A > 1) or (mode == idhmc.METRIC_POOLED and (L, A) != (128, 4)):
                    continue                                    # a pooled metric is a shared one to the kernel: one case of it
                eng = idhmc.Engine(idhmc.GLM(X, Y, _form_source(A), aux=A), 20, idhmc.default_options(max_depth=3, metric_mode=mode), seed=2)
                assert eng.padded_dim() == L
                assert eng.glm_form() == (1 if coop_expected(L, A, mode != idhmc.METRIC_PER_CHAIN) else 0), (L, A, mode)
                eng.set_q(rng.uniform(-0.1, 0.1, (20, Dx + A)))
                eng.set_eps(0.01)
                eng.nuts_transition(1)
                assert np.isfinite(eng.lq).all() and (eng.tree_stats()["steps"] >= 1).all()
                eng.close()
    b = idhmc.Engine(idhmc.DiagGaussian(np.zeros(8), sigma=np.ones(8)), 4)
    assert b.glm_form() == -1
    b.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_leapfrog_and_stepsize_search(idhmc, oracle, tmp_path, family):
    Dx, n, C = 100, 128, 6
    D = Dx + SHAPE[family][2]
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, C, seed=21)
    start(eng, chains, family, Dx)
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


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
def test_nuts_transitions(idhmc, oracle, tmp_path, family, shared):
    """single-transition launches, then several per launch (idhmc_nuts_transitions): a ragged last group of 16 (37 chains), per-chain
    and shared unit metric; then a small eps whose trees stop at max_depth"""
    Dx, n, C, depth, T = 25, 200, 37, 4, 2
    D = Dx + SHAPE[family][2]
    opt = idhmc.default_options(max_depth=depth, metric_mode=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, C, seed=5, opt=opt,
                                       oopt=oracle.default_options(max_depth=depth))
    assert eng.glm_form() == (1 if coop_expected(128, SHAPE[family][2], shared) else 0)
    start(eng, chains, family, Dx)
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
            assert reached >= T * C // 2                  # trees that ran to max_depth
    eng.close()


@pytest.mark.parametrize("family", SHIPPED_AUX)
def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path, family):
    Dx, n, C, N = 25, 200, 5, 8
    A = SHAPE[family][2]
    D = Dx + A
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    X, Y = problem_aux(family, n, Dx, seed=9)
    eng = idhmc.Engine(make(idhmc, family, X, Y), C, idhmc.default_options(**short), seed=77)
    draws, stats = eng.mcmc_with_warmup(N)
    om = oracle.OracleModel.custom(D, c_source_aux(family), oracle_params_aux(X, Y, A, consts(family)), str(tmp_path))
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, C, oracle.default_options(**short), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps)
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats.T, ost[:, :N])
    eng.close()


def test_an_overflowing_chain_is_a_rejected_start(idhmc, oracle, tmp_path):
    """one chain of 37 with a0 = -800 (dexp(800) = +inf): lq = -inf in the per-wave form (evaluation) and after a NUTS transition on
    the matrix cores, exactly as the oracle has it; the other chains of its workgroup keep their oracle bits; no device error"""
    family, Dx, n, C, bad = "GAUSSIAN_IDENTITY_LOGSIGMA", 25, 200, 37, 20
    D = Dx + 1
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, C, seed=6, opt=idhmc.default_options(max_depth=4),
                                       oopt=oracle.default_options(max_depth=4))
    assert eng.glm_form() == 1
    q = start_aux(family, C, Dx)
    q[bad, Dx] = -800.0
    start(eng, chains, family, Dx, q)
    ok = np.arange(C) != bad
    lq = eng.lq
    assert lq[bad] == -np.inf and chains[bad].lq == -np.inf and np.isfinite(lq[ok]).all()
    assert same_bits(lq, [c.lq for c in chains]) and same_bits(eng.grad[ok], np.stack([c.grad[:D] for c in chains])[ok])
    eng.set_eps(0.02)
    for it in (1, 2):
        eng.nuts_transition(it)
        for ch in chains:
            ch.sample_tree(0.02, it)
        lq = eng.lq
        assert lq[bad] == -np.inf and same_bits(lq, [c.lq for c in chains])
        assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        assert same_bits(eng.grad[ok], np.stack([c.grad[:D] for c in chains])[ok])
    eng.close()


def test_gaussian_local_optimum_is_the_map(idhmc):
    """find_local_optimum maximises l(q) - penalty/2 |q|^2; a Newton solve of the same objective in (beta, log sigma) gives the MAP"""
    family, Dx, n, C, pen = "GAUSSIAN_IDENTITY_LOGSIGMA", 8, 400, 6, 1e-4
    D = Dx + 1
    X, Y = problem_aux(family, n, Dx, seed=2)
    mu, tau = np.full(D, 0.1), np.full(D, 0.5)
    eng = idhmc.Engine(make(idhmc, family, X, Y, mu, tau), C, seed=4)
    q0 = np.random.default_rng(1).uniform(-0.2, 0.2, (C, D))
    q0[:, Dx] += TRUE_A[family][0]
    eng.set_q(q0)
    eng.find_local_optimum(pen, 200)
    q = np.zeros(D)
    q[Dx] = TRUE_A[family][0]
    for _ in range(50):
        g = numpy_density_aux(family, X, Y, q, mu, tau)[1] - pen * q
        w2 = np.exp(-2.0 * q[Dx])
        e = Y - X @ q[:Dx]
        H = np.zeros((D, D))
        H[:Dx, :Dx] = -w2 * X.T @ X
        H[:Dx, Dx] = H[Dx, :Dx] = -2.0 * w2 * X.T @ e
        H[Dx, Dx] = -2.0 * w2 * e @ e
        H -= np.diag(tau) + pen * np.eye(D)
        q = q - np.linalg.solve(H, g)
    assert np.abs(numpy_density_aux(family, X, Y, q, mu, tau)[1] - pen * q).max() < 1e-10
    np.testing.assert_allclose(eng.q, np.broadcast_to(q, (C, D)), rtol=0, atol=1e-6)
    eng.close()


def test_gaussian_threaded_mcmc_recovers_the_scale(idhmc):
    """threaded_mcmc's shapes, and the pooled posterior mean of log sigma within 4 posterior standard deviations (about
    4 / sqrt(2 n)) of the log of the least-squares residual standard deviation: the sign and the scale of s"""
    Dx, n, C, N, sigma = 6, 2000, 8, 150, 0.6
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, Dx)) * 0.5
    X[:, 0] = 1.0
    beta = np.array([0.5, -0.3, 0.2, 0.0, 0.4, -0.1])
    Y = X @ beta + sigma * rng.standard_normal(n)
    stages = idhmc.default_warmup_stages(middle_steps=20, doubling_stages=2, init_steps=30, terminating_steps=20)
    model = idhmc.GLM(X, Y, idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1)
    chains, stats = idhmc.threaded_mcmc(model, N, nchains=C, warmup_stages=stages, seed=3)
    assert len(chains) == C and all(ch.shape == (N, Dx + 1) for ch in chains) and stats.shape == (C, N)
    draws = np.concatenate(chains)
    assert np.isfinite(draws).all()
    res = Y - X @ np.linalg.lstsq(X, Y, rcond=None)[0]
    want = np.log(np.sqrt(res @ res / (n - Dx)))
    assert abs(draws[:, Dx].mean() - want) < 4.0 / np.sqrt(2.0 * n), (draws[:, Dx].mean(), want)
    sd = draws.std(0)
    assert np.all(np.abs(draws[:, :Dx].mean(0) - beta) < 5 * sd[:Dx] + 0.05)


def test_logistic_as_a_glm_source_is_still_the_builtin(idhmc):
    """A = 0 is intact: BERNOULLI_LOGIT through IDHMC_MODEL_GLM equals the built-in logistic regression, bit for bit"""
    n, C, D, eps = 300, 37, 100, 0.05
    X, y = problem("BERNOULLI_LOGIT", n, D, seed=D)
    mu, tau = prior(D)
    opt = idhmc.default_options(max_depth=6)
    a = idhmc.Engine(idhmc.GLM(X, y, idhmc.glm.BERNOULLI_LOGIT, prior_mu=mu, prior_tau=tau), C, opt, seed=9)
    b = idhmc.Engine(idhmc.LogisticRegression(X, y, mu, tau), C, opt, seed=9)
    assert a.glm_form() == b.glm_form() == 1

    def same():
        return same_bits(a.q, b.q) and same_bits(a.lq, b.lq) and same_bits(a.grad, b.grad)
    a.random_position()
    b.random_position()
    assert same()
    a.set_eps(eps)
    b.set_eps(eps)
    a.nuts_transition(1)
    b.nuts_transition(1)
    assert same() and np.array_equal(a.tree_stats(), b.tree_stats())
    a.nuts_transitions(2, 3)
    b.nuts_transitions(2, 3)
    assert same() and np.array_equal(a.tree_stats(), b.tree_stats())
    a.close()
    b.close()
