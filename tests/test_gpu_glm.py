"""User-defined GLM likelihoods (IDHMC_MODEL_GLM) on the device.  The logistic likelihood as a GLM source is bit-identical to the
built-in LogisticRegression (one template, two observations); each shipped source is bit-identical to the CPU oracle running its
C restatement (tests/test_glm_cpu.py, through oracle.OracleModel.custom) and within 1e-12 of numpy, in both device forms: one chain
per wavefront (evaluation, leapfrog, stepsize search, local optimum; NUTS at L > 256) and the matrix-core gradient of the NUTS
kernel (L <= 256).  Every GLM context compiles its source with hipRTC, so each test creates few."""
import numpy as np
import pytest

from test_glm_cpu import SHIPPED, c_source, constants, numpy_density, oracle_params, problem

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def prior(D, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)


def glm(idhmc, family, X, Y, mu=None, tau=None):
    return idhmc.GLM(X, Y, getattr(idhmc.glm, family), constants(family), mu, tau)


def setup(idhmc, oracle, tmp_path, family, n, D, C, seed, opt=None, oopt=None):
    X, Y = problem(family, n, D, seed=n + D)
    mu, tau = prior(D)
    eng = idhmc.Engine(glm(idhmc, family, X, Y, mu, tau), C, opt, seed=seed)
    om = oracle.OracleModel.custom(D, c_source(family), oracle_params(X, Y, constants(family), mu, tau), str(tmp_path))
    chains = [oracle.OracleChain(om, oopt, seed=seed, chain_id=c) for c in range(C)]
    return X, Y, mu, tau, eng, chains


def start(eng, chains, D, scale=0.3):
    """a common random start near the origin (the oracle's random_position draws from U(-2, 2): too far out for a count model)"""
    q = np.random.default_rng(D).uniform(-scale, scale, (len(chains), D)) / np.sqrt(D)
    eng.set_q(q)
    for c, ch in enumerate(chains):
        ch.set_q(q[c])


@pytest.mark.parametrize("D", [25, 100, 200, 300])
def test_logistic_as_a_glm_source_is_the_builtin(idhmc, D):
    """BERNOULLI_LOGIT through IDHMC_MODEL_GLM (hipRTC) and IDHMC_MODEL_LOGISTIC_REGRESSION (ahead of time): the same bits after a
    random position, one NUTS transition and a fused launch of several, in the matrix-core form (D <= 256) and the per-wave one"""
    n, C, eps = 300, 37, 0.05
    X, y = problem("BERNOULLI_LOGIT", n, D, seed=D)
    mu, tau = prior(D)
    opt = idhmc.default_options(max_depth=6)
    a = idhmc.Engine(idhmc.GLM(X, y, idhmc.glm.BERNOULLI_LOGIT, prior_mu=mu, prior_tau=tau), C, opt, seed=9)
    b = idhmc.Engine(idhmc.LogisticRegression(X, y, mu, tau), C, opt, seed=9)

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


@pytest.mark.parametrize("family", SHIPPED)
@pytest.mark.parametrize("D,n", [(25, 1), (25, 37), (25, 128), (25, 1000), (300, 1000)])
def test_density_both_forms(idhmc, oracle, tmp_path, family, D, n):
    """lq and grad l: the per-wave form (evaluation), and after one NUTS transition the form the NUTS kernel ran (matrix cores at
    D <= 256) -- each bit-identical to the oracle and within 1e-12 of numpy's closed form"""
    C = 18
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, D, C, seed=3, opt=idhmc.default_options(max_depth=5),
                                       oopt=oracle.default_options(max_depth=5))
    start(eng, chains, D)

    def check():
        q, g, lq = eng.q, eng.grad, eng.lq
        assert same_bits(lq, [c.lq for c in chains]) and same_bits(g, np.stack([c.grad[:D] for c in chains]))
        for c in (0, C - 1):
            l_ref, g_ref, lscale, gscale = numpy_density(family, X, Y, q[c], mu, tau)
            assert abs(lq[c] - l_ref) <= 1e-12 * lscale
            assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)
    check()
    eng.set_eps(0.02)
    eng.nuts_transition(1)
    for ch in chains:
        ch.sample_tree(0.02, 1)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    check()
    eng.close()


@pytest.mark.parametrize("family", SHIPPED)
def test_leapfrog_and_stepsize_search(idhmc, oracle, tmp_path, family):
    D, n, C = 100, 128, 6
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, D, C, seed=21)
    start(eng, chains, D)
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
@pytest.mark.parametrize("family", SHIPPED)
def test_nuts_transitions(idhmc, oracle, tmp_path, family, shared):
    """single-transition launches, then several per launch (idhmc_nuts_transitions): the matrix-core form with a ragged last group
    of 16 (37 chains), per-chain and shared unit metric; then a small eps whose trees stop at max_depth"""
    D, n, C, depth, T = 25, 200, 37, 4, 2
    opt = idhmc.default_options(max_depth=depth, metric_mode=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, D, C, seed=5, opt=opt,
                                       oopt=oracle.default_options(max_depth=depth))
    start(eng, chains, D)
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


@pytest.mark.parametrize("family", SHIPPED)
def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path, family):
    D, n, C, N = 25, 200, 5, 8
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    X, Y = problem(family, n, D, seed=9)
    eng = idhmc.Engine(glm(idhmc, family, X, Y), C, idhmc.default_options(**short), seed=77)
    draws, stats = eng.mcmc_with_warmup(N)
    om = oracle.OracleModel.custom(D, c_source(family), oracle_params(X, Y, constants(family)), str(tmp_path))
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, C, oracle.default_options(**short), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps)
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats.T, ost[:, :N])
    eng.close()


def test_poisson_local_optimum_is_the_map(idhmc):
    """find_local_optimum maximises l(q) - penalty/2 |q|^2; a Newton solve of the same objective in numpy gives the MAP"""
    D, n, C, pen = 8, 400, 6, 1e-4
    X, Y = problem("POISSON_LOG", n, D, seed=2)
    mu, tau = np.full(D, 0.1), np.full(D, 0.5)
    eng = idhmc.Engine(glm(idhmc, "POISSON_LOG", X, Y, mu, tau), C, seed=4)
    eng.set_q(np.random.default_rng(1).uniform(-0.2, 0.2, (C, D)))
    eng.find_local_optimum(pen, 200)
    q = np.zeros(D)
    for _ in range(50):
        g = numpy_density("POISSON_LOG", X, Y, q, mu, tau)[1] - pen * q
        H = -(X.T * np.exp(X @ q)) @ X - np.diag(tau) - pen * np.eye(D)
        q = q - np.linalg.solve(H, g)
    assert np.abs(numpy_density("POISSON_LOG", X, Y, q, mu, tau)[1] - pen * q).max() < 1e-10
    np.testing.assert_allclose(eng.q, np.broadcast_to(q, (C, D)), rtol=0, atol=1e-6)
    eng.close()


def test_poisson_threaded_mcmc(idhmc):
    """threaded_mcmc's shapes, and a posterior mean near the true coefficients at n = 2000"""
    D, n, C, N = 6, 2000, 8, 150
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, D)) * 0.5
    X[:, 0] = 1.0
    beta = np.array([0.5, -0.3, 0.2, 0.0, 0.4, -0.1])
    Y = rng.poisson(np.exp(X @ beta)).astype(float)
    stages = idhmc.default_warmup_stages(middle_steps=20, doubling_stages=2, init_steps=30, terminating_steps=20)
    chains, stats = idhmc.threaded_mcmc(idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG), N, nchains=C, warmup_stages=stages, seed=3)
    assert len(chains) == C and all(ch.shape == (N, D) for ch in chains) and stats.shape == (C, N)
    draws = np.concatenate(chains)
    assert np.isfinite(draws).all()
    sd = draws.std(0)
    assert np.all(np.abs(draws.mean(0) - beta) < 5 * sd + 0.05), (draws.mean(0), beta, sd)


def test_a_compile_error_is_reported(idhmc):
    X, Y = problem("POISSON_LOG", 50, 4)
    bad = "__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v) { r = z +; v = 0.0; }"
    with pytest.raises(idhmc.IdhmcError) as e:
        idhmc.Engine(idhmc.GLM(X, Y, bad), 8)
    assert e.value.code == idhmc.ERR_BAD_ARG and "did not compile" in str(e.value) and "user_glm.hip" in str(e.value)
    missing = "__device__ void not_the_observation(double z) {}"
    with pytest.raises(idhmc.IdhmcError) as e:
        idhmc.Engine(idhmc.GLM(X, Y, missing), 8)
    assert e.value.code == idhmc.ERR_BAD_ARG and "did not compile" in str(e.value)
    eng = idhmc.Engine(idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG), 8)   # the device is fine afterwards
    eng.random_position()
    assert np.isfinite(eng.lq).all()
    eng.close()
