"""Bayesian logistic regression (IDHMC_MODEL_LOGISTIC_REGRESSION) on the device against the CPU oracle running the density's C
restatement (tests/test_logistic_cpu.py, through oracle.OracleModel.custom), bit-exact fp64.  Two device forms follow one
arithmetic: one chain per wavefront (evaluation, leapfrog, stepsize search, local optimum; NUTS at L > 256)
and the workgroup-cooperative matrix-core gradient of the NUTS kernel (L <= 256, 16 chains per v_mfma_f64_16x16x4_f64 tile)."""
import numpy as np
import pytest

from test_logistic_cpu import C_SRC, numpy_density, oracle_params, problem

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def prior(D, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)


def setup(idhmc, oracle, tmp_path, n, D, C, seed, opt=None, oopt=None, prior_args=True):
    X, y = problem(n, D, seed=n + D)
    mu, tau = prior(D) if prior_args else (None, None)
    eng = idhmc.Engine(idhmc.LogisticRegression(X, y, mu, tau), C, opt, seed=seed)
    om = oracle.OracleModel.custom(D, C_SRC, oracle_params(X, y, mu, tau), str(tmp_path))
    chains = [oracle.OracleChain(om, oopt, seed=seed, chain_id=c) for c in range(C)]
    return X, y, mu, tau, eng, chains


@pytest.mark.parametrize("n", [1, 37, 128, 1000])
@pytest.mark.parametrize("D", [25, 100, 200, 300])
def test_density_both_forms(idhmc, oracle, tmp_path, D, n):
    """lq and grad l: the per-wave form (evaluation at a random position) and, after one NUTS transition, the form the NUTS
    kernel ran (matrix cores at D <= 256) -- each bit-identical to the oracle and within 1e-12 of numpy's closed form"""
    C = 18
    X, y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, n, D, C, seed=3, oopt=oracle.default_options(max_depth=5),
                                       opt=idhmc.default_options(max_depth=5))
    eng.random_position()
    for ch in chains:
        ch.random_position()

    def check():
        q, g, lq = eng.q, eng.grad, eng.lq
        assert same_bits(lq, [c.lq for c in chains]) and same_bits(g, np.stack([c.grad[:D] for c in chains]))
        for c in (0, C - 1):
            l_ref, g_ref, scale = numpy_density(X, y, q[c], mu, tau)
            assert abs(lq[c] - l_ref) <= 1e-12 * abs(l_ref)
            assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * scale + 1e-300)
    check()
    eng.set_eps(0.05)
    eng.nuts_transition(1)
    for ch in chains:
        ch.sample_tree(0.05, 1)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    check()


@pytest.mark.parametrize("D,n", [(25, 1000), (100, 37), (300, 128)])
def test_leapfrog_and_stepsize_search(idhmc, oracle, tmp_path, D, n):
    C = 6
    X, y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, n, D, C, seed=21)
    eng.random_position()
    eng.refresh_momentum(1)
    eng.leapfrog(0.02, 3)
    eng.leapfrog(-0.02, 1)
    for ch in chains:
        ch.random_position()
        ch.rand_p(1)
        for e in (0.02, 0.02, 0.02, -0.02):
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


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("D,n,C,eps,depth", [(25, 1000, 37, 0.05, 6), (100, 128, 16, 0.04, 6), (200, 37, 37, 0.05, 5),
                                             (300, 100, 9, 0.04, 5), (100, 1000, 20, 0.002, 3)])
def test_nuts_transitions(idhmc, oracle, tmp_path, D, n, C, eps, depth, shared):
    """single-transition launches, then several transitions per launch (idhmc_nuts_transitions): both forms, a ragged last group
    of 16, per-chain and shared unit metric, and (eps = 0.002, depth 3) trees that stop at max_depth"""
    T = 3
    opt = idhmc.default_options(max_depth=depth, metric_mode=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    X, y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, n, D, C, seed=5, opt=opt,
                                       oopt=oracle.default_options(max_depth=depth))
    eng.random_position()
    eng.set_eps(eps)
    for ch in chains:
        ch.random_position()
    reached = 0
    for it in range(1, T + 1):
        eng.nuts_transition(it)
        st = eng.tree_stats()
        ost = [ch.sample_tree(eps, it) for ch in chains]
        for f in ("depth", "steps", "term_left", "term_right"):
            np.testing.assert_array_equal(st[f], [getattr(s, f) for s in ost], err_msg="%s @%d" % (f, it))
        assert same_bits(st["pi"], [s.pi for s in ost]) and same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        reached += int((st["depth"] == depth).sum())
    if eps == 0.002:
        assert reached >= T * C // 2                  # trees that ran to max_depth
    eng.nuts_transitions(T + 1, T)
    for it in range(T + 1, 2 * T + 1):
        for ch in chains:
            ch.sample_tree(eps, it)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    assert same_bits(eng.grad, np.stack([c.grad[:D] for c in chains])) and same_bits(eng.lq, [c.lq for c in chains])


@pytest.mark.parametrize("D,n", [(25, 200), (300, 40)])
def test_full_warmup_matches_oracle(idhmc, oracle, tmp_path, D, n):
    C, N = 5, 10
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    opt = idhmc.default_options(**short)
    X, y = problem(n, D, seed=9)
    eng = idhmc.Engine(idhmc.LogisticRegression(X, y), C, opt, seed=77)
    draws, stats = eng.mcmc_with_warmup(N)
    om = oracle.OracleModel.custom(D, C_SRC, oracle_params(X, y), str(tmp_path))
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, C, oracle.default_options(**short), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps)
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats.T, ost[:, :N])


def test_local_optimum_is_the_map(idhmc):
    """find_local_optimum maximises l(q) - penalty/2 |q|^2; a Newton solve of the same objective in numpy gives the MAP"""
    D, n, C, pen = 8, 400, 6, 1e-4
    X, y = problem(n, D, seed=2, scale=1.0)
    mu, tau = np.full(D, 0.1), np.full(D, 0.5)
    eng = idhmc.Engine(idhmc.LogisticRegression(X, y, mu, tau), C, seed=4)
    eng.random_position()
    eng.find_local_optimum(pen, 200)
    q = np.zeros(D)
    for _ in range(50):
        _, g, _ = numpy_density(X, y, q, mu, tau)
        g = g - pen * q
        s = 1.0 / (1.0 + np.exp(-(X @ q)))
        H = -(X.T * (s * (1 - s))) @ X - np.diag(tau) - pen * np.eye(D)
        q = q - np.linalg.solve(H, g)
    assert np.abs(numpy_density(X, y, q, mu, tau)[1] - pen * q).max() < 1e-10
    np.testing.assert_allclose(eng.q, np.broadcast_to(q, (C, D)), rtol=0, atol=1e-6)


def test_threaded_mcmc_shapes(idhmc):
    D, n, C, N = 30, 300, 4, 20
    X, y = problem(n, D, seed=8)
    stages = idhmc.default_warmup_stages(middle_steps=10, doubling_stages=2, init_steps=15, terminating_steps=10)
    chains, stats = idhmc.threaded_mcmc(idhmc.LogisticRegression(X, y), N, nchains=C, warmup_stages=stages, seed=3)
    assert len(chains) == C and all(ch.shape == (N, D) for ch in chains) and stats.shape == (C, N)
    assert all(np.isfinite(ch).all() for ch in chains)
    draws = np.concatenate(chains)
    assert np.abs(draws.mean(0)).max() < 3.0
