"""Negative-binomial, gamma and beta regression on the device.  dlgamma_psi itself over its whole domain, each
shipped source, and the negative binomial through every driver and with coefficient groups, are bit-identical to the CPU oracle
running the C restatements of tests/test_glm_dispersion_cpu.py (the C twin of dlgamma_psi inside test_glm_aux_cpu.C_BODY_AUX or
test_glm_hier_cpu.C_BODY_HIER, through oracle.OracleModel.custom), in both device forms: one chain per wavefront and the matrix-core
gradient of the NUTS kernel.  No tolerance on the device side.  Every context compiles its source with hipRTC (about a second), so
engines are shared across assertions."""
import numpy as np
import pytest
from scipy import optimize

import test_glm_aux_cpu as AUX
import test_glm_hier_cpu as HIER
from test_glm_dispersion_cpu import (SHIPPED, TRUE_A, c_source_disp, c_source_disp_hier, make, numpy_density_disp, problem_disp,
                                     problem_grouped, response, start_disp, start_grouped)

pytestmark = pytest.mark.gpu
NB = "NEG_BINOMIAL_LOG_LOGPHI"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def prior(D, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)


def setup(idhmc, oracle, tmp_path, family, n, Dx, C, seed, opt=None, oopt=None):
    D = Dx + 1
    X, Y = problem_disp(family, n, Dx, seed=n + Dx)
    mu, tau = prior(D)
    eng = idhmc.Engine(make(idhmc, family, X, Y, mu, tau), C, opt, seed=seed)
    om = oracle.OracleModel.custom(D, c_source_disp(family), AUX.oracle_params_aux(X, Y, 1, None, mu, tau), str(tmp_path))
    chains = [oracle.OracleChain(om, oopt, seed=seed, chain_id=c) for c in range(C)]
    return X, Y, mu, tau, eng, chains


def start(eng, chains, q):
    eng.set_q(q)
    for c, ch in enumerate(chains):
        ch.set_q(q[c])
    return q


def check_bits(eng, chains, D):
    assert same_bits(eng.lq, [c.lq for c in chains]) and same_bits(eng.grad, np.stack([c.grad[:D] for c in chains]))


def check_density(eng, chains, family, X, Y, mu, tau, D, ends, grp=None):
    check_bits(eng, chains, D)
    q, g, lq = eng.q, eng.grad, eng.lq
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_disp(family, X, Y, q[c], mu, tau, grp)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


@pytest.mark.parametrize("lo,hi", [(-690.0, 690.0), (-3.0, 4.0)])
def test_dlgamma_psi_is_the_twin_over_its_domain(idhmc, oracle, tmp_path, lo, hi):
    """v = ln Gamma(x), s = -x psi(x), x = exp(a0) (y = 1; one column of zeros in X, so z = 0): 256 chains whose a0 runs over
    [-690, 690] (x from 1e-300 to 1e299), and over [-3, 4] (x from 0.05 to 55: both sides of the w = 8 switch and every shift count).
    lq and grad after evaluation (per wavefront) and after one NUTS transition (matrix cores, L = 128) have the oracle's bits."""
    family, C, D = "TEST_LGAMMA_PSI", 256, 2
    X, Y = np.zeros((1, 1)), np.ones(1)
    eng = idhmc.Engine(make(idhmc, family, X, Y), C, idhmc.default_options(max_depth=3), seed=4)
    om = oracle.OracleModel.custom(D, c_source_disp(family), AUX.oracle_params_aux(X, Y, 1), str(tmp_path))
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=3), seed=4, chain_id=c) for c in range(C)]
    assert eng.glm_form() == 1 and eng.padded_dim() == 128
    q = np.stack([np.random.default_rng(2).uniform(-1.0, 1.0, C), np.linspace(lo, hi, C)], 1)
    start(eng, chains, q)
    check_bits(eng, chains, D)
    x = np.exp(q[:, 1])
    shifts = np.where(x < 8.0, np.ceil(8.0 - x), 0.0)
    assert np.isfinite(eng.lq).all() and np.isfinite(eng.grad).all()
    if hi < 10.0:
        assert set(shifts.astype(int)) == set(range(9))
    eps = 1e-3
    eng.set_eps(eps)
    eng.nuts_transition(1)
    for ch in chains:
        ch.sample_tree(eps, 1)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    check_bits(eng, chains, D)
    assert np.isfinite(eng.lq).all()
    eng.close()


@pytest.mark.parametrize("family", SHIPPED)
@pytest.mark.parametrize("Dx", [25, 127, 200, 300])
@pytest.mark.parametrize("n", [37, 130])
def test_density_both_forms(idhmc, oracle, tmp_path, family, Dx, n):
    """lq and grad l from the per-wave form (evaluation) and, after one NUTS transition, from the form the NUTS kernel ran: the
    matrix cores at Dx = 25, 127 (L = 128; at 127 the log dispersion is index 127, the last lane's second residue) and 200
    (L = 256), the per-wave form at 300 (L = 512).  n = 130: two observation blocks, the second almost all padding; 18 chains
    are ragged against the 16-chain tile.  Bit-identical to the oracle, and within 1e-12 of numpy + scipy on the first and last chain."""
    C, D = 18, Dx + 1
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, family, n, Dx, C, seed=3, opt=idhmc.default_options(max_depth=4),
                                       oopt=oracle.default_options(max_depth=4))
    assert eng.glm_form() == (1 if Dx <= 200 else 0) and eng.padded_dim() == (128 if Dx <= 127 else 256 if Dx <= 200 else 512)
    start(eng, chains, start_disp(family, C, Dx))
    check_density(eng, chains, family, X, Y, mu, tau, D, (0, C - 1))
    eng.set_eps(0.02)
    eng.nuts_transition(1)
    for ch in chains:
        ch.sample_tree(0.02, 1)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    check_density(eng, chains, family, X, Y, mu, tau, D, (0, C - 1))
    eng.close()


def test_negative_binomial_leapfrog_and_stepsize_search(idhmc, oracle, tmp_path):
    Dx, n, C = 25, 130, 37
    D = Dx + 1
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, NB, n, Dx, C, seed=21)
    start(eng, chains, start_disp(NB, C, Dx))
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
def test_negative_binomial_nuts_transitions(idhmc, oracle, tmp_path, shared):
    """single-transition launches, then a fused launch of three (idhmc_nuts_transitions): a ragged last group of 16 (37 chains),
    per-chain and shared unit metric; then a small eps whose trees stop at max_depth"""
    Dx, n, C, depth, T = 25, 130, 37, 4, 3
    D = Dx + 1
    opt = idhmc.default_options(max_depth=depth, metric_mode=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, NB, n, Dx, C, seed=5, opt=opt, oopt=oracle.default_options(max_depth=depth))
    assert eng.glm_form() == 1
    start(eng, chains, start_disp(NB, C, Dx))
    it = 0
    for eps in (0.03, 0.0005):
        eng.set_eps(eps)
        reached = 0
        for _ in range(2):
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
            ost = [ch.sample_tree(eps, it + 1 + k) for ch in chains]
        it += T
        st = eng.tree_stats()
        np.testing.assert_array_equal(st["depth"], [s.depth for s in ost])
        np.testing.assert_array_equal(st["steps"], [s.steps for s in ost])
        assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        check_bits(eng, chains, D)
        if eps < 0.001:
            assert reached >= C                           # trees that ran to max_depth
    eng.close()


def test_negative_binomial_short_warmup_matches_oracle(idhmc, oracle, tmp_path):
    Dx, n, C, N = 25, 130, 5, 8
    D = Dx + 1
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    X, Y = problem_disp(NB, n, Dx, seed=9)
    eng = idhmc.Engine(make(idhmc, NB, X, Y), C, idhmc.default_options(**short), seed=77)
    draws, stats = eng.mcmc_with_warmup(N)
    om = oracle.OracleModel.custom(D, c_source_disp(NB), AUX.oracle_params_aux(X, Y, 1), str(tmp_path))
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, C, oracle.default_options(**short), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps)
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats.T, ost[:, :N])
    eng.close()


def test_negative_binomial_with_groups(idhmc, oracle, tmp_path):
    """H = 1: a random-intercept block of 8 one-hot columns beside 4 ungrouped ones, n = 130, q = [u | log phi | omega]; the twin
    goes through test_glm_hier_cpu.C_BODY_HIER.  Bit-identical after evaluation and after each of two transitions."""
    Dx, n, C = 12, 130, 18
    D = Dx + 2
    grp = HIER.blocks(Dx, 1, 8)
    X, Y, mu, tau = problem_grouped(n, Dx, grp)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(make(idhmc, NB, X, Y, mu, tau, groups=grp), C, opt, seed=11)
    om = oracle.OracleModel.custom(D, c_source_disp_hier(NB), HIER.oracle_params_hier(X, Y, 1, grp, None, mu, tau), str(tmp_path))
    chains = [oracle.OracleChain(om, oopt, seed=11, chain_id=c) for c in range(C)]
    assert eng.glm_form() == 1 and eng.padded_dim() == 128 and eng.D == D
    start(eng, chains, start_grouped(C, Dx))
    check_density(eng, chains, NB, X, Y, mu, tau, D, (0, C - 1), grp)
    eng.set_eps(0.02)
    for it in (1, 2):
        eng.nuts_transition(it)
        st = eng.tree_stats()
        ost = [ch.sample_tree(0.02, it) for ch in chains]
        np.testing.assert_array_equal(st["depth"], [s.depth for s in ost])
        np.testing.assert_array_equal(st["steps"], [s.steps for s in ost])
        assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        check_density(eng, chains, NB, X, Y, mu, tau, D, (0, C - 1), grp)
    eng.close()


def test_a_degenerate_dispersion_is_a_rejected_start(idhmc, oracle, tmp_path):
    """one chain of 37 with a0 = -800 (phi = dexp(-800) = 0, ln Gamma(0) = +inf): lq = -inf in the per-wave form (evaluation) and after
    NUTS transitions on the matrix cores, exactly as the oracle has it; the other chains of its workgroup keep their oracle bits"""
    Dx, n, C, bad = 25, 130, 37, 20
    D = Dx + 1
    X, Y, mu, tau, eng, chains = setup(idhmc, oracle, tmp_path, NB, n, Dx, C, seed=6, opt=idhmc.default_options(max_depth=4),
                                       oopt=oracle.default_options(max_depth=4))
    assert eng.glm_form() == 1
    q = start_disp(NB, C, Dx)
    q[bad, Dx] = -800.0
    start(eng, chains, q)
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


def test_negative_binomial_local_optimum_is_the_map(idhmc):
    """find_local_optimum maximises l(q) - penalty / 2 |q|^2; a scipy minimisation of the numpy closed form of the same objective
    (n = 500, Dx = 5, true phi = 3) gives the MAP in (beta, log phi): agreement within 1e-6 in every coordinate"""
    Dx, n, C, pen = 5, 500, 6, 1e-4
    D = Dx + 1
    X, Y = problem_disp(NB, n, Dx, seed=2)
    mu, tau = np.full(D, 0.1), np.full(D, 0.5)

    def objective(q):
        l, g = numpy_density_disp(NB, X, Y, q, mu, tau)[:2]
        return -(l - 0.5 * pen * q @ q), -(g - pen * q)
    q0 = np.r_[np.zeros(Dx), TRUE_A[NB]]
    res = optimize.minimize(objective, q0, jac=True, method="BFGS", options=dict(gtol=1e-9, maxiter=500))
    res = optimize.minimize(objective, res.x, jac=True, method="BFGS", options=dict(gtol=1e-11, maxiter=500))
    assert np.abs(objective(res.x)[1]).max() < 1e-7 and abs(res.x[Dx] - np.log(3.0)) < 0.5
    eng = idhmc.Engine(make(idhmc, NB, X, Y, mu, tau), C, seed=4)
    start0 = np.random.default_rng(1).uniform(-0.2, 0.2, (C, D))
    start0[:, Dx] += TRUE_A[NB]
    eng.set_q(start0)
    eng.find_local_optimum(pen, 200)
    np.testing.assert_allclose(eng.q, np.broadcast_to(res.x, (C, D)), rtol=0, atol=1e-6)
    eng.close()


def test_gamma_threaded_mcmc_shapes(idhmc):
    """threaded_mcmc on a gamma regression built with gamma_response: the shapes, every draw finite, and the pooled mean of the log
    shape within 0.5 of the truth (n = 400: its posterior standard deviation is about 0.07)"""
    Dx, n, C, N = 4, 400, 4, 60
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, Dx)) * 0.5
    X[:, 0] = 1.0
    y = np.exp(response("GAMMA_LOG_LOGSHAPE", X @ np.array([0.5, -0.3, 0.2, 0.4]), rng))
    stages = idhmc.default_warmup_stages(middle_steps=20, doubling_stages=2, init_steps=30, terminating_steps=20)
    model = idhmc.GLM(X, idhmc.glm.gamma_response(y), idhmc.glm.GAMMA_LOG_LOGSHAPE, aux=1)
    chains, stats = idhmc.threaded_mcmc(model, N, nchains=C, warmup_stages=stages, seed=3)
    assert len(chains) == C and all(ch.shape == (N, Dx + 1) for ch in chains) and stats.shape == (C, N)
    draws = np.concatenate(chains)
    assert np.isfinite(draws).all() and abs(draws[:, Dx].mean() - TRUE_A["GAMMA_LOG_LOGSHAPE"]) < 0.5
