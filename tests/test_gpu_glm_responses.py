"""GLMs with several responses on one design matrix (GLM(..., chains_per_response=R), idhmc_create_glm_responses)
on the device.  The reference is code the feature does not touch: the CPU oracle running the C restatements of
tests/test_glm_cpu.py and its siblings, one oracle model per response and OracleChain(chain_id = the GLOBAL chain id), or a
single-response context of the existing entry points.  For one chain the arithmetic is the one of a single-response model on its Y
and every random number is addressed by the global chain id, so every comparison is of bits; numpy's closed form is compared at
the 1e-12 x scale of tests/test_gpu_glm.py.  Every context compiles its source with hipRTC: at most four per test."""
import ctypes as C

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
import test_glm_cpu as FLAT
import test_glm_dispersion_cpu as DISP
import test_glm_hier_cpu as HIER
from test_glm_responses_cpu import responses
from test_gpu_glm import prior, same_bits, start

pytestmark = pytest.mark.gpu

NB = "NEG_BINOMIAL_LOG_LOGPHI"
GAUSS = "GAUSSIAN_IDENTITY_LOGSIGMA"


def oracle_models(oracle, D, c_src, params, workdir):
    """one oracle model per response: the restatement is compiled once, each model points it at its own params"""
    first = oracle.OracleModel.custom(D, c_src, params[0], str(workdir))
    out = [first]
    for p in params[1:]:
        m = oracle.OracleModel(3, D)
        m._userlib = first._userlib
        m.params = np.ascontiguousarray(p, dtype=np.float64)
        m.c.fn = first.c.fn
        m.c.params = m.params.ctypes.data_as(C.POINTER(C.c_double))
        out.append(m)
    return out


def oracle_chains(oracle, models, R, ids, oopt, seed):
    """the oracle's chain of every global id in ids, on the model of its response"""
    return [oracle.OracleChain(models[g // R], oopt, seed=seed, chain_id=g) for g in ids]


def flat_setup(idhmc, oracle, tmp_path, family, M, R, n, D, seed, depth, metric=None):
    X, Y = responses(family, M, n, D, seed=n + D)
    mu, tau = prior(D)
    kw = dict(max_depth=depth)
    if metric is not None:
        kw["metric_mode"] = metric
    eng = idhmc.Engine(idhmc.GLM(X, Y, getattr(idhmc.glm, family), None, mu, tau, chains_per_response=R), M * R, idhmc.default_options(**kw), seed=seed)
    models = oracle_models(oracle, D, FLAT.c_source(family), [FLAT.oracle_params(X, Y[m], None, mu, tau) for m in range(M)], tmp_path)
    chains = oracle_chains(oracle, models, R, range(M * R), oracle.default_options(max_depth=depth), seed)
    return X, Y, mu, tau, eng, chains


def check_state(eng, chains, D, what=("q", "lq", "grad")):
    if "q" in what:
        assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    if "p" in what:
        assert same_bits(eng.p, np.stack([c.p[:D] for c in chains]))
    assert same_bits(eng.lq, [c.lq for c in chains]) and same_bits(eng.grad, np.stack([c.grad[:D] for c in chains]))


def check_stats(st, ost):
    for f in ("depth", "steps", "term_left", "term_right"):
        np.testing.assert_array_equal(st[f], [getattr(s, f) for s in ost], err_msg=f)
    assert same_bits(st["pi"], [s.pi for s in ost]) and same_bits(st["acceptance_rate"], [s.acceptance_rate for s in ost])


# ---- 1. density and one transition, both device forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["POISSON_LOG", "BINOMIAL_LOGIT"])
@pytest.mark.parametrize("D,n", [(25, 1), (25, 37), (25, 300), (200, 300), (300, 300)])
def test_density_and_one_transition(idhmc, oracle, tmp_path, family, D, n):
    """M = 5 responses of R = 7 chains: 35 chains are three workgroups of the matrix-core kernel, whose 16-chain tiles mix up to
    three responses and end in a partial one.  L = 128 and 256 on the matrix cores with one and three observation blocks, L = 512 one
    chain per wavefront.  lq and grad after set_q are the per-wave form's, after the transition the NUTS kernel's."""
    M, R = 5, 7
    C_ = M * R
    X, Y, mu, tau, eng, chains = flat_setup(idhmc, oracle, tmp_path, family, M, R, n, D, seed=3, depth=5)
    assert eng.glm_form() == (1 if D <= 256 else 0) and eng.padded_dim() == (128 if D <= 128 else 256 if D <= 256 else 512)
    assert eng.glm_responses() == (M, R)
    # one position for every chain: chains of one response agree, chains of different responses do not (each Y has its own seed)
    q0 = np.random.default_rng(D + 1).uniform(-0.3, 0.3, D) / np.sqrt(D)
    eng.set_q(np.broadcast_to(q0, (C_, D)))
    for ch in chains:
        ch.set_q(q0)
    check_state(eng, chains, D)
    lq = eng.lq.reshape(M, R)
    distinct = len({Y[m].tobytes() for m in range(M)})     # (at n = 1 two seeds may draw the same observation)
    assert distinct >= 3 and Y[0].tobytes() != Y[1].tobytes()
    assert np.all(lq == lq[:, :1]) and len(set(lq[:, 0])) == distinct
    assert lq[0, R - 1] != lq[1, 0] and not same_bits(eng.grad[R - 1], eng.grad[R])

    def closed_form():
        q, g, lq = eng.q, eng.grad, eng.lq
        for c in (0, R, C_ - 1):
            l_ref, g_ref, lscale, gscale = FLAT.numpy_density(family, X, Y[c // R], q[c], mu, tau)
            assert abs(lq[c] - l_ref) <= 1e-12 * lscale
            assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)
    start(eng, chains, D)
    check_state(eng, chains, D)
    closed_form()
    eng.set_eps(0.02)
    eng.nuts_transition(1)
    check_stats(eng.tree_stats(), [ch.sample_tree(0.02, 1) for ch in chains])
    check_state(eng, chains, D)
    closed_form()
    assert eng.poll_abort() == 0
    eng.close()


# ---- 2. several transitions per launch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_several_transitions_per_launch(idhmc, oracle, tmp_path, shared):
    """nuts_transitions(2, 3): the queue hands out (transition, chain) pairs, so a wavefront -- a row of the tile -- changes chain and
    response inside the launch"""
    M, R, D, n = 5, 7, 25, 300
    X, Y, mu, tau, eng, chains = flat_setup(idhmc, oracle, tmp_path, "BINOMIAL_LOGIT", M, R, n, D, seed=5, depth=5,
                                            metric=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    assert eng.glm_form() == 1
    start(eng, chains, D)
    eng.set_eps(0.03)
    eng.nuts_transitions(2, 3)
    ost = None
    for it in (2, 3, 4):
        ost = [ch.sample_tree(0.03, it) for ch in chains]
    check_state(eng, chains, D)
    check_stats(eng.tree_stats(), ost)
    assert eng.poll_abort() == 0
    eng.close()


# ---- 3. with auxiliary coordinates, with groups ----------------------------------------------------------------------------------------
def aux_case(idhmc, n):
    """GAUSSIAN_IDENTITY_LOGSIGMA, A = 1, Dx = 20"""
    Dx, M = 20, 3
    X = AUX.problem_aux(GAUSS, n, Dx, seed=7)[0]
    Y = np.empty((M, n, 1))
    for m in range(M):
        rng = np.random.default_rng(70 + m)
        Y[m, :, 0] = X @ (rng.standard_normal(Dx) / np.sqrt(Dx)) + 0.7 * rng.standard_normal(n)
    D = Dx + 1
    mu, tau = prior(D)
    model = idhmc.GLM(X, Y, idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, None, mu, tau, aux=1, chains_per_response=6)
    params = [AUX.oracle_params_aux(X, Y[m], 1, None, mu, tau) for m in range(M)]
    return model, D, AUX.c_source_aux(GAUSS), params, lambda C_: AUX.start_aux(GAUSS, C_, Dx)


def hier_case(idhmc, n):
    """NEG_BINOMIAL_LOG_LOGPHI with H = 2 groups, A = 1, Dx = 24: D = 27"""
    Dx, M = 24, 3
    grp = HIER.blocks(Dx, 2, 8)
    rng = np.random.default_rng(9)
    X = HIER.design(n, Dx, grp, True, rng)
    Y = np.empty((M, n, 1))
    for m in range(M):
        rng = np.random.default_rng(90 + m)
        beta = np.where(grp >= 0, 0.6 * rng.standard_normal(Dx), rng.standard_normal(Dx) / np.sqrt(Dx))
        Y[m, :, 0] = DISP.response(NB, X @ beta, rng)
    D = Dx + 3
    mu, tau = prior(D)
    model = idhmc.GLM(X, Y, idhmc.glm.NEG_BINOMIAL_LOG_LOGPHI, None, mu, tau, aux=1, groups=grp, chains_per_response=6)
    params = [HIER.oracle_params_hier(X, Y[m], 1, grp, None, mu, tau) for m in range(M)]

    def q0(C_):
        r = np.random.default_rng(Dx)
        return np.concatenate([r.uniform(-0.3, 0.3, (C_, Dx)), DISP.TRUE_A[NB] + r.uniform(-0.2, 0.2, (C_, 1)),
                               HIER.OMEGA0 + r.uniform(-0.3, 0.3, (C_, 2))], 1)
    return model, D, DISP.c_source_disp_hier(NB), params, q0


@pytest.mark.parametrize("case", ["aux", "hier"])
def test_with_auxiliary_coordinates_and_groups(idhmc, oracle, tmp_path, case):
    """M = 3, R = 6 at n = 130 (two observation blocks): density, leapfrog(eps, 3), find_initial_stepsize, find_local_optimum and a
    transition, each against the oracle as the single-response tests of these models have it"""
    M, R, n, seed = 3, 6, 130, 21
    C_ = M * R
    model, D, c_src, params, q0 = (aux_case if case == "aux" else hier_case)(idhmc, n)
    assert (model.M, model.R, model.D) == (M, R, D)
    eng = idhmc.Engine(model, C_, idhmc.default_options(max_depth=4), seed=seed)
    assert eng.glm_form() == 1 and eng.glm_responses() == (M, R)
    models = oracle_models(oracle, D, c_src, params, tmp_path)
    chains = oracle_chains(oracle, models, R, range(C_), oracle.default_options(max_depth=4), seed)
    q = q0(C_)

    def restart():
        eng.set_q(q)
        for c, ch in enumerate(chains):
            ch.set_q(q[c])
    restart()
    check_state(eng, chains, D)
    assert len(set(eng.lq)) == C_
    eng.refresh_momentum(1)
    eng.leapfrog(0.01, 3)
    for ch in chains:
        ch.rand_p(1)
        for _ in range(3):
            ch.leapfrog(0.01)
    check_state(eng, chains, D, ("q", "p", "lq", "grad"))
    assert same_bits(eng.logdensity(), [c.logdensity() for c in chains])
    eng.refresh_momentum(0)
    eng.find_initial_stepsize()
    ref = []
    for ch in chains:
        ch.rand_p(0)
        rc, e = ch.find_initial_stepsize()
        assert rc == 0
        ref.append(e)
    assert same_bits(eng.eps, ref)
    restart()
    eng.find_local_optimum(1e-4, 30)
    for ch in chains:
        assert ch.find_local_optimum(1e-4, 30) == 0
    check_state(eng, chains, D)
    restart()
    eng.set_eps(0.02)
    eng.nuts_transition(1)
    check_stats(eng.tree_stats(), [ch.sample_tree(0.02, 1) for ch in chains])
    check_state(eng, chains, D)
    eng.close()


# ---- 4. sharding and M = 1 -----------------------------------------------------------------------------------------------------------
def shard_problem(idhmc):
    M, R, D, n = 3, 6, 25, 140
    X, Y = responses("POISSON_LOG", M, n, D, seed=4)
    mu, tau = prior(D)
    return M, R, X, Y, mu, tau, idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, None, mu, tau, chains_per_response=R)


def shard_run(eng):
    """a random position, then two transitions (from a tenth of it: U(-2, 2) is far out for a count model)"""
    eng.random_position()
    first = (eng.q, eng.lq, eng.grad)
    eng.set_q(first[0] * 0.1)
    eng.set_eps(0.02)
    eng.nuts_transition(1)
    eng.nuts_transition(2)
    out = first + (eng.q, eng.lq, eng.grad, eng.tree_stats())
    eng.close()
    return out


def shard_same(got, want, lo, hi):
    return all(same_bits(g, w[lo:hi]) for g, w in zip(got[:6], want[:6])) and np.array_equal(got[6], want[6][lo:hi])


def test_a_shard_is_a_slice_of_the_full_context(idhmc):
    """the response of a chain is a function of its global id: a context of chains 5..13 (the end of response 0, response 1, the
    beginning of response 2) holds the bits of chains 5..13 of the full context"""
    M, R, X, Y, mu, tau, model = shard_problem(idhmc)
    opt = idhmc.default_options(max_depth=5)
    want = shard_run(idhmc.Engine(model, M * R, opt, seed=13))
    part = idhmc.Engine(model, 9, opt, seed=13, first_chain=5)
    assert part.glm_responses() == (M, R)
    assert shard_same(shard_run(part), want, 5, 14)


def test_single_response_contexts_are_the_blocks_of_the_full_one(idhmc):
    """three single-response Engines of the existing entry point (Y[m], first_chain = 6 m, 6 chains) against the full context"""
    M, R, X, Y, mu, tau, model = shard_problem(idhmc)
    opt = idhmc.default_options(max_depth=5)
    want = shard_run(idhmc.Engine(model, M * R, opt, seed=13))
    for m in range(M):
        one = idhmc.Engine(idhmc.GLM(X, Y[m], idhmc.glm.POISSON_LOG, None, mu, tau), R, opt, seed=13, first_chain=R * m)
        assert one.glm_responses() == (1, 0)
        assert shard_same(shard_run(one), want, R * m, R * m + R)


def test_one_response_is_the_plain_context(idhmc):
    """chains_per_response = C with M = 1 against the plain GLM: the same form, bytes and bits"""
    D, n, C_, seed = 25, 140, 20, 13
    X, Y = responses("BINOMIAL_LOGIT", 1, n, D, seed=4)
    mu, tau = prior(D)
    opt = idhmc.default_options(max_depth=5)
    a = idhmc.Engine(idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, None, mu, tau, chains_per_response=C_), C_, opt, seed=seed)
    b = idhmc.Engine(idhmc.GLM(X, Y[0], idhmc.glm.BINOMIAL_LOGIT, None, mu, tau), C_, opt, seed=seed)
    assert a.glm_responses() == (1, C_) and b.glm_responses() == (1, 0)
    assert a.glm_form() == b.glm_form() == 1 and a.device_bytes() == b.device_bytes()

    def same():
        return same_bits(a.q, b.q) and same_bits(a.lq, b.lq) and same_bits(a.grad, b.grad)
    q = np.random.default_rng(2).uniform(-0.2, 0.2, (C_, D))
    for e in (a, b):
        e.set_q(q)
        e.set_eps(0.03)
    assert same()
    for e in (a, b):
        e.nuts_transitions(1, 3)
    assert same() and np.array_equal(a.tree_stats(), b.tree_stats())
    a.close()
    b.close()


# ---- 5. the drivers ------------------------------------------------------------------------------------------------------------------
def test_warmup_and_draws_per_response(idhmc, oracle, tmp_path):
    """mcmc_with_warmup with a shortened warm-up, per-chain stepsize and metric: the draws of one chain of each response are the
    oracle's; R-hat per response; the pooled statistics are refused when the context is made"""
    family, D, n, M, R, N, seed = "BERNOULLI_LOGIT", 10, 60, 4, 8, 12, 77
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    X, Y = responses(family, M, n, D, seed=9)
    model = idhmc.GLM(X, Y, idhmc.glm.BERNOULLI_LOGIT, chains_per_response=R)
    eng = idhmc.Engine(model, M * R, idhmc.default_options(**short), seed=seed)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == 1
    draws, stats = eng.mcmc_with_warmup(N)
    assert draws.shape == (N, M * R, D) and np.isfinite(draws).all()
    eps = eng.eps
    models = oracle_models(oracle, D, FLAT.c_source(family), [FLAT.oracle_params(X, Y[m]) for m in range(M)], tmp_path)
    for m in range(M):
        g = R * m + (3 * m + 1) % R                         # a different place in each response's block
        rc, och, ost, oeps = oracle.threaded_mcmc(models[m], N, 1, oracle.default_options(**short), seed=seed, first_chain=g, nthreads=1)
        assert rc == 0 and same_bits(eps[g:g + 1], oeps)
        assert same_bits(draws[:, g], och[0, :N, :D]) and np.array_equal(stats[:, g], ost[0, :N])
    r = idhmc.rhat_by_response(model, draws.mean(0), draws.var(0, ddof=1), N)
    assert r.shape == (4, 10) and np.isfinite(r).all()
    assert idhmc.glm.by_response(model, draws).shape == (M, N, R, D)
    eng.close()
    for kw, word in ((dict(eps_mode=idhmc.EPS_GLOBAL), "GLOBAL"), (dict(metric_mode=idhmc.METRIC_POOLED), "POOLED")):
        with pytest.raises(idhmc.IdhmcError) as e:
            idhmc.Engine(model, M * R, idhmc.default_options(**kw), seed=seed)
        assert e.value.code == idhmc.ERR_BAD_ARG and word in str(e.value) and "different posteriors" in str(e.value)
