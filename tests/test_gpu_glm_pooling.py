"""Per-response stepsize and metric of a GLM with several responses (EPS_PER_RESPONSE, METRIC_PER_RESPONSE) on the
device.  The reference is code the feature leaves alone: for every response m a single-response context of the existing entry points
on the same chains -- GLM(X, Y[m]) with first_chain = m R and R chains, EPS_GLOBAL in place of EPS_PER_RESPONSE, METRIC_POOLED in
place of METRIC_PER_RESPONSE -- whose bits the new modes must hold through every public step; besides it the CPU oracle's global
stepsize stage on the response's chains, and numpy's pooled variance on the stored draws (the formula and the 1e-10 of
tests/test_gpu_warmup.py::test_pooled_metric).  Every other comparison is of bits.  The data helpers are those of
tests/test_gpu_glm_responses.py, copied."""
import ctypes as C

import numpy as np
import pytest

import test_glm_cpu as FLAT
import test_glm_dispersion_cpu as DISP
import test_glm_hier_cpu as HIER
from test_glm_responses_cpu import responses
from test_gpu_glm import prior, same_bits

pytestmark = pytest.mark.gpu

NB = "NEG_BINOMIAL_LOG_LOGPHI"


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


class Problem:
    """M responses on one design matrix: the model of all of them, and the single-response model of each"""

    def __init__(self, idhmc, family, M, R, D, n, seed=None):
        self.M, self.R, self.D, self.family = M, R, D, family
        self.X, self.Y = responses(family, M, n, D, seed=n + D if seed is None else seed)
        self.mu, self.tau = prior(D)
        src = getattr(idhmc.glm, family)
        self.full = idhmc.GLM(self.X, self.Y, src, None, self.mu, self.tau, chains_per_response=R)
        self.one = lambda m: idhmc.GLM(self.X, self.Y[m], src, None, self.mu, self.tau)


def options(idhmc, eps, metric, **kw):
    return idhmc.default_options(eps_mode=getattr(idhmc, "EPS_" + eps), metric_mode=getattr(idhmc, "METRIC_" + metric), **kw)


def near_start(eng):
    """a random position, then a tenth of it (U(-2, 2) is far out for a count model)"""
    eng.random_position()
    eng.set_q(0.1 * eng.q)


def searched_stage(N, adapt_metric):
    """random_position, set_q(0.1 q), refresh_momentum(0), find_initial_stepsize, tuning_stage(N, adapt_metric, 0, store_draws=True)"""
    def run(eng, lo=0):
        near_start(eng)
        q0 = eng.q
        eng.refresh_momentum(0)
        eng.find_initial_stepsize()
        eps0 = eng.eps
        draws, stats = eng.tuning_stage(N, adapt_metric, 0, store_draws=True)
        return dict(q0=q0, eps0=eps0, draws=draws, stats=stats, eps=eng.eps, minv=eng.minv, q=eng.q)
    return run


def fixed_stage(N, adapt_metric, eps=0.02):
    """random_position, set_q(0.1 q), set_eps(eps), tuning_stage(N, adapt_metric, 0, store_draws=True)"""
    def run(eng, lo=0):
        near_start(eng)
        eng.set_eps(eps)
        draws, stats = eng.tuning_stage(N, adapt_metric, 0, store_draws=True)
        return dict(draws=draws, stats=stats, eps=eng.eps, minv=eng.minv, q=eng.q)
    return run


def same_slice(got, want, lo, hi):
    """`got` (a context of chains lo .. hi - 1) holds the bits of those chains of `want`"""
    for k, g in got.items():
        w = want[k]
        w = w[:, lo:hi] if k in ("draws", "stats") else w[lo:hi]
        if k == "stats":
            assert np.array_equal(g, w), k
        else:
            assert same_bits(g, w), k


def against_single_responses(idhmc, pb, model, run, new, ref, seed, which=None, **opt):
    """the full context in the `new` modes against one single-response context per response in the `ref` modes (run(engine, lo): the
    sequence under test on a context whose first chain is lo); returns the full one's"""
    M, R = pb.M, pb.R
    eng = idhmc.Engine(model, M * R, options(idhmc, *new, **opt), seed=seed)
    assert eng.glm_responses() == (M, R)
    want = run(eng, 0)
    eng.close()
    for m in (range(M) if which is None else which):
        one = idhmc.Engine(pb.one(m), R, options(idhmc, *ref, **opt), seed=seed, first_chain=R * m)
        assert one.glm_responses() == (1, 0)
        same_slice(run(one, R * m), want, R * m, R * m + R)
        one.close()
    return want


def by_response(a, M, R):
    return a.reshape((M, R) + a.shape[1:])


def equal_inside_distinct_between(a, M, R):
    a = by_response(a, M, R)
    return np.array_equal(a, np.broadcast_to(a[:, :1], a.shape)) and len({a[m, 0].tobytes() for m in range(M)}) == M


# ---- 1. the stepsize alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n", [(25, 37), (300, 300)])
def test_stepsize_per_response(idhmc, oracle, tmp_path, D, n):
    """M = 5 responses of R = 7 chains: 35 chains are three workgroups of the matrix-core kernel whose tiles mix responses (D = 25), one
    chain per wavefront at D = 300.  After the search every chain of a response holds exp(mean log eps) of its searches, after the
    stage exp(logeps_bar) of the response's dual averaging: the bits of the five EPS_GLOBAL contexts, and of the oracle's
    global_eps_stage on the response's chains, which shares no code with the device."""
    M, R, depth, seed = 5, 7, 5, 3
    pb = Problem(idhmc, "POISSON_LOG", M, R, D, n)
    got = against_single_responses(idhmc, pb, pb.full, searched_stage(6, False), ("PER_RESPONSE", "PER_CHAIN"), ("GLOBAL", "PER_CHAIN"),
                                   seed, max_depth=depth)
    assert equal_inside_distinct_between(got["eps0"], M, R) and equal_inside_distinct_between(got["eps"], M, R)
    assert np.array_equal(got["minv"], np.ones((M * R, D)))
    models = oracle_models(oracle, D, FLAT.c_source("POISSON_LOG"),
                           [FLAT.oracle_params(pb.X, pb.Y[m], None, pb.mu, pb.tau) for m in range(M)], tmp_path)
    oopt = oracle.default_options(max_depth=depth)
    for m in range(M):
        chains = [oracle.OracleChain(models[m], oopt, seed=seed, chain_id=g) for g in range(R * m, R * m + R)]
        for g, ch in zip(range(R * m, R * m + R), chains):
            ch.set_q(got["q0"][g])
            ch.rand_p(0)
        eps0 = oracle.global_initial_eps(chains)
        assert same_bits(got["eps0"][R * m], eps0)
        used, final = oracle.global_eps_stage(chains, 6, 0, eps0, oopt)
        assert same_bits(got["eps"][R * m], final)
        assert same_bits(got["q"][R * m:R * m + R], np.stack([ch.q[:D] for ch in chains]))


# ---- 2. the metric ----------------------------------------------------------------------------------------------------------------------
def test_metric_per_response(idhmc):
    """both new modes, one adapting stage with a metric window: the rows of M^-1 agree inside a response and differ between them, are
    the bits of the single-response POOLED + GLOBAL contexts, and numpy's pooled variance of the response's stored draws with the
    reference's regularisation at the pooled count (src/hamiltonian.jl:156-158) to 1e-10"""
    M, R, D, n, N = 5, 7, 25, 37, 8
    pb = Problem(idhmc, "POISSON_LOG", M, R, D, n)
    got = against_single_responses(idhmc, pb, pb.full, fixed_stage(N, True), ("PER_RESPONSE", "PER_RESPONSE"), ("GLOBAL", "POOLED"),
                                   3, max_depth=5)
    assert equal_inside_distinct_between(got["minv"], M, R) and equal_inside_distinct_between(got["eps"], M, R)
    for m in range(M):
        x = got["draws"][:, R * m:R * m + R].reshape(N * R, D)
        Nt, lam = float(N * R), 5.0 / N
        S = ((x - x.mean(axis=0)) ** 2).sum(axis=0)
        ref = S * Nt / ((Nt + lam) * (Nt - 1.0)) + 1e-3 * lam / (Nt + lam)
        assert np.allclose(got["minv"][R * m], ref, rtol=1e-10, atol=0)


# ---- 3. the segment rule, more chains than lanes, one chain ---------------------------------------------------------------------------------
def test_a_response_that_straddles_a_segment(idhmc):
    """R = 400: a response is reduced by one wavefront in seven strides, and response 2 (ids 800 .. 1199) straddles id 1024, the end
    of a segment of the pooled sums: two partials, added in segment order, as the single-response context at first_chain = 800 forms
    them"""
    pb = Problem(idhmc, "BERNOULLI_LOGIT", 3, 400, 10, 20)
    assert 2 * 400 < idhmc.POOL_SEGMENT < 3 * 400
    got = against_single_responses(idhmc, pb, pb.full, searched_stage(4, True), ("PER_RESPONSE", "PER_RESPONSE"), ("GLOBAL", "POOLED"),
                                   5, which=(0, 2), max_depth=4)
    assert equal_inside_distinct_between(got["minv"], 3, 400) and equal_inside_distinct_between(got["eps"], 3, 400)


def test_one_chain_per_response(idhmc):
    """R = 1, M = 6: every chain is its own response, against six contexts of one chain"""
    pb = Problem(idhmc, "BERNOULLI_LOGIT", 6, 1, 10, 20)
    got = against_single_responses(idhmc, pb, pb.full, searched_stage(4, True), ("PER_RESPONSE", "PER_RESPONSE"), ("GLOBAL", "POOLED"),
                                   5, max_depth=4)
    assert len(set(got["eps"])) == 6 and len({row.tobytes() for row in got["minv"]}) == 6


# ---- 4. each new mode next to an existing one ------------------------------------------------------------------------------------------
def mixed_problem(idhmc):
    return Problem(idhmc, "POISSON_LOG", 3, 6, 25, 140, seed=4)


def test_stepsize_per_response_with_a_shared_metric(idhmc):
    """(EPS_PER_RESPONSE, METRIC_SHARED) against (EPS_GLOBAL, METRIC_SHARED)"""
    pb = mixed_problem(idhmc)
    got = against_single_responses(idhmc, pb, pb.full, searched_stage(6, False), ("PER_RESPONSE", "SHARED"), ("GLOBAL", "SHARED"),
                                   13, max_depth=5)
    assert equal_inside_distinct_between(got["eps"], pb.M, pb.R)


def test_metric_per_response_with_a_stepsize_per_chain(idhmc):
    """(EPS_PER_CHAIN, METRIC_PER_RESPONSE) against (EPS_PER_CHAIN, METRIC_POOLED)"""
    pb = mixed_problem(idhmc)
    got = against_single_responses(idhmc, pb, pb.full, searched_stage(6, True), ("PER_CHAIN", "PER_RESPONSE"), ("PER_CHAIN", "POOLED"),
                                   13, max_depth=5)
    assert equal_inside_distinct_between(got["minv"], pb.M, pb.R) and len(set(got["eps"])) == pb.M * pb.R


def test_the_stage_stays_fused_and_the_entry_points_that_refuse(idhmc, monkeypatch):
    """With a stepsize per chain the stepsize adapts inside the transition kernel and the per-response metric is formed once at the
    stage's end, so the stage keeps its launches of several transitions: the drivers fuse on this context (fused_launch_info), and the
    result is the one of a context that may not (IDHMC_FUSE=0).  The per-response stepsize adapts between transitions: the flag that
    adapts inside one is refused by both entry points, and the context-wide entry points keep refusing with the messages they have."""
    import torch
    pb = mixed_problem(idhmc)
    C_ = pb.M * pb.R

    def no_records(eng):
        near_start(eng)
        eng.set_eps(0.02)
        eng.tuning_stage(6, True, 0, store_draws=False, store_stats=False)
        return dict(eps=eng.eps, minv=eng.minv, q=eng.q, stats=eng.tree_stats()[None])
    opt = options(idhmc, "PER_CHAIN", "PER_RESPONSE", max_depth=5)
    fused = idhmc.Engine(pb.full, C_, opt, seed=13)
    monkeypatch.setenv("IDHMC_FUSE", "0")
    plain = idhmc.Engine(pb.full, C_, opt, seed=13)
    monkeypatch.delenv("IDHMC_FUSE")
    assert fused.fused_launch_info() == (True, True) and plain.fused_launch_info() == (True, False)
    same_slice(no_records(fused), no_records(plain), 0, C_)
    eng = idhmc.Engine(pb.full, C_, options(idhmc, "PER_RESPONSE", "PER_CHAIN", max_depth=5), seed=13)
    buf = torch.zeros(2 * 129 + 128, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for call, text in ((lambda: eng.nuts_transition(1, idhmc.T_ADAPT_EPS), "the per-response stepsize adapts between transitions"),
                       (lambda: eng.nuts_transitions(1, 2, idhmc.T_ADAPT_EPS), "the per-response stepsize adapts between transitions"),
                       (lambda: eng.da_adapt_global(buf.data_ptr()), "context is not in global-eps mode"),
                       (lambda: fused.pool_partials(0, buf.data_ptr(), 0, 1), "context is not in pooled-metric mode"),
                       (lambda: fused.pool_consume(0, buf.data_ptr(), 1, 0.5), "context is not in pooled-metric mode")):
        with pytest.raises(idhmc.IdhmcError) as e:
            call()
        assert e.value.code == idhmc.ERR_BAD_ARG and text in str(e.value)
    for e_ in (eng, fused, plain):
        e_.close()


# ---- 5. auxiliary coordinates, groups, dispersion ---------------------------------------------------------------------------------------
class HierCase:
    """NEG_BINOMIAL_LOG_LOGPHI with H = 2 groups, A = 1, Dx = 24 (D = 27) at n = 130, M = 3, R = 6 (the hier_case of
    tests/test_gpu_glm_responses.py): the search and one adapting metric stage"""
    Dx, M, R, n, seed = 24, 3, 6, 130, 21

    def __init__(self, idhmc):
        Dx, M, R, n = self.Dx, self.M, self.R, self.n
        grp = HIER.blocks(Dx, 2, 8)
        rng = np.random.default_rng(9)
        X = HIER.design(n, Dx, grp, True, rng)
        Y = np.empty((M, n, 1))
        for m in range(M):
            rng = np.random.default_rng(90 + m)
            beta = np.where(grp >= 0, 0.6 * rng.standard_normal(Dx), rng.standard_normal(Dx) / np.sqrt(Dx))
            Y[m, :, 0] = DISP.response(NB, X @ beta, rng)
        mu, tau = prior(Dx + 3)
        src = idhmc.glm.NEG_BINOMIAL_LOG_LOGPHI
        self.one = lambda m: idhmc.GLM(X, Y[m], src, None, mu, tau, aux=1, groups=grp)
        self.full = idhmc.GLM(X, Y, src, None, mu, tau, aux=1, groups=grp, chains_per_response=R)
        r = np.random.default_rng(Dx)
        self.q0 = np.concatenate([r.uniform(-0.3, 0.3, (M * R, Dx)), DISP.TRUE_A[NB] + r.uniform(-0.2, 0.2, (M * R, 1)),
                                  HIER.OMEGA0 + r.uniform(-0.3, 0.3, (M * R, 2))], 1)

    def run(self, eng, lo):
        eng.set_q(self.q0[lo:lo + eng.C])
        eng.refresh_momentum(0)
        eng.find_initial_stepsize()
        eps0 = eng.eps
        draws, stats = eng.tuning_stage(8, True, 0, store_draws=True)
        return dict(eps0=eps0, draws=draws, stats=stats, eps=eng.eps, minv=eng.minv)


@pytest.fixture(scope="module")
def hier(idhmc):
    """the case and what the full context in both new modes computes, once for the three comparisons"""
    case = HierCase(idhmc)
    eng = idhmc.Engine(case.full, case.M * case.R, options(idhmc, "PER_RESPONSE", "PER_RESPONSE", max_depth=4), seed=case.seed)
    assert eng.glm_responses() == (case.M, case.R) and eng.glm_form() == 1
    want = case.run(eng, 0)
    eng.close()
    for v in want.values():
        v.setflags(write=False)
    return case, want


@pytest.mark.parametrize("m", [0, 1, 2])
def test_with_auxiliary_coordinates_and_groups(idhmc, hier, m):
    """response m of the full context against its single-response GLOBAL + POOLED context"""
    case, want = hier
    M, R = case.M, case.R
    if m == 0:
        assert equal_inside_distinct_between(want["minv"], M, R) and equal_inside_distinct_between(want["eps"], M, R)
        assert equal_inside_distinct_between(want["eps0"], M, R)
    one = idhmc.Engine(case.one(m), R, options(idhmc, "GLOBAL", "POOLED", max_depth=4), seed=case.seed, first_chain=R * m)
    same_slice(case.run(one, R * m), want, R * m, R * m + R)
    one.close()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
def test_warmup_and_draws(idhmc):
    """mcmc_with_warmup with the shortened schedule of tests/test_gpu_glm_responses.py::test_warmup_and_draws_per_response in both new
    modes: draws, records, final stepsizes and metrics of the four single-response GLOBAL + POOLED contexts.  That identity with a mode
    whose statistics are tested carries their validity over; no threshold of its own."""
    M, R, D, n, N = 4, 8, 10, 60, 12
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    X, Y = responses("BERNOULLI_LOGIT", M, n, D, seed=9)

    class pb:
        pass
    pb.M, pb.R = M, R
    pb.one = lambda m: idhmc.GLM(X, Y[m], idhmc.glm.BERNOULLI_LOGIT)
    full = idhmc.GLM(X, Y, idhmc.glm.BERNOULLI_LOGIT, chains_per_response=R)

    def run(eng, lo):
        draws, stats = eng.mcmc_with_warmup(N)
        return dict(draws=draws, stats=stats, eps=eng.eps, minv=eng.minv)
    got = against_single_responses(idhmc, pb, full, run, ("PER_RESPONSE", "PER_RESPONSE"), ("GLOBAL", "POOLED"), 77, **short)
    assert equal_inside_distinct_between(got["minv"], M, R) and equal_inside_distinct_between(got["eps"], M, R)
    draws = got["draws"]
    assert draws.shape == (N, M * R, D) and np.isfinite(draws).all()
    r = idhmc.rhat_by_response(full, draws.mean(0), draws.var(0, ddof=1), N)
    assert r.shape == (4, 10) and np.isfinite(r).all()


# ---- 7. shards -----------------------------------------------------------------------------------------------------------------------------
def test_shards_of_whole_responses(idhmc):
    """contexts over chains [0, 14) and [14, 35) hold the bits of the full context; a one-rank native communicator changes nothing and
    carries the status agreements only (one after the search, one at the end of the stage)"""
    M, R, D, n, N = 5, 7, 25, 37, 8
    pb = Problem(idhmc, "POISSON_LOG", M, R, D, n)
    opt = options(idhmc, "PER_RESPONSE", "PER_RESPONSE", max_depth=5)

    def run(eng):
        near_start(eng)
        eng.refresh_momentum(0)
        eng.find_initial_stepsize()
        eps0 = eng.eps
        eng.set_eps(0.02)
        draws, stats = eng.tuning_stage(N, True, 0, store_draws=True)
        return dict(eps0=eps0, draws=draws, stats=stats, eps=eng.eps, minv=eng.minv)
    eng = idhmc.Engine(pb.full, M * R, opt, seed=3)
    want = run(eng)
    eng.close()
    for lo, hi, native in ((0, 14, False), (14, 35, True)):
        part = idhmc.Engine(pb.full, hi - lo, opt, seed=3, first_chain=lo)
        if native:
            idhmc.distributed.attach_global_eps_native(part, rank=0, world=1)
            assert part.comm_info() == (1, 0, 0)
        same_slice(run(part), want, lo, hi)
        if native:
            assert part.comm_info() == (1, 0, 2)
            part.comm_destroy()
        part.close()


# ---- 8. one response ----------------------------------------------------------------------------------------------------------------------
def test_one_response_is_the_plain_context_in_the_context_wide_modes(idhmc):
    """M = 1 with chains_per_response = 20 in the new modes against the plain GLM in GLOBAL + POOLED"""
    D, n, C_ = 25, 140, 20
    X, Y = responses("BINOMIAL_LOGIT", 1, n, D, seed=4)
    mu, tau = prior(D)
    src = idhmc.glm.BINOMIAL_LOGIT
    run = searched_stage(8, True)
    a = idhmc.Engine(idhmc.GLM(X, Y, src, None, mu, tau, chains_per_response=C_), C_, options(idhmc, "PER_RESPONSE", "PER_RESPONSE", max_depth=5), seed=13)
    b = idhmc.Engine(idhmc.GLM(X, Y[0], src, None, mu, tau), C_, options(idhmc, "GLOBAL", "POOLED", max_depth=5), seed=13)
    assert a.glm_responses() == (1, C_) and b.glm_responses() == (1, 0)
    same_slice(run(a), run(b), 0, C_)
    a.close()
    b.close()


# ---- 9. underflow ----------------------------------------------------------------------------------------------------------------------------
def test_underflow_of_one_response(idhmc):
    """eps of response 1's chains is 1e-12: the stage raises ERR_EPS_UNDERFLOW as the single-response GLOBAL context with that eps
    does (the dual averaging starts from eps, and a response's eps below 1e-10 is an error of all its chains, as k_eps_from_global
    has it).  After da_init alone the exchange record counts R chains with a pending status: none of responses 0 and 2."""
    import torch
    M, R, D, n = 3, 7, 25, 37
    pb = Problem(idhmc, "POISSON_LOG", M, R, D, n)
    eps = np.repeat([0.02, 1e-12, 0.02], R)
    eng = idhmc.Engine(pb.full, M * R, options(idhmc, "PER_RESPONSE", "PER_CHAIN", max_depth=4), seed=3)
    near_start(eng)
    eng.set_eps(eps)
    eng.da_init()
    buf = torch.zeros(idhmc.XCHG_DOUBLES, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.accept_sum(buf.data_ptr())
    eng.synchronize()
    assert buf.cpu().numpy()[2:].tolist() == [M * R, R]
    after = by_response(eng.eps, M, R)
    assert np.all(after[1] == after[1, 0]) and after[1, 0] < 1e-10 and abs(after[1, 0] / 1e-12 - 1.0) < 1e-12
    with pytest.raises(idhmc.IdhmcError) as e:
        eng.tuning_stage(2, False, 0)
    assert e.value.code == idhmc.ERR_EPS_UNDERFLOW and "warmup" in str(e.value)
    assert eng.poll_abort(0) == 0                 # reported once, then cleared
    # the reference: response 1 alone fails in the same way, and holds the same eps when it does
    eps_full = eng.eps
    eng.close()
    one = idhmc.Engine(pb.one(1), R, options(idhmc, "GLOBAL", "PER_CHAIN", max_depth=4), seed=3, first_chain=R)
    near_start(one)
    one.set_eps(eps[R:2 * R])
    with pytest.raises(idhmc.IdhmcError) as e:
        one.tuning_stage(2, False, 0)
    assert e.value.code == idhmc.ERR_EPS_UNDERFLOW and "warmup" in str(e.value)
    assert same_bits(one.eps, eps_full[R:2 * R])
    one.close()
