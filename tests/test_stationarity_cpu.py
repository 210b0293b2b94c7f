"""Exact stationarity of the CPU oracle's NUTS transition (tests/stationarity.py): every chain starts at an exact draw from the
target, takes transitions with a fixed, per-chain stepsize and a per-chain metric mismatched to the target, and must still be an
exact draw.  The GPU kernels equal the oracle bit for bit, so this is also where the statistics and the stepsizes of
test_gpu_stationarity.py are calibrated; the negative controls prove the statistics have the power to see a wrong sampler."""
import numpy as np
import pytest

import stationarity as S

C = 1 << 13
SEED = 5
NOACC_EPS, NOACC_STEPS = 1.6, 3      # shared with test_gpu_stationarity.py


def run_chains(oracle, om, q0, minv, eps, T, max_depth=10, p0=None, seed=SEED):
    """T transitions of every chain from q0 (and with p0: the first one keeps that momentum instead of drawing one);
    returns the positions after each transition and the tree statistics"""
    n, D = q0.shape
    opt = oracle.default_options(max_depth=max_depth)
    out = np.empty((T, n, D))
    ts = np.empty((T, n), dtype=oracle.STATS_DTYPE)
    for c in range(n):
        ch = oracle.OracleChain(om, opt, seed=seed, chain_id=c)
        ch.set_minv(minv[c])
        ch.set_q(q0[c])
        if p0 is not None:
            ch.set_p(p0[c])
        for t in range(T):
            st = ch.sample_tree(eps[c], t + 1, refresh_p=p0 is None or t > 0)
            out[t, c] = ch.q[:D]
            ts[t, c] = (st.pi, st.acceptance_rate, st.term_left, st.term_right, st.depth, st.steps)
    return out, ts


def test_diagonal_gaussian(oracle):
    """D = 8, per-chain metric sigma^2 U(0.3, 3), per-chain stepsize U(0.2, 0.6) drawn independently of the state"""
    D, T = 8, 3
    rng = np.random.default_rng(1)
    mu, sigma = S.diag_target(D)
    q0 = S.diag_gaussian(rng, C, mu, sigma)
    minv = sigma ** 2 * rng.uniform(0.3, 3.0, (C, D))
    eps = rng.uniform(0.2, 0.6, C)
    qs, ts = run_chains(oracle, oracle.OracleModel.diag(mu, 1.0 / sigma ** 2), q0, minv, eps, T)
    fam = S.Family()
    for t in range(T):
        S.add_gaussian(fam, (qs[t] - mu) / sigma, "transition %d" % (t + 1))
    S.assert_stationary(fam, "oracle, diagonal Gaussian")
    term = S.terminations(ts)
    assert S.moved_fraction(q0, qs[0]) > 0.9
    assert S.mean_corr((q0 - mu) / sigma, (qs[0] - mu) / sigma) < 0.5
    assert term["mean_depth"] >= 2 and term["turning"] > 0.9, term


def test_truncated_normal(oracle, tmp_path):
    """a user density (the oracle's callback model) that is -Inf outside the box |q_i| < 1: trajectories hit the wall and end
    in divergences, which must leave the target as invariant as U-turns do"""
    D, T, a = 6, 2, 2.0
    rng = np.random.default_rng(2)
    om = oracle.OracleModel.custom(D, S.TRUNCNORM_C, [a], str(tmp_path))
    q0 = S.truncnorm_draws(rng, C, D, a)
    minv = rng.uniform(0.3, 3.0, (C, D)) * 0.77           # 0.77 ~ the variance of N(0, 1) truncated to (-2, 2)
    eps = rng.uniform(0.1, 0.3, C)
    qs, ts = run_chains(oracle, om, q0, minv, eps, T)
    fam = S.Family()
    for t in range(T):
        S.add_uniform(fam, S.truncnorm_u(qs[t], a), "transition %d" % (t + 1))
    S.assert_stationary(fam, "oracle, truncated normal")
    term = S.terminations(ts)
    assert S.moved_fraction(q0, qs[0]) > 0.8
    assert term["divergence"] >= 0.01 and term["mean_depth"] >= 2, term


def test_logistic(oracle, tmp_path):
    """a user density with an energy-dependent orbit period (the separable logistic), where which point of the trajectory a
    transition returns matters more than for a Gaussian: 2^15 chains of D = 2"""
    D, T, n = 2, 3, 1 << 15
    rng = np.random.default_rng(6)
    loc, scale = np.zeros(D), np.ones(D)
    om = oracle.OracleModel.custom(D, S.LOGISTIC_C, np.concatenate([loc, scale]), str(tmp_path))
    q0 = S.logistic_draws(rng, n, loc, scale)
    minv = np.pi ** 2 / 3.0 * rng.uniform(0.3, 3.0, (n, D))
    eps = rng.uniform(0.3, 0.8, n)
    qs, ts = run_chains(oracle, om, q0, minv, eps, T)
    fam = S.Family()
    for t in range(T):
        S.add_uniform(fam, S.logistic_u(qs[t], loc, scale), "transition %d" % (t + 1))
    S.assert_stationary(fam, "oracle, logistic")
    term = S.terminations(ts)
    assert S.moved_fraction(q0, qs[0]) > 0.9
    assert term["mean_depth"] >= 2, term


def diag_start(D, n, seed):
    rng = np.random.default_rng(seed)
    mu, sigma = S.diag_target(D)
    q0 = S.diag_gaussian(rng, n, mu, sigma)
    minv = sigma ** 2 * rng.uniform(0.3, 3.0, (n, D))
    return rng, mu, sigma, q0, minv


@pytest.mark.parametrize("momentum", ["right", "wrong"])
def test_momentum_variance_control(oracle, momentum):
    """negative control: a transition that keeps a momentum drawn with variance minv where 1/minv belongs is not invariant and
    must be rejected; the same transition with a correctly drawn momentum must pass"""
    D = 8
    rng, mu, sigma, q0, minv = diag_start(D, C, 3)
    n = rng.standard_normal((C, D))
    p0 = n / np.sqrt(minv) if momentum == "right" else n * np.sqrt(minv)
    eps = rng.uniform(0.2, 0.6, C)
    qs, ts = run_chains(oracle, oracle.OracleModel.diag(mu, 1.0 / sigma ** 2), q0, minv, eps, 1, p0=p0)
    fam = S.Family()
    S.add_gaussian(fam, (qs[0] - mu) / sigma, "kept momentum")
    if momentum == "right":
        assert S.moved_fraction(q0, qs[0]) > 0.9
    (S.assert_stationary if momentum == "right" else S.assert_rejects)(fam, "oracle, %s momentum" % momentum)


def test_leapfrog_without_accept_step_control(oracle):
    """negative control: leapfrog steps near the stability limit with no accept step move an exact draw off the target"""
    D, steps = 8, NOACC_STEPS
    rng, mu, sigma, q0, minv = diag_start(D, C, 4)
    p0 = rng.standard_normal((C, D)) / np.sqrt(minv)
    eps = NOACC_EPS * np.sqrt(np.min(1.0 / (minv / sigma ** 2), axis=1))      # the limit is 2 / max(sqrt(minv) / sigma)
    om = oracle.OracleModel.diag(mu, 1.0 / sigma ** 2)
    q1 = np.empty_like(q0)
    for c in range(C):
        ch = oracle.OracleChain(om, seed=SEED, chain_id=c)
        ch.set_minv(minv[c])
        ch.set_q(q0[c])
        ch.set_p(p0[c])
        for _ in range(steps):
            ch.leapfrog(eps[c])
        q1[c] = ch.q[:D]
    fam = S.Family()
    S.add_gaussian(fam, (q1 - mu) / sigma, "leapfrog without accept")
    S.assert_rejects(fam, "oracle, leapfrog without accept step")
