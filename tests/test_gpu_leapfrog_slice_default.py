"""The default single-step sweep of a separable density streams q and p only, so its Infinity-Cache slice is sized for two arrays:
every ceil(C L 2 8 / 192 MiB)-th chain, where the store mode's slice takes every ceil(C L 3 8 / 192 MiB)-th.  Only the cache policy of
a chain's loads and stores depends on the stride, so slice and stream chains alike equal the oracle bit for bit.  And the placement
search's walk over whole sets hands the fastest of the kept set's three pairs to q and p: whatever it picks, the results are the
oracle's and nothing it allocated on the way stays behind."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 1024


def workload():
    return np.sin(np.arange(D, dtype=np.float64)), np.logspace(-1, 1, D)


def oracle_chain(oracle, mu, sig, c, sweeps):
    ch = oracle.OracleChain(oracle.OracleModel.diag(mu, 1.0 / sig ** 2), seed=3, chain_id=c)
    ch.set_minv(sig ** 2)
    ch.random_position()
    ch.rand_p(2)
    for _ in range(sweeps):
        ch.leapfrog(0.1)
    return ch


def swept(idhmc, C):
    """a default-options engine (shared metric) after four sweeps: (q, p, lq, pi, grad) and what the getters said"""
    mu, sig = workload()
    opt = idhmc.default_options(metric_mode=idhmc.METRIC_SHARED)
    assert opt.leapfrog_grad_mode == idhmc.GRAD_RECOMPUTE
    eng = idhmc.Engine(idhmc.DiagGaussian(mu, sigma=sig), C, opt, seed=3)
    try:
        info = (eng.leapfrog_slice_info(), eng.placement_info())
        eng.set_minv(sig ** 2)
        eng.random_position()
        eng.refresh_momentum(2)
        for _ in range(4):
            eng.leapfrog(0.1, 1)
        q, p, lq, pi = eng.q, eng.p, eng.lq, eng.logdensity()
        return (q, p, lq, pi, eng.grad), info
    finally:
        eng.close()


def assert_chains_match(oracle, arrays, chains):
    q, p, lq, pi, g = arrays
    mu, sig = workload()
    for c in chains:
        ch = oracle_chain(oracle, mu, sig, c, 4)
        assert np.array_equal(q[c], ch.q[:D]) and np.array_equal(p[c], ch.p[:D]), c
        assert np.array_equal(g[c], ch.grad[:D]), c
        assert lq[c] == ch.lq and pi[c] == ch.logdensity(), c


@pytest.mark.parametrize("C, strides", [(32768, (4, 3)), (2048, (1, 1))])
def test_both_strides(idhmc, oracle, monkeypatch, C, strides):
    assert (-(-C * D * 3 * 8 // (192 << 20)), -(-C * D * 2 * 8 // (192 << 20))) == strides
    monkeypatch.setenv("IDHMC_PLACEMENT_TRIES", "1")       # plain allocations: the placement search is not what is tested here
    arrays, (slice_info, _) = swept(idhmc, C)
    assert slice_info == strides
    # slice chains of both strides (0, 3, 4, C - 1 - (C - 1) % 3 ...) and stream chains, at both ends and in the middle of the sweep
    chains = sorted({0, 1, 3, 4, C // 2, C // 2 + 1, C - 3, C - 1})
    if strides[1] > 1:
        assert any(c % strides[1] == 0 for c in chains) and any(c % strides[1] != 0 for c in chains)
    assert_chains_match(oracle, arrays, chains)


def test_whole_set_walk_reorders_and_leaks_nothing(idhmc, oracle, monkeypatch):
    C = 8192                                               # 64 MiB per array: the smallest size at which the search runs
    monkeypatch.setenv("IDHMC_PLACEMENT_PAIRS", "0")       # straight to the walk over whole sets
    arrays, (_, (gbps, ncand)) = swept(idhmc, C)
    assert ncand >= 1 and gbps > 0.0                       # (no rate is asserted: the class of the memory a test gets is not under its control)
    assert_chains_match(oracle, arrays, [0, 1, C - 1])
    _, (_, (_, ncand2)) = swept(idhmc, C)                  # a second engine of the same size after close()
    assert ncand2 >= 1
