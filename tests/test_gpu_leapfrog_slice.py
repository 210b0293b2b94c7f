"""The single-step leapfrog keeps a slice of the chains in the Infinity Cache: every lf_stride-th chain (lf_stride = ceil(C L 3 8 /
192 MiB), 1 when the whole state fits) is loaded and stored with the default cache policy, the others non-temporally.  Only the cache
policy differs, so chains of both sets must equal the oracle bit for bit after several sweeps, in the store mode and in the gradient
recompute mode, at a stride > 1 and at stride 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 1024


def workload():
    return np.sin(np.arange(D, dtype=np.float64)), np.logspace(-1, 1, D)


@pytest.mark.parametrize("C, stride", [(32768, 4), (2048, 1)])
@pytest.mark.parametrize("regrad", [False, True])
def test_slice_and_stream_chains_match_the_oracle(idhmc, oracle, monkeypatch, C, stride, regrad):
    mu, sig = workload()
    assert -(-C * D * 3 * 8 // (192 << 20)) == stride
    monkeypatch.setenv("IDHMC_PLACEMENT_TRIES", "1")       # plain allocations: the placement search is not what is tested here
    eng = idhmc.Engine(idhmc.DiagGaussian(mu, sigma=sig), C, idhmc.default_options(metric_mode=idhmc.METRIC_SHARED), seed=3)
    try:
        eng.set_minv(sig ** 2)
        if regrad:
            eng.set_leapfrog_grad_mode(idhmc.GRAD_RECOMPUTE)
        eng.random_position()
        eng.refresh_momentum(2)
        for _ in range(4):
            eng.leapfrog(0.1, 1)
        q, p, lq, pi = eng.q, eng.p, eng.lq, eng.logdensity()
        g = eng.grad
    finally:
        eng.close()
    # chains of the resident slice (c % stride == 0) and of the stream, at both ends and in the middle of the sweep
    chains = sorted({0, stride, 1, stride + 1, C // 2, C // 2 + 1, C - stride, C - 1})
    if stride > 1:
        assert any(c % stride == 0 for c in chains) and any(c % stride != 0 for c in chains)
    om = oracle.OracleModel.diag(mu, 1.0 / sig ** 2)
    for c in chains:
        ch = oracle.OracleChain(om, seed=3, chain_id=c)
        ch.set_minv(sig ** 2)
        ch.random_position()
        ch.rand_p(2)
        for _ in range(4):
            ch.leapfrog(0.1)
        assert np.array_equal(q[c], ch.q[:D]) and np.array_equal(p[c], ch.p[:D]), c
        assert np.array_equal(g[c], ch.grad[:D]), c
        assert lq[c] == ch.lq and pi[c] == ch.logdensity(), c
