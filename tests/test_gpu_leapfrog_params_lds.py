"""The single-step leapfrog serves the parameters all chains share -- mu and tau of the density, M^-1 of a shared metric -- from LDS:
each workgroup stages them once per launch, its four waves together, behind one barrier; a per-chain M^-1 still streams from global
memory.  Only where the values are read from changes, so q, p, lq, pi and the gradient must equal the CPU oracle bit for bit (`==` on
raw doubles) after four sweeps, in the recompute mode and in the store mode.  Each shape is the smallest at which one thing can go
wrong: fewer chains than waves of a workgroup (idle waves in the fill and at the barrier), a last workgroup with three live waves and
more chains than resident waves, every chunk count that takes another kernel form or staging size, a density without parameters, a
per-chain metric, and new metric values between launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 0.05
SWEEPS = 4


def models(pkg, O, kind, D):
    if kind == "iso":
        return pkg.IsoGaussian(D), O.OracleModel.iso(D), np.linspace(0.5, 2.0, D)
    sig = np.logspace(-1, 1, D)
    mu = np.sin(np.arange(D, dtype=np.float64))
    return pkg.DiagGaussian(mu, sigma=sig), O.OracleModel.diag(mu, 1.0 / sig ** 2), sig ** 2


def state(eng):
    """q, p, lq, pi and only then the gradient (asking for it re-evaluates a stale array)"""
    q, p, lq, pi = eng.q, eng.p, eng.lq, eng.logdensity()
    return {"q": q, "p": p, "lq": lq, "pi": pi, "grad": eng.grad}


def assert_chain_equal(got, c, ch, D, what):
    want = {"q": ch.q[:D], "p": ch.p[:D], "lq": ch.lq, "pi": ch.logdensity(), "grad": ch.grad[:D]}
    for k, w in want.items():
        g = np.asarray(got[k][c], dtype=np.float64)
        w = np.asarray(w, dtype=np.float64)
        same = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
        assert same.all(), "%s: chain %d: %s: %d of %d values differ" % (what, c, k, (~same).sum(), same.size)


def engine(pkg, O, monkeypatch, kind, D, C, seed, store, metric_mode):
    monkeypatch.setenv("IDHMC_PLACEMENT_TRIES", "1")       # plain allocations: the placement search is not what is tested here
    gm, _, _ = models(pkg, O, kind, D)
    eng = pkg.Engine(gm, C, pkg.default_options(metric_mode=metric_mode), seed=seed)
    eng.set_leapfrog_grad_mode(pkg.GRAD_STORE if store else pkg.GRAD_RECOMPUTE)
    return eng


# (kind, D, C, oracle chains)
SHARED = [
    ("diag", 1024, 3, (0, 1, 2)),                               # fewer chains than waves of one workgroup
    ("diag", 1000, 4099, (0, 1, 2047, 2048, 4096, 4098)),       # pads; three live waves in the last workgroup; > 2048 chains
    ("diag", 100, 9, range(9)),                                 # NCH 1
    ("diag", 300, 9, range(9)),                                 # NCH 3
    ("diag", 1100, 9, range(9)),                                # NCH 9: chunk by chunk
    ("diag", 2048, 9, range(9)),                                # NCH 16: chunk by chunk, 48 KiB staged
    ("iso", 32, 9, range(9)),                                   # no mu, tau: M^-1 alone
    ("iso", 1024, 9, range(9)),
]


@pytest.mark.parametrize("store", [False, True], ids=["recompute", "store"])
@pytest.mark.parametrize("kind,D,C,chains", SHARED, ids=["%s%d-C%d" % s[:3] for s in SHARED])
def test_shared_parameters_match_the_oracle(idhmc, oracle, monkeypatch, kind, D, C, chains, store):
    _, om, minv = models(idhmc, oracle, kind, D)
    eng = engine(idhmc, oracle, monkeypatch, kind, D, C, 11, store, idhmc.METRIC_SHARED)
    try:
        eng.set_minv(minv)
        eng.random_position()
        eng.refresh_momentum(1)
        for _ in range(SWEEPS):
            eng.leapfrog(EPS, 1)
        got = state(eng)
    finally:
        eng.close()
    for c in chains:
        ch = oracle.OracleChain(om, seed=11, chain_id=c)
        ch.set_minv(minv)
        ch.random_position()
        ch.rand_p(1)
        for _ in range(SWEEPS):
            ch.leapfrog(EPS)
        assert_chain_equal(got, c, ch, D, "%s %d, %d chains" % (kind, D, C))


@pytest.mark.parametrize("store", [False, True], ids=["recompute", "store"])
def test_per_chain_metric_and_stepsize(idhmc, oracle, monkeypatch, store):
    """M^-1 from global memory, mu and tau from LDS; every chain its own stepsize"""
    kind, D, C = "diag", 1024, 9
    _, om, _ = models(idhmc, oracle, kind, D)
    eps = np.linspace(0.02, 0.08, C)
    minv = np.linspace(0.5, 2.0, C * D).reshape(C, D)
    eng = engine(idhmc, oracle, monkeypatch, kind, D, C, 8, store, idhmc.METRIC_PER_CHAIN)
    try:
        eng.set_minv(minv)
        eng.random_position()
        eng.refresh_momentum(4)
        eng.set_eps(eps)
        for _ in range(SWEEPS):
            eng.leapfrog(None, 1)
        got = state(eng)
    finally:
        eng.close()
    for c in range(C):
        ch = oracle.OracleChain(om, seed=8, chain_id=c)
        ch.set_minv(minv[c])
        ch.random_position()
        ch.rand_p(4)
        for _ in range(SWEEPS):
            ch.leapfrog(float(eps[c]))
        assert_chain_equal(got, c, ch, D, "per-chain metric, own stepsize")


@pytest.mark.parametrize("store", [False, True], ids=["recompute", "store"])
def test_new_metric_between_launches_is_seen(idhmc, oracle, monkeypatch, store):
    """two sweeps, set_minv to other values and a momentum refresh, two more sweeps: the staged copy never outlives its launch"""
    kind, D, C = "diag", 1024, 9
    _, om, minv = models(idhmc, oracle, kind, D)
    minv2 = np.linspace(2.0, 0.25, D)
    eng = engine(idhmc, oracle, monkeypatch, kind, D, C, 5, store, idhmc.METRIC_SHARED)
    try:
        eng.set_minv(minv)
        eng.random_position()
        eng.refresh_momentum(1)
        for _ in range(2):
            eng.leapfrog(EPS, 1)
        eng.set_minv(minv2)
        eng.refresh_momentum(2)
        for _ in range(2):
            eng.leapfrog(EPS, 1)
        got = state(eng)
    finally:
        eng.close()
    for c in range(C):
        ch = oracle.OracleChain(om, seed=5, chain_id=c)
        ch.set_minv(minv)
        ch.random_position()
        ch.rand_p(1)
        for _ in range(2):
            ch.leapfrog(EPS)
        ch.set_minv(minv2)
        ch.rand_p(2)
        for _ in range(2):
            ch.leapfrog(EPS)
        assert_chain_equal(got, c, ch, D, "set_minv between launches")
