"""The single-step leapfrog of a separable density re-derives grad l(q) from q by default (IDHMC_GRAD_RECOMPUTE is what
idhmc_default_options sets): the sweep neither reads nor writes the gradient array, and every call that needs the array brings it up
to date first.  Everything below is `==` on the raw doubles: against the CPU oracle, and against an engine in the store mode taken
through the same calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [("iso", 32), ("diag", 100), ("diag", 1024)]
C = 7
EPS = 0.05


def models(pkg, O, kind, D):
    if kind == "iso":
        return pkg.IsoGaussian(D), O.OracleModel.iso(D), np.ones(D)
    sig = np.logspace(-1, 1, D)
    mu = np.sin(np.arange(D, dtype=np.float64))
    return pkg.DiagGaussian(mu, sigma=sig), O.OracleModel.diag(mu, 1.0 / sig ** 2), sig ** 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits_equal(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    same = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), "%s: %d of %d values differ" % (what, (~same).sum(), same.size)


def state(eng):
    """q, p, lq, pi and only then the gradient (asking for it re-evaluates a stale array)"""
    q, p, lq, pi = eng.q, eng.p, eng.lq, eng.logdensity()
    return {"q": q, "p": p, "lq": lq, "pi": pi, "grad": eng.grad}


def assert_same_state(a, b, what):
    for k in ("q", "p", "lq", "pi", "grad"):
        assert_bits_equal(a[k], b[k], "%s: %s" % (what, k))


def oracle_state(chains, D):
    return {"q": np.stack([c.q[:D] for c in chains]), "p": np.stack([c.p[:D] for c in chains]),
            "lq": np.array([c.lq for c in chains]), "pi": np.array([c.logdensity() for c in chains]),
            "grad": np.stack([c.grad[:D] for c in chains])}


def started(pkg, O, kind, D, seed, store, **optkw):
    """an engine after random_position and a momentum refresh; store: switched to GRAD_STORE on the live context"""
    gm, _, minv = models(pkg, O, kind, D)
    eng = pkg.Engine(gm, C, pkg.default_options(**optkw), seed=seed)
    if store:
        eng.set_leapfrog_grad_mode(pkg.GRAD_STORE)
    eng.set_minv(minv)
    eng.random_position()
    eng.refresh_momentum(1)
    return eng


def oracle_chains(O, kind, D, seed, pkg):
    _, om, minv = models(pkg, O, kind, D)
    chains = [O.OracleChain(om, seed=seed, chain_id=c) for c in range(C)]
    for ch in chains:
        ch.set_minv(minv)
        ch.random_position()
        ch.rand_p(1)
    return chains


def test_default_options_recompute(idhmc):
    assert idhmc.default_options().leapfrog_grad_mode == idhmc.GRAD_RECOMPUTE
    assert idhmc.GRAD_STORE == 0          # what a zero-initialised idhmc_options holds
    assert idhmc.engine.Options().leapfrog_grad_mode == idhmc.GRAD_STORE


@pytest.mark.parametrize("kind,D", SHAPES)
def test_default_single_steps_bit_exact(idhmc, oracle, kind, D):
    chains = oracle_chains(oracle, kind, D, 42, idhmc)
    for ch in chains:
        for _ in range(4):
            ch.leapfrog(EPS)
    want = oracle_state(chains, D)
    got = {}
    for store in (False, True):
        eng = started(idhmc, oracle, kind, D, 42, store)
        try:
            for _ in range(4):
                eng.leapfrog(EPS, 1)
            got[store] = state(eng)
        finally:
            eng.close()
        assert_same_state(got[store], want, "store mode" if store else "default mode")
    assert_same_state(got[False], got[True], "default against store")


def both(idhmc, oracle, kind, D, seed, calls, **optkw):
    """the default engine and a store-mode engine through the same calls; their final states"""
    out = []
    for store in (False, True):
        eng = started(idhmc, oracle, kind, D, seed, store, **optkw)
        try:
            calls(eng, store)
            out.append(state(eng))
        finally:
            eng.close()
    assert_same_state(out[0], out[1], "default against store")
    return out[0]


@pytest.mark.parametrize("kind,D", SHAPES)
def test_transition_between_single_steps(idhmc, oracle, kind, D):
    def calls(eng, store):
        eng.set_eps(0.04)
        eng.leapfrog(EPS, 1)
        eng.nuts_transition(2)
        eng.refresh_momentum(3)       # (a transition leaves the momentum array unspecified)
        eng.leapfrog(EPS, 1)
    got = both(idhmc, oracle, kind, D, 9, calls)
    chains = oracle_chains(oracle, kind, D, 9, idhmc)
    for ch in chains:
        ch.leapfrog(EPS)
        ch.sample_tree(0.04, 2)
        ch.rand_p(3)
        ch.leapfrog(EPS)
    assert_same_state(got, oracle_state(chains, D), "leapfrog, transition, leapfrog")


@pytest.mark.parametrize("kind,D", SHAPES)
def test_local_optimum_after_single_step(idhmc, oracle, kind, D):
    def calls(eng, store):
        eng.leapfrog(EPS, 1)
        eng.find_local_optimum(1e-4, 10)
    got = both(idhmc, oracle, kind, D, 5, calls)
    chains = oracle_chains(oracle, kind, D, 5, idhmc)
    for ch in chains:
        ch.leapfrog(EPS)
        ch.find_local_optimum(1e-4, 10)
    want = oracle_state(chains, D)
    for k in ("q", "lq", "grad"):
        assert_bits_equal(got[k], want[k], "find_local_optimum after a stale gradient: " + k)


@pytest.mark.parametrize("kind,D", SHAPES)
def test_set_q_after_single_step(idhmc, oracle, kind, D):
    q_new = np.random.default_rng(1).standard_normal((C, D))

    def calls(eng, store):
        eng.leapfrog(EPS, 1)
        eng.set_q(q_new)
    got = both(idhmc, oracle, kind, D, 6, calls)
    chains = oracle_chains(oracle, kind, D, 6, idhmc)
    for c, ch in enumerate(chains):
        ch.leapfrog(EPS)
        ch.set_q(q_new[c])
    want = oracle_state(chains, D)
    for k in ("q", "lq", "grad"):
        assert_bits_equal(got[k], want[k], "set_q after a stale gradient: " + k)


@pytest.mark.parametrize("kind,D", SHAPES)
def test_switch_to_store_mode_mid_run(idhmc, oracle, kind, D):
    def calls(eng, store):
        eng.leapfrog(EPS, 1)
        eng.set_leapfrog_grad_mode(idhmc.GRAD_STORE)      # the store sweep reads the array the first step left stale
        eng.leapfrog(EPS, 1)
    got = both(idhmc, oracle, kind, D, 7, calls)
    chains = oracle_chains(oracle, kind, D, 7, idhmc)
    for ch in chains:
        ch.leapfrog(EPS)
        ch.leapfrog(EPS)
    assert_same_state(got, oracle_state(chains, D), "recompute step, then store step")


@pytest.mark.parametrize("kind,D", SHAPES)
def test_own_eps_per_chain_metric(idhmc, oracle, kind, D):
    eps = np.linspace(0.02, 0.08, C)
    minv = np.linspace(0.5, 2.0, C * D).reshape(C, D)

    def calls(eng, store):
        eng.set_minv(minv)
        eng.refresh_momentum(4)
        eng.set_eps(eps)
        eng.leapfrog(None, 1)
    got = both(idhmc, oracle, kind, D, 8, calls, metric_mode=idhmc.METRIC_PER_CHAIN)
    chains = oracle_chains(oracle, kind, D, 8, idhmc)
    for c, ch in enumerate(chains):
        ch.set_minv(minv[c])
        ch.rand_p(4)
        ch.leapfrog(float(eps[c]))
    assert_same_state(got, oracle_state(chains, D), "leapfrog_own_eps with a per-chain metric")
