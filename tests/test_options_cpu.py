"""Non-default options, without a GPU: the option sets that tests/test_gpu_options.py passes to the device, and the proof that the
comparator itself honours them.  Every default is one number, so a kernel that read a literal instead of its option -- or two fields
copied crosswise when the context is made -- passes every test that runs at the defaults; so would an oracle with the same fault.  Here

  * the initial stepsize search of the C oracle (oracle/idhmc_oracle.c) under three sets of (a_min, a_max, eps0, C) is held against
    the numpy restatement (oracle/numpy_warmup.py) for an exactly equal eps, on the two Gaussians numpy_tree.py can run;
  * every search result is classified from eps alone -- eps0: the first ratio was in the band; eps0 * C^k: the crossing ended in the
    band; anything else: bisection -- and over the cases each of in band, upward crossing, downward crossing, bisection after an
    upward and after a downward crossing occurs;
  * ss_maxiter_crossing = 3 from eps0 = 1e-3, and ss_maxiter_bisect = 2 with the band narrowed to [0.4, 0.6], make the oracle return -1, respectively
    -2, for some chains and 0 for others (the restatement raises the reference's two errors for the same chains);
  * 20 steps of dual averaging with non-default delta, gamma, kappa and t0 agree with the restatement's recursion to 1e-9 on eps;
  * stepsize_search = 0, eps_init and adapt_metric = 0 in mcmc_with_warmup are what the same stages made by hand give;
  * and with each option set the oracle's result differs from its result under the default options: a pair of implementations
    that both ignored an option could not pass."""
import ctypes
import functools
import math

import numpy as np
import pytest

from oracle import numpy_tree as NT
from oracle import numpy_warmup as NW
from test_deep_trees_cpu import oracle_models, problem

# ---- the stepsize search ----------------------------------------------------------------------------------------------------------------
SEARCH_SETS = {
    "wide_steps": dict(ss_a_min=0.6, ss_a_max=0.9, ss_eps0=0.3, ss_C=3.0),
    "small_start": dict(ss_a_min=0.25, ss_a_max=0.75, ss_eps0=0.01, ss_C=1.5),
    "narrow_band": dict(ss_a_min=0.49, ss_a_max=0.51, ss_eps0=1.0, ss_C=2.0),
}
FAILURE_SETS = {
    "crossing": (dict(ss_maxiter_crossing=3, ss_eps0=1e-3), -1),
    "bisection": (dict(ss_maxiter_bisect=2, ss_a_min=0.4, ss_a_max=0.6), -2),
}
SEARCH_C = 16
# model -> (problem of tests/test_deep_trees_cpu.py or a Gaussian, the decades over which the 16 starts are scaled)
SEARCH_MODELS = {
    "iso8": ("iso", 8, (-2.0, 4.0)),                       # k_stepsize_search of a separable density
    "diag130": ("diag", 130, (-2.0, 4.0)),                 # the same, two chunks
    "custom128": ("problem", "custom128", (-2.0, 1.0)),    # k_stepsize_search of a general density from here on
    "logistic_mc128": ("problem", "logistic_mc128", (-2.0, 2.0)),
    "glm_responses": ("problem", "glm_responses", (-2.0, 2.0)),
    "dense_coop128": ("problem", "dense_coop128", (-2.0, 4.0)),
}
SEARCH_SEED = 21


def diag_gaussian(D):
    rng = np.random.default_rng(4)
    return rng.standard_normal(D), np.exp(rng.standard_normal(D))


def search_model(name):
    """(D, engine(idhmc) -> Model, oracle models, chains per oracle model or None)"""
    from oracle import oracle as O
    kind, what, _ = SEARCH_MODELS[name]
    if kind == "iso":
        return what, (lambda idhmc: idhmc.IsoGaussian(what)), [O.OracleModel.iso(what)], None
    if kind == "diag":
        mu, sig = diag_gaussian(what)
        return what, (lambda idhmc: idhmc.DiagGaussian(mu, sigma=sig)), [O.OracleModel.diag(mu, 1.0 / sig ** 2)], None
    prob = problem(what)
    return prob["D"], prob["engine"], oracle_models(what), prob["block"]


def search_start(name):
    """16 starts (a Gaussian's: around its mean) scaled over several decades, from a point where the momentum dominates the energy to
    one where the position does"""
    kind, what, (lo, hi) = SEARCH_MODELS[name]
    D = search_model(name)[0]
    rng = np.random.default_rng(D)
    centre = diag_gaussian(D)[0] if kind == "diag" else 0.0
    return centre + rng.standard_normal((SEARCH_C, D)) * (10.0 ** np.linspace(lo, hi, SEARCH_C))[:, None]


def search_minv(name):
    """a per-chain metric, a multiple of the unit matrix scaled over nine decades in an order unrelated to the starts': every chain's
    frequencies, and so the stepsize at which its leapfrog turns unstable, lie elsewhere -- from far above each eps0 of the option
    sets (the search goes up) to far below (it goes down, or stops at its iteration limit)"""
    D = search_model(name)[0]
    order = np.random.default_rng(7).permutation(SEARCH_C)
    return np.repeat((10.0 ** np.linspace(-2.0, 7.0, SEARCH_C))[order][:, None], D, axis=1)


def search_chains(name, **options):
    from oracle import oracle as O
    D, _, models, block = search_model(name)
    opt = O.default_options(**options)
    chains = [O.OracleChain(models[c // block] if block else models[0], opt, seed=SEARCH_SEED, chain_id=c) for c in range(SEARCH_C)]
    minv = search_minv(name)
    for c, q in enumerate(search_start(name)):
        chains[c].set_minv(minv[c])
        chains[c].set_q(q)
        chains[c].rand_p(0)
    return chains


@functools.lru_cache(maxsize=None)
def _search_oracle(name, options):
    out = [ch.find_initial_stepsize() for ch in search_chains(name, **dict(options))]
    rc, eps = np.array([r for r, _ in out]), np.array([e for _, e in out])
    rc.setflags(write=False)
    eps.setflags(write=False)
    return rc, eps


def search_oracle(name, **options):
    """(return code [16], eps [16]) of the oracle's search from search_start(name) with the momentum of transition 0"""
    return _search_oracle(name, tuple(sorted(options.items())))


def classify(eps, ss_eps0, ss_C, **_):
    """from eps alone: "band", "up" / "down" (the crossing ended in the band), "bisect_up" / "bisect_down" """
    if eps == ss_eps0:
        return "band"
    for kind, factor in (("up", ss_C), ("down", 1.0 / ss_C)):
        e = ss_eps0
        for _ in range(400):
            e = e * factor
            if e == eps:
                return kind
    return "bisect_up" if eps > ss_eps0 else "bisect_down"


def test_every_branch_of_the_search_occurs(oracle):
    seen = {}
    for sname, opts in SEARCH_SETS.items():
        for name in SEARCH_MODELS:
            rc, eps = search_oracle(name, **opts)
            assert not rc.any(), (sname, name, rc)
            kinds = [classify(e, **opts) for e in eps]
            print("%-12s %-15s %s" % (sname, name, " ".join(kinds)))
            for k in kinds:
                seen[k] = seen.get(k, 0) + 1
    print(seen)
    assert set(seen) == {"band", "up", "down", "bisect_up", "bisect_down"}, seen


@pytest.mark.parametrize("sname", list(SEARCH_SETS))
@pytest.mark.parametrize("name", list(SEARCH_MODELS))
def test_each_search_option_changes_the_result(oracle, name, sname):
    """the control: the same starts and momenta under the default options give another eps"""
    _, eps = search_oracle(name, **SEARCH_SETS[sname])
    _, default = search_oracle(name)
    assert np.count_nonzero(eps != default) >= SEARCH_C // 2


def _numpy_search(name, par):
    """the restatement's search from the same starts and momenta: eps, or the text of the error it raised, per chain"""
    from oracle import oracle as O
    kind, D, _ = SEARCH_MODELS[name]
    mu, sig = (np.zeros(D), np.ones(D)) if kind == "iso" else diag_gaussian(D)
    Lp = O.padded_len(D)
    minv = search_minv(name)
    out = []
    for c, q in enumerate(search_start(name)):
        H = NT.Hamiltonian(NT.DiagGaussianDensity(mu, 1.0 / sig ** 2), minv[c])
        z = np.zeros(Lp)
        O.lib().orc_randn_export(SEARCH_SEED, c, 0, Lp, z.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        lq, g = H.evaluate(q)
        try:
            out.append(NW.find_initial_stepsize(par, NW.local_acceptance_ratio(H, NT.PhasePoint(q, lq, g, z[:D] / np.sqrt(minv[c])))))
        except RuntimeError as e:
            out.append(str(e))
    return out


@pytest.mark.parametrize("sname", list(SEARCH_SETS))
@pytest.mark.parametrize("name", ["iso8", "diag130"])
def test_the_search_options_against_the_restatement(oracle, name, sname):
    o = SEARCH_SETS[sname]
    rc, eps = search_oracle(name, **o)
    got = _numpy_search(name, NW.InitialStepsizeSearch(o["ss_a_min"], o["ss_a_max"], o["ss_eps0"], o["ss_C"]))
    assert not rc.any() and got == eps.tolist()                     # the same decisions, so exactly the same eps


@pytest.mark.parametrize("fname", list(FAILURE_SETS))
@pytest.mark.parametrize("name", ["iso8", "custom128"])
def test_the_two_failures_of_the_search(oracle, name, fname):
    """some chains fail with the code of this limit, the others succeed; on the Gaussian the restatement raises the reference's error
    of that limit for the same chains and returns the oracle's eps for the others"""
    opts, code = FAILURE_SETS[fname]
    rc, eps = search_oracle(name, **opts)
    print(fname, name, rc.tolist())
    assert set(rc.tolist()) == {0, code}, rc
    if name == "iso8":
        d = dict(ss_a_min=0.25, ss_a_max=0.75, ss_eps0=1.0, ss_C=2.0, ss_maxiter_crossing=400, ss_maxiter_bisect=400)
        d.update(opts)
        got = _numpy_search(name, NW.InitialStepsizeSearch(d["ss_a_min"], d["ss_a_max"], d["ss_eps0"], d["ss_C"], d["ss_maxiter_crossing"],
                                                           d["ss_maxiter_bisect"]))
        word = "searching for eps" if code == -1 else "bisecting"
        for c in range(SEARCH_C):
            assert (word in got[c]) if rc[c] else got[c] == eps[c], (c, rc[c], got[c], eps[c])


# ---- dual averaging -----------------------------------------------------------------------------------------------------------------------
DA_OPTIONS = dict(da_delta=0.65, da_gamma=0.1, da_kappa=0.6, da_t0=25)
DA_N = 20


def da_stage(chains, eps0, N, iter0=0, **options):
    """a tuning stage of N transitions of every chain with its own dual averaging (oracle's orc_da_*), from eps0: dict(used [N][C],
    final [C], rec [N][C], q [N][C][D], minv [C][D] as the stage's metric update would make it)"""
    from oracle import oracle as O
    L = O.lib()
    opt = O.default_options(**options)
    C_, D = len(chains), chains[0].D
    out = dict(used=np.empty((N, C_)), final=np.empty(C_), rec=np.zeros((N, C_), dtype=O.STATS_DTYPE), q=np.empty((N, C_, D)),
               minv=np.empty((C_, D)))
    for c, ch in enumerate(chains):
        da = O.DAState()
        L.orc_da_init(ctypes.byref(da), float(np.broadcast_to(eps0, (C_,))[c]))
        full = np.zeros((N, ch.L))
        for n in range(N):
            e = L.orc_da_current_eps(ctypes.byref(da))
            st = ch.sample_tree(e, iter0 + n + 1)
            out["used"][n, c], out["q"][n, c], full[n] = e, ch.q[:D], ch.q
            out["rec"][n, c] = (st.pi, st.acceptance_rate, st.term_left, st.term_right, st.depth, st.steps)
            L.orc_da_adapt(ctypes.byref(opt), ctypes.byref(da), st.acceptance_rate)
        out["final"][c] = L.orc_da_final_eps(ctypes.byref(da))
        out["minv"][c] = O.metric_from_draws(full, D, 5.0 / N)[0][:D]
    return out


def iso32_chains(C_=6, seed=9, **options):
    from oracle import oracle as O
    chains = [O.OracleChain(O.OracleModel.iso(32), O.default_options(**options), seed=seed, chain_id=c) for c in range(C_)]
    for ch in chains:
        ch.random_position()
    return chains


def test_dual_averaging_options_against_the_restatement(oracle):
    """the oracle's stage under DA_OPTIONS; the restatement's recursion (src/stepsize.jl:208-241) fed the same acceptance rates gives
    every eps used and the final one to 1e-9 -- and the stage under the default constants does not"""
    ref = da_stage(iso32_chains(max_depth=7), 0.05, DA_N, **DA_OPTIONS)
    da = NW.DualAveraging(DA_OPTIONS["da_delta"], DA_OPTIONS["da_gamma"], DA_OPTIONS["da_kappa"], DA_OPTIONS["da_t0"])
    for c in range(ref["used"].shape[1]):
        st = da.initial_state(0.05)
        for n in range(DA_N):
            assert abs(math.exp(st[3]) - ref["used"][n, c]) <= 1e-9 * ref["used"][n, c], (c, n)
            st = da.adapt(st, float(ref["rec"]["acceptance_rate"][n, c]))
        assert abs(math.exp(st[4]) - ref["final"][c]) <= 1e-9 * ref["final"][c]
    default = da_stage(iso32_chains(max_depth=7), 0.05, DA_N)
    assert np.all(default["used"][0] == ref["used"][0]) and np.all(default["used"][1] != ref["used"][1])
    assert np.all(default["final"] != ref["final"])


@pytest.mark.parametrize("option", list(DA_OPTIONS))
def test_each_dual_averaging_option_changes_the_stage(oracle, option):
    """one constant at a time: each of the four is read"""
    ref = da_stage(iso32_chains(max_depth=7), 0.05, DA_N)
    one = da_stage(iso32_chains(max_depth=7), 0.05, DA_N, **{option: DA_OPTIONS[option]})
    assert np.all(one["final"] != ref["final"])


# ---- the driver's own options ----------------------------------------------------------------------------------------------------------------
DRIVER_OPTIONS = dict(stepsize_search=0, eps_init=0.07, adapt_metric=0, init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8,
                      max_depth=6)
DRIVER_N, DRIVER_SEED = 10, 77


def test_the_drivers_options_are_the_stages_made_by_hand(oracle):
    """mcmc_with_warmup under DRIVER_OPTIONS on the diagonal Gaussian: no search (the first stage starts at eps_init), no metric update
    (M^-1 stays the unit matrix) -- the same draws as the four stages and the sampling made call by call; and other draws than with
    the search, with the metric update, or from another eps_init"""
    O = oracle
    D, C_ = 100, 3
    mu, sig = diag_gaussian(D)
    om = O.OracleModel.diag(mu, 1.0 / sig ** 2)
    rc, chains, stats, eps = O.threaded_mcmc(om, DRIVER_N, C_, O.default_options(**DRIVER_OPTIONS), seed=DRIVER_SEED)
    assert rc == 0
    by_hand = [O.OracleChain(om, O.default_options(**DRIVER_OPTIONS), seed=DRIVER_SEED, chain_id=c) for c in range(C_)]
    for ch in by_hand:
        ch.random_position()
    e, it = 0.07, 0
    for n in (12, 8, 16, 8):
        e = da_stage(by_hand, e, n, iter0=it)["final"]
        it += n
    assert np.array_equal(e, eps)
    for c, ch in enumerate(by_hand):
        assert np.all(ch.minv == 1.0)
        for n in range(DRIVER_N):
            st = ch.sample_tree(e[c], it + n + 1)
            assert np.array_equal(ch.q, chains[c, n]) and st.steps == stats[c, n]["steps"]
    for change in (dict(stepsize_search=1), dict(adapt_metric=1), dict(eps_init=0.08)):
        other = O.threaded_mcmc(om, DRIVER_N, C_, O.default_options(**dict(DRIVER_OPTIONS, **change)), seed=DRIVER_SEED)
        assert other[0] == 0 and np.all(other[3] != eps), change
