"""Deep trees on every form of the NUTS kernel, without a GPU: the cases that tests/test_gpu_deep_trees.py runs on the device, run here
through the CPU oracle, and what each of them reaches asserted from the oracle's records alone -- so that the device module compares
trees that are known to be deep, to stop for every reason inside long doublings, and to differ widely within one 16-chain tile.

A case is a model at the smallest shape at which one form of k_nuts exists (the table PROBLEMS), a number of chains, a geometric ladder
of per-chain stepsizes (chain c runs at lo * (hi / lo) ** (c / (C - 1)), tests/test_gpu_accumulators.ladder), a start and a seed.  A run
of a case (RUNS) adds max_depth and min_delta.  Every case runs at max_depth = 10 with the default min_delta = -1000 and with a tight
one, under which the energy error of a middling stepsize counts as a divergence in the middle of a long doubling; one logistic and
one dense case also at max_depth = 12; the two `limit15` cases at 15, the largest depth idhmc_create accepts.  Each run is T_SINGLE = 4
transitions that the device makes one launch each, and T_FUSED = 3 more that it makes in one launch.

What the oracle's records of the first four transitions hold (test_the_runs_reach_what_they_claim prints this table with -s and
asserts the conditions below it):

    run                             depths seen            max_depth  turn>=64  div inside  tile spread
    custom128/10                    3 4 5 6 7 8 9 10       7          1         0           -
    custom128/10/-0.005             1 2 3 4 5 6 7 8 9 10   7          1         2           -
    custom256/10                    3 4 5 6 7 8 9 10       10         1         0           -
    custom256/10/-0.03              0 2 3 4 5 6 7 8 9 10   10         1         1           -
    dense_coop128/10                2 3 4 5 6 7 8 9 10     17         1         0           7
    dense_coop128/10/-0.005         0 .. 10                17         1         1           10
    dense_coop128/12                2 .. 12                4          3         0           9
    dense_coop128/12/-0.005         0 .. 12                4          3         1           12
    dense_coop256/10                2 3 4 5 6 7 8 9 10     11         1         0           8
    dense_coop256/10/-0.01          0 .. 10                11         1         5           10
    dense_gemv/10                   3 4 5 6 7 8 9 10       4          1         0           -
    dense_gemv/10/-0.01             0 3 4 5 6 7 8 9 10     4          1         2           -
    logistic_mc128/10               2 3 4 5 6 7 8 9 10     17         1         0           7
    logistic_mc128/10/-0.01         0 .. 10                17         1         1           10
    logistic_mc128/12               2 .. 12                4          2         0           9
    logistic_mc128/12/-0.01         0 .. 12                4          2         1           12
    logistic_mc256/10               2 3 4 5 6 7 8 9 10     12         2         4           8
    logistic_mc256/10/-0.005        0 .. 10                12         2         3           10
    logistic_wave/10                3 4 5 6 7 8 9 10       7          1         0           -
    logistic_wave/10/-0.01          0 .. 10                7          1         1           -
    glm_poisson/10                  2 3 4 5 6 7 8 9 10     2          2         0           7
    glm_poisson/10/-0.005           0 .. 10                2          2         2           10
    glm_nb128/10                    3 4 5 6 7 8 9 10       8          6         0           7
    glm_nb128/10/-0.005             0 .. 10                8          6         5           10
    glm_nb256/10                    2 3 4 5 6 7 8 9 10     20         6         0           6
    glm_nb256/10/-0.02              0 .. 10                20         2         8           10
    glm_aux4/10                     2 3 4 5 6 7 8 9 10     3          5         0           8
    glm_aux4/10/-0.01               0 .. 10                3          2         2           10
    glm_hier/10                     2 3 4 5 6 7 8 9 10     18         8         0           6
    glm_hier/10/-0.01               0 .. 10                18         8         1           10
    glm_responses/10                1 2 3 4 5 6 7 8 9 10   8          6         0           9
    glm_responses/10/-0.01          0 .. 10                8          4         3           10
    limit15_sep/15                  13 14 15               6          1         0           -
    limit15_general/15              13 14 15               3          2         0           -

    max_depth:   trees that end with REACHED_MAX_DEPTH
    turn>=64:    trees whose last doubling a turning sub-tree stopped after 64 or more of its leaves (steps - (2^depth - 1) >= 64)
    div inside:  divergences at leaf 2 or later of a doubling of 16 or more leaves
    tile spread: the largest difference of tree depths among chains 0..15 (the first workgroup of a cooperative form) in one transition

The comparator is pinned where the device is tested: test_two_restatements_build_the_same_deep_trees holds oracle/numpy_tree.py against
the C oracle at max_depth 10 and 12 and at two tight min_delta, on a diagonal and a dense Gaussian.  Largest deviation between the two
restatements over those cases (printed with -s), and the bounds asserted, four times the largest value of each column:

    case                                       draw, relative to max(1, |q|)   pi, relative to max(1, |pi|)   acceptance rate
    diag   D = 24   max_depth 10   -1000       1.37e-15                        4.21e-16                       7.11e-15
    diag   D = 24   max_depth 10   -0.02       1.37e-15                        4.21e-16                       1.04e-14
    diag   D = 10   max_depth 12   -0.004      1.35e-15                        3.49e-16                       2.66e-15
    dense  D = 17   max_depth 10   -1000       9.44e-16                        6.17e-16                       1.07e-14
    dense  D = 17   max_depth 10   -0.004      9.44e-16                        6.76e-16                       1.07e-14
    dense  D = 6    max_depth 12   -0.02       1.10e-15                        1.41e-15                       3.55e-15

Every one of the 60 transitions of each case was compared (none skipped for a margin below 1e-9).  DRAW_BOUND, PI_BOUND and ACCEPT_BOUND
below are 4 x 1.37e-15, 4 x 1.42e-15 and 4 x 1.07e-14.
"""
import atexit
import ctypes
import functools
import shutil
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
import test_glm_cpu as FLAT
import test_glm_dispersion_cpu as DISP
import test_glm_hier_cpu as HIER
import test_gpu_custom as CUSTOM
import test_logistic_cpu as LOGISTIC
from test_glm_responses_cpu import responses
from test_gpu_accumulators import ladder, prior
from test_gpu_fused import dense_problem

T_SINGLE, T_FUSED = 4, 3
NB = "NEG_BINOMIAL_LOG_LOGPHI"


# ---- the problems: name -> dict(D, padded, form, coop, engine(idhmc) -> Model, oracle(O, workdir) -> [OracleModel per chain block],
#      block (chains per oracle model, None: one model), start(C) -> [C][D] or None for random_position) ---------------------------------
def _one(model):
    return lambda O, work: [model(O, work)]


def custom_problem(D):
    return dict(D=D, padded=(D + 127) // 128 * 128, form=-1, coop=False, block=None, start=None,
                engine=lambda idhmc: idhmc.CustomDensity(D, CUSTOM.HIP_SRC, CUSTOM.PARAMS),
                oracle=_one(lambda O, work: O.OracleModel.custom(D, CUSTOM.C_SRC, CUSTOM.PARAMS, work)))


def dense_mvn_problem(D):
    mu, P = dense_problem(D)
    return dict(D=D, padded=128 if D <= 128 else 256 if D <= 256 else 512, form=-1, coop=D <= 256, block=None, start=None,
                engine=lambda idhmc: idhmc.DenseMVN(mu, P), oracle=_one(lambda O, work: O.OracleModel.dense(mu, P)))


def iso_problem(D):
    return dict(D=D, padded=(D + 127) // 128 * 128, form=-1, coop=False, block=None, start=None,
                engine=lambda idhmc: idhmc.IsoGaussian(D), oracle=_one(lambda O, work: O.OracleModel.iso(D)))


def logistic_problem(D, n):
    X, y = LOGISTIC.problem(n, D, seed=n + D)
    mu, tau = prior(D)
    coop = D <= 256
    return dict(D=D, padded=128 if D <= 128 else 256 if D <= 256 else 512, form=1 if coop else 0, coop=coop, block=None, start=None,
                engine=lambda idhmc: idhmc.LogisticRegression(X, y, mu, tau),
                oracle=_one(lambda O, work: O.OracleModel.custom(D, LOGISTIC.C_SRC, LOGISTIC.oracle_params(X, y, mu, tau), work)))


def near_origin(D, scale=0.3):
    """tests/test_gpu_glm.start: the oracle's random_position draws from U(-2, 2), too far out for a count model"""
    return lambda C: np.random.default_rng(D).uniform(-scale, scale, (C, D)) / np.sqrt(D)


def poisson_problem(D, n):
    family = "POISSON_LOG"
    X, Y = FLAT.problem(family, n, D, seed=n + D)
    mu, tau = prior(D)
    return dict(D=D, padded=128, form=1, coop=True, block=None, start=near_origin(D),
                engine=lambda idhmc: idhmc.GLM(X, Y, getattr(idhmc.glm, family), None, mu, tau),
                oracle=_one(lambda O, work: O.OracleModel.custom(D, FLAT.c_source(family), FLAT.oracle_params(X, Y, None, mu, tau), work)))


def negative_binomial_problem(Dx, n):
    D = Dx + 1
    X, Y = DISP.problem_disp(NB, n, Dx, seed=n + Dx)
    mu, tau = prior(D)
    return dict(D=D, padded=128 if D <= 128 else 256, form=1, coop=True, block=None, start=lambda C: DISP.start_disp(NB, C, Dx),
                engine=lambda idhmc: DISP.make(idhmc, NB, X, Y, mu, tau),
                oracle=_one(lambda O, work: O.OracleModel.custom(D, DISP.c_source_disp(NB), AUX.oracle_params_aux(X, Y, 1, None, mu, tau), work)))


def four_auxiliary_problem(Dx, n):
    family = "TEST_A4"
    D = Dx + 4
    X, Y = AUX.problem_aux(family, n, Dx, seed=n + Dx)
    mu, tau = prior(D)
    return dict(D=D, padded=128, form=1, coop=True, block=None, start=lambda C: AUX.start_aux(family, C, Dx),
                engine=lambda idhmc: AUX.make(idhmc, family, X, Y, mu, tau),
                oracle=_one(lambda O, work: O.OracleModel.custom(D, AUX.c_source_aux(family), AUX.oracle_params_aux(X, Y, 4, None, mu, tau), work)))


def grouped_problem(Dx, n):
    """tests/test_gpu_glm_dispersion.test_negative_binomial_with_groups: H = 1, eight one-hot columns beside four ungrouped ones"""
    D = Dx + 2
    grp = HIER.blocks(Dx, 1, 8)
    X, Y, mu, tau = DISP.problem_grouped(n, Dx, grp)
    return dict(D=D, padded=128, form=1, coop=True, block=None, start=lambda C: DISP.start_grouped(C, Dx),
                engine=lambda idhmc: DISP.make(idhmc, NB, X, Y, mu, tau, groups=grp),
                oracle=_one(lambda O, work: O.OracleModel.custom(D, DISP.c_source_disp_hier(NB),
                                                                 HIER.oracle_params_hier(X, Y, 1, grp, None, mu, tau), work)))


def responses_problem(M, R, D, n):
    """M responses of R chains: a 16-chain tile holds chains of several responses; one oracle model per response"""
    family = "BINOMIAL_LOGIT"
    X, Y = responses(family, M, n, D, seed=n + D)
    mu, tau = prior(D)

    def models(O, work):
        first = O.OracleModel.custom(D, FLAT.c_source(family), FLAT.oracle_params(X, Y[0], None, mu, tau), work)
        out = [first]
        for m in range(1, M):
            om = O.OracleModel(3, D)
            om._userlib, om.params = first._userlib, np.ascontiguousarray(FLAT.oracle_params(X, Y[m], None, mu, tau))
            om.c.fn, om.c.params = first.c.fn, om.params.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            out.append(om)
        return out
    return dict(D=D, padded=128, form=1, coop=True, block=R, start=near_origin(D), oracle=models,
                engine=lambda idhmc: idhmc.GLM(X, Y, getattr(idhmc.glm, family), None, mu, tau, chains_per_response=R))


PROBLEMS = {
    "custom128": lambda: custom_problem(40),
    "custom256": lambda: custom_problem(200),
    "dense_coop128": lambda: dense_mvn_problem(40),
    "dense_coop256": lambda: dense_mvn_problem(200),
    "dense_gemv": lambda: dense_mvn_problem(300),
    "logistic_mc128": lambda: logistic_problem(25, 37),
    "logistic_mc256": lambda: logistic_problem(200, 130),
    "logistic_wave": lambda: logistic_problem(300, 37),
    "glm_poisson": lambda: poisson_problem(25, 130),
    "glm_nb128": lambda: negative_binomial_problem(25, 130),
    "glm_nb256": lambda: negative_binomial_problem(200, 130),
    "glm_aux4": lambda: four_auxiliary_problem(20, 300),
    "glm_hier": lambda: grouped_problem(12, 130),
    "glm_responses": lambda: responses_problem(3, 6, 25, 37),
    "limit15_sep": lambda: iso_problem(12),
    "limit15_general": lambda: custom_problem(8),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    return PROBLEMS[name]()


# ---- the cases: name -> dict(C, eps = (lo, hi, period), seed, shared: also run with METRIC_SHARED on the device, tight: the tight
#      min_delta, deep: also at max_depth 12) -----------------------------------------------------------------------------------------------
CASES = {
    "custom128": dict(C=8, eps=(0.0007, 0.35, None), seed=31, shared=False, tight=-0.005, deep=False),
    "custom256": dict(C=8, eps=(0.00035, 0.24, None), seed=31, shared=False, tight=-0.03, deep=False),
    "dense_coop128": dict(C=18, eps=(0.00035, 0.9, None), seed=9, shared=True, tight=-0.005, deep=True),
    "dense_coop256": dict(C=37, eps=(0.0015, 0.9, 16), seed=9, shared=True, tight=-0.01, deep=False),
    "dense_gemv": dict(C=5, eps=(0.00075, 0.4, None), seed=1, shared=False, tight=-0.01, deep=False),
    "logistic_mc128": dict(C=18, eps=(0.00035, 0.6, None), seed=5, shared=True, tight=-0.01, deep=True),
    "logistic_mc256": dict(C=37, eps=(0.0015, 0.6, 16), seed=5, shared=True, tight=-0.005, deep=False),
    "logistic_wave": dict(C=9, eps=(0.00105, 0.42, None), seed=5, shared=False, tight=-0.01, deep=False),
    "glm_poisson": dict(C=18, eps=(0.0004, 0.15, None), seed=5, shared=False, tight=-0.005, deep=False),
    "glm_nb128": dict(C=18, eps=(0.0004, 0.15, None), seed=5, shared=False, tight=-0.005, deep=False),
    "glm_nb256": dict(C=18, eps=(0.0004, 0.21, None), seed=5, shared=False, tight=-0.02, deep=False),
    "glm_aux4": dict(C=18, eps=(0.00014, 0.08, None), seed=8, shared=False, tight=-0.01, deep=False),
    "glm_hier": dict(C=18, eps=(0.0004, 0.21, None), seed=11, shared=False, tight=-0.01, deep=False),
    "glm_responses": dict(C=18, eps=(0.0008, 0.3, 6), seed=5, shared=False, tight=-0.01, deep=False),
    "limit15_sep": dict(C=4, eps=(0.00005, 0.00028, None), seed=9, shared=False, tight=None, deep=False, max_depth=15),
    "limit15_general": dict(C=4, eps=(0.00005, 0.00028, None), seed=31, shared=False, tight=None, deep=False, max_depth=15),
}
DEFAULT_MIN_DELTA = -1000.0


def _runs():
    out = []
    for name, case in CASES.items():
        for md in [case.get("max_depth", 10)] + ([12] if case["deep"] else []):
            out.append((name, md, DEFAULT_MIN_DELTA))
            if case["tight"] is not None:
                out.append((name, md, case["tight"]))
    return out


RUNS = _runs()


def run_id(run):
    name, md, delta = run
    return "%s/%d" % (name, md) + ("" if delta == DEFAULT_MIN_DELTA else "/%g" % delta)


def stepsizes(name):
    case = CASES[name]
    lo, hi, period = case["eps"]
    return ladder(case["C"], lo, hi, period)


_work = []


def workdir():
    """a directory per compiled restatement (OracleModel.custom writes fixed file names), removed when the process ends"""
    d = tempfile.mkdtemp(prefix="deep_trees_")
    if not _work:
        atexit.register(lambda: [shutil.rmtree(w, ignore_errors=True) for w in _work])
    _work.append(d)
    return d


@functools.lru_cache(maxsize=None)
def oracle_models(name):
    from oracle import oracle as O
    return problem(name)["oracle"](O, workdir())


def oracle_chains(name, max_depth, min_delta, nchains=None):
    """the oracle's chains of a case at its start: (chains, start [C][D])"""
    from oracle import oracle as O
    prob, case = problem(name), CASES[name]
    C, D = nchains or case["C"], prob["D"]
    models = oracle_models(name)
    opt = O.default_options(max_depth=max_depth, min_delta=min_delta)
    chains = [O.OracleChain(models[c // prob["block"]] if prob["block"] else models[0], opt, seed=case["seed"], chain_id=c) for c in range(C)]
    q0 = None if prob["start"] is None else prob["start"](C)
    for c, ch in enumerate(chains):
        if q0 is None:
            ch.random_position()
        else:
            ch.set_q(q0[c])
    return chains, np.stack([ch.q[:D].copy() for ch in chains])


@functools.lru_cache(maxsize=None)
def oracle_run(name, max_depth, min_delta):
    """T_SINGLE + T_FUSED transitions of every chain of a case: dict(start [C][D], q [T][C][D], lq [T][C], grad [T][C][D], rec [T][C]);
    computed once (the chains are independent: one thread each), not to be written to"""
    from oracle import oracle as O
    prob, case = problem(name), CASES[name]
    C, D, T = case["C"], prob["D"], T_SINGLE + T_FUSED
    eps = stepsizes(name)
    chains, q0 = oracle_chains(name, max_depth, min_delta)
    out = dict(start=q0, q=np.empty((T, C, D)), lq=np.empty((T, C)), grad=np.empty((T, C, D)), rec=np.zeros((T, C), dtype=O.STATS_DTYPE))

    def one(c):
        ch = chains[c]
        for t in range(T):
            st = ch.sample_tree(float(eps[c]), t + 1)
            out["q"][t, c], out["lq"][t, c], out["grad"][t, c] = ch.q[:D], ch.lq, ch.grad[:D]
            out["rec"][t, c] = (st.pi, st.acceptance_rate, st.term_left, st.term_right, st.depth, st.steps)
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(one, range(C)))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- what a run reaches -------------------------------------------------------------------------------------------------------------------
def reached(run):
    name, max_depth, min_delta = run
    rec = oracle_run(*run)["rec"][:T_SINGLE]
    full = (1 << rec["depth"].astype(np.int64)) - 1
    last = rec["steps"] - full                                       # leaves of the doubling that failed (0: none failed)
    maxd = (rec["term_left"] == 1) & (rec["term_right"] == 0)
    div = rec["term_left"] == rec["term_right"]
    tile = rec["depth"][:, :16]
    return dict(depths=sorted(set(rec["depth"].ravel().tolist())), max_depth=int(maxd.sum()), turn64=int((~maxd & ~div & (last >= 64)).sum()),
                div_inside=int((div & (rec["depth"] >= 4) & (last >= 2)).sum()),
                spread=int((tile.max(axis=1) - tile.min(axis=1)).max()) if problem(name)["coop"] else None)


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_runs_reach_what_they_claim(oracle, run):
    name, max_depth, min_delta = run
    r = reached(run)
    d = r["depths"]
    print("    %-31s %-22s %-10d %-9d %-11d %s" % (run_id(run), " ".join(map(str, d)) if len(d) < 11 else "%d .. %d" % (d[0], d[-1]),
                                                   r["max_depth"], r["turn64"], r["div_inside"], "-" if r["spread"] is None else r["spread"]))
    assert CASES[name]["C"] >= 16 or not problem(name)["coop"]
    assert r["max_depth"] >= 2
    assert r["turn64"] >= 1
    if max_depth == 15:
        assert set(d) >= {13, 14, 15}                                # the arena's last slots: nothing shallower is wanted here
    else:
        assert set(d) >= set(range(3, max_depth + 1)), d
    if min_delta != DEFAULT_MIN_DELTA:
        assert -0.05 <= min_delta <= -0.002 and r["div_inside"] >= 1
    if r["spread"] is not None:
        assert r["spread"] >= 6


# ---- the comparator, pinned where the device is tested ------------------------------------------------------------------------------------
# kind, D, stepsize ladder of the 6 chains, max_depth, min_delta, seed, whether divergences inside trees (depth >= 3) are among the compared
RESTATEMENT_CASES = [("diag", 24, (0.002, 0.5), 10, DEFAULT_MIN_DELTA, 17, False), ("diag", 24, (0.002, 0.5), 10, -0.02, 17, True),
                     ("diag", 10, (0.0005, 0.5), 12, -0.004, 5, True), ("dense", 17, (0.0005, 0.08), 10, DEFAULT_MIN_DELTA, 29, False),
                     ("dense", 17, (0.0005, 0.08), 10, -0.004, 29, True), ("dense", 6, (0.0002, 0.1), 12, -0.02, 3, False)]
# four times the largest deviation measured over RESTATEMENT_CASES (the module docstring)
DRAW_BOUND, PI_BOUND, ACCEPT_BOUND = 4 * 1.37e-15, 4 * 1.42e-15, 4 * 1.07e-14


@pytest.mark.parametrize("kind,D,eps,max_depth,min_delta,seed,diverges", RESTATEMENT_CASES)
def test_two_restatements_build_the_same_deep_trees(oracle, kind, D, eps, max_depth, min_delta, seed, diverges):
    """tests/test_numpy_restatement.test_two_restatements_build_the_same_trees (and its dense sibling) with trees of up to 4095 leaves and
    a min_delta that matters: oracle/numpy_tree.py against the C oracle, same momenta, directions and exponential draws, 6 chains on a
    ladder of stepsizes, 10 transitions each.  Identical records wherever the oracle's smallest decision margin exceeds 1e-9 -- the
    divergence test delta < min_delta counts among the decisions (orc_chain_last_margin) -- and at most one transition in ten skipped
    for it."""
    from oracle import numpy_tree as NT
    from test_numpy_restatement import _momentum, _randexp_stream
    O = oracle
    if kind == "diag":
        mu, sig = np.cos(np.arange(D, dtype=float)), np.logspace(-0.5, 0.5, D)
        tau, minv = 1.0 / sig ** 2, sig ** 2 * np.linspace(0.7, 1.3, D)
        om, density = O.OracleModel.diag(mu, tau), NT.DiagGaussianDensity(mu, tau)
    else:
        rng = np.random.default_rng(seed)
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        P = (Q / np.logspace(-1.5, 0, D)) @ Q.T
        P = 0.5 * (P + P.T)
        mu, minv = np.cos(np.arange(D, dtype=float)), np.linspace(0.02, 0.05, D)
        om, density = O.OracleModel.dense(mu, P), NT.DenseGaussianDensity(mu, P)
    H = NT.Hamiltonian(density, minv)
    C, T = 6, 10
    step = ladder(C, *eps)
    checked = skipped = inside = 0
    depths, dev = set(), np.zeros(3)
    for chain in range(C):
        ch = O.OracleChain(om, O.default_options(max_depth=max_depth, min_delta=min_delta), seed=seed, chain_id=chain)
        ch.set_minv(minv)
        ch.random_position()
        for it in range(1, T + 1):
            q0 = ch.q[:D].copy()
            dirs = O.lib().orc_rand_directions_export(seed, chain, it)
            p = _momentum(O, seed, chain, it, ch.L, D, 1.0 / np.sqrt(minv))
            st_c = ch.sample_tree(float(step[chain]), it)
            q_np, st_np = NT.sample_tree(H, q0, p, float(step[chain]), dirs, _randexp_stream(O, seed, chain, it), max_depth=max_depth,
                                         min_delta=min_delta)
            if ch.last_margin() < 1e-9:
                skipped += 1
                ch.set_q(q_np)
                continue
            checked += 1
            depths.add(st_c.depth)
            inside += st_c.term_left == st_c.term_right and st_c.depth >= 3
            assert (st_c.depth, st_c.steps, st_c.term_left, st_c.term_right) == \
                   (st_np["depth"], st_np["steps"], st_np["term_left"], st_np["term_right"]), (chain, it)
            dev = np.maximum(dev, [np.max(np.abs(ch.q[:D] - q_np) / np.maximum(1.0, np.abs(q_np))),
                                   abs(st_c.pi - st_np["pi"]) / max(1.0, abs(st_np["pi"])), abs(st_c.acceptance_rate - st_np["acceptance_rate"])])
    print("%-5s D = %-3d max_depth %-3d min_delta %-8g compared %d, skipped %d; deviation: draws %.2e   pi %.2e   acceptance rate %.2e" % (
        kind, D, max_depth, min_delta, checked, skipped, *dev))
    assert checked >= 54 and skipped <= 6
    assert max_depth in depths and len(depths) >= 6 and (inside >= 1 or not diverges)
    assert dev[0] <= DRAW_BOUND and dev[1] <= PI_BOUND and dev[2] <= ACCEPT_BOUND
    assert DRAW_BOUND <= 1e-12 and PI_BOUND <= 1e-10 and ACCEPT_BOUND <= 1e-10      # never above what test_numpy_restatement.py asserts
