"""The device-side reductions of the NUTS kernel's epilogue -- running moments, the E-BFMI sums, the diagnostics counters -- on every form
of the kernel, and on the path that stores nothing (idhmc_mcmc without host arrays: one idhmc_nuts_transitions launch, where a chain's
accumulators are written by one workgroup and read by another inside the launch).

Every case runs two engines from the same model, seed and start: R ("records", created under IDHMC_FUSE=0) launches once per transition
and stores draws and records; S ("silent") stores nothing.  S must hold what R holds, and both what the host twins of
tests/test_accumulators_cpu.py make of R's draws and records: bit for bit, integer for integer.  The Gaussian cases are the ones the CPU
module runs through the oracle (same draws, same records, asserted here), so what they reach is known; the other models' R is held
against the oracle by their own suites."""
import warnings

import numpy as np
import pytest

import test_glm_dispersion_cpu as DISP
from test_accumulators_cpu import (GAUSSIAN_CASES, assert_accumulators_equal, gaussian_problem, oracle_run, same_bits, stayed,
                                   twin_accumulators)
from test_glm_responses_cpu import responses
from test_gpu_custom import HIP_SRC, PARAMS
from test_gpu_fused import dense_problem
from test_logistic_cpu import problem as logistic_problem

pytestmark = pytest.mark.gpu


def ladder(C, lo, hi, period=None):
    """chain c runs at lo * (hi / lo) ** (k / (n - 1)), k = c (or c modulo period): from short steps whose trees stop at max_depth to
    steps past the stability limit, whose trees diverge at the first leaf and leave the chain where it is"""
    n = period or C
    return lo * (hi / lo) ** ((np.arange(C) % n) / (n - 1.0))


def prior(D, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)


# ---- the cases: name -> dict(model, C, N, opt, eps, start (None: random_position), minv, env, padded, form, shared) ------------------------
def gaussian_case(idhmc, name):
    case = GAUSSIAN_CASES[name]
    mu, sig, minv, eps = gaussian_problem(name)
    D = case["D"]
    model = idhmc.IsoGaussian(D) if case["kind"] == "iso" else idhmc.DiagGaussian(mu, sigma=sig)
    return dict(model=model, C=case["C"], N=case["N"], eps=eps, start=None, minv=minv, seed=case["seed"], shared=case["shared"],
                opt=dict(max_depth=case["max_depth"]), env={},
                padded=(D + 127) // 128 * 128, form=-1)


def dense_case(idhmc, D, C):
    return dict(model=idhmc.DenseMVN(*dense_problem(D)), C=C, N=24, eps=ladder(C, 0.05, 2.5), start=None, minv=None, seed=9, shared=False,
                opt=dict(max_depth=5), env={}, padded=128 if D <= 128 else 256, form=-1)


def logistic_case(idhmc, Dx, n):
    X, y = logistic_problem(n, Dx, seed=n + Dx)
    return dict(model=idhmc.LogisticRegression(X, y, *prior(Dx)), C=18, N=24, eps=ladder(18, 0.03, 4.0), start=None, minv=None, seed=5,
                shared=False, opt=dict(max_depth=5), env={}, padded=128 if Dx <= 128 else 512, form=1 if Dx <= 256 else 0)


def glm_aux_case(idhmc, Dx, n):
    family, C = "NEG_BINOMIAL_LOG_LOGPHI", 18
    X, Y = DISP.problem_disp(family, n, Dx, seed=n + Dx)
    return dict(model=DISP.make(idhmc, family, X, Y, *prior(Dx + 1)), C=C, N=24, eps=ladder(C, 0.01, 2.0), start=DISP.start_disp(family, C, Dx),
                minv=None, seed=5, shared=False, opt=dict(max_depth=5), env={}, padded=128 if Dx < 128 else 512, form=1 if Dx < 256 else 0)


def glm_responses_case(idhmc):
    M, R, D, n = 3, 6, 25, 37
    X, Y = responses("BINOMIAL_LOGIT", M, n, D, seed=n + D)
    start = np.random.default_rng(D).uniform(-0.3, 0.3, (M * R, D)) / np.sqrt(D)
    return dict(model=idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, None, *prior(D), chains_per_response=R), C=M * R, N=24,
                eps=ladder(M * R, 0.02, 3.0, period=R), start=start, minv=None, seed=5, shared=False, opt=dict(max_depth=5), env={},
                padded=128, form=1)


def custom_case(idhmc):
    return dict(model=idhmc.CustomDensity(40, HIP_SRC, PARAMS), C=8, N=24, eps=ladder(8, 0.05, 4.0), start=None, minv=None, seed=31,
                shared=False, opt=dict(max_depth=5), env={}, padded=128, form=-1)


CASES = {name: (lambda idhmc, name=name: gaussian_case(idhmc, name)) for name in GAUSSIAN_CASES}
CASES.update({
    "dense100": lambda idhmc: dense_case(idhmc, 100, 16),
    "dense256": lambda idhmc: dense_case(idhmc, 256, 37),
    "logistic25_matrix_cores": lambda idhmc: logistic_case(idhmc, 25, 37),
    "logistic300_per_wave": lambda idhmc: logistic_case(idhmc, 300, 130),
    "glm_negative_binomial_matrix_cores": lambda idhmc: glm_aux_case(idhmc, 25, 130),
    "glm_negative_binomial_per_wave": lambda idhmc: glm_aux_case(idhmc, 300, 37),
    "glm_three_responses": glm_responses_case,
    "custom_density": custom_case,
})


def create(idhmc, case, first_chain=0, nchains=None):
    """an engine over chains [first_chain, first_chain + nchains) of a case, at its start, stepsizes and metric"""
    C = case["C"] if nchains is None else nchains
    rows = slice(first_chain, first_chain + C)
    opt = dict(case["opt"])
    if case["shared"]:
        opt["metric_mode"] = idhmc.METRIC_SHARED
    eng = idhmc.Engine(case["model"], C, idhmc.default_options(**opt), seed=case["seed"], first_chain=first_chain)
    if case["minv"] is not None:
        eng.set_minv(case["minv"] if case["shared"] else case["minv"][rows])
    if case["start"] is None:
        eng.random_position()
    else:
        eng.set_q(case["start"][rows])
    eng.set_eps(case["eps"][rows])
    return eng


def create_pair(idhmc, case, monkeypatch):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("IDHMC_FUSE", "0")
    R = create(idhmc, case)
    monkeypatch.delenv("IDHMC_FUSE")
    S = create(idhmc, case)
    for k in case["env"]:
        monkeypatch.delenv(k)
    assert R.fused_launch_info() == (True, False) and S.fused_launch_info() == (True, True)
    return R, S


def read_accumulators(eng):
    mean, var, count = eng.moments()
    return dict(mean=mean, var=var, count=count, counters=eng.diag_counters(), ebfmi=eng.ebfmi())


def check_summary(idhmc, eng, records):
    """tree_summary() against summarize_tree_statistics on the records, as tests/test_diagnostics.py has it"""
    dev, ref = eng.tree_summary(), idhmc.summarize_tree_statistics(records)
    assert dev.N == records.size and dev.termination_counts == ref.termination_counts
    assert np.array_equal(dev.depth_counts, ref.depth_counts)
    assert abs(dev.a_mean - ref.a_mean) < 1e-14 and np.all(np.abs(dev.a_quantiles - ref.a_quantiles) <= 1 / 1024 + 1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_silent_fused_sampling_accumulates_what_the_records_hold(idhmc, monkeypatch, name):
    case = CASES[name](idhmc)
    C, N, D = case["C"], case["N"], case["model"].D
    R, S = create_pair(idhmc, case, monkeypatch)
    assert R.padded_dim() == case["padded"] and R.glm_form() == case["form"] and S.glm_form() == case["form"]
    for e in (R, S):
        e.moments_reset()
        e.diag_reset()
    start = R.q
    draws, records = R.mcmc(N, 0)
    none = S.mcmc(N, 0, store_draws=False, store_stats=False)
    assert none == (None, None)
    assert same_bits(S.q, R.q) and same_bits(R.q, draws[-1])
    if name in GAUSSIAN_CASES:                       # the draws whose properties tests/test_accumulators_cpu.py established
        q0, odraws, orec = oracle_run(name)
        assert same_bits(start, q0) and same_bits(draws, odraws) and np.array_equal(records, orec)
    still = stayed(start, draws)
    print("%s: %d of %d transitions left the chain where it was; depths %s" % (name, still.sum(), still.size, np.bincount(records["depth"].ravel())))
    assert still.any() and not still[:, 0].all()     # the top_zeta == 0 branch, and a chain that moves
    twin = twin_accumulators(idhmc, draws, records)
    got_R, got_S = read_accumulators(R), read_accumulators(S)
    assert got_S["mean"].shape == (C, D) and (got_S["count"] == N).all() and got_S["counters"][0] == N * C
    assert_accumulators_equal(got_R, twin, "records engine against the twin:")
    assert_accumulators_equal(got_S, twin, "silent engine against the twin:")
    assert_accumulators_equal(got_S, got_R, "silent engine against records engine:")
    check_summary(idhmc, S, records)
    if name == "glm_three_responses":
        model = case["model"]
        assert S.glm_responses() == (3, 6)
        got = idhmc.rhat_by_response(model, *S.moments())
        want = idhmc.rhat_by_response(model, twin["mean"], twin["var"], twin["count"])
        assert got.shape == (3, D) and np.isfinite(got).all() and same_bits(got, want)
    R.close()
    S.close()


# ---- windows: one small pair (diag40), every step against the twins of R's draws so far ------------------------------------------------------
class Window:
    """R and S of diag40 driven side by side: R keeps the draw and record of every transition, S makes the same transitions through
    whatever entry point the step names"""

    def __init__(self, idhmc, monkeypatch):
        self.idhmc = idhmc
        self.case = gaussian_case(idhmc, "diag40")
        self.R, self.S = create_pair(idhmc, self.case, monkeypatch)
        self.C = self.case["C"]
        self.draws, self.records = [], []             # of R, one [C][D] / [C] per transition

    def advance(self, n, silent, flags, stored_mcmc=False):
        """n more transitions.  R: mcmc(n) with host arrays, or n flagged launches read back one by one; S: silent(S, number of the
        first transition, n)"""
        it = len(self.draws)
        if stored_mcmc:
            draws, records = self.R.mcmc(n, it)
            self.draws += list(draws)
            self.records += list(records)
        else:
            for k in range(n):
                self.R.nuts_transition(it + 1 + k, flags)
                self.draws.append(self.R.q)
                self.records.append(self.R.tree_stats())
        silent(self.S, it + 1, n)
        assert same_bits(self.S.q, self.R.q) and same_bits(self.R.q, self.draws[-1])

    def twin(self, moments_from=0, diag_from=0):
        """the accumulators after R's transitions [moments_from, now) and [diag_from, now)"""
        idhmc = self.idhmc
        m = twin_accumulators(idhmc, np.stack(self.draws[moments_from:]), np.stack(self.records[moments_from:]))
        d = m if diag_from == moments_from else twin_accumulators(idhmc, np.stack(self.draws[diag_from:]), np.stack(self.records[diag_from:]))
        return dict(mean=m["mean"], var=m["var"], count=m["count"], counters=d["counters"], ebfmi=d["ebfmi"])

    def check(self, what, **kw):
        want = self.twin(**kw)
        assert_accumulators_equal(read_accumulators(self.R), want, what + ", records engine:")
        assert_accumulators_equal(read_accumulators(self.S), want, what + ", silent engine:")

    def close(self):
        self.R.close()
        self.S.close()


def test_counts_continue_across_calls_and_entry_points(idhmc, monkeypatch):
    """mcmc(10), mcmc(1) (the per-transition loop even with fusing on), five nuts_transition(flags), nuts_transitions(7, flags): one
    window of 23 draws"""
    w = Window(idhmc, monkeypatch)
    fl = idhmc.T_ACCUM_MOMENTS | idhmc.T_ACCUM_DIAG
    for e in (w.R, w.S):
        e.moments_reset()
        e.diag_reset()
    mcmc = lambda S, it, n: S.mcmc(n, it - 1, store_draws=False, store_stats=False)
    w.advance(10, mcmc, fl, stored_mcmc=True)
    w.check("mcmc(10)")
    w.advance(1, mcmc, fl, stored_mcmc=True)
    w.check("mcmc(10), mcmc(1)")

    def singles(S, it, n):
        for k in range(n):
            S.nuts_transition(it + k, fl)
    w.advance(5, singles, fl)
    w.check("... five nuts_transition")
    w.advance(7, lambda S, it, n: S.nuts_transitions(it, n, fl), fl)
    w.check("... nuts_transitions(7)")
    for e in (w.R, w.S):
        mean, var, count = e.moments()
        assert (count == 23).all() and e.diag_counters()[0] == 23 * w.C and e.tree_summary().N == 23 * w.C
    # transitions without the flags leave the window alone
    before = read_accumulators(w.S)
    w.S.nuts_transitions(24, 3)
    assert_accumulators_equal(read_accumulators(w.S), before, "unflagged transitions:")
    w.close()


@pytest.mark.parametrize("fused", [False, True])
def test_a_flag_before_any_reset_starts_a_window(idhmc, monkeypatch, fused):
    """no moments_reset / diag_reset: the first flagged launch allocates and zeroes the accumulators itself"""
    case = gaussian_case(idhmc, "diag40")
    fl = idhmc.T_ACCUM_MOMENTS | idhmc.T_ACCUM_DIAG
    eng = create(idhmc, case)
    with pytest.raises(idhmc.IdhmcError):
        eng.moments()
    with pytest.raises(idhmc.IdhmcError):
        eng.diag_counters()
    eng.nuts_transition(1)                           # (unflagged: still nothing to read)
    with pytest.raises(idhmc.IdhmcError):
        eng.ebfmi()
    n = 6
    if fused:
        eng.nuts_transitions(2, n, fl)
    else:
        for it in range(2, 2 + n):
            eng.nuts_transition(it, fl)
    _, draws, records = oracle_run("diag40")
    assert same_bits(eng.q, draws[n])
    assert_accumulators_equal(read_accumulators(eng), twin_accumulators(idhmc, draws[1:1 + n], records[1:1 + n]), "implicit reset:")
    eng.close()


def test_first_draws(idhmc, monkeypatch):
    """After moments_reset(): count 0, mean 0, variance 0.  After one draw: the mean is the draw, the variance exactly 0.0.
    ebfmi() with 0 and with 1 accumulated transitions returns NaN for every chain (k_ebfmi: 0 * inf and 0 / 0), as idhmc.EBFMI does on one
    record (numpy: the mean of no differences over the variance of one number) -- also in a window opened by diag_reset() on a context
    whose sums are no longer zero."""
    case = gaussian_case(idhmc, "diag40")
    C, D = case["C"], case["model"].D
    fl = idhmc.T_ACCUM_MOMENTS | idhmc.T_ACCUM_DIAG
    eng = create(idhmc, case)
    for window in range(2):
        eng.moments_reset()
        eng.diag_reset()
        mean, var, count = eng.moments()
        assert mean.shape == (C, D) and not mean.any() and not var.any() and not count.any()
        assert not eng.diag_counters().any() and eng.tree_summary().N == 0
        e0 = eng.ebfmi()
        assert e0.shape == (C,) and np.isnan(e0).all(), e0
        eng.nuts_transition(1 + 4 * window, fl)
        mean, var, count = eng.moments()
        assert same_bits(mean, eng.q) and same_bits(var, np.zeros((C, D))) and (count == 1).all()
        record = eng.tree_stats()
        assert eng.diag_counters()[0] == C and np.isnan(eng.ebfmi()).all()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                      # (numpy says so too: mean of an empty slice)
            assert np.isnan(idhmc.EBFMI(record[:, None])).all()
        eng.nuts_transitions(2 + 4 * window, 3, fl)              # (leaves sums behind for the second window)
        assert np.isfinite(eng.ebfmi()).all()
    eng.close()


def test_resets_are_independent(idhmc, monkeypatch):
    w = Window(idhmc, monkeypatch)
    fl = idhmc.T_ACCUM_MOMENTS | idhmc.T_ACCUM_DIAG
    fused = lambda S, it, n: S.nuts_transitions(it, n, fl)
    for e in (w.R, w.S):
        e.moments_reset()
        e.diag_reset()
    w.advance(6, fused, fl)
    w.check("six transitions")
    for e in (w.R, w.S):
        diag = (e.diag_counters(), e.ebfmi())
        e.moments_reset()
        mean, var, count = e.moments()
        assert not mean.any() and not var.any() and not count.any()
        assert np.array_equal(e.diag_counters(), diag[0]) and same_bits(e.ebfmi(), diag[1])
    w.advance(5, fused, fl)
    w.check("moments reset after six, five more", moments_from=6, diag_from=0)
    for e in (w.R, w.S):
        moments = e.moments()
        e.diag_reset()
        assert not e.diag_counters().any()
        after = e.moments()
        assert same_bits(after[0], moments[0]) and same_bits(after[1], moments[1]) and np.array_equal(after[2], moments[2])
    w.advance(4, lambda S, it, n: S.mcmc(n, it - 1, store_draws=False, store_stats=False), fl)
    w.check("diagnostics reset after eleven, four more", moments_from=6, diag_from=11)
    w.close()


def test_shards_hold_the_rows_of_the_full_context(idhmc, monkeypatch):
    """contexts over chains [0, 13), [13, 24), [24, 37) against the one over [0, 37): the same moments and E-BFMI row for row, counters
    that add up"""
    case = gaussian_case(idhmc, "diag40")
    N = case["N"]
    bounds = [0, 13, 24, 37]
    full = create(idhmc, case)
    shards = [create(idhmc, case, first_chain=a, nchains=b - a) for a, b in zip(bounds, bounds[1:])]
    for e in [full] + shards:
        e.moments_reset()
        e.diag_reset()
        e.mcmc(N, 0, store_draws=False, store_stats=False)
    want = read_accumulators(full)
    _, draws, records = oracle_run("diag40")
    assert_accumulators_equal(want, twin_accumulators(idhmc, draws, records), "full context:")
    parts = [read_accumulators(e) for e in shards]
    joined = {k: np.concatenate([p[k] for p in parts]) for k in ("mean", "var", "count", "ebfmi")}
    joined["counters"] = np.sum([p["counters"] for p in parts], axis=0, dtype=np.uint64)
    assert_accumulators_equal(joined, want, "shards against the full context:")
    assert same_bits(np.concatenate([e.q for e in shards]), full.q)
    check_summary(idhmc, full, records)
    assert full.tree_summary(joined["counters"]).termination_counts == full.tree_summary().termination_counts
    for e in [full] + shards:
        e.close()
