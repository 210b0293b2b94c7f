"""Posterior summaries reduced on the device (include/idhmc.h "posterior summaries") against the host twins of
tests/test_summary_cpu.py: integers as integers, doubles bit for bit, unless a test says otherwise.  The twins are held against plain
high precision there; here the device must be the twins.

  1  segments and persistence (idhmc_summary_add_draws: 515 chains in one group = two full segments and a partial one, D = 5, two calls)
  2  several groups (35 chains in groups of 7, D = 130)
  3  binning: an explicit range with values on every edge, the range from the moments, lo == hi, bins = 256
  4  sampling with a per-chain metric: the summary of an engine that stores nothing is the twin of the draws another engine stored --
     fused blocks (64 + 6), one launch per transition (IDHMC_FUSE=0), and draws and summary together
  5  the same with a shared metric at D = 300
  6  a negative-binomial GLM with coefficient groups and responses: theta = [beta | a | sigma]
  7  Engine.mcmc_summary: the pilot counts in the moments, not in the histogram
  8  refusals and lifecycle
"""
import ctypes as C

import numpy as np
import pytest

from test_summary_cpu import bits, counts_twin, inv_w_twin, range_twin, summary_twin, theta_twin

pytestmark = pytest.mark.gpu

FIELDS = ("mean", "var", "min", "max")


def assert_summary(got, want, what=""):
    """got: PosteriorSummary, want: summary_twin's dict"""
    assert np.array_equal(got.n, want["n"]), (what, "n", got.n, want["n"])
    assert np.array_equal(got.pos, want["pos"]), (what, "pos")
    for k in FIELDS:
        g, w = getattr(got, k), want[k]
        bad = np.argwhere(bits(g) != bits(w))
        assert g.shape == w.shape and len(bad) == 0, "%s %s: %d of %d differ, first at (group, d) %s: %r against %r" % (
            what, k, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


def assert_histogram(got, theta, G, lo, hi, what=""):
    """the ranges' bits, inv_w's, and the counts of theta [N][C][D] binned with them"""
    bins = got.bins
    iw = inv_w_twin(lo, hi, bins)
    for k, w in (("lo", lo), ("hi", hi), ("inv_w", iw)):
        assert np.array_equal(bits(getattr(got, k)), bits(w)), (what, k)
    want = counts_twin(theta, G, lo, hi, iw, bins)
    assert got.counts.dtype == np.uint32 and np.array_equal(got.counts, want), (what, "counts", np.argwhere(got.counts != want)[:4])
    assert np.all(got.binned == theta.shape[0] * G) and np.all(got.counts.sum(axis=-1, dtype=np.int64) == theta.shape[0] * G)


def gaussian_engine(idhmc, D, Cn, **kw):
    rng = np.random.default_rng(4)
    return idhmc.Engine(idhmc.DiagGaussian(rng.standard_normal(D), np.exp(rng.standard_normal(D))), Cn, idhmc.default_options(max_depth=5), **kw)


# ---- 1, 2: add_draws ---------------------------------------------------------------------------------------------------------------------
def test_segments_and_persistence(idhmc):
    Cn, D = 515, 5
    rng = np.random.default_rng(1)
    draws = rng.standard_normal((5, Cn, D))
    draws[:, :, 1] = np.where(rng.random((5, Cn)) < 0.5, 0.0, -0.0)          # neither zero counts as positive
    draws[:, :, 2] = -3.25                                                   # a column of equal values
    draws[:, :, 3] = 1e8 + rng.standard_normal((5, Cn))
    eng = gaussian_engine(idhmc, D, Cn)
    eng.summary_begin(bins=0)
    assert eng.summary_dims() == (1, Cn, D, 0)
    eng.summary_add_draws(draws[:3])
    assert_summary(eng.summary(), summary_twin(draws[:3], Cn), "first call")
    eng.summary_add_draws(draws[3:])                                        # the state persists across calls
    got, want = eng.summary(), summary_twin(draws, Cn)
    assert_summary(got, want, "second call")
    assert got.n[0] == 5 * Cn and got.pos[0, 1] == 0 and got.counts is None and np.all(got.binned == 0)
    assert bits(got.mean)[0, 2] == bits(-3.25) and bits(got.var)[0, 2] == bits(0.0)
    assert np.all(got.p_positive[0, 3] == 1.0)
    eng.summary_begin(bins=0)                                               # begin again: a fresh summary
    eng.summary_add_draws(draws[3:])
    assert_summary(eng.summary(), summary_twin(draws[3:], Cn), "reopened")
    eng.close()


def test_several_groups(idhmc):
    Cn, G, D = 35, 7, 130
    rng = np.random.default_rng(2)
    draws = rng.standard_normal((4, Cn, D)) * np.logspace(-3, 3, D) + rng.standard_normal(D)
    eng = gaussian_engine(idhmc, D, Cn, first_chain=70)                     # a multiple of 7
    eng.summary_begin(chains_per_group=G, bins=0)
    assert eng.summary_dims() == (5, G, D, 0)
    eng.summary_add_draws(draws)
    assert_summary(eng.summary(), summary_twin(draws, G))
    eng.close()


# ---- 3: binning ---------------------------------------------------------------------------------------------------------------------------
def test_binning(idhmc):
    Cn, G, D, bins = 520, 260, 3, 16                                        # two groups of two segments: the flush uses atomics
    rng = np.random.default_rng(3)
    lo = np.array([[-1.0, 0.0, 2.0], [-1.0, -8.0, 2.0]])
    hi = np.array([[1.0, 4.0, 2.0], [1.0, 8.0, 2.5]])                       # (group 0, d 2): lo == hi
    draws = rng.uniform(-1.5, 1.5, (3, Cn, D))
    edges = -1.0 + np.arange(17) / 8.0                                      # lo, every interior edge, hi: exact in binary
    special = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [-7.0, 7.0, 0.0, -0.0]])
    draws[0, :len(special), 0] = special
    draws[1, Cn - len(special):, 0] = special[::-1]
    draws[:, :, 1] = rng.uniform(-9.0, 9.0, (3, Cn))
    draws[:, :, 2] = np.where(rng.random((3, Cn)) < 0.3, 2.0, rng.uniform(1.5, 3.0, (3, Cn)))
    eng = gaussian_engine(idhmc, D, Cn)
    eng.summary_begin(chains_per_group=G, bins=bins)
    eng.summary_add_draws(draws[:1])                                        # no range yet: counted in the moments, not binned
    first = eng.summary()
    assert np.all(first.binned == 0) and not first.counts.any() and np.all(first.n == G)
    eng.summary_set_range(lo, hi)
    eng.summary_add_draws(draws[1:])
    got = eng.summary()
    assert_summary(got, summary_twin(draws, G), "explicit range")
    assert_histogram(got, draws[1:], G, lo, hi, "explicit range")
    assert got.inv_w[0, 2] == 0.0 and got.counts[0, 2, 1:bins + 1].sum() == 0
    # the range from the moments: the histogram starts again, the moments stay
    const = np.full((1, Cn, D), 0.5)
    eng.summary_begin(chains_per_group=G, bins=bins)
    more = draws.copy()
    more[:, :G, 1] = 0.5                                                    # group 0, d 1: a constant column gives lo == hi
    eng.summary_add_draws(more[:2])
    eng.summary_set_range(span=2.0)
    s = summary_twin(more[:2], G)
    lo2, hi2, _ = range_twin(s["mean"], s["var"], 2.0, bins)
    assert bits(lo2)[0, 1] == bits(hi2)[0, 1] == bits(0.5)
    eng.summary_add_draws(more[2:])
    eng.summary_add_draws(const)
    got = eng.summary()
    assert_summary(got, summary_twin(np.concatenate([more, const]), G), "range from the moments")
    assert_histogram(got, np.concatenate([more[2:], const]), G, lo2, hi2, "range from the moments")
    eng.summary_set_range(span=6.0)                                         # set again: zeroed
    again = eng.summary()
    assert np.all(again.binned == 0) and not again.counts.any() and np.all(again.n == 4 * G)
    eng.close()


def test_bins_256_and_one_segment_per_group(idhmc):
    Cn, G, D, bins = 48, 16, 70, 256                                        # one segment per group: the flush uses plain adds
    rng = np.random.default_rng(5)
    draws = rng.standard_normal((6, Cn, D)) * np.logspace(-2, 2, D)
    eng = gaussian_engine(idhmc, D, Cn)
    eng.summary_begin(chains_per_group=G, bins=bins)
    eng.summary_add_draws(draws[:2])
    eng.summary_set_range(span=1.5)                                         # narrow: both end bins fill
    s = summary_twin(draws[:2], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 1.5, bins)
    eng.summary_add_draws(draws[2:4])
    eng.summary_add_draws(draws[4:])                                        # the table persists across calls
    got = eng.summary()
    assert_summary(got, summary_twin(draws, G))
    assert_histogram(got, draws[2:], G, lo, hi)
    assert got.counts[:, :, 0].sum() > Cn and got.counts[:, :, -1].sum() > Cn          # about 1 / 15 of 4 x 48 x 70 each
    eng.close()


# ---- 4, 5: sampling -----------------------------------------------------------------------------------------------------------------------
def sampling_engine(idhmc, D, shared, summary):
    Cn = 64
    eng = gaussian_engine(idhmc, D, Cn, seed=9)
    rng = np.random.default_rng(D)
    eng.set_minv(rng.uniform(0.5, 2.0, D if shared else (Cn, D)))
    eng.random_position()
    eng.set_eps(0.2)
    if summary:
        eng.summary_begin(chains_per_group=16, bins=32)
        lo, hi = np.full((4, D), -3.0), np.full((4, D), 3.0)
        eng.summary_set_range(lo, hi)
    return eng


@pytest.mark.parametrize("D,shared", [(40, False), (300, True)])
def test_sampling(idhmc, monkeypatch, D, shared):
    N, G = 70, 16                                                           # one full block of 64 transitions, then a partial one of 6
    monkeypatch.delenv("IDHMC_FUSE", raising=False)
    R = sampling_engine(idhmc, D, shared, False)
    draws, _ = R.mcmc(N, 0, store_draws=True, store_stats=False)
    want = summary_twin(draws, G)
    lo, hi = np.full((4, D), -3.0), np.full((4, D), 3.0)

    S = sampling_engine(idhmc, D, shared, True)                             # no host arrays
    assert S.fused_launch_info() == (True, True)
    S.mcmc(N, 0, store_draws=False, store_stats=False)
    got = S.summary()
    assert_summary(got, want, "fused blocks")
    assert_histogram(got, draws, G, lo, hi, "fused blocks")
    assert np.array_equal(bits(S.q), bits(R.q))
    S.close()

    monkeypatch.setenv("IDHMC_FUSE", "0")                                   # the per-transition pack path
    P = sampling_engine(idhmc, D, shared, True)
    monkeypatch.delenv("IDHMC_FUSE")
    assert P.fused_launch_info() == (True, False)
    P.mcmc(N, 0, store_draws=False, store_stats=False)
    got = P.summary()
    assert_summary(got, want, "per transition")
    assert_histogram(got, draws, G, lo, hi, "per transition")
    assert np.array_equal(bits(P.q), bits(R.q))
    P.close()

    B = sampling_engine(idhmc, D, shared, True)                             # draws, records and the summary together
    both, stats = B.mcmc(N, 0, store_draws=True, store_stats=True)
    assert np.array_equal(bits(both), bits(draws)) and (stats["steps"] >= 1).all()
    got = B.summary()
    assert_summary(got, want, "with host arrays")
    assert_histogram(got, draws, G, lo, hi, "with host arrays")
    # the warm-up drivers never feed it
    B.tuning_stage(3, False, N, store_draws=False, store_stats=False)
    assert np.array_equal(B.summary().n, got.n)
    B.close()
    R.close()


# ---- 6: a GLM with coefficient groups and responses --------------------------------------------------------------------------------------------
def test_glm_with_groups_and_responses(idhmc, oracle):
    from test_gpu_glm_pooling import HierCase
    case = HierCase(idhmc)                                                  # NEG_BINOMIAL_LOG_LOGPHI, H = 2, (Dx, n) = (24, 130), M = 3, R = 6
    M, Rr, Dx, N = case.M, case.R, case.Dx, 9
    model = case.full
    assert (model.Dx, model.A, model.H) == (Dx, 1, 2)

    S = idhmc.Engine(model, M * Rr, idhmc.default_options(max_depth=4), seed=case.seed)
    S.set_eps(0.02)
    S.set_q(case.q0)
    draws, _ = S.mcmc(N, 0, store_draws=True, store_stats=False)           # today's path; then the same transitions again (one engine:
    S.set_q(case.q0)                                                        # the run-time build of the density is most of this test's time)
    S.summary_begin(bins=16)                                                # the default group: the chains of a response
    assert S.summary_dims() == (M, Rr, Dx + 3, 16)
    S.mcmc(2, 0, store_draws=False, store_stats=False)
    S.summary_set_range(span=3.0)
    S.mcmc(N - 2, 2, store_draws=False, store_stats=False)
    got = S.summary()
    S.close()
    theta = theta_twin(draws, Dx, 1, 2, np.asarray(model.groups), oracle.lib().orc_exp_export)
    assert_summary(got, summary_twin(theta, Rr))
    s = summary_twin(theta[:2], Rr)
    lo, hi, _ = range_twin(s["mean"], s["var"], 3.0, 16)
    assert_histogram(got, theta[2:], Rr, lo, hi)
    # ... and theta is what the package's own helpers make of the stored draws (libm's exp: not the same bits)
    by = draws.reshape(N, M, Rr, Dx + 3).transpose(1, 0, 2, 3).reshape(M, N * Rr, Dx + 3)
    beta, sigma = idhmc.glm.coefficients(model, by), idhmc.glm.group_scales(model, by)
    assert np.allclose(got.mean[:, :Dx], beta.mean(axis=1), rtol=1e-12, atol=1e-12)
    assert np.allclose(got.mean[:, Dx + 1:], sigma.mean(axis=1), rtol=1e-12, atol=1e-12)
    assert np.allclose(got.mean[:, Dx], by[:, :, Dx].mean(axis=1), rtol=1e-12, atol=1e-12)
    assert np.array_equal(got.pos[:, :Dx], (beta > 0).sum(axis=1)) and np.all(got.pos[:, Dx + 1:] == N * Rr)


# ---- 7: the convenience ------------------------------------------------------------------------------------------------------------------------
def test_mcmc_summary(idhmc):
    from test_glm_responses_cpu import responses
    M, Rr, D, n, N, pilot = 4, 8, 10, 60, 12, 5
    X, Y = responses("BERNOULLI_LOGIT", M, n, D, seed=9)
    model = idhmc.GLM(X, Y, idhmc.glm.BERNOULLI_LOGIT, chains_per_response=Rr)

    eng = idhmc.Engine(model, M * Rr, idhmc.default_options(max_depth=5), seed=5)
    eng.random_position()
    q0 = 0.1 * eng.q
    eng.set_eps(0.1)
    eng.set_q(q0)
    draws, _ = eng.mcmc(N, 3, store_draws=True, store_stats=False)
    eng.set_q(q0)                                                           # the same transitions again, nothing stored
    got = eng.mcmc_summary(N, 3, pilot=pilot, bins=64)
    assert got.chains_per_group == Rr and np.all(got.n == N * Rr) and np.all(got.binned == (N - pilot) * Rr)
    assert np.all(got.counts.sum(axis=-1, dtype=np.int64) == (N - pilot) * Rr)
    assert_summary(got, summary_twin(draws, Rr))
    s = summary_twin(draws[:pilot], Rr)
    lo, hi, _ = range_twin(s["mean"], s["var"], 6.0, 64)
    assert_histogram(got, draws[pilot:], Rr, lo, hi)
    with pytest.raises(idhmc.IdhmcError):                                   # mcmc_summary ends its summary
        eng.summary()
    # the default pilot: the smallest count with pilot * chains_per_group >= 256, at least 2, at most N // 2
    assert np.all(eng.mcmc_summary(100, 0, bins=8).binned == (100 - 32) * Rr)
    assert np.all(eng.mcmc_summary(12, 0, bins=8).binned == 6 * Rr)
    assert np.all(eng.mcmc_summary(20, 0, chains_per_group=32, bins=8).binned == (20 - 8) * 32)
    none = eng.mcmc_summary(4, 0, bins=0)
    assert none.counts is None and np.all(none.n == 4 * Rr)
    eng.close()


# ---- 8: refusals and lifecycle -----------------------------------------------------------------------------------------------------------------
def refused(idhmc, call, *needles):
    with pytest.raises(idhmc.IdhmcError) as e:
        call()
    assert e.value.code == idhmc.ERR_BAD_ARG, str(e.value)
    for s in needles:
        assert s in str(e.value), str(e.value)


def test_refusals(idhmc):
    D = 6
    eng = gaussian_engine(idhmc, D, 35)
    one = np.zeros((1, 35, D))
    refused(idhmc, eng.summary, "no summary is open")
    refused(idhmc, eng.summary_set_range, "no summary is open")
    refused(idhmc, lambda: eng.summary_set_range(np.zeros(D), np.ones(D)), "no summary is open")
    refused(idhmc, lambda: eng.summary_add_draws(one), "no summary is open")
    refused(idhmc, eng.summary_dims, "no summary is open")
    eng.summary_end()                                                       # nothing open: nothing to do
    refused(idhmc, lambda: eng.summary_begin(chains_per_group=4), "chains_per_group = 4", "nchains = 35")
    refused(idhmc, lambda: eng.summary_begin(chains_per_group=-7), "-7")
    refused(idhmc, lambda: eng.summary_begin(bins=-1), "bins = -1")
    refused(idhmc, lambda: eng.summary_begin(bins=257), "bins = 257")
    eng.summary_begin(chains_per_group=7, bins=0)
    refused(idhmc, eng.summary_set_range, "bins = 0")
    eng.summary_begin(chains_per_group=1, bins=8)
    refused(idhmc, eng.summary_set_range, "two values", "holds 0")
    eng.summary_add_draws(one)
    refused(idhmc, eng.summary_set_range, "two values", "holds 1")           # one chain per group: one transition is one value
    eng.summary_add_draws(one)
    eng.summary_set_range()
    lo, hi = np.zeros((35, D)), np.ones((35, D))
    for bad_lo, bad_hi, needle in ((np.nan, 1.0, "nan"), (0.0, np.inf, "inf"), (2.5, 1.0, "2.5")):
        l, h = lo.copy(), hi.copy()
        l[3, 2], h[3, 2] = bad_lo, bad_hi
        refused(idhmc, lambda: eng.summary_set_range(l, h), needle, "group 3, parameter 2")
    refused(idhmc, lambda: eng.summary_set_range(span=np.nan), "span")
    with pytest.raises(ValueError):
        eng.summary_set_range(lo[:3], hi[:3])
    with pytest.raises(ValueError):
        eng.summary_add_draws(np.zeros((2, 34, D)))
    lib = idhmc.load_library()
    dp = C.POINTER(C.c_double)
    assert lib.idhmc_summary_add_draws(eng.h, one.ctypes.data_as(dp), 0) == idhmc.ERR_BAD_ARG and b"cnt = 0" in lib.idhmc_last_error()
    eng.close()
    shifted = gaussian_engine(idhmc, D, 14, first_chain=3)
    refused(idhmc, lambda: shifted.summary_begin(chains_per_group=7), "first_chain_id = 3")
    shifted.close()


def test_count_overflow_and_table_bound_are_refused_before_anything_runs(idhmc):
    eng = gaussian_engine(idhmc, 4, 515)
    eng.summary_begin(bins=4)                                               # one group of 515 chains
    draws = np.zeros((2, 515, 4))
    eng.summary_add_draws(draws)
    lib = idhmc.load_library()
    dp = C.POINTER(C.c_double)
    room = (2 ** 32 - 1) // 515                                             # transitions a group's uint32 count can hold
    eng.summary_set_range(np.zeros((1, 4)), np.ones((1, 4)))
    eng.summary_add_draws(draws)
    # (cnt is checked before a single draw is read: the array holds two)
    assert lib.idhmc_summary_add_draws(eng.h, draws.ctypes.data_as(dp), room - 1) == idhmc.ERR_BAD_ARG
    msg = lib.idhmc_last_error()
    assert b"2^32 - 1" in msg and b"%d more transitions" % (room - 1) in msg and b"(1030 now)" in msg
    refused(idhmc, lambda: eng.mcmc(2 ** 31 - 1, 0, store_draws=False, store_stats=False), "2^32 - 1")
    assert np.all(eng.summary().binned == 2 * 515)                          # neither call changed anything
    eng.close()
    big = gaussian_engine(idhmc, 1000, 2100)
    refused(idhmc, lambda: big.summary_begin(chains_per_group=1, bins=256), "2167200000 bytes", "2 GiB")
    big.summary_begin(chains_per_group=1, bins=128)                         # 1.09e9 bytes: accepted
    big.summary_end()
    big.close()


def test_a_failed_mcmc_invalidates_the_summary(idhmc, monkeypatch):
    from test_gpu_status import arm_underflow, underflow_engine
    monkeypatch.delenv("IDHMC_FUSE", raising=False)
    eng = underflow_engine(idhmc)
    eng.summary_begin(bins=8)
    code = arm_underflow(idhmc, eng)                                        # the caller's own transitions do not feed the summary
    with pytest.raises(idhmc.IdhmcError) as e:
        eng.mcmc(3, 100, store_draws=False, store_stats=False)
    assert e.value.code == code
    refused(idhmc, eng.summary, "invalid", "idhmc_summary_begin again")
    refused(idhmc, eng.summary_set_range, "invalid")
    eng.summary_begin(bins=8)                                               # begin again: usable
    eng.mcmc(3, 100, store_draws=False, store_stats=False)
    assert np.all(eng.summary().n == 3 * eng.C)
    eng.close()


def test_after_summary_end_the_silent_path_is_what_it_was(idhmc, monkeypatch):
    monkeypatch.delenv("IDHMC_FUSE", raising=False)
    a, b = sampling_engine(idhmc, 40, False, True), sampling_engine(idhmc, 40, False, False)
    a.mcmc(5, 0, store_draws=False, store_stats=False)
    a.summary_end()
    b.mcmc(5, 0, store_draws=False, store_stats=False)
    for e in (a, b):
        assert e.fused_launch_info() == (True, True)
        e.mcmc(7, 5, store_draws=False, store_stats=False)
    assert np.array_equal(bits(a.q), bits(b.q)) and np.array_equal(bits(a.lq), bits(b.lq))
    assert a.total_steps() == b.total_steps()
    a.close()
    b.close()
