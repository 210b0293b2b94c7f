"""The NUTS kernel's epilogue reduces every draw on the device: Welford running moments (IDHMC_T_ACCUM_MOMENTS), the E-BFMI running
sums and the 39 + 1024 integer counters (IDHMC_T_ACCUM_DIAG).  This module restates that arithmetic on the host, operation for
operation ("twins": numpy, with the fused multiply-add taken from libm), holds the twins against plain high precision, and fixes the
Gaussian cases that tests/test_gpu_accumulators.py runs on the device -- with the CPU oracle, so that what those cases reach (chains
that stay where they are, every termination, both ends of the acceptance histogram) is checked here and not hoped for there.

Measured on the oracle's draws and records of GAUSSIAN_CASES (test_twins_agree_with_plain_high_precision prints them with -s):

    largest deviation of the twin from the np.longdouble two-pass result
                         mean / max|x|   mean, rtol form   variance, relative   E-BFMI, relative
    diag40               3.16e-16        9.09e-15           2.34e-15            2.63e-14
    diag200              4.68e-16        4.40e-12           3.39e-14            2.02e-14
    diag1024_shared      4.50e-16        2.86e-12           4.72e-15            2.01e-14
    iso300_narrow        3.51e-16        1.62e-12           4.80e-15            6.66e-15
    diag64_few           2.65e-16        4.80e-15           7.10e-16            2.60e-14
    diag640_narrow       4.60e-16        3.03e-11           7.91e-15            1.10e-14

The mean's deviation is taken relative to the largest |draw| of its (chain, coordinate): that is the scale Welford's error bound is
stated in, and a mean can come arbitrarily close to zero (second column: |twin - reference| / |reference|, what an rtol alone would
have to be -- above 1e-12 wherever a mean nearly vanishes, which is why the suite's form carries an atol).  The bounds asserted are four times the largest value of each column
(MEAN_BOUND, VAR_BOUND, EBFMI_BOUND below: Welford's error grows with the condition number of the data and 4x covers a change of
seed), and in addition the forms the suite already asserts elsewhere: rtol 1e-12 / atol 1e-13 for the mean, rtol 1e-10 for the
variance and for E-BFMI.  A (chain, coordinate) whose draws are all equal has mean = that value and variance = 0 exactly; the twin
must return exactly that (the long-double two-pass mean of N equal numbers need not).

    what the oracle's records of each case hold (test_the_gaussian_cases_reach_what_they_claim asserts it)
                         transitions   stayed   max_depth   divergent   turning   depths seen   a == 1   a < 1/1024
    diag40               1110         194      44          97          969       1 2 3 4 5       7        122
    diag200              7200         1473     1027        689         5484      0 1 2 3 4 5 6   47       1039
    diag1024_shared      576          156      126         70          380       0 1 2 3 4 5 6   4        124
    iso300_narrow        1920         517      193         148         1579      0 1 2 3 4 5 6   1        358
    diag64_few           180          61       58          10          112       1 3 4           0        60
    diag640_narrow       576          138      102         71          403       0 1 2 3 4 5 6   4        111
"""
import ctypes
import ctypes.util
import functools
from fractions import Fraction

import numpy as np
import pytest

# ---- the fused multiply-add ----------------------------------------------------------------------------------------------------------
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma_elementwise = np.frompyfunc(_libm.fma, 3, 1)


def fma(a, b, c):
    """a * b + c rounded once (libm), elementwise over float64 arrays"""
    return np.asarray(_fma_elementwise(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)), dtype=np.float64)


def unfused(a, b, c):
    """what fma must not be: the product rounded before the sum (a fault for the sensitivity tests)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)


# ---- the twins -------------------------------------------------------------------------------------------------------------------------
def welford_twin(draws, fused=fma, stale=None, skip_repeats=False):
    """k_nuts, `if (flags & IDHMC_T_ACCUM_MOMENTS)`: draws [N][C][D] -> (mean [C][D], m2 [C][D], n [C]).
    The keyword arguments are faults for the sensitivity tests: another multiply-add; stale = (chain, k): draw k of that chain reads the
    mean that draw k - 1 read (a hand-over that missed the previous transition's store); skip_repeats: a draw equal to the one before it
    is not added."""
    draws = np.asarray(draws, dtype=np.float64)
    N, C, D = draws.shape
    mean, m2, n = np.zeros((C, D)), np.zeros((C, D)), np.zeros(C, dtype=np.int64)
    before = mean.copy()
    for k in range(N):
        q = draws[k]
        live = np.ones(C, dtype=bool)
        if skip_repeats and k > 0:
            live = ~np.all(q.view(np.uint64) == draws[k - 1].view(np.uint64), axis=1)
        seen = mean.copy()
        if stale is not None and stale[1] == k:
            seen[stale[0]] = before[stale[0]]
        before = mean.copy()
        n = n + live
        inv = 1.0 / np.maximum(n, 1).astype(np.float64)[:, None]
        dx = q - seen
        new_mean = fused(dx, inv, seen)
        new_m2 = fused(dx, q - new_mean, m2)
        mean = np.where(live[:, None], new_mean, mean)
        m2 = np.where(live[:, None], new_m2, m2)
    return mean, m2, n


def variance_twin(m2, n):
    """k_moments_get: m2 / (n - 1), 0.0 when n <= 1"""
    nn = np.asarray(n, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(nn > 1.0, m2 / (nn - 1.0), 0.0)


def ebfmi_twin(pi):
    """k_nuts, `if ((flags & IDHMC_T_ACCUM_DIAG) && lane == 0)`: pi [N][C] -> (pi1, prev, s1, s2, d2), each [C]: the sums are taken of
    pi - pi1 (pi1 the first pi of the window) and of pi - prev"""
    pi = np.asarray(pi, dtype=np.float64)
    C = pi.shape[1]
    pi1, prev, s1, s2, d2 = (np.zeros(C) for _ in range(5))
    for k, x in enumerate(pi):
        if k == 0:
            pi1 = x.copy()
        else:
            dl, dp = x - pi1, x - prev
            s1 = s1 + dl
            s2 = fma(dl, dl, s2)
            d2 = fma(dp, dp, d2)
        prev = x.copy()
    return pi1, prev, s1, s2, d2


def ebfmi_from_sums(s1, s2, d2, n):
    """k_ebfmi"""
    n = np.broadcast_to(np.asarray(n, dtype=np.float64), np.shape(s1))
    with np.errstate(divide="ignore", invalid="ignore"):
        var = fma(-(s1 * s1), 1.0 / n, s2) / (n - 1.0)
        return (d2 / (n - 1.0)) / var


def _counters_from_records(idhmc, ts):
    """what the kernel epilogue accumulates, restated in numpy (integers only)"""
    from inplacedhmc_jl_amd import _lib
    ts = np.asarray(ts).ravel()
    cn = np.zeros(_lib.DIAG_COUNTERS, dtype=np.uint64)
    rec = idhmc.xchg_accumulate(idhmc.XCHG_ACCEPT, ts["acceptance_rate"])
    cn[0], cn[1], cn[2] = len(ts), int(rec[0]), int(rec[1])
    maxd = (ts["term_left"] == 1) & (ts["term_right"] == 0)
    div = (ts["term_left"] == ts["term_right"])
    cn[3], cn[4], cn[5] = maxd.sum(), div.sum(), len(ts) - maxd.sum() - div.sum()
    cn[6:39] = np.bincount(np.minimum(ts["depth"], 32), minlength=33)
    bins = np.clip((ts["acceptance_rate"] * 1024).astype(np.int64), 0, 1023)
    cn[39:] = np.bincount(bins, minlength=1024)
    return cn


def twin_accumulators(idhmc, draws, records):
    """everything the accumulators of a context hold after these draws [N][C][D] and records [N][C], in the form of read_accumulators
    of tests/test_gpu_accumulators.py: dict(mean, var, count, counters, ebfmi)"""
    mean, m2, n = welford_twin(draws)
    records = np.asarray(records)
    s = ebfmi_twin(records["pi"])
    return dict(mean=mean, var=variance_twin(m2, n), count=n, counters=_counters_from_records(idhmc, records),
                ebfmi=ebfmi_from_sums(s[2], s[3], s[4], records.shape[0]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_accumulators_equal(got, want, what=""):
    """bit for bit and integer for integer.  (E-BFMI of fewer than two records is 0 / 0: a NaN wherever the other has one -- the sign
    and payload of a NaN are the processor's, not the arithmetic's)"""
    for k in ("mean", "var"):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k].view(np.uint64) != want[k].view(np.uint64))
        assert len(bad) == 0, "%s %s: %d of %d differ, first at (chain, coordinate) %s: %r against %r" % (
            what, k, len(bad), got[k].size, tuple(bad[0]), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    assert np.array_equal(got["count"], want["count"]), (what, "count", got["count"], want["count"])
    bad = np.flatnonzero(got["counters"] != want["counters"])
    assert len(bad) == 0, "%s counters %s: %s against %s" % (what, bad, got["counters"][bad], want["counters"][bad])
    g, w = np.asarray(got["ebfmi"], np.float64), np.asarray(want["ebfmi"], np.float64)
    assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (what, "ebfmi NaN", g, w)
    ok = ~np.isnan(g)
    assert same_bits(g[ok], w[ok]), (what, "ebfmi", g, w)


# ---- the Gaussian cases of tests/test_gpu_accumulators.py ------------------------------------------------------------------------------
# eps: chain c runs at lo * (hi / lo) ** (c / (C - 1)).  The metric is the target's variance times a factor in [0.5, 2), so a unit-scale
# leapfrog is stable below eps = 2 / sqrt(2): the first chains stop at max_depth, the middle ones turn at depths 1 to 5, the last ones
# diverge at once and stay where they are.
GAUSSIAN_CASES = {
    "diag40": dict(kind="diag", D=40, C=37, N=30, max_depth=5, shared=False, eps=(0.15, 1.8), seed=9),
    "diag200": dict(kind="diag", D=200, C=300, N=24, max_depth=6, shared=False, eps=(0.15, 1.8), seed=9),
    "diag1024_shared": dict(kind="diag", D=1024, C=24, N=24, max_depth=6, shared=True, eps=(0.15, 1.8), seed=9),
    "iso300_narrow": dict(kind="iso", D=300, C=64, N=30, max_depth=6, shared=False, eps=(0.2, 2.6), seed=9),
    "diag64_few": dict(kind="diag", D=64, C=3, N=60, max_depth=4, shared=False, eps=(0.15, 1.8), seed=9),
    "diag640_narrow": dict(kind="diag", D=640, C=24, N=24, max_depth=6, shared=False, eps=(0.15, 1.8), seed=9),
}


def gaussian_problem(name):
    """(mu, sigma, minv, eps) of a case: minv of shape (D,) for a shared metric, (C, D) per chain; None for the iso case's unit metric"""
    case = GAUSSIAN_CASES[name]
    D, C = case["D"], case["C"]
    rng = np.random.default_rng(4)
    mu, sig = rng.standard_normal(D), np.exp(rng.standard_normal(D))
    minv = None if case["kind"] == "iso" else sig ** 2 * rng.uniform(0.5, 2.0, D if case["shared"] else (C, D))
    lo, hi = case["eps"]
    return mu, sig, minv, lo * (hi / lo) ** (np.arange(C) / (C - 1.0))


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the CPU oracle's chains of a case: (start [C][D], draws [N][C][D], records [N][C]); computed once, not to be written to"""
    import inplacedhmc_jl_amd as idhmc
    from oracle import oracle as O
    case = GAUSSIAN_CASES[name]
    D, C, N = case["D"], case["C"], case["N"]
    mu, sig, minv, eps = gaussian_problem(name)
    om = O.OracleModel.iso(D) if case["kind"] == "iso" else O.OracleModel.diag(mu, 1.0 / sig ** 2)
    opt = O.default_options(max_depth=case["max_depth"])
    q0, draws, rec = np.empty((C, D)), np.empty((N, C, D)), np.zeros((N, C), dtype=idhmc.TREE_STATS_DTYPE)
    for c in range(C):
        ch = O.OracleChain(om, opt, seed=case["seed"], chain_id=c)
        if minv is not None:
            ch.set_minv(minv if case["shared"] else minv[c])
        ch.random_position()
        q0[c] = ch.q[:D]
        for n in range(N):
            st = ch.sample_tree(float(eps[c]), n + 1)
            draws[n, c] = ch.q[:D]
            rec[n, c] = (st.pi, st.acceptance_rate, st.term_left, st.term_right, st.depth, st.steps)
    for a in (q0, draws, rec):
        a.setflags(write=False)
    return q0, draws, rec


def stayed(start, draws):
    """[N][C]: the transition left the chain where it was (draw n has the bits of draw n - 1; draw 0 those of the start)"""
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    before = np.concatenate([np.ascontiguousarray(start, dtype=np.float64)[None], draws[:-1]])
    return np.all(draws.view(np.uint64) == before.view(np.uint64), axis=2)


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
def _exact_fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _adversarial_triples():
    u = 2.0 ** -53
    tiny, big = 5e-324, 2.0 ** 1023
    t = [
        (1.0 + 2 * u, 1.0 - 2 * u, -1.0),                     # cancellation: the answer is the product's low half, -4 u^2
        (1.0 + 2 * u, 1.0 + 2 * u, -(1.0 + 4 * u)),           # the same, +4 u^2
        (134217729.0, 134217729.0, -18014398777917441.0),     # (2^27 + 1)^2 needs 55 bits; minus its rounded value
        (3.0, 1.0 / 3.0, -1.0),
        (0.1, 10.0, -1.0),
        (1.0 + 2 * u, 1.0 + 2 * u, 2 * u * u),                # a tie of the separately rounded product, broken by the addend
        (1.0 - u, 1.0 - u, 2.0 ** -110),                      # 106-bit product, an addend below its last bit
        (2.0 ** 52 + 1.0, 2.0 ** 52 + 1.0, 1.0),              # 106 bits
        (2.0 ** 52 + 1.0, 2.0 ** 52 - 1.0, -(2.0 ** 104)),
        (tiny, 0.5, tiny), (tiny, 0.75, 0.0), (tiny, 1.5, -tiny), (2.0 ** -537, 2.0 ** -537, tiny),   # subnormal results and ties
        (2.0 ** -1022, 0.5, 2.0 ** -1074), (2.2250738585072014e-308, 1.0 - u, 0.0),
        (2.0 ** -600, 2.0 ** -600, 1.0), (2.0 ** -600, 2.0 ** -600, -tiny),
        (big, 0.5, big * 0.5), (big, 2.0, -big),              # the product alone overflows, the sum does not
        (1e16 + 2.0, 1e-16, -1.0), (-0.0, 5.0, 0.0), (7.0, 0.0, -0.0),
    ]
    rng = np.random.default_rng(1)
    for _ in range(400):                                      # a * b + c with c the negated rounded product: the error of the product
        a, b = rng.standard_normal(2) * 2.0 ** rng.integers(-40, 40)
        t.append((a, b, -(a * b)))
    for _ in range(200):                                      # deep in the subnormals
        a, b, c = rng.standard_normal(3)
        t.append((a * 2.0 ** -540, b * 2.0 ** -540, c * 2.0 ** -1070))
    return t


def test_fma_is_correctly_rounded():
    rng = np.random.default_rng(0)
    tri = [tuple(r) for r in rng.standard_normal((2000, 3)) * 2.0 ** rng.integers(-60, 60, (2000, 3))]
    tri += [(a, b, c * abs(a * b)) for a, b, c in rng.standard_normal((1000, 3))]          # addend of the product's size
    tri += _adversarial_triples()
    a, b, c = (np.array(x) for x in zip(*tri))
    got = fma(a, b, c)
    want = np.array([_exact_fma(*t) for t in tri])
    assert same_bits(got, want)
    # and the adversarial ones are adversarial: rounding the product first gets a good part of them wrong
    adv = len(tri) - len(_adversarial_triples())
    assert np.count_nonzero(unfused(a, b, c)[adv:] != want[adv:]) > 300


def _two_pass(draws):
    """np.longdouble two-pass mean and ddof = 1 variance over the first axis; exact where every draw is the same number"""
    x = np.asarray(draws, dtype=np.longdouble)
    mean = x.sum(axis=0) / x.shape[0]
    var = ((x - mean) ** 2).sum(axis=0) / (x.shape[0] - 1)
    const = np.all(draws == draws[0], axis=0)
    return np.where(const, x[0], mean), np.where(const, np.longdouble(0), var), const


def _ebfmi_longdouble(idhmc, records):
    ts = np.zeros(records.shape, dtype=[("pi", np.longdouble)])
    ts["pi"] = records["pi"]
    return idhmc.EBFMI(ts.T)


# four times the largest value measured over GAUSSIAN_CASES (the module docstring); never above what the suite asserts elsewhere
MEAN_BOUND, VAR_BOUND, EBFMI_BOUND = 4 * 4.68e-16, 4 * 3.39e-14, 4 * 2.63e-14


@pytest.mark.parametrize("name", list(GAUSSIAN_CASES))
def test_twins_agree_with_plain_high_precision(idhmc_cpu, name):
    idhmc = idhmc_cpu
    _, draws, rec = oracle_run(name)
    N = draws.shape[0]
    mean, m2, n = welford_twin(draws)
    var = variance_twin(m2, n)
    assert (n == N).all()
    ref_mean, ref_var, const = _two_pass(draws)
    scale = np.abs(draws).max(axis=0)
    dev_mean = float(np.max(np.abs(mean - ref_mean) / scale))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel_mean = float(np.max(np.where(ref_mean != 0, np.abs(mean - ref_mean) / np.abs(ref_mean), 0)))
        dev_var = float(np.max(np.where(const, 0, np.abs(var - ref_var) / ref_var)))
    assert same_bits(mean[const], draws[0][const]) and np.all(var[const] == 0.0)
    e, e_ref = ebfmi_from_sums(*ebfmi_twin(rec["pi"])[2:], N), _ebfmi_longdouble(idhmc, rec)
    dev_e = float(np.max(np.abs(e - e_ref) / np.abs(e_ref)))
    print("%-16s mean/max|x| %.2e   mean rel %.2e   variance %.2e   E-BFMI %.2e   (%d of %d columns constant)" % (
        name, dev_mean, rel_mean, dev_var, dev_e, const.sum(), const.size))
    assert dev_mean <= MEAN_BOUND and dev_var <= VAR_BOUND and dev_e <= EBFMI_BOUND
    assert MEAN_BOUND <= 1e-12 and VAR_BOUND <= 1e-10 and EBFMI_BOUND <= 1e-10
    assert np.allclose(mean, ref_mean.astype(np.float64), rtol=1e-12, atol=1e-13)
    assert np.allclose(var, ref_var.astype(np.float64), rtol=1e-10, atol=0)
    assert np.allclose(e, e_ref, rtol=1e-10, atol=0)


def _conditions(name):
    q0, draws, rec = oracle_run(name)
    maxd = (rec["term_left"] == 1) & (rec["term_right"] == 0)
    div = rec["term_left"] == rec["term_right"]
    a = rec["acceptance_rate"]
    return dict(transitions=rec.size, stayed=int(stayed(q0, draws).sum()), max_depth=int(maxd.sum()), divergent=int(div.sum()),
                turning=int((~maxd & ~div).sum()), depths=sorted(set(rec["depth"].ravel().tolist())),
                a_one=int((a == 1.0).sum()), a_low=int((a < 1.0 / 1024).sum()))


@pytest.mark.parametrize("name", list(GAUSSIAN_CASES))
def test_the_gaussian_cases_reach_what_they_claim(idhmc_cpu, name):
    c = _conditions(name)
    print("%-16s %s" % (name, c))
    assert c["stayed"] >= 0.05 * c["transitions"]
    assert c["max_depth"] >= 1 and c["divergent"] >= 1 and c["turning"] >= 1
    assert len(c["depths"]) >= 3


def test_both_ends_of_the_acceptance_histogram_occur(idhmc_cpu):
    """a == 1.0 is clamped into bin 1023 (1.0 * 1024 is one past the end), a < 1/1024 falls into bin 0"""
    idhmc = idhmc_cpu
    rec = np.concatenate([oracle_run(name)[2].ravel() for name in GAUSSIAN_CASES])
    a = rec["acceptance_rate"]
    assert (a == 1.0).any() and (a < 1.0 / 1024).any() and a.min() >= 0.0 and a.max() <= 1.0
    cn = _counters_from_records(idhmc, rec)
    assert cn[39 + 1023] >= (a == 1.0).sum() and cn[39] == (a < 1.0 / 1024).sum() and cn[39:].sum() == cn[0] == rec.size


@pytest.fixture(scope="module")
def idhmc_cpu():
    """the package without its native library: the host-side pieces the twins use (dtypes, EBFMI, the exchange records)"""
    import inplacedhmc_jl_amd as pkg
    return pkg


# ---- sensitivity: the comparison fails on each fault a device could have -------------------------------------------------------------------
@pytest.fixture(scope="module")
def diag40(idhmc_cpu):
    q0, draws, rec = oracle_run("diag40")
    return q0, draws, rec, twin_accumulators(idhmc_cpu, draws, rec)


def _with(acc, **kw):
    out = dict(acc)
    out.update(kw)
    return out


def test_the_comparison_accepts_the_twin_itself(idhmc_cpu, diag40):
    _, draws, rec, acc = diag40
    assert_accumulators_equal(twin_accumulators(idhmc_cpu, draws, rec), acc)


def test_a_stale_mean_fails(diag40):
    """one chain, one draw: the mean read is the one the previous transition read (its store not yet visible)"""
    q0, draws, _, acc = diag40
    moved = np.argwhere(~stayed(q0, draws)[2:])            # (a stale mean goes unnoticed only if the chain had not moved)
    k, c = int(moved[0][0]) + 2, int(moved[0][1])
    mean, m2, n = welford_twin(draws, stale=(c, k))
    bad = _with(acc, mean=mean, var=variance_twin(m2, n))
    assert np.count_nonzero(bad["mean"] != acc["mean"]) <= draws.shape[2]          # that chain's row only
    with pytest.raises(AssertionError, match="mean"):
        assert_accumulators_equal(bad, acc)


def test_an_unfused_multiply_add_fails(diag40):
    _, draws, _, acc = diag40
    mean, m2, n = welford_twin(draws, fused=unfused)
    assert np.allclose(mean, acc["mean"], rtol=1e-13, atol=1e-14)                  # invisible to any tolerance the suite had
    with pytest.raises(AssertionError, match="mean"):
        assert_accumulators_equal(_with(acc, mean=mean, var=variance_twin(m2, n)), acc)
    with pytest.raises(AssertionError, match="var"):
        assert_accumulators_equal(_with(acc, var=variance_twin(m2, n)), acc)


def test_a_dropped_workgroup_counter_fails(idhmc_cpu, diag40):
    """the counters reach memory as one atomic add per workgroup and counter: the chains in groups of four (a workgroup's wavefronts),
    one group's addition to one counter lost"""
    _, _, rec, acc = diag40
    groups = [_counters_from_records(idhmc_cpu, rec[:, g:g + 4]) for g in range(0, rec.shape[1], 4)]
    assert_accumulators_equal(_with(acc, counters=np.sum(groups, axis=0, dtype=np.uint64)), acc)
    for index in (0, 2, 4, 6 + 3):                         # the count, the low limb of the acceptance sum, divergences, depth 3
        g = next(i for i, cn in enumerate(groups) if cn[index])
        lost = [cn.copy() for cn in groups]
        lost[g][index] = 0
        with pytest.raises(AssertionError, match="counters"):
            assert_accumulators_equal(_with(acc, counters=np.sum(lost, axis=0, dtype=np.uint64)), acc)


def test_a_skipped_repeated_draw_fails(diag40):
    """a transition that leaves the chain where it was still counts as a draw"""
    q0, draws, _, acc = diag40
    assert stayed(q0, draws)[1:].any()
    mean, m2, n = welford_twin(draws, skip_repeats=True)
    with pytest.raises(AssertionError, match="mean"):
        assert_accumulators_equal(_with(acc, mean=mean, var=variance_twin(m2, n), count=n), acc)
    with pytest.raises(AssertionError, match="count"):
        assert_accumulators_equal(_with(acc, count=n), acc)


# ---- from the counters to the summary (host code of the library) ------------------------------------------------------------------------
def _check_summary_from_counters(idhmc, records):
    got, ref = idhmc.summary_from_counters(_counters_from_records(idhmc, records)), idhmc.summarize_tree_statistics(records)
    assert got.N == ref.N and got.termination_counts == ref.termination_counts and np.array_equal(got.depth_counts, ref.depth_counts)
    assert abs(got.a_mean - ref.a_mean) < 1e-14
    assert np.all(np.abs(got.a_quantiles - ref.a_quantiles) <= 1.0 / 1024 + 1e-12), (got.a_quantiles, ref.a_quantiles)


@pytest.mark.parametrize("name", list(GAUSSIAN_CASES))
def test_summary_from_the_counters_of_each_case(idhmc_cpu, name):
    """acceptance rates that crowd at both ends (chains that diverge at once beside chains that accept everything): a quantile's two
    neighbouring order statistics can lie hundreds of bins apart, and the sample quantile between them"""
    _check_summary_from_counters(idhmc_cpu, oracle_run(name)[2])


@pytest.mark.parametrize("n_low,n_high", [(1, 1), (2, 2), (5, 5), (10, 11), (11, 10), (3, 97), (97, 3), (50, 50)])
def test_quantiles_between_order_statistics_in_different_bins(idhmc_cpu, n_low, n_high):
    idhmc = idhmc_cpu
    rng = np.random.default_rng(n_low + 100 * n_high)
    ts = np.zeros(n_low + n_high, dtype=idhmc.TREE_STATS_DTYPE)
    ts["acceptance_rate"] = rng.permutation(np.r_[rng.uniform(0.0, 0.002, n_low), 1.0 - rng.uniform(0.0, 0.002, n_high)])
    ts["term_left"], ts["term_right"] = -3, 12
    _check_summary_from_counters(idhmc, ts)
