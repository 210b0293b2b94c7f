"""Posterior summaries (include/idhmc.h "posterior summaries") restated on the host, operation for operation: the
reported vector theta, the per-segment running state, the fold of the segments, the histogram range and the binning ("twins": numpy,
the fused multiply-add from libm, exp from the oracle's orc_exp_export).  tests/test_gpu_summary.py compares the device with these
twins bit for bit; this module holds the twins against plain high precision, and tests what needs no device: idhmc_summary_quantiles
and the PosteriorSummary arithmetic.

Bounds.  The twin's mean against the np.longdouble two-pass mean: rtol 1e-12 / atol 1e-13, its variance: rtol 1e-10 -- the forms the
suite asserts for the Welford update in tests/test_accumulators_cpu.py, whose update this is.  A quantile estimate lies in the bin that
holds the k-th order statistic, so it is within one bin width (hi - lo) / bins of it; the factor 1 + 1e-9 covers the rounding of the
bin edges ((theta - lo) inv_w is rounded twice before it is truncated)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from test_accumulators_cpu import fma, welford_twin

SEGMENT = 256


# ---- the twins -------------------------------------------------------------------------------------------------------------------------
def theta_twin(draws, Dx, A, H, groups, dexp):
    """[..., D] sampled coordinates -> the reported vector [beta = u e_grp | a raw | sigma = e], e_g = dexp(omega_g); H = 0: the draws"""
    draws = np.asarray(draws, dtype=np.float64)
    if H == 0:
        return draws.copy()
    e = np.vectorize(dexp, otypes=[np.float64])(draws[..., Dx + A:])
    out = draws.copy()
    grp = np.asarray(groups)
    for c in range(Dx):
        if grp[c] >= 0:
            out[..., c] = draws[..., c] * e[..., grp[c]]
    out[..., Dx + A:] = e
    return out


def segments_twin(theta, G):
    """theta [N][C][D], groups of G chains -> per segment of SEGMENT chains the state after every value, visited transition by
    transition and in ascending chain id inside: a dict of arrays [groups][segments per group][D] (n: [groups][segments per group])"""
    theta = np.asarray(theta, dtype=np.float64)
    N, Cn, D = theta.shape
    assert Cn % G == 0
    groups, spg = Cn // G, -(-G // SEGMENT)
    st = {k: np.zeros((groups, spg, D)) for k in ("mean", "m2", "min", "max")}
    st["pos"] = np.zeros((groups, spg, D), dtype=np.int64)
    st["n"] = np.zeros((groups, spg), dtype=np.int64)
    by_group = theta.reshape(N, groups, G, D)
    for k in range(spg):
        seg = by_group[:, :, k * SEGMENT:(k + 1) * SEGMENT, :]            # [N][groups][m][D]
        m = seg.shape[2]
        seq = seg.transpose(0, 2, 1, 3).reshape(N * m, groups, D)         # the order of the visits, the groups side by side
        mean, m2, n = welford_twin(seq)
        mn, mx = np.full((groups, D), np.inf), np.full((groups, D), -np.inf)
        for x in seq:
            mn = np.where(x < mn, x, mn)
            mx = np.where(x > mx, x, mx)
        st["mean"][:, k], st["m2"][:, k], st["n"][:, k] = mean, m2, n
        st["min"][:, k], st["max"][:, k] = mn, mx
        st["pos"][:, k] = np.count_nonzero(seq > 0.0, axis=0)
    return st


def fold_twin(st):
    """the segments folded in ascending order from segment 0 -> n [groups], mean, var, min, max, pos [groups][D]"""
    n = st["n"][:, 0].copy()
    mean, m2 = st["mean"][:, 0].copy(), st["m2"][:, 0].copy()
    mn, mx, pos = st["min"][:, 0].copy(), st["max"][:, 0].copy(), st["pos"][:, 0].copy()
    for k in range(1, st["n"].shape[1]):
        nb = st["n"][:, k]
        assert np.all(nb > 0)
        na = n
        n = na + nb
        delta = st["mean"][:, k] - mean
        f = (nb.astype(np.float64) / n.astype(np.float64))[:, None]
        mean = fma(delta, f, mean)
        m2 = (m2 + st["m2"][:, k]) + (delta * delta) * (na.astype(np.float64)[:, None] * f)
        mn = np.where(st["min"][:, k] < mn, st["min"][:, k], mn)
        mx = np.where(st["max"][:, k] > mx, st["max"][:, k], mx)
        pos = pos + st["pos"][:, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(n[:, None] > 1, m2 / (n[:, None] - 1).astype(np.float64), 0.0)
    return dict(n=n, mean=mean, var=var, min=mn, max=mx, pos=pos)


def summary_twin(theta, G):
    return fold_twin(segments_twin(theta, G))


def range_twin(mean, var, span, bins):
    sd = np.sqrt(var)
    lo, hi = fma(-span, sd, mean), fma(span, sd, mean)
    return lo, hi, inv_w_twin(lo, hi, bins)


def inv_w_twin(lo, hi, bins):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(hi > lo, float(bins) / (hi - lo), 0.0)


def counts_twin(theta, G, lo, hi, inv_w, bins):
    """theta [N][C][D] binned with the ranges [groups][D] -> counts [groups][D][bins + 2]"""
    theta = np.asarray(theta, dtype=np.float64)
    N, Cn, D = theta.shape
    groups = Cn // G
    x = theta.reshape(N, groups, G, D)
    lo_, hi_, iw_ = lo[None, :, None, :], hi[None, :, None, :], inv_w[None, :, None, :]
    with np.errstate(invalid="ignore"):
        inner = 1 + np.minimum(((x - lo_) * iw_).astype(np.int64), bins - 1)
    b = np.where(x < lo_, 0, np.where(x >= hi_, bins + 1, inner))
    counts = np.zeros((groups, D, bins + 2), dtype=np.uint32)
    for g in range(groups):
        for d in range(D):
            counts[g, d] = np.bincount(b[:, g, :, d].ravel(), minlength=bins + 2)
    return counts


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the twins against plain high precision --------------------------------------------------------------------------------------------
def two_pass(theta, G):
    N, Cn, D = theta.shape
    x = theta.reshape(N, Cn // G, G, D).transpose(1, 0, 2, 3).reshape(Cn // G, N * G, D).astype(np.longdouble)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).sum(axis=1) / (N * G - 1)
    return mean, var


@pytest.mark.parametrize("N,Cn,G,D", [(5, 515, 515, 5), (4, 35, 7, 130), (3, 1024, 512, 3), (70, 64, 16, 8)])
def test_twin_agrees_with_plain_high_precision(N, Cn, G, D):
    rng = np.random.default_rng(N * 1000 + G)
    theta = rng.standard_normal((N, Cn, D)) * np.logspace(-2, 2, D) + np.linspace(-3, 3, D) * np.logspace(-2, 2, D)
    theta[:, :, 0] = 0.625                                    # a column of equal values
    got = summary_twin(theta, G)
    mean, var = two_pass(theta, G)
    assert np.all(got["n"] == N * G)
    dev_mean = np.abs(got["mean"] - mean)
    dev_var = np.abs(got["var"][:, 1:] - var[:, 1:]) / var[:, 1:]
    print("largest deviation: mean %.3g (relative %.3g), variance relative %.3g"
          % (dev_mean.max(), (dev_mean[:, 1:] / np.abs(mean[:, 1:])).max(), dev_var.max()))
    assert np.all(dev_mean <= 1e-13 + 1e-12 * np.abs(mean))
    assert np.all(dev_var <= 1e-10)
    assert np.all(bits(got["mean"][:, 0]) == bits(0.625)) and np.all(bits(got["var"][:, 0]) == bits(0.0))
    assert np.array_equal(got["min"], theta.reshape(N, Cn // G, G, D).min(axis=(0, 2)))
    assert np.array_equal(got["max"], theta.reshape(N, Cn // G, G, D).max(axis=(0, 2)))
    assert np.array_equal(got["pos"], (theta.reshape(N, Cn // G, G, D) > 0).sum(axis=(0, 2)))


def test_signed_zeros_are_not_positive_and_the_first_extreme_stays():
    theta = np.array([0.0, -0.0, -0.0, 0.0]).reshape(2, 2, 1)
    got = summary_twin(theta, 2)
    assert got["pos"][0, 0] == 0
    assert bits(got["min"])[0, 0] == bits(0.0) and bits(got["max"])[0, 0] == bits(0.0)      # x < min is false for -0.0 against +0.0


def test_theta_twin(oracle):
    dexp = oracle.lib().orc_exp_export
    rng = np.random.default_rng(3)
    Dx, A, H = 5, 1, 2
    groups = np.array([0, -1, 1, 1, 0])
    q = rng.standard_normal((3, 4, Dx + A + H))
    th = theta_twin(q, Dx, A, H, groups, dexp)
    e = np.exp(q[..., Dx + A:])
    assert np.allclose(th[..., Dx + A:], e, rtol=1e-15)
    assert np.allclose(th[..., :Dx], q[..., :Dx] * np.where(groups >= 0, e[..., np.maximum(groups, 0)], 1.0), rtol=1e-15)
    assert np.array_equal(th[..., 1], q[..., 1]) and np.array_equal(th[..., Dx], q[..., Dx])
    assert np.array_equal(theta_twin(q, Dx + A + H, 0, 0, None, dexp), q)


def test_binning_twin_never_leaves_the_table():
    bins = 16
    lo, hi = np.array([[-1.0, 2.0]]), np.array([[1.0, 2.0]])            # the second parameter: lo == hi
    iw = inv_w_twin(lo, hi, bins)
    assert iw[0, 1] == 0.0 and iw[0, 0] == 8.0
    x = np.array([-1.0, 1.0, -1.0 + 0.125, np.nextafter(-1.0, -2), np.nextafter(1.0, 0), -5.0, 5.0, 0.0])
    theta = np.stack([x, np.full_like(x, 2.0)], axis=-1).reshape(len(x), 1, 2)
    c = counts_twin(theta, 1, lo, hi, iw, bins)
    assert c.sum(axis=-1).tolist() == [[len(x), len(x)]]
    want = np.zeros(bins + 2, dtype=np.uint32)
    for b in (1, bins + 1, 2, 0, bins, 0, bins + 1, 9):
        want[b] += 1
    assert np.array_equal(c[0, 0], want)
    assert c[0, 1, bins + 1] == len(x)                                   # theta >= hi with lo == hi


# ---- idhmc_summary_quantiles ------------------------------------------------------------------------------------------------------------
def quantiles(idhmc, counts, bins, lo, hi, probs):
    lib = idhmc.load_library()
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    probs = np.ascontiguousarray(probs, dtype=np.float64)
    out = np.empty(len(probs))
    dp = C.POINTER(C.c_double)
    rc = lib.idhmc_summary_quantiles(counts.ctypes.data_as(C.POINTER(C.c_uint32)), bins, lo, hi, probs.ctypes.data_as(dp), len(probs),
                                     out.ctypes.data_as(dp))
    assert rc == 0, lib.idhmc_last_error()
    return out


def test_quantiles_by_hand(idhmc):
    bins = 4
    P = [0.0, 0.25, 0.5, 1.0]
    assert np.all(np.isnan(quantiles(idhmc, np.zeros(bins + 2), bins, 0.0, 4.0, P)))                  # an empty histogram
    assert np.array_equal(quantiles(idhmc, [7, 0, 0, 0, 0, 0], bins, 0.0, 4.0, P), [0.0] * 4)         # everything below lo
    assert np.array_equal(quantiles(idhmc, [0, 0, 0, 0, 0, 7], bins, 0.0, 4.0, P), [4.0] * 4)         # everything from hi on
    # a single bin, [2, 3), of four values: the k-th at 2 + (k - 0.5) / 4; p = 0 is the first, p = 1 the last
    assert np.array_equal(quantiles(idhmc, [0, 0, 0, 4, 0, 0], bins, 0.0, 4.0, P), [2.125, 2.125, 2.375, 2.875])
    # lo == hi: only the end bins can hold anything
    assert np.array_equal(quantiles(idhmc, [3, 0, 0, 0, 0, 5], bins, 1.5, 1.5, [0.0, 0.375, 0.5, 1.0]), [1.5] * 4)
    # 2 below, 3 in [0, 1), 1 in [3, 4), 2 above: k = 1..8
    got = quantiles(idhmc, [2, 3, 0, 0, 1, 2], bins, 0.0, 4.0, np.arange(1, 9) / 8.0)
    assert np.array_equal(got, [0.0, 0.0, 0.5 / 3, 1.5 / 3, 2.5 / 3, 3.5, 4.0, 4.0])
    lib = idhmc.load_library()
    assert lib.idhmc_summary_quantiles(None, 4, 0.0, 1.0, None, 0, None) == 1
    one = np.zeros(3, dtype=np.uint32)
    p, o = np.array([1.5]), np.zeros(1)
    dp = C.POINTER(C.c_double)
    assert lib.idhmc_summary_quantiles(one.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 0.0, 1.0, p.ctypes.data_as(dp), 1, o.ctypes.data_as(dp)) == 1
    assert b"1.5" in lib.idhmc_last_error()
    assert lib.idhmc_summary_quantiles(one.ctypes.data_as(C.POINTER(C.c_uint32)), 0, 0.0, 1.0, p.ctypes.data_as(dp), 1, o.ctypes.data_as(dp)) == 1


@pytest.mark.parametrize("bins,n", [(128, 4096), (16, 1000), (256, 100000)])
def test_quantiles_within_one_bin_of_the_order_statistic(idhmc, bins, n):
    rng = np.random.default_rng(bins)
    x = 3.0 + 0.5 * rng.standard_normal(n)
    theta = x.reshape(n, 1, 1)
    s = summary_twin(theta, 1)
    lo, hi, iw = range_twin(s["mean"], s["var"], 6.0, bins)
    counts = counts_twin(theta, 1, lo, hi, iw, bins)[0, 0]
    P = np.array([0.025, 0.5, 0.975])
    k = np.clip(np.ceil(P * n), 1, n).astype(np.int64)
    assert np.all(k > counts[0]) and np.all(k <= n - counts[-1]), "a compared quantile lies in an end bin"
    got = quantiles(idhmc, counts, bins, lo[0, 0], hi[0, 0], P)
    want = np.sort(x)[k - 1]
    width = (hi[0, 0] - lo[0, 0]) / bins
    print("bins %d: |estimate - order statistic| / bin width = %s" % (bins, np.abs(got - want) / width))
    assert np.all(np.abs(got - want) <= width * (1 + 1e-9))


# ---- PosteriorSummary -------------------------------------------------------------------------------------------------------------------
def make_summary(idhmc, theta, G, bins, span=6.0):
    s = summary_twin(theta, G)
    lo, hi, iw = range_twin(s["mean"], s["var"], span, bins)
    counts = counts_twin(theta, G, lo, hi, iw, bins)
    binned = np.full_like(s["n"], theta.shape[0] * G)
    return idhmc.PosteriorSummary(chains_per_group=G, bins=bins, n=s["n"], binned=binned, mean=s["mean"], var=s["var"], min=s["min"],
                                  max=s["max"], pos=s["pos"], lo=lo, hi=hi, inv_w=iw, counts=counts)


def test_posterior_summary_arithmetic_and_end_bin_warning(idhmc):
    rng = np.random.default_rng(11)
    theta = rng.standard_normal((50, 12, 3)) + np.array([0.0, 1.0, -2.0])
    ps = make_summary(idhmc, theta, 4, 64)
    assert np.array_equal(ps.sd, np.sqrt(ps.var))
    x = theta.reshape(50, 3, 4, 3)
    assert np.array_equal(ps.p_positive, (x > 0).sum(axis=(0, 2)) / 200.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        q = ps.quantiles([0.025, 0.5, 0.975])
    assert q.shape == (3, 3, 3)
    srt = np.sort(x.transpose(1, 0, 2, 3).reshape(3, 200, 3), axis=1)
    width = (ps.hi - ps.lo) / 64
    for i, p in enumerate((0.025, 0.5, 0.975)):
        assert np.all(np.abs(q[:, :, i] - srt[:, int(np.ceil(p * 200)) - 1, :]) <= width * (1 + 1e-9))
    narrow = make_summary(idhmc, theta, 4, 64, span=1.0)                  # a sixth of the values in each end bin
    with pytest.warns(RuntimeWarning, match="end bin"):
        qn = narrow.quantiles([0.025, 0.5])
    assert np.array_equal(qn[:, :, 0], narrow.lo)
    none = idhmc.PosteriorSummary(chains_per_group=4, bins=0, n=ps.n, binned=ps.binned * 0, mean=ps.mean, var=ps.var, min=ps.min,
                                  max=ps.max, pos=ps.pos, lo=ps.lo * 0, hi=ps.hi * 0, inv_w=ps.inv_w * 0)
    with pytest.raises(ValueError):
        none.quantiles([0.5])
