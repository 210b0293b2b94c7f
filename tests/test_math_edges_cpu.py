"""The math layer and the RNG helpers at their edges, input by input ("Math layer and RNG address space"), without
a GPU.  This file holds

  the tables    deterministic inputs per function of csrc/idhmc_math.hpp, chosen branch by branch (exponent sweep, thresholds at
                +-1 ulp, ties, non-finite arguments, cancellation patterns for the reductions), as plain functions;
  the layout    how a table becomes the rows of the device probe of tests/test_gpu_math_edges.py (one row = one chain of 256
                coordinates, the last one the selector of the function) and how results come back out of a row;
  the twin      PROBE_TWIN_C, the probe restated in C against oracle/orc_math.h (and test_glm_dispersion_cpu.TWIN_C), row for row;
  the tests     the twin against an independent reference on exactly those tables: mpmath at 40 digits for the elementary
                functions, numpy's correctly rounded / sqrt rint, fractions.Fraction for fma, a numpy Philox, math.fsum.

The GPU file imports the tables, the layout and the twin and asserts device == twin on raw bits; the bounds asserted here are the
project's own (tests/test_oracle_math.py: log <= 4 ulp, exp <= 2 ulp, log1p <= 4 ulp, sin / cos 1e-15 absolute; DESIGN section 14:
ln Gamma and psi within 5e-14 (1 + |f|)), so both sides are pinned to the true function at every input of every table."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_glm_dispersion_cpu import TWIN_C

W = 256                      # coordinates per probe row (two chunks of 128); coordinate 255 is the selector
(SEL_LOG, SEL_EXP, SEL_LOG1P, SEL_SINCOS, SEL_LOGADDEXP, SEL_LGAMMA_PSI, SEL_DIV, SEL_SQRT, SEL_RINT, SEL_D2I2D, SEL_FMA, SEL_FMA_C,
 SEL_U01, SEL_U01_OPEN0, SEL_PHILOX, SEL_RANDN, SEL_REDUCE) = range(1, 18)
# the compile-time third arguments of dfma_c in the probe and the twin: +-1 (cancellation against products near 1), the smallest
# subnormal (a sticky bit below every product), the largest double (the overflow edge)
FMA_C_CONSTANTS = (1.0, -1.0, 5e-324, 1.7976931348623157e308)

PROBE_TWIN_C = r"""
#include "orc_math.h"
%s
static double tree(const double *v)
{
    double acc[128];
    memcpy(acc, v, sizeof acc);
    return orc_tree128(acc);
}
static double frombits2(uint32_t lo, uint32_t hi) { return orc_frombits(((uint64_t)hi << 32) | lo); }

/* one row = one chain of the device probe: q[255] selects the function, g is what the probe leaves in grad, lq what it returns
   (a non-finite log density is -inf, evaluate_l!) */
void probe_twin(const double *q, double *g, double *lq, long rows)
{
    for (long c = 0; c < rows; ++c, q += 256, g += 256) {
        const int sel = (int)q[255];
        const double l = tree(q);
        lq[c] = isfinite(l) ? l : -INFINITY;
        for (int i = 0; i < 256; ++i) g[i] = 0.0;
        switch (sel) {
        case 1: for (int i = 0; i < 256; ++i) g[i] = orc_log(q[i]); break;
        case 2: for (int i = 0; i < 256; ++i) g[i] = orc_exp(q[i]); break;
        case 3: for (int i = 0; i < 256; ++i) g[i] = orc_log1p(q[i]); break;
        case 4: for (int m = 0; m < 128; ++m) orc_sincos2pi(q[2 * m], &g[2 * m], &g[2 * m + 1]); break;
        case 5:
            for (int m = 0; m < 128; ++m) {
                g[2 * m] = orc_logaddexp(q[2 * m], q[2 * m + 1]);
                g[2 * m + 1] = orc_logaddexp(q[2 * m + 1], q[2 * m]);
            }
            break;
        case 6: for (int m = 0; m < 128; ++m) orc_lgamma_psi(q[2 * m], &g[2 * m], &g[2 * m + 1]); break;
        case 7:
            for (int m = 0; m < 128; ++m) {
                g[2 * m] = q[2 * m] / q[2 * m + 1];
                g[2 * m + 1] = 1.0 / q[2 * m];
            }
            break;
        case 8: for (int i = 0; i < 256; ++i) g[i] = sqrt(q[i]); break;
        case 9: for (int i = 0; i < 256; ++i) g[i] = rint(q[i]); break;
        case 10: for (int i = 0; i < 256; ++i) g[i] = (double)(int)q[i]; break;
        case 11: for (int l2 = 0; l2 < 64; ++l2) g[2 * l2] = fma(q[2 * l2], q[2 * l2 + 1], q[128 + 2 * l2]); break;
        case 12:
            for (int l2 = 0; l2 < 64; ++l2) {
                const double a = q[2 * l2], b = q[2 * l2 + 1];
                g[2 * l2] = fma(a, b, 1.0);
                g[2 * l2 + 1] = fma(a, b, -1.0);
                g[128 + 2 * l2] = fma(a, b, 0x1p-1074);
                g[129 + 2 * l2] = fma(a, b, 0x1.fffffffffffffp+1023);
            }
            break;
        case 13: for (int i = 0; i < 256; ++i) { const uint64_t b = orc_bits(q[i]); g[i] = orc_u01((uint32_t)b, (uint32_t)(b >> 32)); } break;
        case 14: for (int i = 0; i < 256; ++i) { const uint64_t b = orc_bits(q[i]); g[i] = orc_u01_open0((uint32_t)b, (uint32_t)(b >> 32)); } break;
        case 15:
            for (int l2 = 0; l2 < 64; ++l2) {
                const uint64_t c01 = orc_bits(q[2 * l2]), c23 = orc_bits(q[2 * l2 + 1]), k = orc_bits(q[128 + 2 * l2]);
                uint32_t o[4];
                orc_philox4x32((uint32_t)c01, (uint32_t)(c01 >> 32), (uint32_t)c23, (uint32_t)(c23 >> 32), (uint32_t)k, (uint32_t)(k >> 32), o);
                g[2 * l2] = frombits2(o[0], o[1]);
                g[2 * l2 + 1] = frombits2(o[2], o[3]);
            }
            break;
        case 16:                                   /* orc_randn_pair from (u1, u2) on */
            for (int m = 0; m < 128; ++m) {
                const double r = sqrt(-2.0 * orc_log(q[2 * m]));
                double s, cs;
                orc_sincos2pi(q[2 * m + 1], &s, &cs);
                g[2 * m] = r * cs;
                g[2 * m + 1] = r * s;
            }
            break;
        case 17: {                                 /* every lane's copy of wave_sum, wave_sum2 (two patterns) and rows_sum */
            double b[128];
            memcpy(b, q + 128, 127 * sizeof(double));
            b[127] = q[254];
            const double S = tree(q), T = tree(b);
            for (int l2 = 0; l2 < 64; ++l2) {
                const int i = l2 & 15;
                g[2 * l2] = S;
                g[2 * l2 + 1] = S;
                g[128 + 2 * l2] = T;
                g[129 + 2 * l2] = (q[2 * i] + q[2 * (16 + i)]) + (q[2 * (32 + i)] + q[2 * (48 + i)]);
            }
            break;
        }
        default: break;
        }
    }
}
""" % TWIN_C


def build_twin(workdir):
    """PROBE_TWIN_C compiled the way oracle.OracleModel.custom compiles a user density; returns f(q rows) -> (g rows, lq)"""
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(str(workdir), "probe_twin.c"), os.path.join(str(workdir), "probe_twin.so")
    with open(src, "w") as f:
        f.write(PROBE_TWIN_C)
    subprocess.check_call(["gcc", "-O2", "-mavx2", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(here, "..", "oracle"),
                           "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.probe_twin.argtypes = [dp, dp, dp, C.c_long]
    lib.probe_twin.restype = None

    def evaluate(q):
        q = np.ascontiguousarray(q, dtype=np.float64)
        assert q.ndim == 2 and q.shape[1] == W
        g, lq = np.empty_like(q), np.empty(q.shape[0])
        lib.probe_twin(q.ctypes.data_as(dp), g.ctypes.data_as(dp), lq.ctypes.data_as(dp), q.shape[0])
        return g, lq
    evaluate.lib = lib
    return evaluate


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def f64(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def ulp_step(x, k):
    """x moved by k units in the last place (k of either sign; x finite and non-zero, no crossing of zero)"""
    x = np.asarray(x, dtype=np.float64)
    b = u64(x).astype(np.int64)
    b = b.reshape(x.shape) + np.where(x < 0, -1, 1) * np.asarray(k, dtype=np.int64)
    return b.astype(np.uint64).view(np.float64)[()]


def same_bits(a, b, nan_equal=True):
    """element-wise: the same 64 bits (so the sign of zero counts); with nan_equal any NaN equals any NaN, as test_gpu_parity has it"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = u64(a).reshape(a.shape) == u64(b).reshape(b.shape)
    return same | (np.isnan(a) & np.isnan(b)) if nan_equal else same


NAN_PAYLOAD = f64([0x7ff8000000abcdef])[0]
SQRT2_MANT = 0x6a09e667f3bcd                  # 1.4142135623730951, the fold threshold of dlog


# ---- the layout: tables <-> probe rows -----------------------------------------------------------------------------------------------
class Block:
    """One table bound to one selector.  kind 'u': 255 arguments a row (every coordinate but the selector); 'p': 127 (even, odd)
    pairs a row; 'l': 64 lanes a row, columns (x0, y0, x1) = coordinates (2l, 2l + 1, 128 + 2l); 'v': one row per 128-vector a with
    a second pattern b of 127 values in the second chunk."""

    def __init__(self, name, sel, kind, *cols, fill=1.0):
        self.name, self.sel, self.kind = name, sel, kind
        self.cols = [np.ascontiguousarray(c, dtype=np.float64) for c in cols]
        self.n = self.cols[0].shape[0]
        assert all(c.shape[0] == self.n for c in self.cols)
        self.per = {"u": 255, "p": 127, "l": 64, "v": 1}[kind]
        self.nrows = -(-self.n // self.per)
        self.fill = fill

    def _spread(self, col):
        out = np.full(self.nrows * self.per, self.fill)
        out[:self.n] = col
        return out.reshape(self.nrows, self.per)

    def rows(self):
        q = np.full((self.nrows, W), self.fill)
        if self.kind == "u":
            q[:, :255] = self._spread(self.cols[0])
        elif self.kind == "p":
            q[:, 0:254:2] = self._spread(self.cols[0])
            if len(self.cols) > 1:
                q[:, 1:254:2] = self._spread(self.cols[1])
        elif self.kind == "l":
            for k, start in enumerate((0, 1, 128)[:len(self.cols)]):
                q[:, start:start + 128:2] = self._spread(self.cols[k])
        else:
            q[:, :128] = self.cols[0]
            q[:, 128:255] = self.cols[1]
        q[:, 255] = float(self.sel)
        return q

    def outputs(self, g):
        """the results of this block's rows g, aligned with the table: a tuple of arrays of length n ('v': the rows themselves)"""
        g = np.asarray(g)
        assert g.shape == (self.nrows, W)
        if self.kind == "u":
            return (g[:, :255].reshape(-1)[:self.n],)
        if self.kind == "p":
            return g[:, 0:254:2].reshape(-1)[:self.n], g[:, 1:254:2].reshape(-1)[:self.n]
        if self.kind == "l":
            return tuple(g[:, s:s + 128:2].reshape(-1)[:self.n] for s in (0, 1, 128, 129))
        return (g,)


def pack(blocks):
    """all rows of all blocks as one (rows, 256) matrix, and each block's row range"""
    q = np.concatenate([b.rows() for b in blocks])
    ends = np.cumsum([b.nrows for b in blocks])
    return q, {b.name: slice(int(e - b.nrows), int(e)) for b, e in zip(blocks, ends)}


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def exponent_sweep(positive_only=False):
    """every biased exponent 0 .. 2046 with mantissas 0, 1, 2^52 - 1, the three patterns round sqrt 2 and one seeded random one, both
    signs; +-0, +-inf and a quiet NaN with a payload"""
    rng = np.random.default_rng(20260401)
    e = np.arange(2047, dtype=np.uint64)[:, None] << np.uint64(52)
    mant = np.empty((2047, 7), dtype=np.uint64)
    mant[:, :6] = np.array([0, 1, (1 << 52) - 1, SQRT2_MANT - 1, SQRT2_MANT, SQRT2_MANT + 1], dtype=np.uint64)
    mant[:, 6] = rng.integers(0, 1 << 52, 2047, dtype=np.uint64)
    pos = (e | mant).reshape(-1)
    if positive_only:
        return f64(pos)
    return np.concatenate([f64(pos), f64(pos | np.uint64(1 << 63)), [0.0, -0.0, np.inf, -np.inf, NAN_PAYLOAD]])


def sweep_random_mantissas():
    """the sweep's seeded column alone: one value per exponent"""
    return exponent_sweep(positive_only=True).reshape(2047, 7)[:, 6].copy()


def table_log():
    k = np.arange(1, 201)
    p2 = 2.0 ** -np.arange(1, 54, dtype=np.float64)
    tiny = 2.0 ** -1022
    return np.concatenate([exponent_sweep(positive_only=True), [NAN_PAYLOAD, np.inf, -0.0, -1.0, -np.inf, -5e-324],
                           ulp_step(np.ones(200), k), ulp_step(np.ones(200), -k), 1.0 + p2[:52], 1.0 - p2,
                           [np.nextafter(tiny, 0.0), tiny, np.nextafter(tiny, 1.0), 5e-324]])


LN2_LD = np.log(np.longdouble(2.0))
EXP_HI, EXP_LO = 709.782712893384, -708.3964185322641


def table_exp():
    k = np.arange(-1022, 1025)
    half = ((k.astype(np.longdouble) + np.longdouble(0.5)) * LN2_LD).astype(np.float64)
    whole = (k.astype(np.longdouble) * LN2_LD).astype(np.float64)
    near = np.concatenate([ulp_step(half, d) for d in range(-3, 4)])
    p2 = 2.0 ** -np.arange(0, 1075, dtype=np.float64)
    thr = np.concatenate([ulp_step(np.full(3, t), [-1, 0, 1]) for t in (EXP_HI, EXP_LO)])
    return np.concatenate([near, whole, thr, [0.0, -0.0, np.inf, -np.inf, NAN_PAYLOAD, 710.0, -745.2, -1e9, 1e9], p2, -p2])


def table_log1p():
    p2 = 2.0 ** -np.arange(0, 1075, dtype=np.float64)
    up = 2.0 ** np.arange(0, 1024, dtype=np.float64)
    return np.concatenate([p2, -p2, up, [-1.0, np.nextafter(-1.0, 0.0), -1.0 + 2.0 ** -52, np.nextafter(-1.0, -2.0), -2.0, -1e300, -np.inf,
                                         0.0, -0.0, np.inf, NAN_PAYLOAD, 1.7976931348623157e308]])


def table_sincos():
    rng = np.random.default_rng(20260402)
    out = [np.array([0.0, 5e-324, 1e-323, 1.5e-323])]
    for k in range(1, 8):
        out.append(ulp_step(np.full(7, k / 8.0), np.arange(-3, 4)))           # the ties of rint(4u) at odd k
    out.append(ulp_step(np.full(3, 1.0), [-1, -2, -3]))
    out.append(2.0 ** -np.arange(1, 1075, dtype=np.float64))
    out.append(rng.integers(0, 1 << 53, 4000).astype(np.float64) * 2.0 ** -53)
    return np.concatenate(out)


def table_logaddexp():
    """(x, y): equal arguments, differences of +-(0, 1 ulp, 36, 37, 708, 709, 745, 1e300), each of +-inf and NaN on either side"""
    xs, ys = [], []
    for x in (0.0, 1.5, -3.25, 700.0, -700.0, 1e300, -1e300, 1e-300, -0.0):
        for d in (0.0, None, 36.0, 37.0, 708.0, 709.0, 745.0, 1e300):
            for sgn in (1.0, -1.0):
                y = x + sgn * d if d is not None else float(ulp_step([x if x != 0.0 else 5e-324], int(sgn))[0])
                xs.append(x)
                ys.append(y)
    special = [np.inf, -np.inf, NAN_PAYLOAD]
    for s in special:
        for o in (0.0, 1.5, -1e300, np.inf, -np.inf, NAN_PAYLOAD):
            xs.append(s)
            ys.append(o)
    return np.array(xs), np.array(ys)


# the largest x whose (x - 1/2) * log x is finite in fp64, and the largest x whose ln Gamma(x) rounds to a finite double: between them
# the device's Stirling form used to overflow while the true value does not (test_lgamma_overflow_edge states both properties)
PSI_ZERO = 1.4616321449683623


def lgamma_edges():
    """by bisection on the doubles, deterministic: x1 = the largest double with x * log(x) finite (numpy's log; the device's dlog is
    within 4 ulp of it, so x1 +- 64 ulp brackets the device's edge), x2 = the largest with x * (log(x) - 1) finite, which is where
    ln Gamma(x) itself leaves the doubles (to the 1e-15 that separates the two forms; the test states it against mpmath)"""
    def last_finite(f):
        lo, hi = int(u64([1e305])[0]), int(u64([1e306])[0])
        while hi - lo > 1:
            mid = (lo + hi) // 2
            with np.errstate(over="ignore"):
                ok = np.isfinite(f(f64([mid])[0]))
            lo, hi = (mid, hi) if ok else (lo, mid)
        return f64([lo])[0]
    return last_finite(lambda x: x * np.log(x)), last_finite(lambda x: x * (np.log(x) - 1.0))


def table_lgamma_psi():
    rng = np.random.default_rng(20260403)
    sub = f64(rng.integers(1, 1 << 52, 40, dtype=np.uint64))
    p1024 = f64([0x0004000000000000])                                          # 2^-1024: 1 / x overflows from here down
    ints = np.arange(1.0, 10.0)
    x1, x2 = lgamma_edges()
    big = np.concatenate([10.0 ** np.linspace(300.0, 308.2, 200), [1.7e308, 1.7976931348623157e308],
                          ulp_step(np.full(9, x1), np.arange(-64, 65, 16)), ulp_step(np.full(5, x1), [-2, -1, 0, 1, 2]),
                          np.linspace(x1, x2, 40), ulp_step(np.full(9, x2), np.arange(-64, 65, 16)), ulp_step(np.full(5, x2), [-2, -1, 0, 1, 2])])
    return np.concatenate([sub, [5e-324, 1e-310, np.nextafter(2.0 ** -1022, 0.0), 2.0 ** -1022, 2.0 ** -1023],
                           ulp_step(np.full(9, p1024[0]), np.arange(-4, 5)),
                           ulp_step(ints, -1), ints, ulp_step(ints, 1), ulp_step(np.full(3, PSI_ZERO), [-1, 0, 1]),
                           10.0 ** np.linspace(-300.0, 299.0, 120), np.linspace(0.01, 12.0, 150), big,
                           [0.0, -0.0, -1.5, -5e-324, -np.inf, np.inf, NAN_PAYLOAD]])


def table_div():
    """(a, b): one a per exponent against a seeded b, a 64 x 64 grid over the exponent range (quotients from far below the subnormals
    to far above the largest double), quotients at the overflow edge and inside the subnormals, zeros and non-finite arguments"""
    rng = np.random.default_rng(20260404)
    r = sweep_random_mantissas()
    sgn = np.where(rng.integers(0, 2, r.size) == 1, -1.0, 1.0)
    a = [r * sgn, r]
    b = [rng.permutation(r) * np.where(rng.integers(0, 2, r.size) == 1, -1.0, 1.0), 1.0 + rng.random(r.size)]
    grid = r[::32]
    a.append(np.repeat(grid, grid.size))
    b.append(np.tile(grid[::-1], grid.size))
    big, one = 1.7976931348623157e308, 1.0
    edge_a = [big, big, big, big, 2.0 ** -1022, 2.0 ** -1022, 2.0 ** -1022, 3.0 * 2.0 ** -1074, 5e-324, 5e-324, 1.0, 1.0, 2.0 ** -1022 * 1.5,
              0.0, -0.0, 1.0, -1.0, 0.0, np.inf, np.inf, 1.0, NAN_PAYLOAD, 1.0, 2.0 ** 1023, 2.0 ** 1023]
    edge_b = [np.nextafter(one, 0.0), one, np.nextafter(one, 2.0), 0.5, 2.0, 3.0, np.nextafter(one, 2.0), 2.0, 2.0, 4.0, big, 3.0, 2.0 ** 52,
              1.0, 1.0, 0.0, -0.0, 0.0, np.inf, 2.0, -np.inf, 1.0, NAN_PAYLOAD, 0.5, np.nextafter(0.5, 1.0)]
    a.append(np.array(edge_a))
    b.append(np.array(edge_b))
    return np.concatenate(a), np.concatenate(b)


def table_sqrt():
    return np.concatenate([exponent_sweep(positive_only=True), [-0.0, -1.0, -5e-324, np.inf, -np.inf, NAN_PAYLOAD, 2.0, 4.0, 0.25]])


def table_rint():
    n = np.concatenate([np.arange(0.0, 41.0), 2.0 ** np.arange(6, 52, dtype=np.float64), [2.0 ** 51 - 1.0, 2.0 ** 52 - 1.0]])
    half = n + 0.5
    other = np.array([0.0, 0.49999999999999994, 0.5000000000000001, 2.0 ** 52 - 1.0, 2.0 ** 52, 2.0 ** 52 + 1.0, 2.0 ** 53, 5e-324, 1e300,
                      0.25, 0.75, 1.25, 2.75])
    t = np.concatenate([half, ulp_step(half, 1), ulp_step(half, -1), other])
    return np.concatenate([t, -t, [np.inf, -np.inf, NAN_PAYLOAD]])


def table_d2i2d():
    """doubles whose truncation fits int32, the extremes among them"""
    rng = np.random.default_rng(20260405)
    t = np.array([0.0, 0.5, 0.99, 1.0, 1.5, 2.5, 1023.999, 2147483646.0, 2147483647.0, 2147483647.5, np.nextafter(2147483648.0, 0.0),
                  5e-324, 2.0 ** 30, 2.0 ** 24 + 1.0])
    return np.concatenate([t, -t, [-2147483648.0, -2147483648.5, np.nextafter(-2147483649.0, 0.0)],
                           rng.uniform(-2147483648.0, 2147483647.0, 200), rng.integers(-2 ** 31, 2 ** 31, 200).astype(np.float64)])


def fma_pairs():
    """(a, b) whose product needs more than 53 bits next to the probe's compile-time constants: products within a few 2^-53 of +-1
    (cancellation against +-1, and a sum one sticky bit from a tie), exact products, products at the overflow edge, tiny products"""
    rng = np.random.default_rng(20260406)
    e = 2.0 ** -52
    a = [1.0 + e, 1.0 + e, 1.0 - e / 2, 2.0, -2.0, 1.0 + 2.0 ** -26, 1.0 + 2.0 ** -27, 3.0, 2.0 ** -537, 2.0 ** -538, 2.0 ** 512, -2.0 ** 512,
         2.0 ** 1023, 1e-300, 0.0, -0.0, 1.0, 1.0 + e, 0.5 + e / 4]
    b = [1.0 - e, -(1.0 - e), 1.0 + e, 0.5, 0.5, 1.0 - 2.0 ** -26, 1.0 + 2.0 ** -27, 1.0 / 3.0, 2.0 ** -537, 2.0 ** -538, 2.0 ** 511, 2.0 ** 511,
         1.0 - e / 2, 1e-300, 1.0, 1.0, 5e-324, 1.0 + e, 2.0 ** -1074]
    a, b = np.array(a), np.array(b)
    ra = ulp_step(np.ones(300), rng.integers(-1 << 27, 1 << 27, 300))
    rb = 1.0 / ra                                                              # a * rb = 1 + O(2^-53): an inexact product next to +-1
    rc = rng.uniform(0.5, 2.0, 150) * 2.0 ** rng.integers(-30, 30, 150)
    rd = rng.uniform(0.5, 2.0, 150) * np.where(rng.integers(0, 2, 150) == 1, -1.0, 1.0)
    return np.concatenate([a, ra, -ra, rc]), np.concatenate([b, rb, rb, rd])


def table_fma():
    """(a, b, c): fma_pairs() with each of the probe's constants as a run-time c; exact cancellation c = -fl(a b) (the result is the
    rounding error of the product, which an unfused a * b + c turns into 0); double-rounding traps c = fl(a b) * 2^53 +- ... , where
    rounding the product first moves the sum across a tie; zeros of either sign"""
    a, b = fma_pairs()
    A = [np.tile(a, len(FMA_C_CONSTANTS))]
    B = [np.tile(b, len(FMA_C_CONSTANTS))]
    Cc = [np.repeat(np.array(FMA_C_CONSTANTS), a.size)]
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
    ok = np.isfinite(p) & (np.abs(p) > 1e-200) & (np.abs(p) < 1e200)
    A += [a[ok], a[ok], a[ok], a[ok]]
    B += [b[ok], b[ok], b[ok], b[ok]]
    Cc += [-p[ok], p[ok] * 2.0 ** 53, -p[ok] * 2.0 ** 52, ulp_step(-p[ok], 1)]
    z = np.array([0.0, -0.0])
    A.append(np.repeat(z, 4))
    B.append(np.tile(np.repeat(np.array([1.0, -1.0]), 2), 2))
    Cc.append(np.tile(z, 4))
    return np.concatenate(A), np.concatenate(B), np.concatenate(Cc)


U32_EDGES = (0, 1, 0x7ff, 0x800, 0xffffffff)


def table_u01():
    """(lo, hi) from U32_EDGES squared, then seeded words, packed lo | hi << 32 into the bits of one coordinate"""
    rng = np.random.default_rng(20260407)
    lo = np.array([l for l in U32_EDGES for _ in U32_EDGES] + rng.integers(0, 1 << 32, 485).tolist(), dtype=np.uint64)
    hi = np.array([h for _ in U32_EDGES for h in U32_EDGES] + rng.integers(0, 1 << 32, 485).tolist(), dtype=np.uint64)
    return lo, hi


PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def table_philox():
    """(counter[4], key[2]) as uint64 arrays of shape (n, 6): the three Random123 known-answer inputs, then 1000 seeded sets; in the
    first 64 of those word k % 6 has only its top bit set beside seeded low bits, in the next 64 every word has its top bit set"""
    rng = np.random.default_rng(20260408)
    w = rng.integers(0, 1 << 32, (1000, 6), dtype=np.uint64)
    for k in range(64):
        w[k, k % 6] |= np.uint64(0x80000000)
    w[64:128] |= np.uint64(0x80000000)
    kat = np.array([list(c) + list(k) for c, k, _ in PHILOX_KAT], dtype=np.uint64)
    return np.concatenate([kat, w])


def table_randn():
    rng = np.random.default_rng(20260409)
    u1e = np.array([2.0 ** -53, 1.0, np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0), 2.0 ** -52, np.nextafter(1.0, 0.0)])
    u2e = np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.875, 1.0 - 2.0 ** -53, 2.0 ** -53])
    u1 = np.concatenate([np.repeat(u1e, u2e.size), (rng.integers(0, 1 << 53, 500).astype(np.float64) + 1.0) * 2.0 ** -53])
    u2 = np.concatenate([np.tile(u2e, u1e.size), rng.integers(0, 1 << 53, 500).astype(np.float64) * 2.0 ** -53])
    return u1, u2


def cancellation_vectors():
    """For every level of the lane butterfly (xor 1, 2, 4, 8, 16, 32: element stride s = 2, 4, ..., 64), two vectors of ones with
    +1e300 at element o and -1e300 at element o + s (o = 0 and o = 128 - 2 s).  The ones that share a block of s elements with a
    1e300 are absorbed by it; the two blocks cancel exactly at that level and no earlier; every other block sums exactly.  So the tree
    gives 128 - 2 s, and any order that brings the two together at another level gives something else.  Returns (vectors, exact
    tree results)."""
    v, want = [], []
    for s in (2, 4, 8, 16, 32, 64):
        for o in (0, 128 - 2 * s):
            a = np.ones(128)
            a[o], a[o + s] = 1e300, -1e300
            v.append(a)
            want.append(128.0 - 2.0 * s)
    return np.array(v), np.array(want)


def table_reduce():
    """(a, b): 128-vectors a and a different pattern b of 127 values for wave_sum2's second sum (its 128th element repeats the 127th,
    the selector's place).  Seeded normals at three scales, the cancellation vectors, one inf, one NaN, all -0, subnormals."""
    rng = np.random.default_rng(20260410)
    normals = [rng.standard_normal(128) * s for s in (1.0, 1e-150, 1e150) for _ in range(4)]
    canc, _ = cancellation_vectors()
    one_inf, one_nan = rng.standard_normal(128), rng.standard_normal(128)
    one_inf[77], one_nan[41] = np.inf, np.nan
    sub = f64(rng.integers(0, 1 << 30, 128, dtype=np.uint64))
    sub2 = -f64(rng.integers(0, 1 << 51, 128, dtype=np.uint64))
    a = np.array(normals + list(canc) + [one_inf, one_nan, np.full(128, -0.0), sub, sub2, np.where(np.arange(128) % 2 == 0, 1e308, -1e308)])
    b = np.roll(a, 5, axis=0)[:, ::-1][:, :127].copy()                         # another vector of the set, reversed
    return a, b


def all_blocks():
    """every table bound to its selector, in the order the GPU test packs them"""
    lo, hi = table_u01()
    bits01 = f64(lo | (hi << np.uint64(32)))
    ph = table_philox()
    fa, fb, fc = table_fma()
    pa, pb = fma_pairs()
    return [Block("sweep/log", SEL_LOG, "u", exponent_sweep()), Block("sweep/exp", SEL_EXP, "u", exponent_sweep()),
            Block("sweep/log1p", SEL_LOG1P, "u", exponent_sweep()), Block("sweep/rint", SEL_RINT, "u", exponent_sweep()),
            Block("log", SEL_LOG, "u", table_log()), Block("exp", SEL_EXP, "u", table_exp()), Block("log1p", SEL_LOG1P, "u", table_log1p()),
            Block("sincos", SEL_SINCOS, "p", table_sincos()), Block("logaddexp", SEL_LOGADDEXP, "p", *table_logaddexp()),
            Block("lgamma_psi", SEL_LGAMMA_PSI, "p", table_lgamma_psi()), Block("div", SEL_DIV, "p", *table_div()),
            Block("sqrt", SEL_SQRT, "u", table_sqrt()), Block("rint", SEL_RINT, "u", table_rint()),
            Block("d2i2d", SEL_D2I2D, "u", table_d2i2d()), Block("fma", SEL_FMA, "l", fa, fb, fc), Block("fma_c", SEL_FMA_C, "l", pa, pb),
            Block("u01", SEL_U01, "u", bits01), Block("u01_open0", SEL_U01_OPEN0, "u", bits01),
            Block("philox", SEL_PHILOX, "l", f64(ph[:, 0] | (ph[:, 1] << np.uint64(32))), f64(ph[:, 2] | (ph[:, 3] << np.uint64(32))),
                  f64(ph[:, 4] | (ph[:, 5] << np.uint64(32)))),
            Block("randn", SEL_RANDN, "p", *table_randn()), Block("reduce", SEL_REDUCE, "v", *table_reduce())]


# ---- independent references ------------------------------------------------------------------------------------------------------------
def philox_reference(words):
    """Philox-4x32-10 (Salmon et al., SC'11) in numpy uint64 arithmetic: words (n, 6) -> (n, 4)"""
    w = np.asarray(words, dtype=np.uint64)
    c0, c1, c2, c3, k0, k1 = (w[:, i].copy() for i in range(6))
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], 1)


_TWO1024 = Fraction(2) ** 1024
_OVERFLOW = _TWO1024 - Fraction(2) ** 970            # the exact values from here up round to infinity


def round_fraction(v, zero_sign=0.0):
    """the double nearest the exact rational v, ties to even (int / int is correctly rounded in Python); an exact zero takes the
    sign given"""
    if v == 0:
        return zero_sign
    if abs(v) >= _OVERFLOW:
        return math.inf if v > 0 else -math.inf
    return v.numerator / v.denominator


def fma_reference(a, b, c):
    """fma(a, b, c) for finite doubles: the exact a b + c rounded once.  An exact zero is +0 under round-to-nearest unless product and
    addend are both zeros of negative sign."""
    p = Fraction(a) * Fraction(b)
    ps = math.copysign(1.0, a) * math.copysign(1.0, b)
    zero = -0.0 if (p == 0 and c == 0 and ps < 0 and math.copysign(1.0, c) < 0) else 0.0
    return round_fraction(p + Fraction(c), zero)


def tree_sum(v):
    """the canonical adjacent pairwise tree over 128 values, in numpy"""
    v = np.array(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        while v.size > 1:
            v = v[0::2] + v[1::2]
    return v[0]


def ulps_mp(got, ref):
    """|got - ref| in units of the spacing of doubles at ref (ref an mpmath number)"""
    import mpmath
    return float(abs(mpmath.mpf(float(got)) - ref) / mpmath.mpf(float(np.spacing(abs(float(ref))))))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(tmp_path_factory.mktemp("probe_twin"))


@pytest.fixture(scope="module")
def results(twin):
    """every block's twin results: name -> (block, outputs)"""
    blocks = all_blocks()
    q, where = pack(blocks)
    g, lq = twin(q)
    return {b.name: (b, b.outputs(g[where[b.name]])) for b in blocks}, q, g, lq


@pytest.fixture(scope="module")
def mp():
    import mpmath                                        # here, so that the GPU tests' import of this module does not need it
    mpmath.mp.dps = 40
    return mpmath


# ---- the tables themselves -----------------------------------------------------------------------------------------------------------
def test_tables_are_deterministic_and_enter_their_branches():
    a, b = all_blocks(), all_blocks()
    for x, y in zip(a, b):
        assert same_bits(x.rows(), y.rows(), nan_equal=False).all(), x.name
    sizes = {x.name: x.n for x in a}
    print("table sizes:", sizes, "rows:", sum(x.nrows for x in a))
    assert all(n <= 30000 for n in sizes.values()) and sum(x.nrows for x in a) <= 1024
    sweep = exponent_sweep()
    assert sweep.size == 2 * 2047 * 7 + 5 and set((u64(sweep[:2047 * 7]) >> np.uint64(52)).tolist()) == set(range(2047))
    x = table_log()
    m = f64((u64(x) & np.uint64((1 << 52) - 1)) | np.uint64(0x3ff0000000000000))
    sub = (x > 0) & (x < 2.0 ** -1022)
    assert sub.sum() >= 8 and (m == 1.4142135623730951).sum() >= 2047 and (m == np.nextafter(1.4142135623730951, 2.0)).sum() >= 2047
    x = table_exp()
    k = np.rint(x[np.isfinite(x)] * 1.4426950408889634)
    assert {-1022.0, 1024.0} <= set(k.tolist()) and (x > EXP_HI).any() and (x < EXP_LO).any() and (x == EXP_HI).any() and (x == EXP_LO).any()
    x = table_log1p()
    with np.errstate(invalid="ignore"):
        assert ((1.0 + x == 1.0) & (x != 0)).any() and (1.0 + x == np.inf).any() and (x < -1.0).any() and (x == -1.0).any()
    u = table_sincos()
    assert ((u >= 0) & (u < 1)).all() and set(np.rint(4.0 * u).tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert all((4.0 * u == t).any() for t in (0.5, 1.5, 2.5, 3.5))
    x = table_lgamma_psi()
    assert ((x > 0) & (x < 2.0 ** -1022)).sum() >= 40 and (x > 1e299).sum() >= 200 and (x == 2.0 ** -1024).any()


def test_cancellation_vectors_depend_on_the_association():
    """each vector's exact tree result, and a plain left-to-right sum (another association) gives other bits: the vector can tell
    the canonical order from a different one"""
    v, want = cancellation_vectors()
    assert len(v) == 12
    for a, w in zip(v, want):
        ltr = 0.0
        for x in a:
            ltr = ltr + x
        assert tree_sum(a) == w and u64([ltr])[0] != u64([w])[0], (w, ltr)
        # exchanging the two last levels (rows 0 + 2, 1 + 3) is another association too, where those levels decide
    a = v[8]                                             # s = 32, the xor-16 level
    r = [tree_sum(np.concatenate([a[32 * k:32 * k + 32], np.zeros(96)])) for k in range(4)]
    assert (r[0] + r[2]) + (r[1] + r[3]) != (r[0] + r[1]) + (r[2] + r[3])


# ---- the twin against the independent references ------------------------------------------------------------------------------------
def check_unary(mp, x, got, ref_fn, bound_ulps, exact):
    """exact(x) -> the required result where the function's value is not a finite real (or None); else |got - ref| <= bound_ulps"""
    worst, at = 0.0, None
    for xi, gi in zip(x.tolist(), got.tolist()):
        e = exact(xi)
        if e is not None:
            assert same_bits(gi, e), (xi, gi, e)
            continue
        assert math.isfinite(gi), (xi, gi)
        err = ulps_mp(gi, ref_fn(mp.mpf(xi)))
        if err > worst:
            worst, at = err, xi
    assert worst <= bound_ulps, (worst, at)
    return worst, at


def log_exact(x):
    if x != x:
        return math.nan
    if x < 0:
        return math.nan
    if x == 0:
        return -math.inf
    return math.inf if x == math.inf else (0.0 if x == 1.0 else None)


def test_log(results, mp):
    for name in ("log", "sweep/log"):
        b, (got,) = results[0][name]
        worst = check_unary(mp, b.cols[0], got, mp.log, 4.0, log_exact)
        print("%s: %d inputs, worst %.3g ulp at %r" % (name, b.n, worst[0], worst[1]))


def exp_exact(x):
    if x != x:
        return math.nan
    if x > EXP_HI:
        return math.inf
    return 0.0 if x < EXP_LO else None


def test_exp_and_its_contract(results, mp):
    """exp <= 2 ulp; 0 (positive) below the lower threshold, +inf above the upper one, and never a subnormal result: the smallest
    argument that is not cut off gives a normal number"""
    for name in ("exp", "sweep/exp"):
        b, (got,) = results[0][name]
        worst = check_unary(mp, b.cols[0], got, mp.exp, 2.0, exp_exact)
        print("%s: %d inputs, worst %.3g ulp at %r" % (name, b.n, worst[0], worst[1]))
        x = b.cols[0]
        assert (got[x >= EXP_LO] >= 2.0 ** -1022).all() and np.isfinite(got[x <= EXP_HI]).all()
        assert same_bits(got[x < EXP_LO], 0.0).all() and (got[x > EXP_HI] == np.inf).all()
        assert same_bits(got[x == 0.0], 1.0).all()


def log1p_exact(x):
    if x != x or x < -1.0:
        return math.nan
    if x == -1.0:
        return -math.inf
    if x == math.inf:
        return math.inf
    return x if x == 0.0 else None                        # the sign of zero is kept


def test_log1p(results, mp):
    for name in ("log1p", "sweep/log1p"):
        b, (got,) = results[0][name]
        worst = check_unary(mp, b.cols[0], got, mp.log1p, 4.0, log1p_exact)
        print("%s: %d inputs, worst %.3g ulp at %r" % (name, b.n, worst[0], worst[1]))


def test_sincos2pi(results, mp):
    b, (s, c) = results[0]["sincos"]
    worst = 0.0
    for u, si, ci in zip(b.cols[0].tolist(), s.tolist(), c.tolist()):
        t = 2 * mp.pi * mp.mpf(u)
        worst = max(worst, float(abs(mp.mpf(si) - mp.sin(t))), float(abs(mp.mpf(ci) - mp.cos(t))))
    print("sincos2pi: %d inputs, worst absolute error %.3g" % (b.n, worst))
    assert worst < 1e-15
    u = b.cols[0]
    assert (s[u == 0.25] == 1.0).all() and (c[u == 0.5] == -1.0).all() and (s[u == 0.75] == -1.0).all() and same_bits(s[u == 0.0], 0.0).all()


def test_logaddexp(results, mp):
    """Non-finite arguments short-circuit to `x > y ? x : y` (reference src/InplaceDHMC.jl:27-30): the larger one when neither is a
    NaN, which is also the limit of log(e^x + e^y); with a NaN the second argument, as test_oracle_math pins it.  Finite arguments:
    r = M + log1p(exp(-d)), M the larger one and d >= 0 the rounded difference.  The last addition rounds once (ulp(r) / 2); log1p <=
    ln 2 is within 4 ulp of itself (4 * 1.2e-16) of a 2-ulp exp (another 2 * 2.3e-16 * e / (1 + e) <= 2.3e-16), and rounding d moves
    exp(-d) by d e^-d 2^-53 <= 5e-17: ulp(r) / 2 + 8e-16 in all."""
    b, (xy, yx) = results[0]["logaddexp"]
    x, y = b.cols
    worst = 0.0
    for xi, yi, g1, g2 in zip(x.tolist(), y.tolist(), xy.tolist(), yx.tolist()):
        if not (math.isfinite(xi) and math.isfinite(yi)):
            assert same_bits(g1, xi if xi > yi else yi) and same_bits(g2, yi if yi > xi else xi), (xi, yi, g1, g2)
            if xi == xi and yi == yi:
                assert g1 == max(xi, yi) == g2
            continue
        M, m = mp.mpf(max(xi, yi)), mp.mpf(min(xi, yi))
        ref = M + mp.log1p(mp.exp(m - M))
        bound = 0.5 * float(np.spacing(abs(float(ref)))) + 8e-16
        assert abs(mp.mpf(g1) - ref) <= bound and abs(mp.mpf(g2) - ref) <= bound, (xi, yi, g1, g2, ref)
        assert g1 == g2 or xi == yi
        worst = max(worst, float(abs(mp.mpf(g1) - ref)) / bound)
    print("logaddexp: %d pairs, worst error %.3g of the bound" % (b.n, worst))


LGAMMA_BOUND = 5e-14


def within_lgamma_bound(mp, got, ref):
    """|got - f| <= 5e-14 (1 + |f|).  Where f leaves the doubles the same statement reads: got is the infinity of
    f's sign exactly if some value inside the bound already rounds to it, and must be it if every value inside the bound does."""
    big = mp.mpf(2) ** 1024 - mp.mpf(2) ** 970
    slack = LGAMMA_BOUND * (1 + abs(ref))
    if math.isinf(got):
        return abs(ref) + slack >= big and (got > 0) == (ref > 0)
    return abs(ref) - slack < big and abs(mp.mpf(got) - ref) <= slack


def test_lgamma_psi(results, mp):
    b, (lg, ps) = results[0]["lgamma_psi"]
    x = b.cols[0]
    worst = [0.0, 0.0]
    for xi, l, p in zip(x.tolist(), lg.tolist(), ps.tolist()):
        if xi != xi:
            assert l != l and p != p
        elif not xi > 0.0:
            assert l == math.inf and p != p, (xi, l, p)
        elif xi == math.inf:
            assert l == math.inf and p == math.inf
        else:
            X = mp.mpf(xi)
            rl, rp = mp.loggamma(X), mp.digamma(X)
            assert within_lgamma_bound(mp, l, rl), ("ln Gamma", xi, l, rl)
            assert within_lgamma_bound(mp, p, rp), ("psi", xi, p, rp)
            if math.isfinite(l):
                worst[0] = max(worst[0], float(abs(mp.mpf(l) - rl) / (1 + abs(rl))))
            if math.isfinite(p):
                worst[1] = max(worst[1], float(abs(mp.mpf(p) - rp) / (1 + abs(rp))))
    print("lgamma_psi: %d inputs, worst |error| / (1 + |f|): ln Gamma %.3g, psi %.3g" % (b.n, worst[0], worst[1]))
    assert (ps[(x > 0) & (x < 2.0 ** -1024)] == -np.inf).all() and np.isfinite(ps[x == 2.0 ** -1022]).all()
    assert abs(ps[x == PSI_ZERO][0]) < 1e-15


def test_lgamma_overflow_edge(results, mp):
    """Between x1 (past it (x - 1/2) log x overflows) and x2 (past it ln Gamma(x) does) lie 9.3e12 doubles whose ln Gamma is a
    finite double; the table holds 40 of them and both ends, and the twin's result there is finite."""
    x1, x2 = lgamma_edges()
    with np.errstate(over="ignore"):
        assert x1 < x2 and np.isfinite(x1 * np.log(x1)) and not np.isfinite(np.nextafter(x1, np.inf) * np.log(np.nextafter(x1, np.inf)))
    big = mp.mpf(2) ** 1024 - mp.mpf(2) ** 970
    assert mp.loggamma(mp.mpf(float(ulp_step(x2, -64)))) < big < mp.loggamma(mp.mpf(float(ulp_step(x2, 64))))
    b, (lg, _) = results[0]["lgamma_psi"]
    x = b.cols[0]
    inside = (x > ulp_step(x1, 64)) & (x < ulp_step(x2, -64))
    assert inside.sum() >= 38 and np.isfinite(lg[inside]).all()
    assert (lg[x > ulp_step(x2, 64)] == np.inf).all()


def test_primitives_are_correctly_rounded(results):
    """the premise of DESIGN section 4 on the host side: the twin's / sqrt rint, (int), (double) and fma against numpy's correctly
    rounded operations and exact rational arithmetic"""
    R = results[0]
    b, (quo, inv) = R["div"]
    a, d = b.cols
    with np.errstate(all="ignore"):
        assert same_bits(quo, a / d).all() and same_bits(inv, 1.0 / a).all()
        sub = np.abs(a / d)
    assert ((sub > 0) & (sub < 2.0 ** -1022)).sum() >= 50 and np.isinf(sub[np.isfinite(a) & (d != 0)]).sum() >= 50
    for k in np.flatnonzero(np.isfinite(a) & np.isfinite(d) & (d != 0) & (a != 0))[::37]:          # numpy's own division against the rationals
        assert same_bits(quo[k], round_fraction(Fraction(float(a[k])) / Fraction(float(d[k])), math.copysign(0.0, a[k] * np.sign(d[k]))))
    b, (got,) = R["sqrt"]
    with np.errstate(invalid="ignore"):
        assert same_bits(got, np.sqrt(b.cols[0])).all()
    for name in ("rint", "sweep/rint"):
        b, (got,) = R[name]
        assert same_bits(got, np.rint(b.cols[0])).all()
    b, (got,) = R["rint"]
    x = b.cols[0]
    assert same_bits(got[x == 0.5], 0.0).all() and same_bits(got[x == -0.5], -0.0).all() and (got[x == 2.5] == 2.0).all()
    b, (got,) = R["d2i2d"]
    assert same_bits(got, np.trunc(b.cols[0]) + 0.0).all() and got.min() == -2147483648.0 and got.max() == 2147483647.0
    b, (got, _, _, _) = R["fma"]
    fa, fb, fc = b.cols
    want = np.array([fma_reference(*t) for t in zip(fa.tolist(), fb.tolist(), fc.tolist())])
    assert same_bits(got, want, nan_equal=False).all(), np.flatnonzero(~same_bits(got, want))[:5]
    with np.errstate(all="ignore"):
        assert (~same_bits(want, fa * fb + fc)).sum() >= 500                   # triples on which the unfused form differs
    b, outs = R["fma_c"]
    pa, pb = b.cols
    for cst, got in zip(FMA_C_CONSTANTS, outs):
        want = np.array([fma_reference(x, y, cst) for x, y in zip(pa.tolist(), pb.tolist())])
        assert same_bits(got, want, nan_equal=False).all(), (cst, np.flatnonzero(~same_bits(got, want))[:5])


def test_rng_helpers(results):
    R = results[0]
    lo, hi = table_u01()
    v = ((hi << np.uint64(32)) | lo) >> np.uint64(11)
    b, (got,) = R["u01"]
    want = np.array([int(t) / 2.0 ** 53 for t in v])                           # v < 2^53: exact
    assert same_bits(got, want, nan_equal=False).all() and got.min() == 0.0 and got.max() == 1.0 - 2.0 ** -53
    b, (got,) = R["u01_open0"]
    want = np.array([(int(t) + 1) / 2.0 ** 53 for t in v])
    assert same_bits(got, want, nan_equal=False).all() and got.min() == 2.0 ** -53 and got.max() == 1.0
    b, (o01, o23, _, _) = R["philox"]
    words = table_philox()
    ref = philox_reference(words)
    for k, (_, _, out) in enumerate(PHILOX_KAT):
        assert tuple(int(t) for t in ref[k]) == out
    assert np.array_equal(u64(o01), ref[:, 0] | (ref[:, 1] << np.uint64(32))) and np.array_equal(u64(o23), ref[:, 2] | (ref[:, 3] << np.uint64(32)))


def test_randn_from_uniforms(results, mp):
    """n = sqrt(-2 ln u1) (cos, sin)(2 pi u2): the radius carries log's 4 ulp, halved by the root, and two roundings (< 4 * 2.3e-16
    relative), the angle 1e-15 absolute: r * 2e-15 in all"""
    b, (n0, n1) = results[0]["randn"]
    u1, u2 = b.cols
    for a, c, g0, g1 in zip(u1.tolist(), u2.tolist(), n0.tolist(), n1.tolist()):
        r = mp.sqrt(-2 * mp.log(mp.mpf(a)))
        t = 2 * mp.pi * mp.mpf(c)
        bound = float(r) * 2e-15
        assert abs(mp.mpf(g0) - r * mp.cos(t)) <= bound and abs(mp.mpf(g1) - r * mp.sin(t)) <= bound, (a, c, g0, g1)
    assert np.abs(np.stack([n0, n1])).max() < 8.6 and (n0[u1 == 1.0] == 0.0).all()


def test_reductions(results):
    """every lane's copy is the tree's value; the tree is the canonical order (numpy restatement), exact on the cancellation
    vectors, and within 7 roundings (2^-53 sum |a_i| each) of math.fsum where the sum is finite"""
    b, (g,) = results[0]["reduce"]
    a, bb = b.cols
    _, want = cancellation_vectors()
    for k in range(b.n):
        second = np.concatenate([bb[k], bb[k][-1:]])
        S, T = tree_sum(a[k]), tree_sum(second)
        assert same_bits(g[k, 0:128], S).all() and same_bits(g[k, 128::2], T).all(), k
        x0 = a[k][0::2]
        with np.errstate(invalid="ignore", over="ignore"):
            rows = (x0[0:16] + x0[16:32]) + (x0[32:48] + x0[48:64])
        assert same_bits(g[k, 129::2], np.tile(rows, 4)).all(), k
        if np.isfinite(a[k]).all() and np.isfinite(S):
            sc = 2.0 ** -8 if np.abs(a[k]).max() > 1e300 else 1.0    # exact there, and keeps the sum of |a_i| inside the doubles
            assert abs(sc * S - math.fsum(sc * a[k])) <= 7 * 2.0 ** -53 * math.fsum(np.abs(sc * a[k])), k
    assert same_bits(g[12:24, 0], want).all()
    assert same_bits(g[26, 0], -0.0) and g[24, 0] == np.inf and g[25, 0] != g[25, 0]


def test_probe_log_density_is_the_first_chunks_tree(results):
    _, q, g, lq = results
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.array([tree_sum(r[:128]) for r in q])
    want = np.where(np.isfinite(want), want, -np.inf)
    assert same_bits(lq, want, nan_equal=False).all()
