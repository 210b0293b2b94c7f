"""Exact stationarity: the statistics behind test_stationarity_cpu.py and test_gpu_stationarity.py.

A NUTS transition with a fixed stepsize and metric leaves its target exactly invariant.  Start every chain at an exact,
independent draw from the target, apply transitions, and the chains are still exact independent draws: every statistic
below then has an exact null distribution (chains are independent; no effective sample size enters).  The only slack is
the divergence threshold (min_delta = -1000 nats), whose weight is about e^-1000.

Draws are reduced to standard form before they are judged: z = the standardised coordinates for the Gaussians (iid N(0, 1)
under the target), u = F(x) per coordinate for the other densities (iid U(0, 1)).  Every statistic becomes a p-value and all
p-values of one test form one family, judged by a single Bonferroni threshold FWER / m: seeds are fixed, so a correct kernel
passes deterministically, and a legitimate change that moves bits moves each test's false-alarm chance by at most FWER.

Non-triviality is measured too, since a transition that does nothing is also exactly invariant."""
import numpy as np
from scipy import special, stats

FWER = 1e-4        # family-wise false-alarm rate of one test


# ---- exact samplers and their probability-integral transforms ----------------------------------------------------

def diag_target(D):
    """the diagonal Gaussian of these tests: scales over one decade"""
    sigma = np.logspace(-0.5, 0.5, D)
    mu = np.sin(np.arange(D, dtype=np.float64))
    return mu, sigma


def diag_gaussian(rng, n, mu, sigma):
    return mu + sigma * rng.standard_normal((n, len(mu)))


def dense_mvn(D, seed=7):
    """the dense MVN of test_gpu_dense.dense_problem (same construction, same seed) with its eigen-decomposition:
    Sigma = Q diag(lam) Q', P = Sigma^-1"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = np.logspace(-2, 0, D)
    P = (Q / lam) @ Q.T
    P = 0.5 * (P + P.T)
    mu = np.cos(np.arange(D, dtype=np.float64))
    return dict(mu=mu, P=P, Q=Q, lam=lam)


def dense_draws(rng, n, prob):
    """q = mu + Q diag(sqrt(lam)) n"""
    return prob["mu"] + (rng.standard_normal((n, len(prob["mu"]))) * np.sqrt(prob["lam"])) @ prob["Q"].T


def dense_z(q, prob):
    return ((q - prob["mu"]) @ prob["Q"]) / np.sqrt(prob["lam"])


def logistic_draws(rng, n, loc, scale):
    u = rng.random((n, len(loc)))
    return loc + scale * (np.log(u) - np.log1p(-u))


def logistic_u(x, loc, scale):
    return special.expit((x - loc) / scale)


def truncnorm_draws(rng, n, D, a):
    """N(0, 1) truncated to |x| < a, iid over D coordinates"""
    return stats.truncnorm(-a, a).rvs(size=(n, D), random_state=rng)


def truncnorm_u(x, a):
    return stats.truncnorm(-a, a).cdf(x)


# ---- the decision rule ------------------------------------------------------------------------------------------

class Family:
    """all p-values of one test, judged together at family-wise rate FWER (Bonferroni)"""

    def __init__(self, fwer=FWER):
        self.fwer = fwer
        self.groups = []            # (name, array of p-values)

    def add(self, name, p):
        self.groups.append((name, np.atleast_1d(np.asarray(p, dtype=np.float64)).ravel()))

    @property
    def m(self):
        return sum(p.size for _, p in self.groups)

    @property
    def threshold(self):
        return self.fwer / max(self.m, 1)

    def worst(self):
        """(name, smallest p-value) over the family"""
        return min(((name, float(p.min())) for name, p in self.groups if p.size), key=lambda t: t[1])

    def rejects(self):
        return self.worst()[1] < self.threshold

    def report(self):
        name, p = self.worst()
        return "%d p-values, threshold %.3g; smallest %.3g in %s" % (self.m, self.threshold, p, name)

    def z_crit(self):
        """two-sided normal quantile of the per-statistic threshold: the z-score a single mean needs to be rejected"""
        return float(stats.norm.isf(self.threshold / 2))


def assert_stationary(fam, what=""):
    assert not fam.rejects(), "%s: not stationary: %s" % (what, fam.report())


def assert_rejects(fam, what=""):
    assert fam.rejects(), "%s: the statistics do not reject: %s" % (what, fam.report())


def _two_sided(zscore):
    return 2.0 * stats.norm.sf(np.abs(zscore))


def ks_columns(u):
    """per-column two-sided KS p-values of u (n, D) against U(0, 1)"""
    n = u.shape[0]
    s = np.sort(u, axis=0)
    i = np.arange(1, n + 1, dtype=np.float64)[:, None]
    d = np.maximum((i / n - s).max(axis=0), (s - (i - 1) / n).max(axis=0))
    return stats.kstwo.sf(d, n)


def add_gaussian(fam, z, tag):
    """z (n, D) should be iid N(0, 1): per-coordinate mean and mean of z^2 - 1 as z-scores, per-coordinate KS, the sum of
    the squared mean z-scores against chi^2_D (a small bias spread over many coordinates), KS of |z|^2 against chi^2_D"""
    n, D = z.shape
    m = z.mean(axis=0) * np.sqrt(n)
    v = (np.square(z).mean(axis=0) - 1.0) * np.sqrt(n / 2.0)
    fam.add(tag + " mean z", _two_sided(m))
    fam.add(tag + " mean z^2-1", _two_sided(v))
    fam.add(tag + " KS z", ks_columns(special.ndtr(z)))
    fam.add(tag + " chi2 of mean z-scores", stats.chi2.sf(np.dot(m, m), D))
    fam.add(tag + " KS |z|^2", stats.kstest(np.einsum("ij,ij->i", z, z), stats.chi2(D).cdf).pvalue)


def add_uniform(fam, u, tag):
    """u (n, D) should be iid U(0, 1): per-coordinate mean (var 1/12), second moment (mean 1/3, var 4/45), KS, and the
    sum of the squared mean z-scores against chi^2_D"""
    n, D = u.shape
    m = (u.mean(axis=0) - 0.5) * np.sqrt(12.0 * n)
    s = (np.square(u).mean(axis=0) - 1.0 / 3.0) * np.sqrt(45.0 * n / 4.0)
    fam.add(tag + " mean u", _two_sided(m))
    fam.add(tag + " mean u^2", _two_sided(s))
    fam.add(tag + " KS u", ks_columns(u))
    fam.add(tag + " chi2 of mean z-scores", stats.chi2.sf(np.dot(m, m), D))


def add_mean_one(fam, x, tag):
    """x (n,) iid with mean 1 (exp of the energy change of a volume-preserving map from an exact start)"""
    n = x.size
    fam.add(tag + " E[exp(dH)] = 1", _two_sided((x.mean() - 1.0) / (x.std(ddof=1) / np.sqrt(n))))


def add_nonpositive_mean(fam, x, tag):
    """x (n,) with E[x] <= 0 (Jensen on E[exp(dH)] = 1): one-sided"""
    n = x.size
    fam.add(tag + " E[dH] <= 0", stats.norm.sf(x.mean() / (x.std(ddof=1) / np.sqrt(n))))


def add_uncorrelated(fam, a, b, tag):
    """a, b (n, k): column-wise correlations are zero (Fisher: sqrt(n) r ~ N(0, 1) for independent columns)"""
    n = a.shape[0]
    a = (a - a.mean(axis=0)) / a.std(axis=0)
    b = (b - b.mean(axis=0)) / b.std(axis=0)
    r = (a * b).mean(axis=0)
    fam.add(tag, _two_sided(r * np.sqrt(n)))


# ---- non-triviality ---------------------------------------------------------------------------------------------

def moved_fraction(q0, q1):
    return float(np.mean(np.any(q0 != q1, axis=1)))


def mean_corr(z0, z1):
    """mean over coordinates of the correlation of a coordinate before and after"""
    a = (z0 - z0.mean(axis=0)) / z0.std(axis=0)
    b = (z1 - z1.mean(axis=0)) / z1.std(axis=0)
    return float((a * b).mean(axis=0).mean())


def terminations(ts):
    """fractions of trees ending at the depth limit, in a divergence, in a U-turn (src/tree.jl:285, :300)"""
    left, right = np.asarray(ts["term_left"]), np.asarray(ts["term_right"])
    n = left.size
    maxd = np.mean((left == 1) & (right == 0))
    div = np.mean(left == right)
    return dict(max_depth=float(maxd), divergence=float(div), turning=float(1.0 - maxd - div),
                mean_depth=float(np.mean(ts["depth"])), n=n)


def detectable_bias(n, fam):
    """the smallest mean shift, in units of sigma, that one coordinate's mean z-score rejects at this family's threshold"""
    return fam.z_crit() / np.sqrt(n)


# ---- two user densities, as HIP source for the engine (hipRTC) and as C source for the oracle ----------------------
# The separable logistic: l(q) = -sum |x_i| + 2 log1p(exp(-|x_i|)), x_i = (q_i - loc_i) / scale_i, grad = -tanh(x/2) / scale;
# params = [loc (D), scale (D)].  Reaches the device dexp / dlog1p.
LOGISTIC_HIP = r"""
template <int NCH>
__device__ double logdensity_and_gradient(const Vec<NCH> &q, Vec<NCH> &grad, const UserCtx &ctx)
{
    const double *loc = ctx.params, *scale = ctx.params + ctx.D;
    double l0 = 0.0, l1 = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int i0 = 128 * j + 2 * ctx.lane;
        double g0 = 0.0, g1 = 0.0;
        if (i0 < ctx.D) {
            const double x = (q.c[j].x - loc[i0]) / scale[i0], ax = x < 0.0 ? -x : x, e = dexp(-ax);
            l0 = l0 + (ax + 2.0 * dlog1p(e));
            const double t = (1.0 - e) / ((1.0 + e) * scale[i0]);
            g0 = x < 0.0 ? t : -t;
        }
        if (i0 + 1 < ctx.D) {
            const double x = (q.c[j].y - loc[i0 + 1]) / scale[i0 + 1], ax = x < 0.0 ? -x : x, e = dexp(-ax);
            l1 = l1 + (ax + 2.0 * dlog1p(e));
            const double t = (1.0 - e) / ((1.0 + e) * scale[i0 + 1]);
            g1 = x < 0.0 ? t : -t;
        }
        grad.c[j].x = g0;
        grad.c[j].y = g1;
    }
    return -wave_sum(l0, l1);
}
"""

LOGISTIC_C = r"""
#include "orc_math.h"
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    const double *loc = params, *scale = params + D;
    double lac[128];
    for (int r = 0; r < 128; ++r) lac[r] = 0.0;
    for (int j = 0; j < L; j += 128)
        for (int r = 0; r < 128; ++r) {
            const int i = j + r;
            grad[i] = 0.0;
            if (i >= D) continue;
            const double x = (q[i] - loc[i]) / scale[i], ax = x < 0.0 ? -x : x, e = orc_exp(-ax);
            lac[r] = lac[r] + (ax + 2.0 * orc_log1p(e));
            const double t = (1.0 - e) / ((1.0 + e) * scale[i]);
            grad[i] = x < 0.0 ? t : -t;
        }
    return -orc_tree128(lac);
}
"""

# N(0, 1) truncated to the box |q_i| < a = params[0]: l(q) = -|q|^2 / 2 inside, -Inf outside (a non-finite log density is
# -Inf, src/kinetic_energy.jl:80-84), so a trajectory that leaves the box ends in a divergence.
TRUNCNORM_HIP = r"""
template <int NCH>
__device__ double logdensity_and_gradient(const Vec<NCH> &q, Vec<NCH> &grad, const UserCtx &ctx)
{
    const double a = ctx.params[0];
    double l0 = 0.0, l1 = 0.0, o0 = 0.0, o1 = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int i0 = 128 * j + 2 * ctx.lane;
        const double x = q.c[j].x, y = q.c[j].y;
        grad.c[j].x = (i0 < ctx.D) ? -x : 0.0;
        grad.c[j].y = (i0 + 1 < ctx.D) ? -y : 0.0;
        l0 = l0 + x * x;
        l1 = l1 + y * y;
        o0 = o0 + ((i0 < ctx.D && !(x < a && x > -a)) ? 1.0 : 0.0);
        o1 = o1 + ((i0 + 1 < ctx.D && !(y < a && y > -a)) ? 1.0 : 0.0);
    }
    const double outside = wave_sum(o0, o1);
    const double l = -0.5 * wave_sum(l0, l1);
    return outside > 0.0 ? -__builtin_inf() : l;
}
"""

TRUNCNORM_C = r"""
#include "orc_math.h"
#include <math.h>
double logdensity_and_gradient(const double *q, double *grad, int D, int L, const double *params)
{
    const double a = params[0];
    double lac[128];
    int outside = 0;
    for (int r = 0; r < 128; ++r) lac[r] = 0.0;
    for (int j = 0; j < L; j += 128)
        for (int r = 0; r < 128; ++r) {
            const int i = j + r;
            const double x = q[i];
            grad[i] = i < D ? -x : 0.0;
            lac[r] = lac[r] + x * x;
            if (i < D && !(x < a && x > -a)) outside = 1;
        }
    const double l = -0.5 * orc_tree128(lac);
    return outside ? -INFINITY : l;
}
"""
