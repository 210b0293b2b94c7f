"""Ready-made observation sources for GLM(X, Y, source, constants) (include/idhmc.h, IDHMC_MODEL_GLM).

Each defines glm_observation(z, o, r, v): v = -log p(y | z) up to a term that depends on the data only, r = d log p(y | z) / dz.
None of them returns a NaN for a finite z whose product with the count is finite (a count of 2^53 at z = 1e300 is inf - inf in the
Poisson sources); each is finite wherever the log density itself is a double (Poisson: exp of the linear predictor below 709.78;
STUDENT_T_IDENTITY: (y - z) / sigma finite, and below |u| = 1e100 nu inside what the arithmetic holds -- u^2 / nu, (nu + 1) |u| and
sigma (nu + u^2) finite, which every nu between 1e-108 and 1e208 is at sigma = 1; everything else: every finite z).  Two statements hold for every source on this page,
and tests/test_glm_terms_edges_cpu.py asserts them with every end named below:
  * The engine accumulates -2 log p, so a chain's l(q) is finite while 2 v is.  Where v is an exponential that ends at
    709.08 = log(max / 2), not at dexp's own 709.78: Poisson's linear predictor, Weibull's w, gamma's w and a0 + w.  Between the
    two v, r and s are finite and l(q) reads -inf.
  * dexp returns 0 below -708.39, where exp is below the smallest normal double 2.2e-308, so a term c exp(x) of v, r or s is dropped
    there: an absolute error below 2.3e-308 |c| (c a count, phi, k or a distance log t - z), whatever the other terms are.  Apart from
    that every output is within 1e-12 of the sum of the magnitudes of its terms over the whole promised range.

  POISSON_LOG         K = 1: y = count;                     log mu = z
  POISSON_LOG_OFFSET  K = 2: y = (count, log exposure);     log mu = z + log exposure
  BINOMIAL_LOGIT      K = 2: y = (successes, trials);       logit p = z
  BERNOULLI_LOGIT     K = 1: y = 0 or 1;                    logit p = z  (the built-in LogisticRegression's arithmetic)
  STUDENT_T_IDENTITY  K = 1, constants (nu, sigma):         y = z + sigma t_nu

Sources with sampled auxiliary parameters, for GLM(..., aux=A) (IDHMC_MODEL_GLM_AUX).  Each defines
glm_observation(z, o, a, r, v, s): a[j], j < o.A, are the chain's auxiliary coordinates (unconstrained: the source applies the
transform), v = -log p(y | z, a) including the terms that depend on a, r = d log p / dz, s[j] = d log p / da_j.

  GAUSSIAN_IDENTITY_LOGSIGMA   K = 1, A = 1 (log sigma):                    y = z + sigma eps
  STUDENT_T_IDENTITY_LOGSIGMA  K = 1, A = 1 (log sigma), constant nu:       y = z + sigma t_nu
  WEIBULL_LOG_LOGSHAPE         K = 2: y = (log t, event: 1 observed, 0 right-censored), A = 1 (log shape k);  log scale = z

Each is finite wherever the log density itself is, and that ends at the arguments of dexp:
  GAUSSIAN_IDENTITY_LOGSIGMA   a0 > -709.78 (exp(-a0) finite) and |y - z| exp(-a0) < 1.3e154 (its square finite); every larger a0
                               is fine (past 708.4 exp(-a0) is 0 and v = a0).  In particular every |a0| <= 300 with |y - z| <= 1e3.
  STUDENT_T_IDENTITY_LOGSIGMA  a0 > -708.39 (sigma = exp(a0) not 0) and (y - z) / sigma finite; every larger a0 is fine (past 709.78
                               sigma is inf, u is 0 and v = a0); nu as for STUDENT_T_IDENTITY, and sigma (nu + u^2) a normal double
                               (it is a product here).  In particular every |a0| <= 700 with |y - z| <= 1e3 at nu = 1 .. 4.
  WEIBULL_LOG_LOGSHAPE         a0 < 709.78 (k = exp(a0) finite) and w = k (log t - z) < 709.08 (twice the cumulative hazard exp(w)
                               finite); every more negative finite w is fine (the score w H leaves the doubles before v does).
Past those ends v is +inf or NaN, which the engine reads as l(q) = -inf: the ordinary rejected point.

Sources whose sampled dispersion sits inside a gamma function, for GLM(..., aux=1); a[0] is the log of the
dispersion.  They call dlgamma_psi(x, lg, psi) of idhmc_math.hpp: ln Gamma(x) and psi(x) = d/dx ln Gamma(x), x > 0, from one call
(dlgamma(x) and ddigamma(x) return one of the two).  A source of the user's, GLM or CustomDensity, may call all three.

  NEG_BINOMIAL_LOG_LOGPHI  K = 1: y = count, A = 1 (log phi);  log mu = z, variance mu + mu^2 / phi   (drops -ln Gamma(y + 1))
  GAMMA_LOG_LOGSHAPE       K = 1: y = log of the response (gamma_response), A = 1 (log shape k);  log mu = z   (drops -log y)
  BETA_LOGIT_LOGPHI        K = 2: y = (log y, log(1 - y)) (beta_response), A = 1 (log precision phi);  logit mu = z; the
                           density's shapes are p = phi mu, q = phi (1 - mu)   (drops -log y - log(1 - y))

Each is finite wherever the log density itself is, and that ends at:
  NEG_BINOMIAL_LOG_LOGPHI  -708.39 < a0 < 703 (phi = exp(a0) not 0, ln Gamma(phi) finite); every |a0| <= 700 with |z| <= 700.
                           At large phi the score phi (psi(y + phi) - psi(phi) - softplus(z - a0)) is a difference of terms of
                           size phi |psi(phi)| and loses about phi 1e-16 |psi(phi)| absolutely as the model approaches its
                           Poisson limit (1e-10 at phi = 1e5; measured against mpmath: at most 1.3 times that for
                           phi = 1e5 .. 1e15, counts 0 .. 7 and mu <= phi): stated, not engineered around.
  GAMMA_LOG_LOGSHAPE       -708.39 < a0 < 703 (k = exp(a0) not 0, ln Gamma(k) finite) and 2 k exp(log y - z) finite: w = log y - z
                           below 709.08 and a0 + w below 709.08; every more negative w is fine.
  BETA_LOGIT_LOGPHI        -708.39 < a0 < 703 (phi not 0, ln Gamma(phi) finite) and p = phi sigma(z), q = phi sigma(-z) both at
                           least 2.3e-308 (a p or q that underflows to 0 has ln Gamma = +inf, a subnormal one psi = -inf):
                           -|z| + a0 > -708 and |z| < 708.39 (past it exp(-|z|) is 0 and so is p or q, whatever a0).  In particular
                           |z| <= 700 with -5 <= a0 <= 700, and |z| <= 40 with |a0| <= 650.
Past those ends v is +inf or NaN as above.

Every source above works unchanged with coefficient groups, GLM(..., groups=...): the sampled coordinates are
[u (Dx) | a (A) | omega (H)]; coefficients(model, draws) turns draws into beta = s * u, group_scales(model, draws) into
sigma = exp(omega).

Every source above also works unchanged with several responses, GLM(..., chains_per_response=R): Y is (M, n, K)
and the chain of global id g samples the posterior of Y[g // R].  response_of_chain(model, nchains, first_chain) names each chain's
response and by_response(model, draws, first_chain) sorts draws (or any per-chain array) by it.

Priors beyond the Gaussian, GLM(..., prior_kind=..., prior_nu=...) (idhmc_create_glm_priors): every sampled
coordinate has a kind next to its prior_mu and prior_tau, and every source above works unchanged with them.  d = q - mu:

  PRIOR_NORMAL              q ~ N(mu, 1 / tau)                                          (the default, on every coordinate)
  PRIOR_STUDENT_T           q = mu + t_nu / sqrt(tau)                                   (Cauchy: nu = 1)
  PRIOR_LOG_HALF_NORMAL     exp(q) is half-normal with scale exp(mu)
  PRIOR_LOG_HALF_STUDENT_T  exp(q) is half-t_nu with scale exp(mu)                      (half-Cauchy: nu = 1)
  PRIOR_LOG_EXPONENTIAL     exp(q) is exponential with mean exp(mu)

The log kinds are for the coordinates that are logarithms -- a (the A auxiliary coordinates of the sources above) and omega (the H
group scales) -- and include the Jacobian of exp; they take tau = 1.  priors(Dx, A, H, coefficients=, aux=, scales=) assembles the
four keyword arguments from normal(), student_t(), half_normal(), half_student_t() and exponential().

Each is finite wherever the log density itself is, and that ends at the arguments of dexp and at the square of d:
  PRIOR_STUDENT_T           tau d^2 finite: |d| < 1.3e154 / sqrt(tau); and nu inside what the row's arithmetic holds: tau d^2 / nu
                            finite (below it -2 log p is +inf where the density is not) and (nu + 1) tau |d| finite (the gradient).
  PRIOR_LOG_HALF_NORMAL     2 d < 709.78 (exp(2 d) finite); every more negative d is fine (exp(2 d) is 0 and -2 log p = -2 d).
  PRIOR_LOG_HALF_STUDENT_T  2 d < 709.78, as above, for -2 log p; its gradient is finite while (nu + 1) exp(2 d) is:
                            2 d < 709.78 - log(nu + 1); and exp(2 d) / nu finite, as for PRIOR_STUDENT_T.
  PRIOR_LOG_EXPONENTIAL     d < 709.08 (2 exp(d) finite); every more negative d is fine.
Past those ends -2 log p is +inf, which the engine reads as l(q) = -inf: the ordinary rejected point.  Inside them each row is
within 1e-12 of the magnitude of its terms, with the floor 2.3e-308 max(1, nu + 1, (nu + 1) / nu) for the two t kinds: tau d, tau d^2
and their quotient by nu are multiples of 4.9e-324 once they are in the subnormals.

Per-coefficient local scales, GLM(..., local=..., slab_scale=...) (idhmc_create_glm_local): the horseshoe and its
regularised form, and every source above works unchanged with them.  The J flagged columns of X, in ascending column order, each get
a sampled coordinate lambda_k, the LOGARITHM of the column's local scale: q = [u (Dx) | a (A) | omega (H) | lambda (J)].  A flagged
column of group g has s = exp(omega_g) exp(lambda_k) (exp(lambda_k) alone in no group) and beta_c = u_c st, with st = s without a
slab and st = s / sqrt(1 + s^2 / S^2) with the fixed slab scale S (evaluated as 1 / sqrt(1 / s^2 + 1 / S^2): st -> S as s grows).
local_scales(model, draws) gives exp(lambda), coefficients() and group_scales() take the longer vector, priors(Dx, A, H, J,
local_scales=...) has the fourth role, and horseshoe(Dx, columns, global_scale, ...) assembles the whole model: u ~ N(0, 1),
half-t(nu_local) on every local scale, half-t(nu_global, global_scale) on the scale of the group the columns form.
With a slab every finite q is finite but for one corner, omega_g past 709.78 met by lambda_k below -708.39 or the reverse: inf * 0
is NaN, the rejected point (and accurate while omega_g and lambda_k are each above -708.39: below it dexp gives 0 and
the product with the other factor is lost, whatever its size).  Without one, omega_g + lambda_k past 709.78 makes s infinite and the coefficient infinite or
NaN: l reads as -inf, the ordinary rejected point.  With a slab and s below about 1.5e-154 the square of 1 / s overflows and st is 0
where it should be s: an absolute error below 1.5e-154 |u| in the coefficient (the overflow itself sits at 7.5e-155), stated and not
engineered around.  d log st / d log s is formed as a difference and is accurate to 1e-16 absolutely, not relatively, where s >> S.

Factor terms by level index, GLM(..., factors=[idx, ...]) (idhmc_create_glm_factors): a random intercept per subject,
site or item, (1 | subject), and every source above works unchanged with them.  X holds the Dd dense columns; factor f has N_f levels and
an index idx_f[i] in 0 .. N_f-1 per observation, and its levels are the columns off_f .. off_f + N_f - 1 of the model, off_f = Dd + N_0 +
.. + N_{f-1}, which are never stored: z_i = (X b)_i + sum_f b[off_f + idx_f[i]].  Groups, local scales and priors count all Dx = Dd +
sum N_f columns.  expand_factors(X, factors) is the same model with its indicator columns written out -- the engine computes the same
bits on both -- factor_columns(model, f) the slice of factor f, and random_intercepts(Dd, levels, ...) the groups and priors that give
each factor a sampled scale of its own.

Random slopes, factors=[subject, term(subject, values=x)] (idhmc_create_glm_slopes): a term may carry a finite value
w_f[i] per observation next to its level index, and then z_i takes w_f[i] b[off_f + idx_f[i]] (one fma) where a plain term adds
b[off_f + idx_f[i]].  Its N_f columns are columns of the model like any other term's and are never stored; two terms may share one index
array.  (1 + x | subject) is factors=[subject, term(subject, values=x)] with **random_intercepts(Dd, [N, N]) (random_effects is the same
function under the name that fits): the intercepts and the slopes each get a sampled scale of their own, and the two are independent
unless the terms are paired (below).  expand_factors writes w_f[i] where it writes 1.0 for a plain term, and the
engine computes the same bits on both; factor_values(factors, n) is GLM()'s validation of the values.

Correlated random effects, correlated=[pair(0, 1, eta=2.0)] (idhmc_create_glm_corr): up to two pairs of terms with equal
level counts, each with one more sampled coordinate zeta = atanh rho at the end of q.  Level k's column of the second term becomes
rho u_first + sqrt(1 - rho^2) u_second before any scale applies; eta > 0 is LKJ(eta) on the correlation, eta = 0 leaves zeta to its entry
in the prior arrays (normal or Student-t).  correlated_effects(Dd, levels, pairs, eta) assembles groups, priors and correlated;
correlations(model, draws) gives rho and coefficients(model, draws) applies the mix.  A covariance among three or four terms is a
correlation block, correlated=[block((0, 1, 2), eta=2.0)] (idhmc_create_glm_block): the effects of a level are
sigma .* (L u) with L the K x K Cholesky factor of a sampled correlation matrix, LKJ(eta) on it; block_effects assembles the model,
cholesky_factors, correlation_matrix and correlations read draws.  More than one block, K > 4 and a block next to pairs are out of
scope.

Structured terms, structured=[ar1(0, eta=2.0)] or [rw1(0)] (idhmc_create_glm_struct): dependence among the levels of
one term, level k being position k of the sequence.  ut_0 = u_0, ut_k = phi ut_{k-1} + c u_k takes u's place before any scale applies:
the stationary unit-variance AR(1) with a sampled phi = tanh(zeta), zeta one more coordinate at the very end of q, or the first-order
random walk (phi = c = 1, no coordinate).  Up to two structured terms; a structured term is in no pair and takes no local scale.
structured_effects(Dd, levels, structured) assembles groups, priors and structured; autocorrelations(model, draws) gives phi and
coefficients(model, draws) applies the scan.  RW2, a sum-to-zero constraint, seasonal and spatial structures are GMRF terms (below);
AR(p) is out of scope.

GMRF terms, gmrf=[gmrf(0, Q, sum_to_zero=kappa)] (idhmc_create_glm_gmrf): the levels u of one term get
log p(u) = -1/2 u' Q u - 1/2 kappa (sum u)^2 with a sparse symmetric precision Q in place of the iid N(0, 1); no coordinate is added, so
coefficients(), the reported vector and the device summaries are unchanged.  icar_precision(edges, N), rw1_precision(N),
rw2_precision(N) and seasonal_precision(N, period) build the common Q, scale_precision(Q) gives it unit typical marginal variance,
gmrf_effects(Dd, levels, gmrf) assembles groups, priors and gmrf.  Up to two GMRF terms; such a term is in no pair, not structured and
takes no local scale.  Still out of scope: AR(p), a sampled CAR or Leroux autocorrelation, the BYM2 mixing parameter, hard constraints.
"""
import collections

import numpy as np

PRIOR_NORMAL, PRIOR_STUDENT_T, PRIOR_LOG_HALF_NORMAL, PRIOR_LOG_HALF_STUDENT_T, PRIOR_LOG_EXPONENTIAL = range(5)
PRIOR_NAMES = ("NORMAL", "STUDENT_T", "LOG_HALF_NORMAL", "LOG_HALF_STUDENT_T", "LOG_EXPONENTIAL")

POISSON_LOG = r"""
__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)
{
    const double e = dexp(z);
    v = e - o.y[0] * z;
    r = o.y[0] - e;
}
"""

POISSON_LOG_OFFSET = r"""
__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)
{
    const double eta = z + o.y[1];
    const double e = dexp(eta);
    v = e - o.y[0] * eta;
    r = o.y[0] - e;
}
"""

# -log p = s softplus(-z) + (m - s) softplus(z): a sum of non-negative terms for every z
BINOMIAL_LOGIT = r"""
__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)
{
    const double s = o.y[0], f = o.y[1] - o.y[0];
    const double e = dexp(-__builtin_fabs(z));
    const double l = dlog1p(e);
    const double a = z > 0.0 ? z : 0.0, b = z > 0.0 ? 0.0 : -z;
    v = s * (b + l) + f * (a + l);
    const double d = 1.0 + e;
    const double sp = (z >= 0.0 ? 1.0 : e) / d, sn = (z >= 0.0 ? e : 1.0) / d;
    r = s * sn - f * sp;
}
"""

BERNOULLI_LOGIT = r"""
__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)
{
    const double y = o.y[0];
    const double s = y != 0.0 ? -z : z;
    const double e = dexp(-__builtin_fabs(s));
    v = (s > 0.0 ? s : 0.0) + dlog1p(e);
    const double sg = (s >= 0.0 ? 1.0 : e) / (1.0 + e);
    r = y != 0.0 ? sg : -sg;
}
"""

# u = (y - z) / sigma;  -log p = (nu + 1) / 2 log1p(u^2 / nu);  past |u| = 1e100 (u^2 would overflow) the same quantities from
# 1 / u: log1p(u^2 / nu) = 2 log|u| - log nu + log1p(nu / u^2)
STUDENT_T_IDENTITY = r"""
__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)
{
    const double nu = o.c[0], sg = o.c[1];
    const double u = (o.y[0] - z) / sg;
    const double h = 0.5 * (nu + 1.0);
    if (__builtin_fabs(u) < 1e100) {
        v = h * dlog1p(u * u / nu);
        r = (nu + 1.0) * u / (sg * (nu + u * u));
    } else {
        const double iu = 1.0 / u;
        v = h * (2.0 * dlog(__builtin_fabs(u)) - dlog(nu) + dlog1p(nu * iu * iu));
        r = (nu + 1.0) * iu / (sg * (nu * iu * iu + 1.0));
    }
}
"""

# data columns and constants each source expects
SHAPES = {"POISSON_LOG": (1, 0), "POISSON_LOG_OFFSET": (2, 0), "BINOMIAL_LOGIT": (2, 0), "BERNOULLI_LOGIT": (1, 0),
          "STUDENT_T_IDENTITY": (1, 2)}

# u = (y - z) / sigma with sigma = exp(a0);  -log p = u^2 / 2 + a0
GAUSSIAN_IDENTITY_LOGSIGMA = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double w = dexp(-a[0]);
    const double u = (o.y[0] - z) * w;
    v = 0.5 * (u * u) + a[0];
    r = u * w;
    s[0] = u * u - 1.0;
}
"""

# STUDENT_T_IDENTITY with sigma = exp(a0) sampled; the 1 / u branch past |u| = 1e100 as there
STUDENT_T_IDENTITY_LOGSIGMA = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double nu = o.c[0], sg = dexp(a[0]);
    const double u = (o.y[0] - z) / sg;
    const double h = 0.5 * (nu + 1.0);
    if (__builtin_fabs(u) < 1e100) {
        v = h * dlog1p(u * u / nu) + a[0];
        r = (nu + 1.0) * u / (sg * (nu + u * u));
        s[0] = (nu + 1.0) * (u * u) / (nu + u * u) - 1.0;
    } else {
        const double iu = 1.0 / u;
        v = h * (2.0 * dlog(__builtin_fabs(u)) - dlog(nu) + dlog1p(nu * iu * iu)) + a[0];
        r = (nu + 1.0) * iu / (sg * (nu * iu * iu + 1.0));
        s[0] = (nu + 1.0) / (nu * iu * iu + 1.0) - 1.0;
    }
}
"""

# accelerated failure time: shape k = exp(a0), scale exp(z);  w = k (log t - z), cumulative hazard H = exp(w)
# log p = delta (a0 - log t + w) - H  (delta = 0: right-censored at t, log S = -H)
WEIBULL_LOG_LOGSHAPE = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double lt = o.y[0], dl = o.y[1];
    const double k = dexp(a[0]);
    const double w = k * (lt - z);
    const double H = dexp(w);
    v = H - dl * (a[0] - lt + w);
    r = k * (H - dl);
    s[0] = dl + w * (dl - H);
}
"""

# data columns, constants and auxiliary coordinates each of these expects
AUX_SHAPES = {"GAUSSIAN_IDENTITY_LOGSIGMA": (1, 0, 1), "STUDENT_T_IDENTITY_LOGSIGMA": (1, 1, 1), "WEIBULL_LOG_LOGSHAPE": (2, 0, 1)}

# phi = exp(a0), t = z - a0 = log(mu / phi);  -log p = (y + phi) softplus(t) - y t - (ln Gamma(y + phi) - ln Gamma(phi))
# softplus and the sigmoid in BINOMIAL_LOGIT's stable forms; y = 0 gives ln Gamma(phi) - ln Gamma(phi) = 0 exactly
NEG_BINOMIAL_LOG_LOGPHI = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double y = o.y[0];
    const double ph = dexp(a[0]);
    const double t = z - a[0];
    const double e = dexp(-__builtin_fabs(t));
    const double sp = (t > 0.0 ? t : 0.0) + dlog1p(e);
    const double sg = (t >= 0.0 ? 1.0 : e) / (1.0 + e);
    const double yp = y + ph;
    double l1, p1, l0, p0;
    dlgamma_psi(yp, l1, p1);
    dlgamma_psi(ph, l0, p0);
    v = (yp * sp - y * t) - (l1 - l0);
    r = y - yp * sg;
    s[0] = ph * ((p1 - p0) - sp) - r;
}
"""

# shape k = exp(a0), mean exp(z);  w = log(y / mu), E = y / mu;  log p = k (a0 + w - E) - ln Gamma(k) - log y
GAMMA_LOG_LOGSHAPE = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double k = dexp(a[0]);
    const double w = o.y[0] - z;
    const double E = dexp(w);
    const double u = (a[0] + w) - E;
    double lg, ps;
    dlgamma_psi(k, lg, ps);
    v = lg - k * u;
    r = k * (E - 1.0);
    s[0] = k * ((u + 1.0) - ps);
}
"""

# precision phi = exp(a0), mean sigma(z);  p = phi sigma(z) and q = phi sigma(-z), each from its own sigmoid (phi - p would lose q
# where sigma(z) is near 1);  log p(y) = ln Gamma(phi) - ln Gamma(p) - ln Gamma(q) + (p - 1) log y + (q - 1) log(1 - y)
BETA_LOGIT_LOGPHI = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double y0 = o.y[0], y1 = o.y[1];
    const double ph = dexp(a[0]);
    const double e = dexp(-__builtin_fabs(z));
    const double d = 1.0 + e;
    const double sz = (z >= 0.0 ? 1.0 : e) / d, sn = (z >= 0.0 ? e : 1.0) / d;
    const double p = ph * sz, q = ph * sn;
    const double m = p * sn;
    double lp, pp, lq, pq, lf, pf;
    dlgamma_psi(p, lp, pp);
    dlgamma_psi(q, lq, pq);
    dlgamma_psi(ph, lf, pf);
    v = (((lp + lq) - lf) - p * y0) - q * y1;
    r = m * (((y0 - y1) - pp) + pq);
    s[0] = (((ph * pf - p * pp) - q * pq) + p * y0) + q * y1;
}
"""

# data columns, constants and auxiliary coordinates each of these expects
DISPERSION_SHAPES = {"NEG_BINOMIAL_LOG_LOGPHI": (1, 0, 1), "GAMMA_LOG_LOGSHAPE": (1, 0, 1), "BETA_LOGIT_LOGPHI": (2, 0, 1)}


def gamma_response(y):
    """Y of GAMMA_LOG_LOGSHAPE from positive responses: log y, shape (n,)"""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1 or y.size == 0:
        raise ValueError("gamma_response: y must be a non-empty 1-D sequence")
    if not (np.isfinite(y).all() and (y > 0.0).all()):
        raise ValueError("gamma_response: every y must be finite and > 0 (the gamma density's support)")
    return np.log(y)


def beta_response(y):
    """Y of BETA_LOGIT_LOGPHI from proportions strictly inside (0, 1): the columns (log y, log(1 - y)), shape (n, 2)"""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1 or y.size == 0:
        raise ValueError("beta_response: y must be a non-empty 1-D sequence")
    if not (np.isfinite(y).all() and (y > 0.0).all() and (y < 1.0).all()):
        raise ValueError("beta_response: every y must be finite and strictly between 0 and 1 (the beta density's support)")
    return np.stack([np.log(y), np.log1p(-y)], 1)


def _responses(model):
    R = getattr(model, "R", None)
    if R is None:
        raise ValueError("the model has one response (GLM(..., chains_per_response=R) makes one with several)")
    return int(model.M), int(R)


def response_of_chain(model, nchains, first_chain=0):
    """the response each chain of a context samples: integer ids, shape (nchains,), chain c being global chain first_chain + c
    (response = global id // chains_per_response)"""
    M, R = _responses(model)
    nchains, first_chain = int(nchains), int(first_chain)
    if nchains < 1 or first_chain < 0 or first_chain + nchains > M * R:
        raise ValueError("chains %d .. %d are not among the M * chains_per_response = %d * %d chains of the model"
                         % (first_chain, first_chain + nchains - 1, M, R))
    return (first_chain + np.arange(nchains, dtype=np.int64)) // R


def by_response(model, draws, first_chain=0):
    """per-chain values sorted by response: (..., C, D) becomes (C // R, ..., R, D), R = chains_per_response, the leading axis running
    over the responses the C chains cover (all M of them for a context that holds every chain; response first_chain // R comes
    first).  The chains must cover whole responses: first_chain and C multiples of R."""
    M, R = _responses(model)
    draws = np.asarray(draws)
    if draws.ndim < 2:
        raise ValueError("draws must have shape (..., chains, D), got %s" % (draws.shape,))
    C = draws.shape[-2]
    first_chain = int(first_chain)
    response_of_chain(model, C, first_chain)                    # the range check
    if first_chain % R or C % R:
        raise ValueError("chains %d .. %d cover a part of a response only (chains_per_response = %d): whole responses are needed"
                         % (first_chain, first_chain + C - 1, R))
    out = draws.reshape(draws.shape[:-2] + (C // R, R, draws.shape[-1]))
    return np.moveaxis(out, -3, 0)


def _sampled(model, draws):
    """draws as float64, checked against the model's D = Dx + A + H + J + P + Bz + Sz"""
    draws = np.asarray(draws, dtype=np.float64)
    D = (model.Dx + model.A + getattr(model, "H", 0) + getattr(model, "J", 0) + getattr(model, "P", 0) + getattr(model, "Bz", 0)
         + getattr(model, "Sz", 0))
    if draws.shape[-1] != D:
        raise ValueError("draws must have %d coordinates along the last axis, got %d" % (D, draws.shape[-1]))
    return draws


def group_scales(model, draws):
    """sigma_g = exp(omega_g) of a GLM with coefficient groups, shape draws.shape[:-1] + (H,) (H = 0: an empty last axis).  Any
    leading axes: (M, ..., R, D) from by_response works as (..., C, D) does."""
    draws = _sampled(model, draws)
    Dx, A, H = model.Dx, model.A, getattr(model, "H", 0)
    return np.exp(draws[..., Dx + A:Dx + A + H])


def local_scales(model, draws):
    """exp(lambda_k) of a GLM with local scales, shape draws.shape[:-1] + (J,) (J = 0: an empty last axis): the local scale of the k-th
    flagged column, in ascending column order.  Any leading axes, as group_scales."""
    draws = _sampled(model, draws)
    lam0 = model.Dx + model.A + getattr(model, "H", 0)
    with np.errstate(over="ignore"):                            # (a local scale of inf is a value, not an error: the slab bounds its column)
        return np.exp(draws[..., lam0:lam0 + getattr(model, "J", 0)])


def _rho_c(zeta):
    """rho and c of zeta by the device's expressions: s = exp(-|zeta|), t = s s, rho = copysign((1 - t) / (1 + t), zeta), c = 2 s / (1 + t)"""
    s = np.exp(-np.abs(zeta))
    t = s * s
    return np.copysign((1.0 - t) / (1.0 + t), zeta), (2.0 * s) / (1.0 + t)


def correlations(model, draws):
    """rho_p = tanh(zeta_p) of a GLM with correlated pairs of terms (GLM(..., correlated=)), shape draws.shape[:-1] + (P,) (P = 0: an empty
    last axis), computed as the device computes it: exactly +-1 past |zeta| of about 19, never beyond.  Any leading axes, as group_scales."""
    draws = _sampled(model, draws)
    P, Sz = getattr(model, "P", 0), getattr(model, "Sz", 0)
    if getattr(model, "BK", 0):
        # a block: the K (K - 1) / 2 lower entries R_ji of its correlation matrix, row-major, where the pairs' rho would stand
        R = correlation_matrix(model, draws)
        return np.stack([R[..., j, i] for j in range(1, model.BK) for i in range(j)], -1)
    return _rho_c(draws[..., draws.shape[-1] - Sz - P:draws.shape[-1] - Sz])[0]


def cholesky_factors(model, draws):
    """L of a GLM with a correlation block (GLM(..., correlated=[glm.block(..)])), shape draws.shape[:-1] + (K, K), lower triangular with
    L_00 = 1, from the canonical partial correlations z_ji = tanh(zeta_ji) by the device's expressions: L_j0 = z_j0,
    L_j1 = z_j1 c_j0, L_j2 = z_j2 (c_j0 c_j1), L_jj = c_j0 .. c_j,j-1, c = sqrt(1 - z^2) computed as 2 s / (1 + s^2), s = exp(-|zeta|).
    Row j is the block's j-th term, in the order the block names them.  Any leading axes, as group_scales."""
    draws = _sampled(model, draws)
    K, Sz = getattr(model, "BK", 0), getattr(model, "Sz", 0)
    if not K:
        raise ValueError("the model has no correlation block (GLM(..., correlated=[glm.block(terms)]))")
    nz = K * (K - 1) // 2
    z, c = _rho_c(draws[..., draws.shape[-1] - Sz - nz:draws.shape[-1] - Sz])
    L = np.zeros(draws.shape[:-1] + (K, K))
    L[..., 0, 0] = 1.0
    for j in range(1, K):
        s = None
        for i in range(j):
            e = j * (j - 1) // 2 + i
            L[..., j, i] = z[..., e] if s is None else z[..., e] * s
            s = c[..., e] if s is None else s * c[..., e]
        L[..., j, j] = s
    return L


def correlation_matrix(model, draws):
    """R = L L' of a GLM with a correlation block, shape draws.shape[:-1] + (K, K): symmetric, the diagonal exactly 1, the lower entries
    as the device summaries report them -- R_j0 = z_j0, and for i >= 1 L_ji L_ii + sum_k<i L_jk L_ik, k ascending."""
    L = cholesky_factors(model, draws)
    K = L.shape[-1]
    R = np.zeros_like(L)
    for j in range(K):
        R[..., j, j] = 1.0
        for i in range(j):
            x = L[..., j, 0] if i == 0 else L[..., j, i] * L[..., i, i]
            for k in range(i):
                x = L[..., j, k] * L[..., i, k] + x
            R[..., j, i] = R[..., i, j] = x
    return R


def autocorrelations(model, draws):
    """phi = tanh(zeta) of the AR(1) terms of a GLM with structured terms (GLM(..., structured=)), in list order, shape
    draws.shape[:-1] + (Sz,) (no AR(1) term: an empty last axis), computed as the device computes it.  A random walk has no phi to
    report (it is 1).  Any leading axes, as group_scales."""
    draws = _sampled(model, draws)
    Sz = getattr(model, "Sz", 0)
    return _rho_c(draws[..., draws.shape[-1] - Sz:])[0]


def struct_scan(x, phi, c):
    """the forward scan of a structured term along the last axis of x (N levels): x_0, c x_k for k >= 1, then per stage h = 1, 2, 4, ..
    < N every k >= h takes p x_{k-h} + x_k from the values before the stage, p = phi^h by squaring -- ut_0 = u_0,
    ut_k = phi ut_{k-1} + c u_k in the device's association (numpy rounds the product where the device fuses it).  phi, c: arrays of
    x.shape[:-1], or numbers"""
    x = np.array(x, dtype=np.float64)
    p = np.asarray(phi, dtype=np.float64)[..., None] * np.ones(x.shape[:-1] + (1,))
    x[..., 1:] = np.asarray(c, dtype=np.float64)[..., None] * x[..., 1:]
    N, h = x.shape[-1], 1
    while h < N:
        x[..., h:] = p * x[..., :N - h] + x[..., h:]
        p = p * p
        h *= 2
    return x


def _mixed(model, draws):
    """u with the second column of every pair replaced by rho u_first + c u_second (draws checked by _sampled)"""
    u = draws[..., :model.Dx].copy()
    P, Sz = getattr(model, "P", 0), getattr(model, "Sz", 0)
    if P:
        rho, c = _rho_c(draws[..., draws.shape[-1] - Sz - P:draws.shape[-1] - Sz])
        for p in range(P):
            a, b = factor_columns(model, int(model.pair_first[p])), factor_columns(model, int(model.pair_second[p]))
            u[..., b] = rho[..., p:p + 1] * draws[..., a] + c[..., p:p + 1] * draws[..., b]
    if getattr(model, "BK", 0):
        # a block: row j >= 1 takes L_jj u_j + sum_i<j L_ji u_i, i ascending, from the raw u of the block's terms
        L = cholesky_factors(model, draws)
        cols = [factor_columns(model, int(t)) for t in model.block_term]
        for j in range(1, model.BK):
            x = L[..., j, j, None] * draws[..., cols[j]]
            for i in range(j):
                x = L[..., j, i, None] * draws[..., cols[i]] + x
            u[..., cols[j]] = x
    z = 0
    for i in range(getattr(model, "S", 0)):
        cols = factor_columns(model, int(model.struct_term[i]))
        phi, c = 1.0, 1.0
        if int(model.struct_kind[i]) == STRUCT_AR1:
            phi, c = _rho_c(draws[..., draws.shape[-1] - Sz + z])
            z += 1
        u[..., cols] = struct_scan(draws[..., cols], phi, c)
    return u


def coefficients(model, draws):
    """the coefficients beta = s * u of a GLM from draws in the sampled coordinates, shape draws.shape[:-1] + (Dx,):
    beta_c = exp(omega_g) u_c for a column of group g, u_c for a column in no group (and for a model without groups).  Any leading
    axes: (M, ..., R, D) from by_response works as (..., C, D) does.  With local scales a flagged column has beta_c = u_c st, st from
    s = exp(omega_g) exp(lambda_k) (exp(lambda_k) in no group) by the kernels' operations: s itself without a slab, and with
    slab_scale S  i = 1 / s, nn = i i + 1 / S^2, st = 1 / sqrt(nn).  With correlated pairs the mix comes first: the second column of a
    pair is rho u_first + sqrt(1 - rho^2) u_second where the above say u_c, so that the effects of a level are sigma .* (L u).  With
    structured terms the scan comes first in the same way: a term's columns are ut_0 = u_0, ut_k = phi ut_{k-1} + c u_k (struct_scan)."""
    draws = _sampled(model, draws)
    sigma = group_scales(model, draws)
    u = _mixed(model, draws)
    J = getattr(model, "J", 0)
    if sigma.shape[-1] == 0 and J == 0:
        return u.copy()
    if sigma.shape[-1] == 0:
        s = np.ones_like(u)
        grouped = np.zeros(model.Dx, bool)
    else:
        grp = np.asarray(model.groups)
        grouped = grp >= 0
        s = np.where(grouped, sigma[..., np.maximum(grp, 0)], 1.0)
    if J == 0:
        return s * u
    cols = np.flatnonzero(model.local)
    f = local_scales(model, draws)
    sl = np.where(grouped[cols], s[..., cols] * f, f)
    S = getattr(model, "slab_scale", None)
    if S:
        with np.errstate(divide="ignore", over="ignore"):
            i = 1.0 / sl
            sl = 1.0 / np.sqrt(i * i + 1.0 / (S * S))
    s = s.copy()
    s[..., cols] = sl
    return s * u


def local_flags(local, slab_scale, Dx):
    """GLM()'s validation of local and slab_scale: (local int32 (Dx,) or None, J, slab_scale float or None).  The checks are
    idhmc_create_glm_local's; all flags zero without a slab is the model without the keywords."""
    loc = None
    if local is not None:
        if local is True:
            loc = np.ones(Dx, np.int32)
        else:
            raw = np.asarray(local)
            if raw.ndim != 1 or raw.shape[0] != Dx:
                raise ValueError("local must be True or have one entry per column of X (%d), got shape %s" % (Dx, raw.shape))
            if raw.dtype != np.bool_ and not (np.issubdtype(raw.dtype, np.number) and np.isin(raw, (0, 1)).all()):
                raise ValueError("every entry of local must be 0 or 1 (or a boolean)")
            loc = np.ascontiguousarray(raw != 0, dtype=np.int32)
    J = int(loc.sum()) if loc is not None else 0
    S = None
    if slab_scale is not None:
        if isinstance(slab_scale, bool) or not isinstance(slab_scale, (int, float, np.integer, np.floating)):
            raise ValueError("slab_scale must be a number (got %r)" % (slab_scale,))
        S = float(slab_scale)
        if not (np.isfinite(S) and S >= 0.0):
            raise ValueError("slab_scale = %r must be finite and >= 0 (0 or None: no slab)" % S)
        if S > 0.0 and J == 0:
            raise ValueError("slab_scale = %r needs a column with a local scale (local is None or all zeros)" % S)
        if S == 0.0:
            S = None
    if J == 0:
        loc = None
    return loc, J, S


# ---- factor terms ---------------------------------------------------------------------------------------------------------------------
Term = collections.namedtuple("Term", "index values levels")


def term(index, values=None, levels=None):
    """a factor term for GLM(..., factors=[...]): the level index of every observation, optionally a value per observation (a random
    slope: the term adds values[i] * b[level of i] to z_i where a term without values adds b[level of i]), optionally the number of
    levels (default: max(index) + 1).  term(idx) is the bare array idx and term(idx, levels=N) the pair (idx, N).  Validated by GLM()
    (factor_terms, factor_values)."""
    return Term(index, values, levels)


Members = collections.namedtuple("Members", "index weights levels")


def members(index, weights=None, levels=None):
    """a factor term of WIDTH M for GLM(..., factors=[...]) (idhmc_create_glm_multi): observation i has up to M levels index[i, m] with
    weights[i, m] and the term adds sum_m weights[i, m] * b[index[i, m]] to z_i -- a multi-membership effect (weights summing to 1 over
    the members), a match between two teams (+1, -1), a spline basis (glm.bspline).  index is (n, M) integers, M in 1..4, -1 marking an
    absent entry: the present entries of a row come first and their levels are strictly ascending.  weights is (n, M), default 1.0 on
    every present entry; the weight of an absent entry is ignored.  levels defaults to max(index) + 1.  Validated by GLM()
    (factor_terms, factor_members)."""
    return Members(index, weights, levels)


def _member_planes(f, entry, n):
    """(N, index int32 (M, n), weights float64 (M, n)) of a members() entry; every check of idhmc_create_glm_multi's on it, naming the entry"""
    raw = np.asarray(entry.index)
    if raw.ndim != 2 or raw.shape[0] != n:
        raise ValueError("factors[%d]: the index of glm.members must have shape (%d, M), got %s" % (f, n, raw.shape))
    if raw.dtype == np.bool_ or not np.issubdtype(raw.dtype, np.integer):
        raise ValueError("factors[%d] must be integers (level indices), got dtype %s" % (f, raw.dtype))
    M = raw.shape[1]
    if not 1 <= M <= 4:
        raise ValueError("factors[%d]: width %d (a term has 1..4 levels per observation)" % (f, M))
    N = entry.levels
    if N is not None and (isinstance(N, bool) or not isinstance(N, (int, np.integer)) or N < 1):
        raise ValueError("factors[%d]: the number of levels must be a positive integer (got %r)" % (f, N))
    N = max(int(raw.max()) + 1, 1) if N is None else int(N)
    if N > 1024:
        raise ValueError("factors[%d]: %d levels (a GLM is limited to D <= 1024)" % (f, N))
    bad = np.argwhere((raw < -1) | (raw >= N))
    if bad.size:
        i, m = bad[0]
        raise ValueError("factors[%d]: plane %d, observation %d: level %d is outside -1..%d" % (f, m, i, raw[i, m], N - 1))
    if M == 1 and (raw < 0).any():
        raise ValueError("factors[%d]: plane 0, observation %d: an absent entry (-1) in a term of width 1" % (f, np.flatnonzero(raw[:, 0] < 0)[0]))
    for m in range(1, M):
        bad = np.flatnonzero((raw[:, m] >= 0) & (raw[:, m - 1] < 0))
        if bad.size:
            raise ValueError("factors[%d]: plane %d, observation %d: a present entry behind an absent one" % (f, m, bad[0]))
        bad = np.flatnonzero((raw[:, m] >= 0) & (raw[:, m] <= raw[:, m - 1]))
        if bad.size:
            raise ValueError("factors[%d]: plane %d, observation %d: level %d after level %d (the levels of an observation must be strictly "
                             "ascending)" % (f, m, bad[0], raw[bad[0], m], raw[bad[0], m - 1]))
    if entry.weights is None:
        w = np.ones(raw.shape)
    else:
        w = np.asarray(entry.weights)
        if w.shape != raw.shape:
            raise ValueError("factors[%d]: weights must have the shape of index, %s, got %s" % (f, raw.shape, w.shape))
        if w.dtype == np.bool_ or not (np.issubdtype(w.dtype, np.integer) or np.issubdtype(w.dtype, np.floating)):
            raise ValueError("factors[%d]: weights must be real numbers, got dtype %s" % (f, w.dtype))
        w = w.astype(np.float64)
        bad = np.argwhere(~np.isfinite(w) & (raw >= 0))
        if bad.size:
            raise ValueError("factors[%d]: plane %d, observation %d: the weight is not finite" % (f, bad[0][1], bad[0][0]))
    w = np.where(raw >= 0, w, 0.0)
    return N, np.ascontiguousarray(raw.T, dtype=np.int32), np.ascontiguousarray(w.T)


def factor_members(factors, n):
    """GLM()'s table of members: (width int32 (F,), index int32 (P, n), values float64 (P, n)) with the planes of term 0 first, or three
    None when no entry is a members().  With one, EVERY term is in the table: a plain term is one plane of 1.0, a term() with values one
    plane of its values.  Absent entries carry the value 0.0.  The checks are idhmc_create_glm_multi's."""
    lev, idx = factor_terms(factors, n)
    if lev is None or not any(isinstance(e, Members) for e in factors):
        return None, None, None
    has, val = factor_values(factors, n)
    width, planes, values = np.empty(lev.size, np.int32), [], []
    for f, entry in enumerate(factors):
        if isinstance(entry, Members):
            _, pi, pv = _member_planes(f, entry, n)
        else:
            pi, pv = idx[f][None], (val[f][None] if has is not None and has[f] else np.ones((1, n)))
        width[f] = pi.shape[0]
        planes.append(pi)
        values.append(pv)
    if int(width.sum()) > 8:
        raise ValueError("the widths of the terms sum to %d planes: at most 8" % int(width.sum()))
    return width, np.ascontiguousarray(np.concatenate(planes), dtype=np.int32), np.ascontiguousarray(np.concatenate(values))


def factor_terms(factors, n):
    """GLM()'s validation of factors: (levels int32 (F,), index int32 (F, n)), or (None, None) for None and for an empty list.  Each
    entry is an integer array of shape (n,), a pair (array, N), a term() or a members(); N defaults to max + 1.  The checks are
    idhmc_create_glm_factors'.  The values of a term() are factor_values' business; of a members() entry the row holds its first plane
    (-1 where the observation has no member), and the whole table is factor_members' business."""
    if factors is None:
        return None, None
    if isinstance(factors, np.ndarray) or not isinstance(factors, (list, tuple)):
        raise ValueError("factors must be a list of index arrays (n,) or of pairs (index, levels), got %s" % type(factors).__name__)
    if len(factors) == 0:
        return None, None
    if len(factors) > 4:
        raise ValueError("at most 4 factors (got %d)" % len(factors))
    lev, idx = np.empty(len(factors), np.int32), np.empty((len(factors), n), np.int32)
    for f, entry in enumerate(factors):
        N, given = None, False
        if isinstance(entry, Members):
            lev[f], planes, _ = _member_planes(f, entry, n)
            idx[f] = planes[0]
            continue
        if isinstance(entry, Term):
            entry, N = entry.index, entry.levels
            given = N is not None
        elif isinstance(entry, tuple):
            if len(entry) != 2:
                raise ValueError("factors[%d] must be an index array, a pair (index, levels) or a glm.term(index, values, levels) -- or a "
                                 "glm.members(index, weights, levels)" % f)
            entry, N = entry
            given = True
        if given:
            if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or N < 1:
                raise ValueError("factors[%d]: the number of levels must be a positive integer (got %r)" % (f, N))
        raw = np.asarray(entry)
        if raw.ndim != 1 or raw.shape[0] != n:
            raise ValueError("factors[%d] must have one index per observation, shape (%d,), got %s" % (f, n, raw.shape))
        if raw.dtype == np.bool_ or not np.issubdtype(raw.dtype, np.integer):
            raise ValueError("factors[%d] must be integers (level indices), got dtype %s" % (f, raw.dtype))
        if raw.min() < 0:
            raise ValueError("factors[%d]: a level index is 0 .. N-1, got %d" % (f, raw.min()))
        N = int(raw.max()) + 1 if N is None else int(N)
        if raw.max() >= N:
            raise ValueError("factors[%d]: index %d is outside 0..%d (the factor's %d levels)" % (f, raw.max(), N - 1, N))
        if N > 1024:
            raise ValueError("factors[%d]: %d levels (a GLM is limited to D <= 1024)" % (f, N))
        lev[f], idx[f] = N, raw
    return lev, idx


def factor_values(factors, n):
    """GLM()'s validation of the values of factor terms: (has int32 (F,), values float64 (F, n)), or (None, None) when no entry has
    values.  has[f] is 1 for a term() with values and its row holds them; the row of every other entry is 0.0 and is not read.  The
    checks are idhmc_create_glm_slopes', naming the entry: shape (n,), a real numeric dtype (no bool), all finite."""
    lev, idx = factor_terms(factors, n)
    if lev is None or not any(isinstance(e, Term) and e.values is not None for e in factors):
        return None, None
    has, val = np.zeros(lev.size, np.int32), np.zeros((lev.size, n), np.float64)
    for f, entry in enumerate(factors):
        if not isinstance(entry, Term) or entry.values is None:
            continue
        raw = np.asarray(entry.values)
        if raw.ndim != 1 or raw.shape[0] != n:
            raise ValueError("factors[%d]: values must have one value per observation, shape (%d,), got %s" % (f, n, raw.shape))
        if raw.dtype == np.bool_ or not (np.issubdtype(raw.dtype, np.integer) or np.issubdtype(raw.dtype, np.floating)):
            raise ValueError("factors[%d]: values must be real numbers, got dtype %s" % (f, raw.dtype))
        raw = raw.astype(np.float64)
        bad = np.flatnonzero(~np.isfinite(raw))
        if bad.size:
            raise ValueError("factors[%d]: values[%d] = %r is not finite" % (f, bad[0], float(raw[bad[0]])))
        has[f], val[f] = 1, raw
    return has, val


def factor_columns(model, f):
    """the columns of factor f (any term, with values or without) among the Dx columns of a GLM with factor terms: slice(off_f, off_f + N_f), off_f = Dd + N_0 + .. + N_{f-1}"""
    F = getattr(model, "F", 0)
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not 0 <= f < F:
        raise ValueError("factor %r: the model has factors 0..%d" % (f, F - 1) if F else "the model has no factor terms (GLM(..., factors=))")
    off = model.Dd + int(model.levels[:f].sum())
    return slice(off, off + int(model.levels[f]))


def expand_factors(X, factors):
    """the n x Dx design matrix with one column per level -- the documented equivalent of GLM(X, ..., factors=factors): the dense
    columns of X, then for factor 0, 1, .. one column per level holding 1.0 (for a term() with values: values[i]) where the observation
    has that level and 0.0 elsewhere; for a members() entry weights[i, m] in the column of level index[i, m], every present entry.  The
    engine computes the same bits on both."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be an (n, Dd) matrix, got shape %s" % (X.shape,))
    lev, idx = factor_terms(factors, X.shape[0])
    if lev is None:
        return X.copy()
    has, val = factor_values(factors, X.shape[0])
    width, midx, mval = factor_members(factors, X.shape[0])
    out = np.zeros((X.shape[0], X.shape[1] + int(lev.sum())))
    out[:, :X.shape[1]] = X
    off = X.shape[1]
    rows = np.arange(X.shape[0])
    for f in range(lev.size):
        if width is not None:
            # (the levels of an observation are distinct within a term: no entry is written twice)
            for p in range(int(width[:f].sum()), int(width[:f + 1].sum())):
                here = midx[p] >= 0
                out[rows[here], off + midx[p][here]] = mval[p][here]
        else:
            out[rows, off + idx[f]] = 1.0 if has is None or not has[f] else val[f]
        off += int(lev[f])
    return out


def bspline_knots(n_basis, degree=3, lo=0.0, hi=1.0):
    """the n_basis + degree + 1 uniform knots of glm.bspline: t[degree] = lo and t[n_basis] = hi exactly, the interior ones
    lo + j h with h = (hi - lo) / (n_basis - degree), and degree more at spacing h on either side"""
    K = n_basis - degree
    h = (hi - lo) / K
    t = np.empty(n_basis + degree + 1)
    for j in range(K):
        t[degree + j] = lo + j * h
    t[n_basis] = hi
    for j in range(1, degree + 1):
        t[degree - j] = lo - j * h
        t[n_basis + j] = hi + j * h
    return t


def bspline(x, n_basis, degree=3, lo=None, hi=None):
    """a B-spline basis as a factor term: glm.members(index, weights, levels=n_basis) of width degree + 1 (degree 1..3), observation i
    having the degree + 1 adjacent basis functions that are non-zero at x[i], evaluated by the Cox-de Boor recursion on uniform knots
    (bspline_knots) over [lo, hi], which defaults to the range of x.  The weights of a row are >= 0 and sum to 1.  With an RW2 precision
    on the term's levels (glm.smooth_effects) this is a penalised spline, s(x); the basis is never stored as columns.  x outside
    [lo, hi] is refused; x = hi belongs to the last interval."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1 or x.size < 1 or not np.isfinite(x).all():
        raise ValueError("x must be a non-empty vector of finite numbers, got shape %s" % (x.shape,))
    if isinstance(degree, bool) or not isinstance(degree, (int, np.integer)) or not 1 <= degree <= 3:
        raise ValueError("degree = %r must be 1, 2 or 3" % (degree,))
    degree = int(degree)
    if isinstance(n_basis, bool) or not isinstance(n_basis, (int, np.integer)) or not degree + 1 <= n_basis <= 1024:
        raise ValueError("n_basis = %r must be an integer in degree + 1 = %d .. 1024" % (n_basis, degree + 1))
    n_basis = int(n_basis)
    lo = float(x.min()) if lo is None else float(lo)
    hi = float(x.max()) if hi is None else float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("[lo, hi] = [%r, %r] must be a finite interval of positive length" % (lo, hi))
    bad = np.flatnonzero((x < lo) | (x > hi))
    if bad.size:
        raise ValueError("x[%d] = %r is outside [lo, hi] = [%r, %r]" % (bad[0], float(x[bad[0]]), lo, hi))
    t = bspline_knots(n_basis, degree, lo, hi)
    # the knot interval of every x: t[k] <= x < t[k + 1], k in degree .. n_basis - 1 (x = hi: the last one)
    k = np.clip(np.searchsorted(t, x, side="right") - 1, degree, n_basis - 1)
    # de Boor's triangular scheme for the degree + 1 functions that are non-zero on the interval (N[j] is B_{k - degree + j})
    N = np.zeros((degree + 1, x.size))
    N[0] = 1.0
    for j in range(1, degree + 1):
        saved = np.zeros(x.size)
        for r in range(j):
            right, left = t[k + r + 1] - x, x - t[k + 1 - j + r]
            tmp = N[r] / (t[k + r + 1] - t[k + 1 - j + r])
            N[r] = saved + right * tmp
            saved = left * tmp
        N[j] = saved
    index = (k - degree)[:, None] + np.arange(degree + 1)[None, :]
    return Members(np.ascontiguousarray(index, dtype=np.int32), np.ascontiguousarray(N.T), n_basis)


# ---- correlated pairs of terms --------------------------------------------------------------------------------------------------------
Pair = collections.namedtuple("Pair", "first second eta")


def pair(first, second, eta=2.0):
    """a correlated pair of factor terms for GLM(..., correlated=[...]): level k of term `first` and level k of term `second` share a
    sampled correlation rho = tanh(zeta).  eta > 0: LKJ(eta) on the 2 x 2 correlation, (rho + 1) / 2 ~ Beta(eta, eta) (eta = 1: uniform);
    eta = 0: the entry of zeta in prior_mu, prior_tau, prior_kind, prior_nu applies (normal or Student-t on Fisher's z).  Validated by
    GLM() (pair_terms, pair_priors)."""
    return Pair(first, second, eta)


def pair_terms(correlated, levels):
    """GLM()'s validation of correlated: (first int32 (P,), second int32 (P,), eta float64 (P,)), or (None, None, None) for None and for
    an empty list.  levels: the level counts of the model's terms (None: no factor terms).  The checks are idhmc_create_glm_corr's,
    naming the pair."""
    if correlated is None:
        return None, None, None
    if not isinstance(correlated, (list, tuple)) or isinstance(correlated, (Pair, Block)):
        raise ValueError("correlated must be a list of glm.pair(first, second, eta), got %s" % type(correlated).__name__)
    if len(correlated) == 0:
        return None, None, None
    if any(isinstance(e, Block) for e in correlated):
        block_terms(correlated, levels)                         # (a block is the single entry: no pairs)
        return None, None, None
    if len(correlated) > 2:
        raise ValueError("at most 2 correlated pairs (got %d)" % len(correlated))
    if levels is None:
        raise ValueError("correlated pairs need factor terms (GLM(..., factors=))")
    F = len(levels)
    first, second, eta = np.empty(len(correlated), np.int32), np.empty(len(correlated), np.int32), np.empty(len(correlated))
    used = set()
    for p, entry in enumerate(correlated):
        if not isinstance(entry, Pair):
            raise ValueError("correlated[%d] must be a glm.pair(first, second, eta)" % p)
        for name, t in (("first", entry.first), ("second", entry.second)):
            if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t < F:
                raise ValueError("correlated[%d]: %s = %r is outside 0..%d (the model's terms)" % (p, name, t, F - 1))
        a, b = int(entry.first), int(entry.second)
        if a == b:
            raise ValueError("correlated[%d]: first = second = %d (a pair is two distinct terms)" % (p, a))
        for t in (a, b):
            if t in used:
                raise ValueError("correlated[%d]: term %d is in two pairs" % (p, t))
            used.add(t)
        if int(levels[a]) != int(levels[b]):
            raise ValueError("correlated[%d]: terms %d and %d have %d and %d levels (a pair needs equal level counts)"
                             % (p, a, b, int(levels[a]), int(levels[b])))
        e = entry.eta
        if isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating)) or not (np.isfinite(e) and e >= 0.0):
            raise ValueError("correlated[%d]: eta = %r must be finite and >= 0 (0: the prior arrays' entry of zeta applies)" % (p, e))
        first[p], second[p], eta[p] = a, b, float(e)
    return first, second, eta


def pair_priors(eta, D, mu, tau, kind, nu):
    """GLM()'s checks of the zetas' entries in the prior arrays (the last P of D): no log kind; with eta > 0 the defaults"""
    P = eta.size
    for p in range(P):
        cz = D - P + p
        k = 0 if kind is None else int(kind[cz])
        if k >= PRIOR_LOG_HALF_NORMAL:
            raise ValueError("correlated[%d]: prior_kind[%d] = PRIOR_%s is a prior on exp(q): coordinate %d is zeta = atanh rho, not a logarithm "
                             "(normal and student_t are for a zeta)" % (p, cz, PRIOR_NAMES[k], cz))
        if eta[p] > 0.0 and (k != 0 or (nu is not None and nu[cz] != 0.0) or (mu is not None and mu[cz] != 0.0)
                             or (tau is not None and tau[cz] != 1.0)):
            raise ValueError("correlated[%d]: eta = %r is the LKJ prior of zeta: the entry of coordinate %d in the prior arrays must be the "
                             "default (kind 0, mu 0, tau 1, nu 0) and is not applied" % (p, float(eta[p]), cz))


# ---- a correlation block of three or four terms ------------------------------------------------------------------------------------------
Block = collections.namedtuple("Block", "terms eta")


def block(terms, eta=2.0):
    """a correlation block of factor terms for GLM(..., correlated=[glm.block(terms, eta)]), its single entry: K = 2, 3 or 4 distinct terms
    of equal level counts whose effects at level k share a sampled K x K correlation matrix R = L L' -- (1 + x1 + x2 | subject) is
    block((0, 1, 2)).  The order of `terms` is the row order of L.  The block adds K (K - 1) / 2 coordinates zeta_ji = atanh z_ji (z the
    canonical partial correlations), row-major, where a pair's zeta would stand.  eta > 0: LKJ(eta) on R (eta = 1: uniform over
    correlation matrices); eta = 0: the zetas' entries in prior_mu, prior_tau, prior_kind, prior_nu apply (normal or Student-t).
    Validated by GLM() (block_terms, block_priors)."""
    return Block(tuple(terms) if isinstance(terms, (list, tuple, np.ndarray)) else terms, eta)


def block_terms(correlated, levels):
    """GLM()'s validation of a block in correlated: (terms int32 (K,), eta float), or (None, None) when correlated holds none.  levels: the
    level counts of the model's terms (None: no factor terms).  The checks are idhmc_create_glm_block's."""
    if not isinstance(correlated, (list, tuple)) or isinstance(correlated, (Pair, Block)) or not any(isinstance(e, Block) for e in correlated):
        return None, None
    if len(correlated) != 1:
        raise ValueError("correlated: a glm.block is the single entry of correlated (a model has pairs or one block, not both; got %d entries)"
                         % len(correlated))
    b = correlated[0]
    if levels is None:
        raise ValueError("a correlation block needs factor terms (GLM(..., factors=))")
    F = len(levels)
    if not isinstance(b.terms, tuple) or len(b.terms) not in (2, 3, 4):
        raise ValueError("correlated[0]: a block names K = 2, 3 or 4 terms (got %r)" % (b.terms,))
    out = []
    for r, t in enumerate(b.terms):
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t < F:
            raise ValueError("correlated[0]: terms[%d] = %r is outside 0..%d (the model's terms)" % (r, t, F - 1))
        if int(t) in out:
            raise ValueError("correlated[0]: term %d is listed twice" % int(t))
        out.append(int(t))
        if int(levels[int(t)]) != int(levels[out[0]]):
            raise ValueError("correlated[0]: terms %d and %d have %d and %d levels (a block needs equal level counts)"
                             % (out[0], int(t), int(levels[out[0]]), int(levels[int(t)])))
    e = b.eta
    if isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating)) or not (np.isfinite(e) and e >= 0.0):
        raise ValueError("correlated[0]: eta = %r must be finite and >= 0 (0: the prior arrays' entries of the zetas apply)" % (e,))
    return np.array(out, np.int32), float(e)


def block_priors(eta, nz, D, mu, tau, kind, nu):
    """GLM()'s checks of the block's zetas' entries in the prior arrays (the last nz of D): no log kind; with eta > 0 the defaults"""
    for cz in range(D - nz, D):
        k = 0 if kind is None else int(kind[cz])
        if k >= PRIOR_LOG_HALF_NORMAL:
            raise ValueError("correlated[0]: prior_kind[%d] = PRIOR_%s is a prior on exp(q): coordinate %d is a zeta = atanh z, not a logarithm "
                             "(normal and student_t are for a zeta)" % (cz, PRIOR_NAMES[k], cz))
        if eta > 0.0 and (k != 0 or (nu is not None and nu[cz] != 0.0) or (mu is not None and mu[cz] != 0.0)
                          or (tau is not None and tau[cz] != 1.0)):
            raise ValueError("correlated[0]: eta = %r is the LKJ prior of the zetas: the entry of coordinate %d in the prior arrays must be the "
                             "default (kind 0, mu 0, tau 1, nu 0) and is not applied" % (eta, cz))


def block_effects(Dd, levels, terms, eta=2.0, A=0, scale=None, coefficients=None, aux=None):
    """the keyword arguments of GLM() for a correlation block: what random_intercepts(Dd, levels, A, scale, coefficients, aux) returns, its
    prior arrays extended by the K (K - 1) / 2 zetas, plus `correlated` = [glm.block(terms, eta)] -- (1 + x1 + x2 | subject) is
    GLM(X, Y, source, factors=[subject, glm.term(subject, values=x1), glm.term(subject, values=x2)],
        **glm.block_effects(X.shape[1], [N, N, N], (0, 1, 2), eta=2.0)).
    eta: LKJ(eta) on the correlation matrix (0 is not offered here: it needs prior entries on the zetas, which GLM()'s keywords take)."""
    if isinstance(eta, bool) or not isinstance(eta, (int, float, np.integer, np.floating)) or not (np.isfinite(eta) and eta > 0.0):
        raise ValueError("eta = %r must be finite and > 0" % (eta,))
    corr = [block(terms, float(eta))]
    t, _ = block_terms(corr, [int(N) for N in levels])
    kw = random_intercepts(Dd, levels, A, scale, coefficients, aux)
    nz = t.size * (t.size - 1) // 2
    kw["prior_mu"] = np.r_[kw["prior_mu"], np.zeros(nz)]
    kw["prior_tau"] = np.r_[kw["prior_tau"], np.ones(nz)]
    kw["prior_kind"] = np.r_[kw["prior_kind"], np.zeros(nz, np.int32)].astype(np.int32)
    kw["prior_nu"] = np.r_[kw["prior_nu"], np.zeros(nz)]
    kw["correlated"] = corr
    return kw


def correlated_effects(Dd, levels, pairs, eta=2.0, A=0, scale=None, coefficients=None, aux=None):
    """the keyword arguments of GLM() for correlated random effects: what random_intercepts(Dd, levels, A, scale, coefficients, aux)
    returns, its prior arrays extended by the P zetas, plus `correlated` -- (1 + x | subject) with a sampled correlation between
    intercept and slope is
    GLM(X, Y, source, factors=[subject, glm.term(subject, values=x)], **glm.correlated_effects(X.shape[1], [N, N], [(0, 1)], eta=2.0)).
    pairs: up to two (first, second) tuples of term indices; eta: one number or one per pair, LKJ(eta) on each correlation (0 is not
    offered here: it needs a prior entry on zeta, which GLM()'s keywords take)."""
    pairs = list(pairs)
    if len(pairs) > 2:
        raise ValueError("at most 2 correlated pairs (got %d)" % len(pairs))
    etas = [eta] * len(pairs) if np.ndim(eta) == 0 else list(eta)
    if len(etas) != len(pairs):
        raise ValueError("eta must be one number or one per pair (%d)" % len(pairs))
    corr = []
    for p, (ab, e) in enumerate(zip(pairs, etas)):
        if not isinstance(ab, (tuple, list)) or len(ab) != 2:
            raise ValueError("pairs[%d] must be (first, second)" % p)
        if not (np.isfinite(e) and e > 0.0):
            raise ValueError("pairs[%d]: eta = %r must be finite and > 0" % (p, e))
        corr.append(pair(ab[0], ab[1], float(e)))
    pair_terms(corr, [int(N) for N in levels])
    kw = random_intercepts(Dd, levels, A, scale, coefficients, aux)
    P = len(corr)
    kw["prior_mu"] = np.r_[kw["prior_mu"], np.zeros(P)]
    kw["prior_tau"] = np.r_[kw["prior_tau"], np.ones(P)]
    kw["prior_kind"] = np.r_[kw["prior_kind"], np.zeros(P, np.int32)].astype(np.int32)
    kw["prior_nu"] = np.r_[kw["prior_nu"], np.zeros(P)]
    kw["correlated"] = corr
    return kw


# ---- structured terms: AR(1) and random-walk effects across a term's levels ------------------------------------------------------------
STRUCT_AR1, STRUCT_RW1 = 1, 2
STRUCT_NAMES = {STRUCT_AR1: "ar1", STRUCT_RW1: "rw1"}
Structure = collections.namedtuple("Structure", "term kind eta")


def ar1(term, eta=2.0):
    """an AR(1) structure on factor term `term` for GLM(..., structured=[...]): its levels, in index order, are the stationary
    unit-variance process ut_0 = u_0, ut_k = phi ut_{k-1} + sqrt(1 - phi^2) u_k with a sampled phi = tanh(zeta).  eta > 0:
    (phi + 1) / 2 ~ Beta(eta, eta) (eta = 1: uniform on (-1, 1)); eta = 0: the entry of zeta in prior_mu, prior_tau, prior_kind, prior_nu
    applies (normal or Student-t on atanh phi).  Validated by GLM() (struct_terms, struct_priors)."""
    return Structure(term, STRUCT_AR1, eta)


def rw1(term):
    """a first-order random walk on factor term `term` for GLM(..., structured=[...]): ut_k = u_0 + .. + u_k in index order, the
    increments u_k (k >= 1) being what the term's priors and its group's scale act on.  No coordinate is added."""
    return Structure(term, STRUCT_RW1, 0.0)


def struct_terms(structured, levels, correlated=None, local=None, Dd=0):
    """GLM()'s validation of structured: (term int32 (S,), kind int32 (S,), eta float64 (S,)), or (None, None, None) for None and for an
    empty list.  levels: the level counts of the model's terms (None: no factor terms); correlated: the model's pairs (a term is
    structured or paired, not both); local, Dd: the model's local-scale flags over its columns and its dense columns (a structured term
    takes no local scale).  The checks are idhmc_create_glm_struct's, naming the entry."""
    if structured is None:
        return None, None, None
    if not isinstance(structured, (list, tuple)) or isinstance(structured, Structure):
        raise ValueError("structured must be a list of glm.ar1(term, eta) / glm.rw1(term), got %s" % type(structured).__name__)
    if len(structured) == 0:
        return None, None, None
    if len(structured) > 2:
        raise ValueError("at most 2 structured terms (got %d)" % len(structured))
    if levels is None:
        raise ValueError("structured terms need factor terms (GLM(..., factors=))")
    F = len(levels)
    term, kind, eta = np.empty(len(structured), np.int32), np.empty(len(structured), np.int32), np.empty(len(structured))
    paired = {}
    for p, pr in enumerate(correlated or ()):
        if isinstance(pr, Pair):
            paired.setdefault(pr.first, p)
            paired.setdefault(pr.second, p)
        elif isinstance(pr, Block):                             # (a block's terms are refused as a pair's are)
            for t in pr.terms:
                paired.setdefault(t, p)
    off = int(Dd) + np.r_[0, np.cumsum([int(N) for N in levels])]
    used = set()
    for i, entry in enumerate(structured):
        if not isinstance(entry, Structure):
            raise ValueError("structured[%d] must be a glm.ar1(term, eta) or a glm.rw1(term)" % i)
        t = entry.term
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t < F:
            raise ValueError("structured[%d]: term = %r is outside 0..%d (the model's terms)" % (i, t, F - 1))
        t = int(t)
        if t in used:
            raise ValueError("structured[%d]: term %d is listed twice" % (i, t))
        used.add(t)
        k = entry.kind
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k not in (STRUCT_AR1, STRUCT_RW1):
            raise ValueError("structured[%d]: kind = %r must be glm.STRUCT_AR1 (1) or glm.STRUCT_RW1 (2)" % (i, k))
        e = entry.eta
        if isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating)) or not (np.isfinite(e) and e >= 0.0):
            raise ValueError("structured[%d]: eta = %r must be finite and >= 0 (0: the prior arrays' entry of zeta applies)" % (i, e))
        if k == STRUCT_RW1 and e != 0.0:
            raise ValueError("structured[%d]: eta = %r on a random walk, which has no zeta (eta must be 0)" % (i, e))
        if int(levels[t]) < 2:
            raise ValueError("structured[%d]: term %d has %d level (a structured term needs at least 2)" % (i, t, int(levels[t])))
        if t in paired:
            raise ValueError("structured[%d]: term %d is in correlated[%d] (a term is structured or paired, not both)" % (i, t, paired[t]))
        if local is not None:
            flagged = np.flatnonzero(np.asarray(local)[off[t]:off[t + 1]])
            if flagged.size:
                raise ValueError("structured[%d]: local[%d] is set on level %d of term %d (a structured term takes no local scale)"
                                 % (i, off[t] + flagged[0], flagged[0], t))
        term[i], kind[i], eta[i] = t, int(k), float(e)
    return term, kind, eta


def struct_priors(kind, eta, D, mu, tau, prior_kind, nu):
    """GLM()'s checks of the AR(1) zetas' entries in the prior arrays (the last Sz of D, in list order): no log kind; with eta > 0 the
    defaults"""
    Sz = int((np.asarray(kind) == STRUCT_AR1).sum())
    z = 0
    for i in range(len(kind)):
        if kind[i] != STRUCT_AR1:
            continue
        cz = D - Sz + z
        z += 1
        k = 0 if prior_kind is None else int(prior_kind[cz])
        if k >= PRIOR_LOG_HALF_NORMAL:
            raise ValueError("structured[%d]: prior_kind[%d] = PRIOR_%s is a prior on exp(q): coordinate %d is zeta = atanh phi, not a logarithm "
                             "(normal and student_t are for a zeta)" % (i, cz, PRIOR_NAMES[k], cz))
        if eta[i] > 0.0 and (k != 0 or (nu is not None and nu[cz] != 0.0) or (mu is not None and mu[cz] != 0.0)
                             or (tau is not None and tau[cz] != 1.0)):
            raise ValueError("structured[%d]: eta = %r is the Beta(eta, eta) prior of zeta: the entry of coordinate %d in the prior arrays must "
                             "be the default (kind 0, mu 0, tau 1, nu 0) and is not applied" % (i, float(eta[i]), cz))


def structured_effects(Dd, levels, structured, correlated=None, eta=2.0, A=0, scale=None, coefficients=None, aux=None):
    """the keyword arguments of GLM() for structured effects: what correlated_effects(Dd, levels, correlated, eta, A, scale, coefficients,
    aux) returns (random_intercepts(...) when no pair is given), its prior arrays extended by the AR(1) terms' zetas, plus `structured`
    -- a week effect with a sampled scale and autocorrelation, next to a subject intercept, is
    GLM(X, Y, source, factors=[(week, 52), subject], **glm.structured_effects(X.shape[1], [52, N], [glm.ar1(0)])).
    structured: up to two glm.ar1(term, eta) / glm.rw1(term); correlated: (first, second) tuples as correlated_effects takes them, with
    `eta` theirs.  An ar1 with eta = 0 needs a prior entry on its zeta, which GLM()'s keywords take."""
    structured = list(structured)
    lev = [int(N) for N in levels]
    if correlated:
        kw = correlated_effects(Dd, lev, correlated, eta, A, scale, coefficients, aux)
    else:
        kw = random_intercepts(Dd, lev, A, scale, coefficients, aux)
    struct_terms(structured, lev, kw.get("correlated"))
    Sz = sum(1 for e in structured if e.kind == STRUCT_AR1)
    kw["prior_mu"] = np.r_[kw["prior_mu"], np.zeros(Sz)]
    kw["prior_tau"] = np.r_[kw["prior_tau"], np.ones(Sz)]
    kw["prior_kind"] = np.r_[kw["prior_kind"], np.zeros(Sz, np.int32)].astype(np.int32)
    kw["prior_nu"] = np.r_[kw["prior_nu"], np.zeros(Sz)]
    kw["structured"] = structured
    return kw


# ---- GMRF terms: a sparse precision on a term's levels (ICAR, RW2, seasonal, generic) ---------------------------------------------------
Gmrf = collections.namedtuple("Gmrf", "term indptr indices data kappa")


def _csr(Q):
    """Q, a dense symmetric array or an (indptr, indices, data) CSR triple, as (N, indptr int64, indices int32, data float64) with the
    columns ascending within a row; a dense Q keeps its non-zero entries and its whole diagonal"""
    if isinstance(Q, tuple) and len(Q) == 3:
        indptr, indices, data = (np.asarray(a) for a in Q)
        if indptr.ndim != 1 or indptr.size < 2 or indices.ndim != 1 or data.ndim != 1 or indices.size != data.size:
            raise ValueError("Q as (indptr, indices, data): indptr of N + 1 entries and indices, data of equal length")
        if not (np.issubdtype(indptr.dtype, np.integer) and np.issubdtype(indices.dtype, np.integer)):
            raise ValueError("Q as (indptr, indices, data): indptr and indices must be integers")
        if indptr[0] != 0 or indptr[-1] != data.size or (np.diff(indptr) < 0).any():
            raise ValueError("Q as (indptr, indices, data): indptr must not decrease, from 0 to len(data)")
        return indptr.size - 1, indptr.astype(np.int64), indices.astype(np.int32), data.astype(np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    if Q.ndim != 2 or Q.shape[0] != Q.shape[1] or Q.shape[0] < 1:
        raise ValueError("Q must be a square matrix or an (indptr, indices, data) triple, got shape %s" % (Q.shape,))
    keep = (Q != 0.0) | np.eye(Q.shape[0], dtype=bool)
    rows, cols = np.nonzero(keep)
    return Q.shape[0], np.r_[0, np.cumsum(keep.sum(1))].astype(np.int64), cols.astype(np.int32), Q[rows, cols]


def _dense(N, indptr, indices, data):
    Q = np.zeros((N, N))
    for k in range(N):
        Q[k, indices[indptr[k]:indptr[k + 1]]] = data[indptr[k]:indptr[k + 1]]
    return Q


def gmrf(term, Q, sum_to_zero=0.0):
    """a Gaussian Markov random field prior on the levels u of factor term `term` for GLM(..., gmrf=[...]):
    log p(u) = -1/2 u' Q u - 1/2 kappa (sum u)^2, kappa = sum_to_zero >= 0 (a soft sum-to-zero constraint; 0: none).  Q: a dense
    symmetric (N, N) array or an (indptr, indices, data) CSR triple; every row holds its positive diagonal and at most 128 entries.
    The table's checks are idhmc_create_glm_gmrf's.  Raises ValueError when numpy.linalg.eigvalsh of the dense Q + kappa 11' has an
    eigenvalue below -N eps ||Q||_2, the symmetric eigensolver's backward-error bound: such a Q is no precision.  A Q that is only
    positive semi-definite with kappa = 0 (an ICAR, a random walk) is accepted and improper along its null space -- the likelihood, or
    sum_to_zero > 0 for the constant direction, has to identify it."""
    N, indptr, indices, data = _csr(Q)
    k = sum_to_zero
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not (np.isfinite(k) and k >= 0.0):
        raise ValueError("sum_to_zero = %r must be finite and >= 0" % (k,))
    if N > 1024:
        raise ValueError("Q has %d rows: a GLM is limited to D <= 1024" % N)
    if not np.isfinite(data).all():
        raise ValueError("Q holds a non-finite value")
    for r in range(N):
        cols = indices[indptr[r]:indptr[r + 1]]
        if cols.size < 1 or cols.size > 128:
            raise ValueError("row %d of Q has %d entries (1..128: the diagonal is always there)" % (r, cols.size))
        if cols.min() < 0 or cols.max() >= N or (np.diff(cols) <= 0).any():
            raise ValueError("row %d of Q: columns must be strictly ascending inside 0..%d" % (r, N - 1))
        d = data[indptr[r]:indptr[r + 1]][cols == r]
        if d.size != 1 or not d[0] > 0.0:
            raise ValueError("row %d of Q: the diagonal must be present and > 0" % r)
    dense = _dense(N, indptr, indices, data)
    if not np.array_equal(dense, dense.T) or not np.array_equal(dense != 0.0, (dense != 0.0).T):
        raise ValueError("Q must be symmetric: Q[i][j] and Q[j][i] both present and bit-equal")
    pattern = np.zeros((N, N), bool)
    for r in range(N):
        pattern[r, indices[indptr[r]:indptr[r + 1]]] = True
    if not np.array_equal(pattern, pattern.T):
        raise ValueError("Q must be symmetric: Q[i][j] and Q[j][i] both present and bit-equal")
    ev = np.linalg.eigvalsh(dense + float(k) * np.ones((N, N)))
    if ev.min() < -N * np.finfo(np.float64).eps * np.abs(np.linalg.eigvalsh(dense)).max():
        raise ValueError("Q + kappa 11' has the eigenvalue %g: not a precision (positive semi-definite is the least)" % ev.min())
    return Gmrf(term, indptr, indices, data, float(k))


def icar_precision(edges, N):
    """D - W of an undirected graph on N regions: edges is a sequence of (i, j) pairs, i != j, each neighbourhood once in either order;
    the intrinsic CAR's precision (rank N minus the number of connected components).  An isolated region gets the diagonal 1 (an iid
    N(0, 1) effect), since every row needs a positive diagonal."""
    N = int(N)
    W = np.zeros((N, N))
    for i, j in edges:
        i, j = int(i), int(j)
        if not (0 <= i < N and 0 <= j < N) or i == j:
            raise ValueError("edge (%d, %d): two different regions of 0..%d" % (i, j, N - 1))
        W[i, j] = W[j, i] = 1.0
    d = W.sum(1)
    return np.diag(np.where(d > 0.0, d, 1.0)) - W


def _difference_precision(N, stencil):
    """Delta' Delta of the (N - len(stencil) + 1) x N operator that applies `stencil` along the levels (small integers: exact)"""
    m = len(stencil)
    N = int(N)
    if N < m:
        raise ValueError("N = %d levels: at least %d are needed" % (N, m))
    Dm = np.zeros((N - m + 1, N))
    for r in range(N - m + 1):
        Dm[r, r:r + m] = stencil
    return Dm.T @ Dm


def rw1_precision(N):
    """the first-order random walk's precision, Delta' Delta of the first differences (an ICAR on a line; rank N - 1)"""
    return _difference_precision(N, [-1.0, 1.0])


def rw2_precision(N):
    """the second-order random walk's precision, Delta' Delta of the second differences u_k - 2 u_{k+1} + u_{k+2} (rank N - 2: the
    level and the slope are free) -- also a penalised spline's second-order difference penalty"""
    return _difference_precision(N, [1.0, -2.0, 1.0])


def seasonal_precision(N, period):
    """the seasonal effect's precision, Delta' Delta of the sums of `period` consecutive levels (rank N - period + 1)"""
    period = int(period)
    if period < 2:
        raise ValueError("period = %d: at least 2" % period)
    return _difference_precision(N, [1.0] * period)


def scale_precision(Q):
    """Q scaled so that the geometric mean of the marginal variances -- the diagonal of its generalised inverse under the constraint on
    its null space -- is 1: INLA's scale.model and BYM2's scaling, which make a group scale's prior mean the same thing for every graph.
    Q dense symmetric positive semi-definite, N <= 1024 (host numpy: a symmetric eigendecomposition).  Returns c Q with the diagonal of
    pinv(c Q) of geometric mean 1."""
    Q = np.asarray(Q, dtype=np.float64)
    if Q.ndim != 2 or Q.shape[0] != Q.shape[1] or not 1 <= Q.shape[0] <= 1024 or not np.array_equal(Q, Q.T):
        raise ValueError("Q must be a symmetric matrix of at most 1024 rows, got shape %s" % (Q.shape,))
    w, V = np.linalg.eigh(Q)
    keep = w > Q.shape[0] * np.finfo(np.float64).eps * np.abs(w).max()
    if not keep.any():
        raise ValueError("Q has no positive eigenvalue")
    var = ((V[:, keep] ** 2) / w[keep]).sum(1)
    return Q * np.exp(np.mean(np.log(var)))


def gmrf_terms(gmrfs, levels, correlated=None, structured=None, local=None, Dd=0, mu=None, tau=None, prior_kind=None, nu=None):
    """GLM()'s validation of gmrf: (term int32 (G,), kappa float64 (G,), start int64 (sum N + 1,), col int32, val float64) -- the tables
    of the terms one behind the other -- or five None for None and for an empty list.  The checks are idhmc_create_glm_gmrf's, naming
    the entry."""
    none = (None,) * 5
    if gmrfs is None:
        return none
    if not isinstance(gmrfs, (list, tuple)) or isinstance(gmrfs, Gmrf):
        raise ValueError("gmrf must be a list of glm.gmrf(term, Q, sum_to_zero), got %s" % type(gmrfs).__name__)
    if len(gmrfs) == 0:
        return none
    if len(gmrfs) > 2:
        raise ValueError("at most 2 GMRF terms (got %d)" % len(gmrfs))
    if levels is None:
        raise ValueError("GMRF terms need factor terms (GLM(..., factors=))")
    F = len(levels)
    paired, structd = {}, {}
    for p, pr in enumerate(correlated or ()):
        if isinstance(pr, Pair):
            paired.setdefault(pr.first, p)
            paired.setdefault(pr.second, p)
        elif isinstance(pr, Block):                             # (a block's terms are refused as a pair's are)
            for t in pr.terms:
                paired.setdefault(t, p)
    for i, st in enumerate(structured or ()):
        if isinstance(st, Structure):
            structd.setdefault(st.term, i)
    off = int(Dd) + np.r_[0, np.cumsum([int(N) for N in levels])]
    term, kappa = np.empty(len(gmrfs), np.int32), np.empty(len(gmrfs))
    start, col, val, used = [np.zeros(1, np.int64)], [], [], set()
    for i, e in enumerate(gmrfs):
        if not isinstance(e, Gmrf):
            raise ValueError("gmrf[%d] must be a glm.gmrf(term, Q, sum_to_zero)" % i)
        t = e.term
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t < F:
            raise ValueError("gmrf[%d]: term = %r is outside 0..%d (the model's terms)" % (i, t, F - 1))
        t = int(t)
        if t in used:
            raise ValueError("gmrf[%d]: term %d is listed twice" % (i, t))
        used.add(t)
        if e.indptr.size - 1 != int(levels[t]):
            raise ValueError("gmrf[%d]: Q has %d rows and term %d has %d levels" % (i, e.indptr.size - 1, t, int(levels[t])))
        if t in paired:
            raise ValueError("gmrf[%d]: term %d is in correlated[%d] (a GMRF term is in no pair)" % (i, t, paired[t]))
        if t in structd:
            raise ValueError("gmrf[%d]: term %d is structured[%d] (a term is structured or a GMRF, not both)" % (i, t, structd[t]))
        sl = slice(off[t], off[t + 1])
        if local is not None:
            flagged = np.flatnonzero(np.asarray(local)[sl])
            if flagged.size:
                raise ValueError("gmrf[%d]: local[%d] is set on level %d of term %d (a GMRF term takes no local scale)"
                                 % (i, off[t] + flagged[0], flagged[0], t))
        for name, arr, dflt in (("prior_mu", mu, 0.0), ("prior_tau", tau, 1.0), ("prior_kind", prior_kind, 0), ("prior_nu", nu, 0.0)):
            if arr is not None and (np.asarray(arr)[sl] != dflt).any():
                c = off[t] + int(np.flatnonzero(np.asarray(arr)[sl] != dflt)[0])
                raise ValueError("gmrf[%d]: %s[%d] must be the default %r on a column of term %d: the precision is its prior" % (i, name, c, dflt, t))
        term[i], kappa[i] = t, e.kappa
        start.append(start[-1][-1] + e.indptr[1:].astype(np.int64))
        col.append(e.indices.astype(np.int32))
        val.append(e.data.astype(np.float64))
    return (term, kappa, np.ascontiguousarray(np.concatenate(start)), np.ascontiguousarray(np.concatenate(col)),
            np.ascontiguousarray(np.concatenate(val)))


def gmrf_precision(model, i):
    """the dense precision Q of the model's i-th GMRF term, from the tables the Model holds"""
    if not 0 <= i < getattr(model, "G", 0):
        raise ValueError("GMRF %r: the model has %d" % (i, getattr(model, "G", 0)))
    r0 = sum(int(model.levels[int(t)]) for t in model.gmrf_term[:i])
    N = int(model.levels[int(model.gmrf_term[i])])
    st = model.gmrf_start[r0:r0 + N + 1]
    return _dense(N, st - st[0], model.gmrf_col[st[0]:st[-1]], model.gmrf_val[st[0]:st[-1]])


def gmrf_effects(Dd, levels, gmrf, structured=None, correlated=None, eta=2.0, A=0, scale=None, coefficients=None, aux=None):
    """the keyword arguments of GLM() for GMRF effects: what structured_effects(Dd, levels, structured, correlated, eta, A, scale,
    coefficients, aux) returns (random_intercepts(...) when neither is given), plus `gmrf` -- an ICAR effect over regions with a sampled
    scale next to an iid one on the same index (BYM) is
    GLM(X, Y, source, factors=[(region, N), (region, N)], **glm.gmrf_effects(X.shape[1], [N, N], [glm.gmrf(0, glm.scale_precision(glm.icar_precision(edges, N)), sum_to_zero=1e-3 * N)])).
    Every term gets a group of its own; the columns of a GMRF term keep the default prior entries, which the precision replaces."""
    gmrf = list(gmrf)
    lev = [int(N) for N in levels]
    if structured:
        kw = structured_effects(Dd, lev, structured, correlated, eta, A, scale, coefficients, aux)
    elif correlated:
        kw = correlated_effects(Dd, lev, correlated, eta, A, scale, coefficients, aux)
    else:
        kw = random_intercepts(Dd, lev, A, scale, coefficients, aux)
    gmrf_terms(gmrf, lev, kw.get("correlated"), kw.get("structured"))
    kw["gmrf"] = gmrf
    return kw


def smooth_effects(Dd, n_basis_list, order=2, sum_to_zero=1.0, levels=(), A=0, scale=None, coefficients=None, aux=None):
    """the keyword arguments of GLM() for penalised spline smooths: the first len(n_basis_list) <= 2 terms are glm.bspline terms of
    n_basis_list[f] basis functions each, then come the further terms of `levels`; what gmrf_effects(Dd, n_basis_list + levels,
    [glm.gmrf(f, glm.scale_precision(glm.rw2_precision(N)), sum_to_zero) ..]) returns -- every term a group of its own, whose sampled
    scale is the smooth's (the inverse of the smoothing parameter), the second-order difference penalty (order=1: the first-order one,
    rw1_precision) in place of the iid prior, and kappa = sum_to_zero holding the smooth's level against the intercept --
    GLM(X, Y, source, factors=[glm.bspline(x, 20)], **glm.smooth_effects(X.shape[1], [20])) is y ~ 1 + s(x)."""
    if order not in (1, 2):
        raise ValueError("order = %r must be 1 or 2 (the order of the difference penalty)" % (order,))
    nb = [int(N) for N in n_basis_list]
    if not 1 <= len(nb) <= 2:
        raise ValueError("one or two smooths (a model has at most 2 GMRF terms), got %d" % len(nb))
    prec = rw2_precision if order == 2 else rw1_precision
    terms = [gmrf(f, scale_precision(prec(N)), sum_to_zero) for f, N in enumerate(nb)]
    return gmrf_effects(Dd, nb + [int(N) for N in levels], terms, A=A, scale=scale, coefficients=coefficients, aux=aux)


def random_intercepts(Dd, levels, A=0, scale=None, coefficients=None, aux=None):
    """the keyword arguments groups, prior_mu, prior_tau, prior_kind and prior_nu of GLM() for random intercepts: Dd dense columns in no
    group, then factor f's levels[f] columns forming group f, whose sigma_f = exp(omega_f) is sampled --
    GLM(X, Y, source, factors=[subject, item], **glm.random_intercepts(X.shape[1], [n_subjects, n_items], scale=glm.half_student_t(3))).
    u ~ N(0, 1) on every level (so an intercept is N(0, sigma_f^2)), `scale` the spec(s) of the H = len(levels) group scales,
    `coefficients` those of the Dd dense columns and `aux` those of the auxiliary coordinates, as priors() takes them.
    Every term gets a group of its own, whether it has values or not: a random intercept and slope per subject, (1 + x | subject), is
    GLM(X, Y, source, factors=[subject, glm.term(subject, values=x)], **glm.random_intercepts(X.shape[1], [N, N])), the scale of the
    intercepts and the scale of the slopes sampled independently.  A sampled correlation between the two is correlated_effects()
    (GLM(..., correlated=[glm.pair(0, 1)])); a covariance among three or four terms is block_effects() (glm.block)."""
    Dd = int(Dd)
    lev = [int(N) for N in levels]
    if Dd < 1:
        raise ValueError("Dd = %d: at least one dense column is needed" % Dd)
    if len(lev) < 1 or min(lev) < 1:
        raise ValueError("levels must hold the positive number of levels of each factor, got %r" % (levels,))
    if len(lev) > 4:
        raise ValueError("at most 4 factors, each a group of its own (H <= 4), got %d" % len(lev))
    if coefficients is None or isinstance(coefficients, PriorSpec):
        coefficients = [normal() if coefficients is None else coefficients] * Dd
    coefficients = list(coefficients)
    if len(coefficients) != Dd:
        raise ValueError("coefficients must be one prior spec or a sequence of Dd = %d" % Dd)
    kw = priors(Dd + sum(lev), A, len(lev), coefficients=coefficients + [normal()] * sum(lev), aux=aux, scales=scale)
    kw["groups"] = np.concatenate([np.full(Dd, -1)] + [np.full(N, g) for g, N in enumerate(lev)]).astype(np.int32)
    return kw


random_effects = random_intercepts      # the name that fits terms with values: glm.random_effects(Dd, [N, N]) for (1 + x | subject)


# ---- priors ---------------------------------------------------------------------------------------------------------------------------
def prior_kinds(prior_kind, prior_nu, D, Dx, tau):
    """GLM()'s validation of prior_kind and prior_nu (scalars or length D; kinds as integers or names): (kind int32 (D,), nu (D,)),
    or (None, None) when neither is given.  The checks are idhmc_create_glm_priors'."""
    if prior_kind is None:
        if prior_nu is not None:
            raise ValueError("prior_nu needs prior_kind (only PRIOR_STUDENT_T and PRIOR_LOG_HALF_STUDENT_T take a nu)")
        return None, None
    raw = prior_kind if isinstance(prior_kind, np.ndarray) else np.asarray(prior_kind, dtype=object)      # (names and integers may mix)
    if raw.ndim > 1 or (raw.ndim == 1 and raw.shape[0] != D):
        raise ValueError("prior_kind must be a scalar or have one entry per sampled coordinate (%d), got shape %s" % (D, raw.shape))
    kind = np.empty(D, np.int32)
    for c, k in enumerate(np.broadcast_to(raw, (D,)).tolist()):
        if isinstance(k, str):
            name = k[6:] if k.startswith("PRIOR_") else k
            if name not in PRIOR_NAMES:
                raise ValueError("prior_kind[%d] = %r is not one of %s" % (c, k, ", ".join(PRIOR_NAMES)))
            k = PRIOR_NAMES.index(name)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k <= 4:
            raise ValueError("prior_kind[%d] = %r must be an integer in 0..4 or one of %s" % (c, k, ", ".join(PRIOR_NAMES)))
        kind[c] = k
    if prior_nu is None:
        nu = np.zeros(D)
    else:
        nu = np.asarray(prior_nu, dtype=np.float64)
        if nu.ndim > 1 or (nu.ndim == 1 and nu.shape[0] != D):
            raise ValueError("prior_nu must be a scalar or have one entry per sampled coordinate (%d), got shape %s" % (D, nu.shape))
        nu = np.array(np.broadcast_to(nu, (D,)))
    for c in range(D):
        k = int(kind[c])
        if k in (PRIOR_STUDENT_T, PRIOR_LOG_HALF_STUDENT_T):
            if not (np.isfinite(nu[c]) and nu[c] > 0.0):
                raise ValueError("prior_nu[%d] = %r must be finite and > 0 (PRIOR_%s)" % (c, float(nu[c]), PRIOR_NAMES[k]))
        elif nu[c] != 0.0:
            raise ValueError("prior_nu[%d] = %r must be 0 (PRIOR_%s takes no nu)" % (c, float(nu[c]), PRIOR_NAMES[k]))
        if k >= PRIOR_LOG_HALF_NORMAL:
            if c < Dx:
                raise ValueError("prior_kind[%d] = PRIOR_%s is a prior on exp(q): coordinate %d is a coefficient, not a logarithm (the log "
                                 "kinds are for the auxiliary coordinates and the group scales behind the %d coefficients)"
                                 % (c, PRIOR_NAMES[k], c, Dx))
            if tau is not None and tau[c] != 1.0:
                raise ValueError("prior_tau[%d] = %r must be 1 (PRIOR_%s: its one scale is exp(prior_mu))" % (c, float(tau[c]), PRIOR_NAMES[k]))
    return kind, nu


# one coordinate's prior as priors() takes it: the kind and the three numbers that go with it
PriorSpec = collections.namedtuple("PriorSpec", "kind mu tau nu")


def _positive(what, x):
    x = float(x)
    if not (np.isfinite(x) and x > 0.0):
        raise ValueError("%s = %r must be finite and > 0" % (what, x))
    return x


def _finite(what, x):
    x = float(x)
    if not np.isfinite(x):
        raise ValueError("%s = %r must be finite" % (what, x))
    return x


def normal(mean=0.0, sd=1.0):
    """q ~ N(mean, sd^2)"""
    return PriorSpec(PRIOR_NORMAL, _finite("mean", mean), 1.0 / _positive("sd", sd) ** 2, 0.0)


def student_t(nu, mean=0.0, scale=1.0):
    """q = mean + scale t_nu (Cauchy: nu = 1)"""
    return PriorSpec(PRIOR_STUDENT_T, _finite("mean", mean), 1.0 / _positive("scale", scale) ** 2, _positive("nu", nu))


def half_normal(scale=1.0):
    """sigma = exp(q) is half-normal with this scale"""
    return PriorSpec(PRIOR_LOG_HALF_NORMAL, float(np.log(_positive("scale", scale))), 1.0, 0.0)


def half_student_t(nu, scale=1.0):
    """sigma = exp(q) is half-t_nu with this scale (half-Cauchy: nu = 1)"""
    return PriorSpec(PRIOR_LOG_HALF_STUDENT_T, float(np.log(_positive("scale", scale))), 1.0, _positive("nu", nu))


def exponential(mean=1.0):
    """sigma = exp(q) is exponential with this mean"""
    return PriorSpec(PRIOR_LOG_EXPONENTIAL, float(np.log(_positive("mean", mean))), 1.0, 0.0)


def priors(Dx, A=0, H=0, J=0, coefficients=None, aux=None, scales=None, local_scales=None, *, P=0, correlations=None, S=0,
           autocorrelations=None):
    """the keyword arguments prior_mu, prior_tau, prior_kind and prior_nu of GLM() for Dx coefficients, A auxiliary coordinates, H
    group scales and J local scales (GLM(..., local=)): GLM(X, Y, source, aux=A, groups=g, **glm.priors(Dx, A, H, coefficients=glm.student_t(3), scales=glm.half_student_t(4))).
    Each role takes one spec (for every coordinate of the role) or a sequence of one spec per coordinate; None is normal(0, 1), today's
    prior (on a and omega: a standard normal on the logarithm).  The specs of sigma = exp(q) -- half_normal, half_student_t,
    exponential -- are for aux, scales and local_scales only.  P, correlations (keyword-only): the P zetas of GLM(..., correlated=), the
    coordinates behind the local scales; a spec there (normal or student_t on Fisher's z) is for a pair with eta = 0, a pair with eta > 0
    keeps the default.  S, autocorrelations (keyword-only): the S zetas of the AR(1) terms of GLM(..., structured=), the very last
    coordinates, under the same rules."""
    out = []
    for role, count, spec in (("coefficients", int(Dx), coefficients), ("aux", int(A), aux), ("scales", int(H), scales),
                              ("local_scales", int(J), local_scales), ("correlations", int(P), correlations),
                              ("autocorrelations", int(S), autocorrelations)):
        if count < 0:
            raise ValueError("%s: a count of %d" % (role, count))
        if spec is None:
            spec = normal()
        if isinstance(spec, PriorSpec):
            spec = [spec] * count
        spec = list(spec)
        if len(spec) != count or not all(isinstance(p, PriorSpec) for p in spec):
            raise ValueError("%s must be one prior spec or a sequence of %d (glm.normal, glm.student_t, glm.half_normal, glm.half_student_t, "
                             "glm.exponential)" % (role, count))
        if role in ("coefficients", "correlations", "autocorrelations"):
            for c, p in enumerate(spec):
                if p.kind >= PRIOR_LOG_HALF_NORMAL:
                    raise ValueError("%s[%d]: PRIOR_%s is a prior on exp(q); %s is not a logarithm"
                                     % (role, c, PRIOR_NAMES[p.kind], "a coefficient" if role == "coefficients" else "zeta = atanh rho" if role == "correlations" else "zeta = atanh phi"))
        out += spec
    return {"prior_mu": np.array([p.mu for p in out], np.float64), "prior_tau": np.array([p.tau for p in out], np.float64),
            "prior_kind": np.array([p.kind for p in out], np.int32), "prior_nu": np.array([p.nu for p in out], np.float64)}


def horseshoe(Dx, columns, global_scale, A=0, nu_local=1.0, nu_global=1.0, slab_scale=None, aux=None):
    """the keyword arguments groups, local, slab_scale, prior_mu, prior_tau, prior_kind and prior_nu of GLM() for a (regularised)
    horseshoe on `columns` (column indices or a length-Dx boolean mask) of Dx coefficients, with A auxiliary coordinates:
    GLM(X, Y, source, aux=A, **glm.horseshoe(Dx, columns, tau0, slab_scale=2.0)).  The columns form group 0, whose sigma = exp(omega_0) is
    the global scale with a half-t(nu_global, global_scale) prior; each has a local scale exp(lambda_k) with a half-t(nu_local) prior
    (half-Cauchy on both by default); u ~ N(0, 1) on every column, so an unshrunk column keeps beta_c ~ N(0, 1).  slab_scale: the fixed
    slab of the regularised horseshoe (None: the plain one).  aux: the spec(s) of the auxiliary coordinates, as priors() takes them."""
    Dx = int(Dx)
    cols = np.asarray(columns)
    if cols.dtype == np.bool_:
        if cols.shape != (Dx,):
            raise ValueError("a boolean columns must have one entry per column of X (%d), got shape %s" % (Dx, cols.shape))
        mask = cols.copy()
    else:
        if cols.ndim != 1 or not np.issubdtype(cols.dtype, np.integer) or cols.size == 0 or cols.min() < 0 or cols.max() >= Dx \
                or np.unique(cols).size != cols.size:
            raise ValueError("columns must be distinct column indices in 0..%d (or a boolean mask)" % (Dx - 1))
        mask = np.zeros(Dx, bool)
        mask[cols] = True
    J = int(mask.sum())
    if J == 0:
        raise ValueError("the horseshoe needs at least one column")
    kw = priors(Dx, A, 1, J, aux=aux, scales=half_student_t(nu_global, global_scale), local_scales=half_student_t(nu_local))
    kw["groups"] = np.where(mask, 0, -1).astype(np.int32)
    kw["local"] = mask.astype(np.int32)
    kw["slab_scale"] = None if slab_scale is None else _positive("slab_scale", slab_scale)
    return kw
