"""Ready-made observation sources for GLM(X, Y, source, constants) (include/idhmc.h, IDHMC_MODEL_GLM).

Each defines glm_observation(z, o, r, v): v = -log p(y | z) up to a term that depends on the data only, r = d log p(y | z) / dz.
None of them returns a NaN for a finite z; each is finite wherever the log density itself is (Poisson: exp of the linear
predictor below 709.78; everything else: every finite z).

  POISSON_LOG         K = 1: y = count;                     log mu = z
  POISSON_LOG_OFFSET  K = 2: y = (count, log exposure);     log mu = z + log exposure
  BINOMIAL_LOGIT      K = 2: y = (successes, trials);       logit p = z
  BERNOULLI_LOGIT     K = 1: y = 0 or 1;                    logit p = z  (the built-in LogisticRegression's arithmetic)
  STUDENT_T_IDENTITY  K = 1, constants (nu, sigma):         y = z + sigma t_nu
"""

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
