"""User-defined GLM likelihoods (IDHMC_MODEL_GLM): NUTS leapfrog steps/s of a GLM source on the matrix-core
gradient against the same arithmetic as an IDHMC_MODEL_CUSTOM source (one chain per wavefront), and of the logistic likelihood
as a GLM source against the built-in LogisticRegression; plus idhmc_create's wall time per form (a GLM's is mostly the hipRTC
compile).  Fixed eps, several transitions per launch, a shared metric, seeded synthetic data; each pair runs the same
trajectories (checked: same bits), so their step counts agree.  Prints one JSON document.  GPU box only.

The `gaussian` pair (IDHMC_MODEL_GLM_AUX): a linear regression with a sampled log sigma as an auxiliary-parameter
GLM against the same arithmetic as a custom source; its shapes name the columns of X (the chains have one coordinate more).
--aux-cost adds, per shape and chain count, the cost of the auxiliary coordinates: a fixed-sigma Gaussian as a plain GLM (A = 0),
GAUSSIAN_IDENTITY_LOGSIGMA (A = 1) and a four-parameter Gaussian (A = 4) on the same design, each with the form its NUTS kernel
runs (idhmc_glm_form).

The `hier` pair (GLM(..., groups=...)): a Bernoulli regression whose last min(40, Dx - 5) columns are one-hot
levels of one group with a sampled scale, on the matrix cores against the same arithmetic as a custom source; its shapes name the
columns of X (the chains have one coordinate more, the group's log scale).  --hier-cost adds the same design with H = 0, 1 and 4
groups (the one-hot columns dealt round to the groups), each started from its own Laplace approximation.

The `negbin` pair (NEG_BINOMIAL_LOG_LOGPHI): a negative-binomial regression with a sampled log dispersion on the
matrix cores against the same arithmetic (dlgamma_psi included) as a custom source; its shapes name the columns of X.
--dispersion-cost adds, per shape and chain count, the price of the gamma functions: the negative binomial next to POISSON_LOG on
the same design and counts (each started from its own Laplace approximation; different densities and trees, so steps/s), and a
beta regression (BETA_LOGIT_LOGPHI, three dlgamma_psi calls per observation) on the same design.

--responses M,... (GLM(..., chains_per_response=R)) adds, per shape and chain count C, the Poisson regression with
M responses of C / M chains each on the one design (the first response is the poisson pair's, the others are drawn from its fitted
model, each with its own seed; every chain starts from the first response's Laplace approximation): M = 1 is the plain GLM of the
existing entry point, the poisson pair's glm_poisson.  --chains-per-response R,... names the same rows by R (M = C / R).  --repeats K
makes K engines per row, for the run-to-run spread.

--adapt per-chain|per-response times, for every row of --responses, ONE ADAPTING TUNING STAGE with an adapted metric
window (tuning_stage(--stage-steps, adapt_metric=True), nothing stored) instead of the fixed-eps transitions: per-chain is EPS_PER_CHAIN +
METRIC_PER_CHAIN (the stage is one fused launch), per-response EPS_PER_RESPONSE + METRIC_PER_RESPONSE (one transition and one pooling
launch per transition; on the plain GLM of M = 1 the context-wide EPS_GLOBAL + METRIC_POOLED, which are the same thing there).  With a
pooled stepsize it also reports what sits between two transitions alone, by HIP events: idhmc_time_eps_adapt, and for the global
stepsize the same three launches enqueued by hand (accept_sum, da_adapt_global) between two torch events.

--prior-cost (GLM(..., prior_kind=, prior_nu=)) adds, per shape and chain count, what the priors' table costs: the
poisson pair's GLM with Gaussian priors, the same with a Student-t prior (nu = 3) on every coefficient, and the --hier-cost design
with H = 4 groups under Gaussian priors and with a half-t (nu = 4) on the four scales, each from the Gaussian model's Laplace
approximation.  Meant to run under --lockstep, so that every tree has the same length and ms per transition compares the gradients.

--local-cost (GLM(..., local=, slab_scale=)) adds, per shape DxN and chain count, what the per-coefficient local scales
cost, on the --hier-cost design with H = 1 and the Poisson likelihood (its 0 / 1 responses as counts): (i) without local scales; (ii)
every column with a local scale, no slab -- D lambdas more, so L doubles at D = 100; (iii) the same with slab_scale = 2; (iv) a control
without local scales on 2 D columns, which has the padded length of (ii) and (iii) and so does the same matrix work.  --local-rows picks
rows (i and iv run on a build without the keywords as well).  Meant to run under --lockstep.

--factor-cost (GLM(..., factors=)) runs, per row DdxLEVELSxN of --factor-rows and chain count, a pair on the same data:
the Poisson GLM with Dd dense columns and one factor by level index, its levels a group with a sampled scale (H = 1), and the same model on
the expanded matrix with one indicator column per level.  Both sides run the same trajectories (same_bits), so the ratio of their
steps/s is a time ratio.  --repeats K makes K engines per side (the best is reported, all are listed).  Meant to run under --lockstep
with --pairs ''.

--slope-cost (glm.term(index, values=)) runs, per row DdxLEVELSxN of --slope-rows and chain count, three models on the
same data: "slopes", the Poisson GLM with Dd dense columns, a plain term and a valued term of LEVELS levels each on one index,
(1 + x | s), each term a group with a sampled scale (H = 2); "expanded", the same model on glm.expand_factors' matrix; and "plain", the
factor model with the valued term replaced by a plain one (section 20's kernels on the same shape: what the value costs).  slopes and
expanded run the same trajectories (same_bits), so the ratio of their steps/s is a time ratio; plain is another model with trees of the
same length under --lockstep.  Meant to run under --lockstep with --pairs ''.

--corr-cost (GLM(..., correlated=)) runs, per row DdxLEVELSxN of --corr-rows and chain count, two models on the data
of --slope-cost: (1 + x | s) with a sampled correlation between intercept and slope (one pair, LKJ(2), one more coordinate), and the
same model without `correlated`, which runs the kernels of a build without the feature on the same shape.  Fixed eps and trees of the
same length under --lockstep: corr_over_uncorr is what the mix and its chain rule cost per gradient.  Meant to run under --lockstep
with --pairs ''.

--block-cost (GLM(..., correlated=[glm.block(..)])) runs, per row DdxLEVELSxN of --block-rows and chain count, two
models on the data of --slope-cost with a third valued term on the same index, (1 + x1 + x2 | s): the three terms in a K = 3 correlation
block (LKJ(2), three more coordinates), and the first two paired with the third independent (one more coordinate), which runs the kernels
of a build without the feature on the same shape.  Fixed eps and trees of the same length under --lockstep: block_over_pair is what the
wider mix and chain rule cost per gradient.  Meant to run under --lockstep with --pairs ''.

--struct-cost (GLM(..., structured=)) runs, per row DdxLEVELSxN of --struct-rows and chain count, three models on the
data of --slope-cost: (1 + x | s) with the intercepts an AR(1) sequence along the level index (Beta(2, 2) on (phi + 1) / 2, one more
coordinate), with the intercepts a first-order random walk (no coordinate), and the same model without `structured`, which runs the
kernels of a build without the feature on the same shape.  Fixed eps and trees of the same length under --lockstep: ar1_over_plain and
rw1_over_plain are what the scan and its mirror image cost per gradient.  Meant to run under --lockstep with --pairs ''.

--gmrf-cost (GLM(..., gmrf=)) runs, per row DdxLEVELSxN of --gmrf-rows and chain count, three models on the data of
--slope-cost: (1 + x | s) with an ICAR prior on the intercepts (the rook graph of a 10 x LEVELS/10 grid, scaled, sum_to_zero = 1), with a
second-order random walk on them (five entries per row, no sum-to-zero term), and the same model with the iid prior, which runs the
kernels of a build without the feature on the same shape.  No coordinate is added.  Fixed eps and trees of the same length under
--lockstep: icar_over_plain and rw2_over_plain are what the prior's sparse rows cost per gradient.  Meant to run under --lockstep with
--pairs ''.

--multi-cost (glm.members, glm.bspline) runs, per row BASISxN of --multi-rows and chain count, one cubic smooth of x
(y ~ 1 + x + s(x), Poisson, the iid prior and a sampled scale on the BASIS coefficients) in three ways on the same data: `wide`, the
basis as a factor term of width 4; `expanded`, the same model on glm.expand_factors (BASIS dense columns, four of them non-zero per
observation; the same bits, checked); `width1`, the same columns in a term of width 1 that keeps the first plane alone -- another
model, whose distance to `wide` is what the three further planes cost.  Meant to run under --lockstep with --pairs ''.

    python tools/bench_glm.py [--shapes 100x1000,25x1000] [--chains 16384,65536] [--pairs poisson,logistic,gaussian,hier,negbin]
                              [--transitions 5] [--aux-cost] [--hier-cost] [--dispersion-cost] [--metric shared|per_chain] [--lockstep]
                              [--responses 1,4096] [--chains-per-response 16] [--repeats 1] [--adapt per-chain|per-response] [--stage-steps 25]
                              [--prior-cost] [--local-cost] [--local-rows i,ii,iii,iv]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import inplacedhmc_jl_amd as pkg  # noqa: E402
from bench_logistic import CUSTOM_SRC, PEAK_FP64_MFMA, custom_params, padded  # noqa: E402
from bench_logistic import problem as logistic_problem  # noqa: E402

# the Poisson log-link likelihood as a custom source: bench_logistic's per-wave logistic density with its terms swapped
_LR_TERMS = CUSTOM_SRC[CUSTOM_SRC.index("__device__ void lr_terms"):CUSTOM_SRC.index("template <int NCH>")]
CUSTOM_POISSON_SRC = CUSTOM_SRC.replace(_LR_TERMS, r"""__device__ void lr_terms(double z, double y, double &r, double &v)
{
    const double e = dexp(z);
    v = e - y * z;
    r = y - e;
}
""")


# the Gaussian likelihood with a sampled log sigma (the chain's last coordinate) as a custom source: GAUSSIAN_IDENTITY_LOGSIGMA's
# arithmetic in section 12's order -- z over the D - 1 columns of X, the score summed per residue like v, its tree into the owner lane
CUSTOM_GAUSSIAN_SRC = CUSTOM_SRC.replace(_LR_TERMS, r"""__device__ void lr_terms(double z, double y, double a, double &r, double &v, double &s)
{
    const double w = dexp(-a);
    const double u = (y - z) * w;
    v = 0.5 * (u * u) + a;
    r = u * w;
    s = u * u - 1.0;
}
""").replace("double a0 = 0.0, a1 = 0.0;", "double a0 = 0.0, a1 = 0.0, s0 = 0.0, s1 = 0.0;"
).replace("for (int c = 0; c < D; ++c) {", "for (int c = 0; c < D - 1; ++c) {"
).replace("double rx, vx, ry, vy;", "double rx, vx, ry, vy, ux, uy;\n        const double la = buf[D - 1];"
).replace("lr_terms(zx, yv.x, rx, vx);", "lr_terms(zx, yv.x, la, rx, vx, ux);"
).replace("lr_terms(zy, yv.y, ry, vy);", "lr_terms(zy, yv.y, la, ry, vy, uy);"
).replace("a1 = a1 + vy;", "a1 = a1 + vy;\n        s0 = s0 + (i0 >= n ? 0.0 : ux);\n        s1 = s1 + (i0 + 1 >= n ? 0.0 : uy);"
).replace("    double t0 = 0.0, t1 = 0.0;", r"""    {
        const double S = wave_sum(s0, s1);
        const int c = D - 1;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const bool here = (c >> 7) == j && lane == ((c & 127) >> 1);
            G.c[j].x = here && !(c & 1) ? S : G.c[j].x;
            G.c[j].y = here && (c & 1) ? S : G.c[j].y;
        }
    }
    double t0 = 0.0, t1 = 0.0;""")
assert CUSTOM_GAUSSIAN_SRC.count("la,") == 2 and "s1 = s1 +" in CUSTOM_GAUSSIAN_SRC and "wave_sum(s0, s1)" in CUSTOM_GAUSSIAN_SRC

# the negative binomial with a sampled log phi as a custom source: the Gaussian's frame (section 12's order) around
# NEG_BINOMIAL_LOG_LOGPHI's arithmetic, statement for statement
_G_TERMS = CUSTOM_GAUSSIAN_SRC[CUSTOM_GAUSSIAN_SRC.index("__device__ void lr_terms"):CUSTOM_GAUSSIAN_SRC.index("template <int NCH>")]
CUSTOM_NEGBIN_SRC = CUSTOM_GAUSSIAN_SRC.replace(_G_TERMS, r"""__device__ void lr_terms(double z, double y, double a, double &r, double &v, double &s)
{
    const double ph = dexp(a);
    const double t = z - a;
    const double e = dexp(-__builtin_fabs(t));
    const double sp = (t > 0.0 ? t : 0.0) + dlog1p(e);
    const double sg = (t >= 0.0 ? 1.0 : e) / (1.0 + e);
    const double yp = y + ph;
    double l1, p1, l0, p0;
    dlgamma_psi(yp, l1, p1);
    dlgamma_psi(ph, l0, p0);
    v = (yp * sp - y * t) - (l1 - l0);
    r = y - yp * sg;
    s = ph * ((p1 - p0) - sp) - r;
}
""")
assert CUSTOM_NEGBIN_SRC.count("dlgamma_psi(") == 2 and "wave_sum(s0, s1)" in CUSTOM_NEGBIN_SRC and "u * u" not in CUSTOM_NEGBIN_SRC

# the Bernoulli likelihood with one coefficient group as a custom source, section 13's arithmetic: the chain's last coordinate is the
# group's log scale, params carry the group of every coordinate (as doubles, -1: none) behind tau; b = u e is staged instead of q,
# the chain rule follows G
CUSTOM_HIER_SRC = CUSTOM_SRC.replace("*mu = y + npad, *tau = mu + L;", "*mu = y + npad, *tau = mu + L, *grp = tau + L;"
).replace("    double2 *b2 = reinterpret_cast<double2 *>(buf) + lane;", r"""    const int co = D - 1;
    double om = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) om = (co >> 7) == j ? ((co & 1) ? q.c[j].y : q.c[j].x) : om;
    const double e = dexp(read_lane(om, (co & 127) >> 1));
    const double2 *g2 = reinterpret_cast<const double2 *>(grp) + lane;
    double2 *b2 = reinterpret_cast<double2 *>(buf) + lane;"""
).replace("        for (int j = 0; j < NCH; ++j) b2[j * 64] = q.c[j];", r"""        for (int j = 0; j < NCH; ++j) {
            const double2 id = g2[j * 64];
            b2[j * 64] = make_double2(id.x >= 0.0 ? q.c[j].x * e : q.c[j].x, id.y >= 0.0 ? q.c[j].y * e : q.c[j].y);
        }"""
).replace("for (int c = 0; c < D; ++c) {", "for (int c = 0; c < D - 1; ++c) {"
).replace("    double t0 = 0.0, t1 = 0.0;", r"""    {
        double w0 = 0.0, w1 = 0.0;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const double2 id = g2[j * 64];
            const double bx = id.x >= 0.0 ? q.c[j].x * e : q.c[j].x, by = id.y >= 0.0 ? q.c[j].y * e : q.c[j].y;
            w0 = w0 + (id.x >= 0.0 ? G.c[j].x * bx : 0.0);
            w1 = w1 + (id.y >= 0.0 ? G.c[j].y * by : 0.0);
        }
        const double W = wave_sum(w0, w1);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const bool here = (co >> 7) == j && lane == ((co & 127) >> 1);
            G.c[j].x = here && !(co & 1) ? W : G.c[j].x;
            G.c[j].y = here && (co & 1) ? W : G.c[j].y;
            const double2 id = g2[j * 64];
            G.c[j].x = id.x >= 0.0 ? G.c[j].x * e : G.c[j].x;
            G.c[j].y = id.y >= 0.0 ? G.c[j].y * e : G.c[j].y;
        }
    }
    double t0 = 0.0, t1 = 0.0;""")
assert CUSTOM_HIER_SRC.count("g2[j * 64]") == 3 and "c < D - 1" in CUSTOM_HIER_SRC and "*grp = tau + L" in CUSTOM_HIER_SRC

# a fixed-sigma Gaussian as a plain GLM (constant log sigma), and one with four auxiliary parameters (mean and log scale move with y1)
GAUSSIAN_FIXED_SRC = r"""
__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)
{
    const double w = dexp(-o.c[0]);
    const double u = (o.y[0] - z) * w;
    v = 0.5 * (u * u) + o.c[0];
    r = u * w;
}
"""
GAUSSIAN_A4_SRC = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double ls = a[0] + a[3] * o.y[1];
    const double w = dexp(-ls);
    const double u = (o.y[0] - z - a[1] * o.y[1] - a[2]) * w;
    v = 0.5 * (u * u) + ls;
    r = u * w;
    s[0] = u * u - 1.0;
    s[1] = r * o.y[1];
    s[2] = r;
    s[3] = s[0] * o.y[1];
}
"""


def gaussian_problem(n, D, seed):
    """y = X beta + sigma eps; the Laplace approximation at the MAP in (beta, log sigma), prior N(0, I)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    y = X @ (rng.standard_normal(D) * 0.5) + 0.7 * rng.standard_normal(n)
    q = np.zeros(D + 1)                               # Newton from the least-squares fit (from 0 its full steps in log sigma overshoot)
    q[:D] = np.linalg.lstsq(X, y, rcond=None)[0]
    q[D] = 0.5 * np.log(np.mean((y - X @ q[:D]) ** 2))
    for _ in range(40):
        w2, e = np.exp(-2.0 * q[D]), y - X @ q[:D]
        g = np.concatenate([w2 * X.T @ e, [w2 * e @ e - n]]) - q
        H = np.zeros((D + 1, D + 1))
        H[:D, :D] = w2 * X.T @ X
        H[:D, D] = H[D, :D] = 2.0 * w2 * X.T @ e
        H[D, D] = 2.0 * w2 * e @ e
        H += np.eye(D + 1)
        q = q + np.linalg.solve(H, g)
    return X, y, q, np.linalg.inv(H)


def poisson_problem(n, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    beta = rng.standard_normal(D) * 0.5
    y = rng.poisson(np.exp(X @ beta)).astype(np.float64)
    q = np.zeros(D)                                   # Laplace approximation at the MAP (prior N(0, I))
    for _ in range(40):
        m = np.exp(X @ q)
        H = (X.T * m) @ X + np.eye(D)
        q = q + np.linalg.solve(H, X.T @ (y - m) - q)
    return X, y, q, np.linalg.inv(H)


def newton_laplace(density, q):
    """the maximum of density(q) -> (l, grad l) by damped Newton steps on a finite-difference Hessian, and the Laplace covariance there"""
    D = q.size

    def hessian(q):
        Hm = np.empty((D, D))
        for c in range(D):
            d = np.zeros(D)
            d[c] = 1e-5
            Hm[c] = (density(q + d)[1] - density(q - d)[1]) / 2e-5
        return -0.5 * (Hm + Hm.T)
    for _ in range(60):
        l, g = density(q)
        Hm = hessian(q)
        w = np.linalg.eigvalsh(Hm)[0]
        step = np.linalg.solve(Hm + max(0.0, 0.1 - w) * np.eye(D), g)
        t = 1.0
        with np.errstate(all="ignore"):                # a full step may leave the support: the density is then NaN and the step is halved
            while not density(q + t * step)[0] >= l and t > 1e-6:
                t *= 0.5
        q = q + t * step
        if np.abs(t * step).max() < 1e-10:
            break
    w, V = np.linalg.eigh(hessian(q))
    return q, (V / np.maximum(w, 1e-3)) @ V.T


def negbin_density(X, y, q):
    """(l, grad l) of the negative-binomial regression, q = [beta | log phi], prior N(0, I)"""
    from scipy import special
    D = X.shape[1]
    ph, t = np.exp(q[D]), X @ q[:D] - q[D]
    sp, r = np.logaddexp(0.0, t), y - (y + ph) * special.expit(t)
    l = np.sum(special.gammaln(y + ph) - special.gammaln(ph) - (y + ph) * sp + y * t)
    s = np.sum(ph * (special.digamma(y + ph) - special.digamma(ph) - sp) - r)
    return l - 0.5 * q @ q, np.r_[X.T @ r, s] - q


def beta_density(X, Y, q):
    """(l, grad l) of the beta regression, Y = (log y, log(1 - y)), q = [beta | log phi], prior N(0, I)"""
    from scipy import special
    D = X.shape[1]
    z, ph = X @ q[:D], np.exp(q[D])
    p, k = ph * special.expit(z), ph * special.expit(-z)
    dg = special.digamma
    l = np.sum(special.gammaln(ph) - special.gammaln(p) - special.gammaln(k) + p * Y[:, 0] + k * Y[:, 1])
    r = p * special.expit(-z) * (Y[:, 0] - Y[:, 1] - dg(p) + dg(k))
    s = np.sum(ph * dg(ph) - p * dg(p) - k * dg(k) + p * Y[:, 0] + k * Y[:, 1])
    return l - 0.5 * q @ q, np.r_[X.T @ r, s] - q


def dispersion_design(n, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    return rng, X, X @ (rng.standard_normal(D) * 0.5)


def negbin_problem(n, D, seed):
    """counts with mean exp(X beta) and dispersion phi = 3; the Laplace approximation at the MAP in (beta, log phi), prior N(0, I)"""
    rng, X, z = dispersion_design(n, D, seed)
    y = rng.negative_binomial(3.0, 3.0 / (3.0 + np.exp(z))).astype(np.float64)
    q, cov = newton_laplace(lambda q: negbin_density(X, y, q), np.r_[np.zeros(D), np.log(3.0)])
    return X, y, q, cov


def poisson_laplace(X, y):
    """the Poisson regression's own MAP and Laplace covariance on a design and counts given (prior N(0, I))"""
    D = X.shape[1]
    q = np.zeros(D)
    for _ in range(60):
        m = np.exp(X @ q)
        H = (X.T * m) @ X + np.eye(D)
        q = q + np.linalg.solve(H, X.T @ (y - m) - q)
    return q, np.linalg.inv(H)


def beta_problem(n, D, seed):
    """proportions with mean sigma(X beta) and precision phi = 8 as (log y, log(1 - y)); MAP and Laplace covariance in (beta, log phi)"""
    rng, X, z = dispersion_design(n, D, seed)
    m = 1.0 / (1.0 + np.exp(-z))
    Y = pkg.glm.beta_response(np.clip(rng.beta(8.0 * m, 8.0 * (1.0 - m)), 1e-12, 1.0 - 1e-12))
    q, cov = newton_laplace(lambda q: beta_density(X, Y, q), np.r_[np.zeros(D), np.log(8.0)])
    return X, Y, q, cov


def hier_groups(Dx, H):
    """the last min(40, Dx - 5) columns are the grouped ones, dealt round to the H groups (H = 0: no groups)"""
    grp = np.full(Dx, -1, np.int32)
    if H > 0:
        k = min(40, Dx - 5)
        grp[Dx - k:] = np.arange(k) % H
    return grp


def hier_density(X, y, grp, q):
    """(l, grad l) of the Bernoulli model with groups, prior N(0, I) on the sampled coordinates q = [u | omega]"""
    Dx, H = X.shape[1], int(grp.max()) + 1
    s = np.where(grp >= 0, np.exp(q[Dx:])[np.maximum(grp, 0)], 1.0) if H else np.ones(Dx)
    b = s * q[:Dx]
    z = X @ b
    G = X.T @ (y - 1.0 / (1.0 + np.exp(-z)))
    g = np.concatenate([s * G, [np.sum((G * b)[grp == k]) for k in range(H)]]) - q
    return np.sum(y * z - np.logaddexp(0.0, z)) - 0.5 * q @ q, g


def hier_laplace(X, y, grp):
    """the MAP in (u, omega) by damped Newton steps on a finite-difference Hessian, and the Laplace covariance there"""
    Dx, H = X.shape[1], int(grp.max()) + 1
    D = Dx + H
    q = np.r_[np.zeros(Dx), np.full(H, np.log(0.6))]
    q[:Dx] = 0.1

    def hessian(q):
        Hm = np.empty((D, D))
        for c in range(D):
            d = np.zeros(D)
            d[c] = 1e-5
            Hm[c] = (hier_density(X, y, grp, q + d)[1] - hier_density(X, y, grp, q - d)[1]) / 2e-5
        return -0.5 * (Hm + Hm.T)
    for _ in range(60):
        l, g = hier_density(X, y, grp, q)
        Hm = hessian(q)
        w = np.linalg.eigvalsh(Hm)[0]
        step = np.linalg.solve(Hm + max(0.0, 0.1 - w) * np.eye(D), g)      # a positive definite model of -l
        t = 1.0
        while not hier_density(X, y, grp, q + t * step)[0] >= l and t > 1e-6:
            t *= 0.5
        q = q + t * step
        if np.abs(t * step).max() < 1e-10:
            break
    Hm = hessian(q)
    w, V = np.linalg.eigh(Hm)
    return q, (V / np.maximum(w, 1e-3)) @ V.T


def hier_problem(n, D, seed, H=1):
    """Bernoulli responses from a design whose grouped columns are one-hot levels (scale 0.6); (X, y, MAP, Laplace covariance)"""
    rng = np.random.default_rng(seed)
    grp = hier_groups(D, 1)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    cols = np.flatnonzero(grp >= 0)
    X[:, cols] = 0.0
    X[np.arange(n), cols[rng.integers(0, cols.size, n)]] = 1.0
    beta = np.where(grp >= 0, 0.6, 1.0) * rng.standard_normal(D)
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    q, cov = hier_laplace(X, y, hier_groups(D, H))
    return X, y, q, cov


def model(form, X, y, q_map=None):
    D = X.shape[1]
    if form == "glm_hier_h4_halft":                   # glm_hier_h4 with a half-t (nu = 4) on the four scales
        return pkg.GLM(X, y, pkg.glm.BERNOULLI_LOGIT, groups=hier_groups(D, 4), **pkg.glm.priors(D, 0, 4, scales=pkg.glm.half_student_t(4.0)))
    if form == "glm_poisson_t":                       # glm_poisson with a Student-t (nu = 3) on every coefficient
        return pkg.GLM(X, y, pkg.glm.POISSON_LOG, **pkg.glm.priors(D, coefficients=pkg.glm.student_t(3.0)))
    if form.startswith("glm_local"):                  # the hier design (H = 1) with Poisson counts: _base (and the control), _all, _all_slab
        kw = {} if form == "glm_local_base" else {"local": True, "slab_scale": 2.0 if form.endswith("slab") else None}
        return pkg.GLM(X, y, pkg.glm.POISSON_LOG, groups=hier_groups(D, 1), **kw)
    if form.startswith("glm_hier"):                   # glm_hier (H = 1), glm_hier_h0, glm_hier_h4
        H = int(form[-1]) if form[-2:-1] == "h" else 1
        return pkg.GLM(X, y, pkg.glm.BERNOULLI_LOGIT, groups=hier_groups(D, H) if H else None)
    if form == "custom_hier":                         # the chain's D + 1 coordinates: a zero column of X in the place of the log scale
        grp = np.full(padded(D + 1), -1.0)
        grp[:D] = hier_groups(D, 1)
        return pkg.CustomDensity(D + 1, CUSTOM_HIER_SRC, np.concatenate([custom_params(np.c_[X, np.zeros(len(X))], y), grp]))
    if form == "glm_negbin":
        return pkg.GLM(X, y, pkg.glm.NEG_BINOMIAL_LOG_LOGPHI, aux=1)
    if form == "custom_negbin":                       # the chain's D + 1 coordinates: a zero column of X in the place of log phi
        return pkg.CustomDensity(D + 1, CUSTOM_NEGBIN_SRC, custom_params(np.c_[X, np.zeros(len(X))], y))
    if form == "glm_beta":
        return pkg.GLM(X, y, pkg.glm.BETA_LOGIT_LOGPHI, aux=1)
    if form == "glm_gaussian":
        return pkg.GLM(X, y, pkg.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1)
    if form == "custom_gaussian":                     # the chain's D + 1 coordinates: a zero column of X in the place of log sigma
        return pkg.CustomDensity(D + 1, CUSTOM_GAUSSIAN_SRC, custom_params(np.c_[X, np.zeros(len(X))], y))
    if form == "glm_gaussian_fixed":
        return pkg.GLM(X, y, GAUSSIAN_FIXED_SRC, constants=[q_map[D]])
    if form == "glm_gaussian_a4":
        return pkg.GLM(X, np.c_[y, np.random.default_rng(5).uniform(-1.0, 1.0, len(y))], GAUSSIAN_A4_SRC, aux=4)
    if form == "glm_poisson":
        return pkg.GLM(X, y, pkg.glm.POISSON_LOG)
    if form == "custom_poisson":
        return pkg.CustomDensity(D, CUSTOM_POISSON_SRC, custom_params(X, y))
    if form == "glm_logistic":
        return pkg.GLM(X, y, pkg.glm.BERNOULLI_LOGIT)
    return pkg.LogisticRegression(X, y)


LOCKSTEP = False    # --lockstep: every tree runs to max_depth = 6 (63 steps), see main()


def responses_model(X, y, q_map, M, C):
    """the Poisson regression with M responses of C / M chains: Y[0] = y, the others drawn from the fitted model"""
    Y = np.empty((M, len(y), 1))
    Y[0, :, 0] = y
    mean = np.exp(X @ q_map)
    for m in range(1, M):
        Y[m, :, 0] = np.random.default_rng(1000003 * m + len(y)).poisson(mean)
    return pkg.GLM(X, Y, pkg.glm.POISSON_LOG, chains_per_response=C // M)


def factor_problem(Dd, N, n, seed):
    """a Poisson regression with Dd dense columns and one factor of N levels in a group of its own (H = 1): (X (n, Dd), y, index, the
    keywords of both models, a start q and a narrow covariance around it for `run`)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, Dd)) / np.sqrt(Dd)
    X[:, 0] = 1.0
    idx = rng.integers(0, N, n)
    sigma = 0.5
    u = rng.standard_normal(N)
    beta = np.r_[0.5, 0.3 * rng.standard_normal(Dd - 1)]
    y = rng.poisson(np.exp(X @ beta + sigma * u[idx])).astype(float)
    kw = pkg.glm.random_intercepts(Dd, [N])
    q0 = np.r_[beta, u, np.log(sigma)]
    return X, y, idx, kw, q0, np.eye(q0.size) * 1e-4


def slope_problem(Dd, N, n, seed):
    """a Poisson regression with Dd dense columns and a random intercept and slope per level of one index, (1 + x | s), each of the two
    terms in a group of its own (H = 2): (X (n, Dd), y, index, x, the keywords of the models, a start q and a narrow covariance around it
    for `run`)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, Dd)) / np.sqrt(Dd)
    X[:, 0] = 1.0
    idx = rng.integers(0, N, n)
    x = 0.5 * rng.standard_normal(n)
    s0, s1 = 0.5, 0.3
    u0, u1 = rng.standard_normal(N), rng.standard_normal(N)
    beta = np.r_[0.5, 0.3 * rng.standard_normal(Dd - 1)]
    y = rng.poisson(np.exp(X @ beta + s0 * u0[idx] + s1 * x * u1[idx])).astype(float)
    kw = pkg.glm.random_effects(Dd, [N, N])
    q0 = np.r_[beta, u0, u1, np.log(s0), np.log(s1)]
    return X, y, idx, x, kw, q0, np.eye(q0.size) * 1e-4


def smooth_problem(N, n, seed):
    """a Poisson regression y ~ 1 + x + s(x): (X (n, 2), y, the cubic B-spline term of N basis functions, the keywords of the models --
    the term's N columns a group of its own -- and a start q for `run`)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, n)
    X = np.c_[np.ones(n), x - 0.5]
    term = pkg.glm.bspline(x, N, lo=0.0, hi=1.0)
    sigma, u = 0.5, rng.standard_normal(N)
    y = rng.poisson(np.exp(0.5 + 0.3 * (x - 0.5) + sigma * (term.weights * u[term.index]).sum(1))).astype(float)
    return X, y, term, pkg.glm.random_intercepts(2, [N]), np.r_[0.5, 0.3, u, np.log(sigma)]


def run(form, X, y, q_map, cov, C, T, seed=1, metric=None, mdl=None):
    t0 = time.perf_counter()
    eng = pkg.Engine(model(form, X, y, q_map) if mdl is None else mdl, C, pkg.default_options(metric_mode=pkg.METRIC_SHARED if metric is None else metric,
                                                                      max_depth=6 if LOCKSTEP else 10), seed=seed)
    create_s = time.perf_counter() - t0
    Dx = X.shape[1]
    if form == "glm_gaussian_fixed":                  # the coefficients alone
        q_map, cov = q_map[:Dx], cov[:Dx, :Dx]
    elif form == "glm_gaussian_a4":                   # three more coordinates, near 0 and narrow
        q_map = np.r_[q_map, np.zeros(3)]
        big = np.eye(Dx + 4) * 1e-4
        big[:Dx + 1, :Dx + 1] = cov
        cov = big
    elif form.startswith("glm_local_all"):            # one log local scale per column more, near 0 and narrow
        q_map = np.r_[q_map, np.zeros(Dx)]
        big = np.eye(2 * Dx + 1) * 1e-4
        big[:Dx + 1, :Dx + 1] = cov
        cov = big
    D = q_map.size
    rng = np.random.default_rng(seed)
    eng.set_q(q_map + rng.standard_normal((C, D)) @ np.linalg.cholesky(cov).T)
    eps = 0.5 * np.sqrt(np.linalg.eigvalsh(cov)[0]) * (1e-3 if LOCKSTEP else 1.0)
    eng.set_eps(eps)
    head = (eng.lq[:64].copy(), eng.grad[:64].copy())
    eng.nuts_transitions(1, 2)                        # warm-up (and the module's first launch)
    eng.synchronize()
    s0 = eng.total_steps()
    ms = eng.time_transitions_fused(T, 100)
    steps = eng.total_steps() - s0
    st = eng.tree_stats()
    out = dict(create_s=create_s, ms_per_transition=ms / T, leapfrog_steps_per_s=steps / ms * 1e3, steps=int(steps), eps=float(eps),
               mean_depth=float(st["depth"].mean()), acceptance=float(st["acceptance_rate"].mean()))
    if hasattr(eng, "glm_form"):
        out["glm_form"] = eng.glm_form()
    tail = eng.q[:64].copy()
    eng.close()
    return out, head, tail


def global_adapt_by_hand(eng, n):
    """n times (accept_sum, da_adapt_global) -- the global stepsize's three launches -- between two torch events: milliseconds"""
    import torch
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        buf = torch.zeros(pkg.XCHG_DOUBLES, dtype=torch.float64, device="cuda")
    st.synchronize()
    eng.synchronize()
    eng.set_stream(st.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(n):
        eng.accept_sum(buf.data_ptr())
        eng.da_adapt_global(buf.data_ptr())
    e1.record(st)
    e1.synchronize()
    eng.set_stream(None)
    return e0.elapsed_time(e1)


def run_adapt(X, y, q_map, cov, C, N, adapt, seed=1, mdl=None):
    """one adapting tuning stage of N transitions with a metric window, from the start `run` uses; wall time, the stream idle at both ends"""
    if adapt == "per-chain":
        eps_mode, metric = pkg.EPS_PER_CHAIN, pkg.METRIC_PER_CHAIN
    elif mdl is None:
        eps_mode, metric = pkg.EPS_GLOBAL, pkg.METRIC_POOLED
    else:
        eps_mode, metric = pkg.EPS_PER_RESPONSE, pkg.METRIC_PER_RESPONSE
    t0 = time.perf_counter()
    eng = pkg.Engine(model("glm_poisson", X, y, q_map) if mdl is None else mdl, C,
                     pkg.default_options(eps_mode=eps_mode, metric_mode=metric, max_depth=10), seed=seed)
    create_s = time.perf_counter() - t0
    q0 = q_map + np.random.default_rng(seed).standard_normal((C, q_map.size)) @ np.linalg.cholesky(cov).T
    eps = 0.5 * np.sqrt(np.linalg.eigvalsh(cov)[0])

    def start():
        eng.set_q(q0)
        eng.set_eps(eps)
        eng.set_minv(np.ones(q_map.size))
        eng.synchronize()
    start()
    eng.tuning_stage(2, True, 0, store_draws=False, store_stats=False)      # warm-up (and the module's first launches)
    start()
    s0 = eng.total_steps()
    t0 = time.perf_counter()
    eng.tuning_stage(N, True, 0, store_draws=False, store_stats=False)
    eng.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    steps = eng.total_steps() - s0
    e = eng.eps
    out = dict(create_s=create_s, adapt=adapt, eps_mode=int(eps_mode), metric_mode=int(metric), stage_transitions=N, stage_ms=ms,
               ms_per_transition=ms / N, steps=int(steps), leapfrog_steps_per_s=steps / ms * 1e3, eps_start=float(eps),
               eps_final_mean=float(e.mean()), eps_final_distinct=int(len(set(e))), minv_mean=float(eng.minv[:64].mean()),
               fused=bool(eng.fused_launch_info()[1] and adapt == "per-chain"), glm_form=eng.glm_form())
    if adapt == "per-response":
        n = 400
        eng.da_init()
        if hasattr(eng, "time_eps_adapt"):
            eng.time_eps_adapt(20)
            out["eps_adapt_us_per_transition"] = eng.time_eps_adapt(n) / n * 1e3
            out["eps_adapt_launches"] = 3 if eps_mode == pkg.EPS_GLOBAL else 1
        if eps_mode == pkg.EPS_GLOBAL:
            global_adapt_by_hand(eng, 20)
            out["eps_adapt_by_hand_us_per_transition"] = global_adapt_by_hand(eng, n) / n * 1e3
    eng.close()
    return out


PAIRS = {"poisson": ("glm_poisson", "custom_poisson", poisson_problem),
         "logistic": ("glm_logistic", "builtin_logistic", logistic_problem),
         "gaussian": ("glm_gaussian", "custom_gaussian", gaussian_problem),
         "hier": ("glm_hier", "custom_hier", hier_problem),
         "negbin": ("glm_negbin", "custom_negbin", negbin_problem)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100x1000,25x1000", help="DxN,...")
    ap.add_argument("--chains", default="16384,65536")
    ap.add_argument("--pairs", default="poisson,logistic")
    ap.add_argument("--transitions", type=int, default=5)
    ap.add_argument("--aux-cost", action="store_true", help="the fixed-sigma, A = 1 and A = 4 Gaussians per shape (DESIGN section 12)")
    ap.add_argument("--hier-cost", action="store_true", help="the hier pair's design with H = 0, 1 and 4 groups per shape (DESIGN section 13)")
    ap.add_argument("--dispersion-cost", action="store_true", help="the negative binomial next to POISSON_LOG on the same design and counts, "
                    "and a beta regression, per shape (DESIGN section 14)")
    ap.add_argument("--prior-cost", action="store_true", help="the Poisson GLM with Gaussian and with Student-t priors on the coefficients, and "
                    "the hier design (H = 4) with Gaussian and with half-t priors on the scales, per shape (DESIGN section 18); use --lockstep")
    ap.add_argument("--local-cost", action="store_true", help="the hier design (H = 1, Poisson) without local scales, with one on every "
                    "column, the same with a slab, and a control of twice the columns without any (DESIGN section 19); use --lockstep")
    ap.add_argument("--local-rows", default="i,ii,iii,iv", help="the rows of --local-cost to run")
    ap.add_argument("--factor-cost", action="store_true", help="per row of --factor-rows a pair on the same data: the Poisson GLM with one "
                    "factor by level index (H = 1 on its levels) and the same model on the expanded matrix (DESIGN section 20); use --lockstep, "
                    "and --pairs '' to run nothing else")
    ap.add_argument("--factor-rows", default="20x200x1000,20x200x10000,20x900x10000,100x20x1000", help="DdxLEVELSxN,...")
    ap.add_argument("--factor-sides", default="factor,expanded", help="the sides of each pair to run")
    ap.add_argument("--slope-cost", action="store_true", help="per row of --slope-rows three models on the same data: a plain and a valued "
                    "term on one index (H = 2), the same model on the expanded matrix, and both terms plain (DESIGN section 21); use "
                    "--lockstep, and --pairs '' to run nothing else")
    ap.add_argument("--slope-rows", default="20x100x1000,20x100x10000,20x450x10000,100x10x1000,20x200x1000", help="DdxLEVELSxN,... "
                    "(LEVELS per term: the model has 2 LEVELS level columns)")
    ap.add_argument("--slope-sides", default="slopes,expanded,plain", help="the sides of each row to run")
    ap.add_argument("--corr-cost", action="store_true", help="per row of --corr-rows the model of --slope-cost with the two terms paired "
                    "(a sampled correlation, LKJ(2)) and without (DESIGN section 22); use --lockstep, and --pairs '' to run nothing else")
    ap.add_argument("--corr-rows", default="20x100x1000,20x200x1000", help="DdxLEVELSxN,... (section 21's rows 1 and 1')")
    ap.add_argument("--corr-sides", default="corr,uncorr", help="the sides of each row to run")
    ap.add_argument("--block-cost", action="store_true", help="per row of --block-rows (1 + x1 + x2 | s) with the three terms in a K = 3 "
                    "correlation block, and with the first two paired and the third independent (DESIGN section 26); use --lockstep, and "
                    "--pairs '' to run nothing else")
    ap.add_argument("--block-rows", default="20x70x1000,20x150x1000", help="DdxLEVELSxN,... (LEVELS per term, three terms: the matrix cores "
                    "at L = 256 and the per-wave form at L = 512)")
    ap.add_argument("--block-sides", default="block,pair", help="the sides of each row to run")
    ap.add_argument("--struct-cost", action="store_true", help="per row of --struct-rows the model of --slope-cost with its first term an AR(1) "
                    "sequence, a random walk, and unstructured (DESIGN section 23); use --lockstep, and --pairs '' to run nothing else")
    ap.add_argument("--struct-rows", default="20x100x1000,20x200x1000", help="DdxLEVELSxN,... (section 22's rows: the matrix cores and the per-wave form)")
    ap.add_argument("--struct-sides", default="ar1,rw1,plain", help="the sides of each row to run")
    ap.add_argument("--gmrf-cost", action="store_true", help="per row of --gmrf-rows the model of --slope-cost with an ICAR prior on its first "
                    "term, an RW2 prior, and the iid prior (DESIGN section 25); use --lockstep, and --pairs '' to run nothing else")
    ap.add_argument("--gmrf-rows", default="20x100x1000,20x200x1000", help="DdxLEVELSxN,... (section 23's rows: the matrix cores and the per-wave form)")
    ap.add_argument("--gmrf-sides", default="icar,rw2,plain", help="the sides of each row to run")
    ap.add_argument("--multi-cost", action="store_true", help="per row of --multi-rows one cubic smooth (DESIGN section 27) in three ways on the "
                    "same data: its basis as a term of width 4, as dense columns (glm.expand_factors), and the same columns in a term of width 1")
    ap.add_argument("--multi-rows", default="24x16384", help="BASISxN,...")
    ap.add_argument("--multi-sides", default="wide,expanded,width1", help="the sides of each row to run")
    ap.add_argument("--responses", default="", help="M,...: the Poisson regression with M responses of chains / M chains each on one design "
                    "(DESIGN section 15); 1 is the plain GLM")
    ap.add_argument("--chains-per-response", default="", help="R,...: the rows of --responses with M = chains / R")
    ap.add_argument("--repeats", type=int, default=1, help="engines per row of --responses (the run-to-run spread)")
    ap.add_argument("--adapt", default="", choices=["", "per-chain", "per-response"], help="the rows of --responses time one adapting tuning "
                    "stage with a metric window, stepsize and metric per chain or pooled per response (DESIGN section 16)")
    ap.add_argument("--stage-steps", type=int, default=25, help="transitions of the stage that --adapt times")
    ap.add_argument("--metric", default="shared", choices=["shared", "per_chain"])
    ap.add_argument("--lockstep", action="store_true", help="eps / 1000 and max_depth = 6: every tree of every density takes the same 63 "
                    "steps, so steps/s compares the cost per gradient and not the trees")
    a = ap.parse_args()
    global LOCKSTEP
    LOCKSTEP = a.lockstep
    if a.adapt == "per-response":
        import torch
        torch.zeros(1, device="cuda")      # (torch's device start-up before the first context: the hand-made launches are timed with its events)
    metric = pkg.METRIC_SHARED if a.metric == "shared" else pkg.METRIC_PER_CHAIN
    res = dict(device_peak_fp64_mfma_flops=PEAK_FP64_MFMA, transitions_per_launch=a.transitions, results=[])
    if a.factor_cost:
        sides = a.factor_sides.split(",")
        for spec in a.factor_rows.split(","):
            Dd, N, n = (int(v) for v in spec.split("x"))
            X, y, idx, kw, q0, cov = factor_problem(Dd, N, n, seed=Dd * 7919 + N * 31 + n)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="factor_cost", Dd=Dd, levels=N, n=n, Dx=Dd + N, L=padded(Dd + N + 1), chains=C, metric=a.metric, lockstep=LOCKSTEP)
                seen = {}
                for side in sides:
                    mdl = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=[(idx, N)], **kw) if side == "factor" else \
                        pkg.GLM(pkg.glm.expand_factors(X, [(idx, N)]), y, pkg.glm.POISSON_LOG, **kw)
                    runs = [run("glm_" + side, X, y, q0, cov, C, a.transitions, metric=metric, mdl=mdl) for _ in range(a.repeats)]
                    r = max((u[0] for u in runs), key=lambda u: u["leapfrog_steps_per_s"])
                    r["repeats_leapfrog_steps_per_s"] = [u[0]["leapfrog_steps_per_s"] for u in runs]
                    row[side] = r
                    seen[side] = runs[0][1] + (runs[0][2],)
                    print("# Dd=%d levels=%d n=%d C=%d %s (form %d): %.4e leapfrog steps/s (%s), %.3f ms/transition, create %.2f s" %
                          (Dd, N, n, C, side, r["glm_form"], r["leapfrog_steps_per_s"],
                           " ".join("%.4e" % v for v in r["repeats_leapfrog_steps_per_s"]), r["ms_per_transition"], r["create_s"]),
                          file=sys.stderr, flush=True)
                if len(sides) == 2:
                    fa, fb = sides
                    row["same_bits"] = bool(all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(seen[fa], seen[fb])))
                    row["same_steps"] = row[fa]["steps"] == row[fb]["steps"]
                    row["speedup_%s_over_%s" % (fa, fb)] = row[fa]["leapfrog_steps_per_s"] / row[fb]["leapfrog_steps_per_s"]
                res["results"].append(row)
    if a.slope_cost:
        sides = a.slope_sides.split(",")
        for spec in a.slope_rows.split(","):
            Dd, N, n = (int(v) for v in spec.split("x"))
            X, y, idx, x, kw, q0, cov = slope_problem(Dd, N, n, seed=Dd * 7919 + N * 31 + n)
            valued = [(idx, N), pkg.glm.term(idx, values=x, levels=N)]
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="slope_cost", Dd=Dd, levels=N, n=n, Dx=Dd + 2 * N, L=padded(Dd + 2 * N + 2), chains=C, metric=a.metric, lockstep=LOCKSTEP)
                seen = {}
                for side in sides:
                    mdl = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **kw) if side == "slopes" else \
                        pkg.GLM(pkg.glm.expand_factors(X, valued), y, pkg.glm.POISSON_LOG, **kw) if side == "expanded" else \
                        pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=[(idx, N), (idx, N)], **kw)
                    runs = [run("glm_" + side, X, y, q0, cov, C, a.transitions, metric=metric, mdl=mdl) for _ in range(a.repeats)]
                    r = max((u[0] for u in runs), key=lambda u: u["leapfrog_steps_per_s"])
                    r["repeats_leapfrog_steps_per_s"] = [u[0]["leapfrog_steps_per_s"] for u in runs]
                    row[side] = r
                    seen[side] = runs[0][1] + (runs[0][2],)
                    print("# Dd=%d levels=2x%d n=%d C=%d %s (form %d): %.4e leapfrog steps/s (%s), %.3f ms/transition, create %.2f s" %
                          (Dd, N, n, C, side, r["glm_form"], r["leapfrog_steps_per_s"],
                           " ".join("%.4e" % v for v in r["repeats_leapfrog_steps_per_s"]), r["ms_per_transition"], r["create_s"]),
                          file=sys.stderr, flush=True)
                if "slopes" in seen and "expanded" in seen:
                    row["same_bits"] = bool(all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(seen["slopes"], seen["expanded"])))
                    row["same_steps"] = row["slopes"]["steps"] == row["expanded"]["steps"]
                    row["speedup_slopes_over_expanded"] = row["slopes"]["leapfrog_steps_per_s"] / row["expanded"]["leapfrog_steps_per_s"]
                if "slopes" in seen and "plain" in seen:
                    row["plain_same_steps"] = row["slopes"]["steps"] == row["plain"]["steps"]
                    row["slopes_over_plain"] = row["slopes"]["leapfrog_steps_per_s"] / row["plain"]["leapfrog_steps_per_s"]
                res["results"].append(row)
    if a.corr_cost:
        sides = a.corr_sides.split(",")
        for spec in a.corr_rows.split(","):
            Dd, N, n = (int(v) for v in spec.split("x"))
            X, y, idx, x, kw, q0, cov = slope_problem(Dd, N, n, seed=Dd * 7919 + N * 31 + n)
            valued = [(idx, N), pkg.glm.term(idx, values=x, levels=N)]
            kwc = pkg.glm.correlated_effects(Dd, [N, N], [(0, 1)], eta=2.0)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="corr_cost", Dd=Dd, levels=N, n=n, Dx=Dd + 2 * N, L=padded(Dd + 2 * N + 3), chains=C, metric=a.metric, lockstep=LOCKSTEP)
                for side in sides:
                    if side == "corr":
                        mdl, qs = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **kwc), np.r_[q0, 0.3]
                    else:
                        mdl, qs = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **kw), q0
                    runs = [run("glm_" + side, X, y, qs, np.eye(qs.size) * 1e-4, C, a.transitions, metric=metric, mdl=mdl) for _ in range(a.repeats)]
                    r = max((u[0] for u in runs), key=lambda u: u["leapfrog_steps_per_s"])
                    r["repeats_leapfrog_steps_per_s"] = [u[0]["leapfrog_steps_per_s"] for u in runs]
                    row[side] = r
                    print("# Dd=%d levels=2x%d n=%d C=%d %s (form %d): %.4e leapfrog steps/s (%s), %.3f ms/transition, create %.2f s" %
                          (Dd, N, n, C, side, r["glm_form"], r["leapfrog_steps_per_s"],
                           " ".join("%.4e" % v for v in r["repeats_leapfrog_steps_per_s"]), r["ms_per_transition"], r["create_s"]),
                          file=sys.stderr, flush=True)
                if "corr" in row and "uncorr" in row:
                    row["same_steps"] = row["corr"]["steps"] == row["uncorr"]["steps"]
                    row["corr_over_uncorr"] = row["corr"]["leapfrog_steps_per_s"] / row["uncorr"]["leapfrog_steps_per_s"]
                res["results"].append(row)
    if a.block_cost:
        sides = a.block_sides.split(",")
        for spec in a.block_rows.split(","):
            Dd, N, n = (int(v) for v in spec.split("x"))
            X, y, idx, x, kw, q0, cov = slope_problem(Dd, N, n, seed=Dd * 7919 + N * 31 + n)
            x2 = 0.5 * np.random.default_rng(N + n).standard_normal(n)
            valued = [(idx, N), pkg.glm.term(idx, values=x, levels=N), pkg.glm.term(idx, values=x2, levels=N)]
            u2 = 0.1 * np.random.default_rng(N + n + 1).standard_normal(N)
            q3 = np.r_[q0[:Dd + 2 * N], u2, q0[Dd + 2 * N:], np.log(0.3)]                  # [beta | u0 u1 u2 | omega0 omega1 omega2]
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="block_cost", Dd=Dd, levels=N, n=n, Dx=Dd + 3 * N, L=padded(Dd + 3 * N + 6), chains=C, metric=a.metric, lockstep=LOCKSTEP)
                for side in sides:
                    if side == "block":
                        mdl, qs = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **pkg.glm.block_effects(Dd, [N, N, N], (0, 1, 2), eta=2.0)), np.r_[q3, 0.3, -0.2, 0.1]
                    else:
                        mdl, qs = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **pkg.glm.correlated_effects(Dd, [N, N, N], [(0, 1)], eta=2.0)), np.r_[q3, 0.3]
                    runs = [run("glm_" + side, X, y, qs, np.eye(qs.size) * 1e-4, C, a.transitions, metric=metric, mdl=mdl) for _ in range(a.repeats)]
                    r = max((u[0] for u in runs), key=lambda u: u["leapfrog_steps_per_s"])
                    r["repeats_leapfrog_steps_per_s"] = [u[0]["leapfrog_steps_per_s"] for u in runs]
                    row[side] = r
                    print("# Dd=%d levels=3x%d n=%d C=%d %s (form %d): %.4e leapfrog steps/s (%s), %.3f ms/transition, create %.2f s" %
                          (Dd, N, n, C, side, r["glm_form"], r["leapfrog_steps_per_s"],
                           " ".join("%.4e" % v for v in r["repeats_leapfrog_steps_per_s"]), r["ms_per_transition"], r["create_s"]),
                          file=sys.stderr, flush=True)
                if "block" in row and "pair" in row:
                    row["same_steps"] = row["block"]["steps"] == row["pair"]["steps"]
                    row["block_over_pair"] = row["block"]["leapfrog_steps_per_s"] / row["pair"]["leapfrog_steps_per_s"]
                res["results"].append(row)
    if a.struct_cost:
        sides = a.struct_sides.split(",")
        for spec in a.struct_rows.split(","):
            Dd, N, n = (int(v) for v in spec.split("x"))
            X, y, idx, x, kw, q0, cov = slope_problem(Dd, N, n, seed=Dd * 7919 + N * 31 + n)
            valued = [(idx, N), pkg.glm.term(idx, values=x, levels=N)]
            # (a walk's level k is the sum of k + 1 increments: the start's increments are scaled so that its levels stay the size of q0's)
            qw = q0.copy()
            qw[Dd + 1:Dd + N] = q0[Dd + 1:Dd + N] / np.sqrt(N)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="struct_cost", Dd=Dd, levels=N, n=n, Dx=Dd + 2 * N, L=padded(Dd + 2 * N + 3), chains=C, metric=a.metric, lockstep=LOCKSTEP)
                for side in sides:
                    if side == "ar1":
                        mdl, qs = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **pkg.glm.structured_effects(Dd, [N, N], [pkg.glm.ar1(0)])), np.r_[q0, 0.3]
                    elif side == "rw1":
                        mdl, qs = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **pkg.glm.structured_effects(Dd, [N, N], [pkg.glm.rw1(0)])), qw
                    else:
                        mdl, qs = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **kw), q0
                    runs = [run("glm_" + side, X, y, qs, np.eye(qs.size) * 1e-4, C, a.transitions, metric=metric, mdl=mdl) for _ in range(a.repeats)]
                    r = max((u[0] for u in runs), key=lambda u: u["leapfrog_steps_per_s"])
                    r["repeats_leapfrog_steps_per_s"] = [u[0]["leapfrog_steps_per_s"] for u in runs]
                    row[side] = r
                    print("# Dd=%d levels=2x%d n=%d C=%d %s (form %d): %.4e leapfrog steps/s (%s), %.3f ms/transition, create %.2f s" %
                          (Dd, N, n, C, side, r["glm_form"], r["leapfrog_steps_per_s"],
                           " ".join("%.4e" % v for v in r["repeats_leapfrog_steps_per_s"]), r["ms_per_transition"], r["create_s"]),
                          file=sys.stderr, flush=True)
                for side in ("ar1", "rw1"):
                    if side in row and "plain" in row:
                        row[side + "_same_steps"] = row[side]["steps"] == row["plain"]["steps"]
                        row[side + "_over_plain"] = row[side]["leapfrog_steps_per_s"] / row["plain"]["leapfrog_steps_per_s"]
                res["results"].append(row)
    if a.gmrf_cost:
        sides = a.gmrf_sides.split(",")
        for spec in a.gmrf_rows.split(","):
            Dd, N, n = (int(v) for v in spec.split("x"))
            X, y, idx, x, kw, q0, cov = slope_problem(Dd, N, n, seed=Dd * 7919 + N * 31 + n)
            valued = [(idx, N), pkg.glm.term(idx, values=x, levels=N)]
            cols = N // 10
            edges = [(r * cols + c, r * cols + c + 1) for r in range(10) for c in range(cols - 1)] + \
                    [(r * cols + c, (r + 1) * cols + c) for r in range(9) for c in range(cols)]
            prec = {"icar": (pkg.glm.scale_precision(pkg.glm.icar_precision(edges, N)), 1.0), "rw2": (pkg.glm.rw2_precision(N), 0.0)}
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="gmrf_cost", Dd=Dd, levels=N, n=n, Dx=Dd + 2 * N, L=padded(Dd + 2 * N + 2), chains=C, metric=a.metric, lockstep=LOCKSTEP)
                for side in sides:
                    if side in prec:
                        mdl = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **pkg.glm.gmrf_effects(Dd, [N, N], [pkg.glm.gmrf(0, *prec[side])]))
                        row[side + "_entries"] = int(mdl.gmrf_val.size)
                    else:
                        mdl = pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=valued, **kw)
                    runs = [run("glm_" + side, X, y, q0, np.eye(q0.size) * 1e-4, C, a.transitions, metric=metric, mdl=mdl) for _ in range(a.repeats)]
                    r = max((u[0] for u in runs), key=lambda u: u["leapfrog_steps_per_s"])
                    r["repeats_leapfrog_steps_per_s"] = [u[0]["leapfrog_steps_per_s"] for u in runs]
                    row[side] = r
                    print("# Dd=%d levels=2x%d n=%d C=%d %s (form %d): %.4e leapfrog steps/s (%s), %.3f ms/transition, create %.2f s" %
                          (Dd, N, n, C, side, r["glm_form"], r["leapfrog_steps_per_s"],
                           " ".join("%.4e" % v for v in r["repeats_leapfrog_steps_per_s"]), r["ms_per_transition"], r["create_s"]),
                          file=sys.stderr, flush=True)
                for side in ("icar", "rw2"):
                    if side in row and "plain" in row:
                        row[side + "_same_steps"] = row[side]["steps"] == row["plain"]["steps"]
                        row[side + "_over_plain"] = row[side]["leapfrog_steps_per_s"] / row["plain"]["leapfrog_steps_per_s"]
                res["results"].append(row)
    if a.multi_cost:
        # one cubic smooth of x, the iid prior and a sampled scale on its N coefficients (the penalty is the prior loop's business and
        # costs what --gmrf-cost shows): the basis as a term of width 4, as N dense columns, and -- the price of the three further
        # planes -- the same N columns in a term of width 1 that keeps the first plane alone
        sides = a.multi_sides.split(",")
        for spec in a.multi_rows.split(","):
            N, n = (int(v) for v in spec.split("x"))
            X, y, term, kw, q0 = smooth_problem(N, n, seed=N * 31 + n)
            one = pkg.glm.term(term.index[:, 0], values=term.weights[:, 0], levels=N)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="multi_cost", Dd=2, levels=N, n=n, Dx=2 + N, L=padded(2 + N + 1), chains=C, metric=a.metric, lockstep=LOCKSTEP)
                seen = {}
                for side in sides:
                    mdl = pkg.GLM(pkg.glm.expand_factors(X, [term]), y, pkg.glm.POISSON_LOG, **kw) if side == "expanded" else \
                        pkg.GLM(X, y, pkg.glm.POISSON_LOG, factors=[term if side == "wide" else one], **kw)
                    runs = [run("glm_" + side, X, y, q0, np.eye(q0.size) * 1e-4, C, a.transitions, metric=metric, mdl=mdl) for _ in range(a.repeats)]
                    r = max((u[0] for u in runs), key=lambda u: u["leapfrog_steps_per_s"])
                    r["repeats_leapfrog_steps_per_s"] = [u[0]["leapfrog_steps_per_s"] for u in runs]
                    row[side] = r
                    seen[side] = runs[0][1] + (runs[0][2],)
                    print("# smooth N=%d n=%d C=%d %s (form %d): %.4e leapfrog steps/s (%s), %.3f ms/transition, create %.2f s" %
                          (N, n, C, side, r["glm_form"], r["leapfrog_steps_per_s"],
                           " ".join("%.4e" % v for v in r["repeats_leapfrog_steps_per_s"]), r["ms_per_transition"], r["create_s"]),
                          file=sys.stderr, flush=True)
                if "wide" in row and "expanded" in row:
                    row["same_bits"] = bool(all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(seen["wide"], seen["expanded"])))
                    row["same_steps"] = row["wide"]["steps"] == row["expanded"]["steps"]
                    row["speedup_wide_over_expanded"] = row["wide"]["leapfrog_steps_per_s"] / row["expanded"]["leapfrog_steps_per_s"]
                if "wide" in row and "width1" in row:
                    row["wide_over_width1"] = row["wide"]["leapfrog_steps_per_s"] / row["width1"]["leapfrog_steps_per_s"]
                res["results"].append(row)
    for shape in a.shapes.split(","):
        D, n = (int(v) for v in shape.split("x"))
        L, npad = padded(D), (n + 127) // 128 * 128
        flops = 4 * npad * L
        if a.aux_cost:
            X, y, q_map, cov = gaussian_problem(n, D, seed=D * 7919 + n)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="aux_cost", D=D, n=n, chains=C, metric=a.metric)
                for f in ("glm_gaussian_fixed", "glm_gaussian", "glm_gaussian_a4"):
                    row[f] = run(f, X, y, q_map, cov, C, a.transitions, metric=metric)[0]
                    print("# D=%d n=%d C=%d %s (form %d): %.3e leapfrog steps/s, depth %.2f" %
                          (D, n, C, f, row[f]["glm_form"], row[f]["leapfrog_steps_per_s"], row[f]["mean_depth"]), file=sys.stderr, flush=True)
                res["results"].append(row)
        if a.hier_cost:
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="hier_cost", D=D, n=n, chains=C, metric=a.metric)
                for H in (0, 1, 4):
                    f = "glm_hier_h%d" % H
                    X, y, q_map, cov = hier_problem(n, D, seed=D * 7919 + n, H=H)
                    row[f] = run(f, X, y, q_map, cov, C, a.transitions, metric=metric)[0]
                    print("# D=%d n=%d C=%d %s (form %d): %.3e leapfrog steps/s, depth %.2f" %
                          (D, n, C, f, row[f]["glm_form"], row[f]["leapfrog_steps_per_s"], row[f]["mean_depth"]), file=sys.stderr, flush=True)
                res["results"].append(row)
        if a.dispersion_cost:
            X, y, q_nb, cov_nb = negbin_problem(n, D, seed=D * 7919 + n)
            q_po, cov_po = poisson_laplace(X, y)
            Xb, Yb, q_be, cov_be = beta_problem(n, D, seed=D * 7919 + n)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="dispersion_cost", D=D, n=n, chains=C, metric=a.metric)
                for f, args in (("glm_negbin", (X, y, q_nb, cov_nb)), ("glm_poisson", (X, y, q_po, cov_po)), ("glm_beta", (Xb, Yb, q_be, cov_be))):
                    row[f] = run(f, *args, C, a.transitions, metric=metric)[0]
                    print("# D=%d n=%d C=%d %s (form %d): %.3e leapfrog steps/s, depth %.2f" %
                          (D, n, C, f, row[f]["glm_form"], row[f]["leapfrog_steps_per_s"], row[f]["mean_depth"]), file=sys.stderr, flush=True)
                row["negbin_over_poisson"] = row["glm_negbin"]["leapfrog_steps_per_s"] / row["glm_poisson"]["leapfrog_steps_per_s"]
                res["results"].append(row)
        if a.prior_cost:
            po = poisson_problem(n, D, seed=D * 7919 + n)
            hi = hier_problem(n, D, seed=D * 7919 + n, H=4)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="prior_cost", D=D, n=n, chains=C, metric=a.metric, lockstep=LOCKSTEP)
                for f, args in (("glm_poisson", po), ("glm_poisson_t", po), ("glm_hier_h4", hi), ("glm_hier_h4_halft", hi)):
                    row[f] = run(f, *args, C, a.transitions, metric=metric)[0]
                    print("# D=%d n=%d C=%d %s (form %d): %.3f ms/transition, %.3e leapfrog steps/s, depth %.2f" %
                          (D, n, C, f, row[f]["glm_form"], row[f]["ms_per_transition"], row[f]["leapfrog_steps_per_s"], row[f]["mean_depth"]),
                          file=sys.stderr, flush=True)
                row["student_t_over_gaussian_ms"] = row["glm_poisson_t"]["ms_per_transition"] / row["glm_poisson"]["ms_per_transition"]
                row["half_t_over_gaussian_ms"] = row["glm_hier_h4_halft"]["ms_per_transition"] / row["glm_hier_h4"]["ms_per_transition"]
                res["results"].append(row)
        if a.local_cost:
            rows = a.local_rows.split(",")
            small = hier_problem(n, D, seed=D * 7919 + n, H=1)
            wide = hier_problem(n, 2 * D, seed=D * 7919 + n, H=1) if "iv" in rows else None
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="local_cost", D=D, n=n, chains=C, metric=a.metric, lockstep=LOCKSTEP)
                for tag, f, args in (("i", "glm_local_base", small), ("ii", "glm_local_all", small), ("iii", "glm_local_all_slab", small),
                                     ("iv", "glm_local_base", wide)):
                    if tag not in rows:
                        continue
                    r = run(f, *args, C, a.transitions, metric=metric)[0]
                    r["ms_per_gradient"] = r["ms_per_transition"] * a.transitions / r["steps"] * C
                    row[tag + "_" + f] = r
                    print("# D=%d n=%d C=%d %s %s (Dx = %d, form %d): %.3f ms/transition, %.5f ms/gradient sweep, %.3e leapfrog steps/s, depth %.2f" %
                          (D, n, C, tag, f, args[0].shape[1], r["glm_form"], r["ms_per_transition"], r["ms_per_gradient"], r["leapfrog_steps_per_s"],
                           r["mean_depth"]), file=sys.stderr, flush=True)
                res["results"].append(row)
        if a.responses or a.chains_per_response:
            X, y, q_map, cov = poisson_problem(n, D, seed=D * 7919 + n)
            for C in (int(c) for c in a.chains.split(",")):
                for M in [int(m) for m in a.responses.split(",") if m] + [C // int(r) for r in a.chains_per_response.split(",") if r]:
                    if M < 1 or C % M:
                        raise SystemExit("--responses: M = %d does not divide %d chains" % (M, C))
                    row = dict(pair="responses", D=D, n=n, chains=C, M=M, chains_per_response=C // M, metric=a.metric, runs=[])
                    for _ in range(a.repeats):
                        mdl = None if M == 1 else responses_model(X, y, q_map, M, C)
                        if a.adapt:
                            r = run_adapt(X, y, q_map, cov, C, a.stage_steps, a.adapt, mdl=mdl)
                            row["runs"].append(r)
                            print("# D=%d n=%d C=%d M=%d adapt %s: stage of %d transitions %.2f ms, %.3f ms/transition, %.4e leapfrog steps/s%s" %
                                  (D, n, C, M, a.adapt, a.stage_steps, r["stage_ms"], r["ms_per_transition"], r["leapfrog_steps_per_s"],
                                   "".join(", %s %.2f" % (k, v) for k, v in r.items() if k.startswith("eps_adapt") and k.endswith("transition"))),
                                  file=sys.stderr, flush=True)
                            continue
                        row["runs"].append(run("glm_poisson", X, y, q_map, cov, C, a.transitions, metric=metric, mdl=mdl)[0])
                        r = row["runs"][-1]
                        print("# D=%d n=%d C=%d M=%d (form %d): %.4e leapfrog steps/s, %.2f ms/transition, depth %.2f, create %.2f s" %
                              (D, n, C, M, r["glm_form"], r["leapfrog_steps_per_s"], r["ms_per_transition"], r["mean_depth"], r["create_s"]),
                              file=sys.stderr, flush=True)
                    res["results"].append(row)
        for pair in [p for p in a.pairs.split(",") if p]:
            fa, fb, prob = PAIRS[pair]
            X, y, q_map, cov = prob(n, D, seed=D * 7919 + n)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair=pair, D=D, n=n, L=L, n_pad=npad, chains=C, fp64_ops_per_gradient=flops)
                seen = {}
                for f in (fa, fb):
                    r, head, tail = run(f, X, y, q_map, cov, C, a.transitions, metric=metric)
                    r["fp64_tflops"] = r["leapfrog_steps_per_s"] * flops / 1e12
                    row[f] = r
                    seen[f] = head + (tail,)
                    print("# D=%d n=%d C=%d %s: %.3e leapfrog steps/s, %.2f ms/transition, depth %.2f, create %.2f s" %
                          (D, n, C, f, r["leapfrog_steps_per_s"], r["ms_per_transition"], r["mean_depth"], r["create_s"]),
                          file=sys.stderr, flush=True)
                row["same_bits"] = bool(all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(seen[fa], seen[fb])))
                row["same_steps"] = row[fa]["steps"] == row[fb]["steps"]
                row["speedup_%s_over_%s" % (fa, fb)] = row[fa]["leapfrog_steps_per_s"] / row[fb]["leapfrog_steps_per_s"]
                res["results"].append(row)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
