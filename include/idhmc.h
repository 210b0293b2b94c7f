/*
 * idhmc.h -- C ABI of the MI355X-native many-chain NUTS leapfrog/gradient engine.
 *
 * This is the drop-in boundary for the hot path of chriselrod/InplaceDHMC.jl
 * (src/kinetic_energy.jl, src/hamiltonian.jl, src/tree.jl, src/NUTS.jl,
 * src/stepsize.jl and the two caller loops of src/warmup.jl).  The reference is
 * pure Julia and has no FFI of its own; each entry point below names the
 * reference function (file:line under /root/reference) whose work it replaces
 * for ALL chains of a context at once.  A Julia host binds these with `ccall`
 * (INTEGRATION.md shows the stub); this repository's own hosts are the C++
 * drivers inside the library (idhmc_warmup / idhmc_mcmc) and the Python
 * ctypes mirror in inplacedhmc.jl_amd/.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++ or torch types cross this boundary.
 *  - every function returns an int status (IDHMC_OK = 0); idhmc_last_error()
 *    gives the text.  Numerical trouble (non-finite log density, divergence) is
 *    DATA, reported through idhmc_tree_stats.termination, never an error
 *    (reference convention: src/kinetic_energy.jl:80-84,107-112, src/NUTS.jl:179-180).
 *  - host arrays are chain-major and UNPADDED: element (c, d) of an nchains x D
 *    array is at [c*D + d].  The library owns all device memory.
 *  - one context per device; calls on a context are stream-ordered and not
 *    re-entrant; distinct contexts may be used from distinct host threads
 *    (reference threading model: one chain per thread, src/mcmc.jl:150-157).
 *  - RNG streams are keyed by (seed, GLOBAL chain id, transition number), and the one pooled statistic of the
 *    global-stepsize mode is exchanged as exact integers (see "the global-stepsize exchange"), so results do not
 *    depend on how chains are sharded over devices: bit-identical for 1, 2, 4, 8 ranks (the pooled metric too, for
 *    shards aligned to IDHMC_POOL_SEGMENT chains).
 *  - all arithmetic is IEEE fp64 (the reference is Float64-only,
 *    src/warmup.jl:108-120, src/mcmc.jl:118,143).
 */
#ifndef IDHMC_H
#define IDHMC_H
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define IDHMC_VERSION 4

enum {
    IDHMC_OK = 0,
    IDHMC_ERR_BAD_ARG = 1,        /* programmer error (reference: AssertionError / MethodError) */
    IDHMC_ERR_HIP = 2,            /* a HIP runtime call failed */
    IDHMC_ERR_EPS_UNDERFLOW = 3,  /* dual-averaging eps < 1e-10 (reference src/warmup.jl:291-296) */
    IDHMC_ERR_STEPSIZE_SEARCH = 4,/* bracketing/bisection ran out of iterations (src/stepsize.jl:71,101) */
    IDHMC_ERR_NONFINITE_START = 5,/* starting point has non-finite density (src/stepsize.jl:152-153) */
    IDHMC_ERR_NO_DEVICE = 6,
    IDHMC_ERR_ALLOC = 7,
    IDHMC_ERR_OPTIMIZATION = 8,   /* FindLocalOptimum: no finite optimum after 100 restarts (src/warmup.jl:172) */
    IDHMC_ERR_PEER = 9            /* sharded run: a chain of ANOTHER rank raised one of the errors above; this rank's chains are
                                     fine, but the stage fails on every rank together (the ranks have agreed on it through the
                                     exchange record's slot [3], so none is left waiting in a collective) */
};

/* ---- downward boundary: the user log density -----------------------------
 * Reference contract: logdensity_and_gradient!(grad, model, q, sptr) -> l(q)
 * (src/kinetic_energy.jl:73,89), dimension(model) (src/warmup.jl:102).
 * Built-in device densities needed by BASELINE.json's configs, and the plug-in form:
 *
 * IDHMC_MODEL_CUSTOM -- the user's density as HIP device source, compiled at idhmc_create with hipRTC
 * against the engine's kernel templates (the device counterpart of handing the reference an
 * AbstractProbabilityModel).  `source` must define, at namespace scope,
 *
 *   template <int NCH>
 *   __device__ double logdensity_and_gradient(const Vec<NCH> &q, Vec<NCH> &grad, const UserCtx &ctx);
 *
 * called by the 64 lanes of the chain's wavefront.  Lane l holds elements {128 j + 2 l, 128 j + 2 l + 1},
 * j < NCH, of every vector (q.c[j].x, q.c[j].y); elements >= ctx.D are padding: they arrive as 0 and their
 * gradient must be returned as 0.  It returns l(q) (the same value in every lane) and fills grad l(q);
 * a non-finite return value is treated as -Inf (src/kinetic_energy.jl:80-84).  ctx gives `params`
 * (the `params` array below, in device memory), `nparams`, `D`, `lane`, and `lds` -- one L-double
 * scratch vector in LDS private to the wavefront.  Everything in inplacedhmc.jl_amd/csrc/idhmc_math.hpp
 * and idhmc_device.hpp is in scope (wave_sum, dfma, dlog, dexp, dlog1p, dlgamma_psi, dlgamma, ddigamma, ...).
 * Compile errors are returned through idhmc_last_error().
 *
 * IDHMC_MODEL_LOGISTIC_REGRESSION -- Bayesian logistic regression with a Gaussian prior, the data shared by every chain:
 *   l(q) = sum_i [y_i z_i - softplus(z_i)] - 1/2 sum_c tau_c (q_c - mu_c)^2,   z = X q
 *   grad l(q) = X' (y - sigma(z)) - tau .* (q - mu)
 * `params` is [X row-major n x D | y (n)], so nparams = n (D + 1): n is nparams / (D + 1), and an nparams that is not a
 * positive multiple of D + 1 is refused.  Each y_i is 0 or 1, each X entry finite.  `mu` and `tau` are the prior's mean and
 * precision, each optional (NULL: 0 and 1); every tau_c must be finite and > 0, every mu_c finite.  1 <= D <= 1024, D > 512 needs
 * a SHARED or POOLED metric; the padded length L is a power of two (128 .. 1024) and n rounded up to a multiple of 128, n_pad,
 * satisfies n_pad L <= 2^27 (X and its transpose, kept on the device, take at most 1 GiB each).  The NUTS transition runs both
 * products on the fp64 matrix cores, 16 chains per workgroup, at L <= 256 (D <= 256); everything else one chain per wavefront.
 *
 * IDHMC_MODEL_GLM -- a generalised linear model with the user's likelihood, the same data layout, prior, limits and kernels as
 * LOGISTIC_REGRESSION (whose observation is replaced by the user's):
 *   l(q) = sum_i log p(y_i | z_i) - 1/2 sum_c tau_c (q_c - mu_c)^2,   z = X q
 * `source` defines, at namespace scope, one function per observation, compiled at idhmc_create with hipRTC:
 *
 *   __device__ void glm_observation(double z, const GlmObs &o, double &r, double &v);
 *
 * o.y[k], k < o.K: this observation's data columns (1 <= K <= 4); o.c[j], j < o.nc: the model's constants (device memory).
 * It returns v = -log p(y | z) (up to a term that depends on the data only) and r = d log p(y | z) / dz.  It is called for
 * padded observations too (z = 0, y = 0), whose results are then discarded.  The helpers of idhmc_math.hpp are in scope (dexp,
 * dlog, dlog1p, dfma, ...; dlgamma_psi(x, lg, psi) gives ln Gamma(x) and its derivative psi(x) for x > 0 from one call, dlgamma(x)
 * and ddigamma(x) one of the two: +inf and NaN for x <= 0, so a dispersion that underflows is a rejected point); the build uses
 * -ffp-contract=off, so only explicit dfma calls fuse.  Compile errors are returned through idhmc_last_error().  `params` is [K, nc, c (nc) | X row-major (n x D) | Y row-major (n x K)], so
 * n = (nparams - 2 - nc) / (D + K).  Refused with IDHMC_ERR_BAD_ARG before the device is touched: K not an integer in 1..4,
 * nc not an integer in 0..16, a remainder that is not a positive multiple of D + K, a non-finite value in X, Y or c, a missing
 * or empty source, and whatever LOGISTIC_REGRESSION refuses of the prior, D and n_pad L.
 *
 * IDHMC_MODEL_GLM_AUX -- a GLM whose likelihood has A sampled auxiliary parameters (1 <= A <= 4: a scale, a shape, a dispersion)
 * that every observation sees.  A chain's position is q = [beta (Dx coefficients) | a (A)], D = Dx + A, all unconstrained: the
 * observation applies its own transform (sigma = exp(a[0]), say) and includes the a-dependent normalising terms in v.
 *   l(q) = -sum_i v(z_i, y_i, a) - 1/2 sum_{c < D} tau_c (q_c - mu_c)^2,   z = X beta   (X is n x Dx)
 *   dl/dbeta_c = sum_i X[i][c] r_i - tau_c (beta_c - mu_c),   dl/da_j = sum_i s_ij - tau_{Dx+j} (a_j - mu_{Dx+j})
 *
 *   __device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s);
 *
 * a[j], s[j] for j < o.A; r = d log p(y | z, a) / dz, s[j] = d log p(y | z, a) / da_j, v = -log p(y | z, a) up to a term that
 * depends on the data only; o.y, o.c, o.K, o.nc as for GLM.  The Gaussian prior (mu, tau, length D) covers the auxiliary
 * coordinates.  `params` is [K, nc, A, c (nc) | X row-major (n x Dx) | Y row-major (n x K)] and idhmc_model_desc.D = Dx + A, so
 * n = (nparams - 3 - nc) / (Dx + K).  Refused with IDHMC_ERR_BAD_ARG before the device is touched: A not an integer in 1..4,
 * Dx = D - A < 1, and everything GLM refuses (with Dx in the place of D for X; the limits on D are on the total).  The same
 * kernels as GLM; the NUTS transition uses the matrix cores where the A further tiles fit a CU's LDS (L = 128: every A; L = 256: A = 1, or
 * A = 2 with a SHARED or POOLED metric), one chain per wavefront elsewhere:
 * idhmc_glm_form tells which.
 *
 * Coefficient groups with a sampled scale (idhmc_create_glm, below) -- a hierarchical GLM: H groups (1 <= H <= 4) of columns of X,
 * each with a standard deviation that is itself sampled, in the non-centred parameterisation.  A chain's position is
 * q = [u (Dx) | a (A) | omega (H)], D = Dx + A + H, all unconstrained; groups[c] in {-1, 0 .. H-1} for every column c (-1: in no group):
 *   b_c = groups[c] >= 0 ? exp(omega_groups[c]) u_c : u_c,   z = X b
 *   l(q) = -sum_i v(z_i, y_i, a) - 1/2 sum_{c < D} tau_c (q_c - mu_c)^2
 * The Gaussian prior is on the sampled coordinates: with the defaults (mu = 0, tau = 1) a grouped coefficient is
 * b_c ~ N(0, sigma_g^2), sigma_g = exp(omega_g) log-normal.  glm_observation is the one of GLM (A = 0) or GLM_AUX (A > 0),
 * untouched.  The hierarchy adds no tile: idhmc_glm_form is what it is for the same (L, A, metric) without groups.  Draws come back
 * in the sampled coordinates (u, a, omega).
 *
 * Several responses on one design matrix (idhmc_create_glm_responses, below) -- one context samples M posteriors that share X, the
 * prior, the constants, the source and the groups and differ in Y alone: a regression per gene, per voxel, per metric.  Y is
 * M x n x K row-major and the chain of GLOBAL id g (first_chain_id + c) samples response g / chains_per_response -- a function of the
 * global id only, like the address of its random numbers, so the shards of a run and one context holding all of it compute the same
 * bits.  For one chain every operation is the one a single-response context with Y[g / chains_per_response] performs: the draws are
 * bit-identical to that context's.  The matrix-core form takes 16 chains of any responses per tile and needs no further LDS:
 * idhmc_glm_form is what it is for the same (L, A, metric) with one response.  Stepsize and metric are per chain (or the fixed
 * SHARED metric) or pooled over the chains_per_response chains of each response (IDHMC_EPS_PER_RESPONSE,
 * IDHMC_METRIC_PER_RESPONSE, below); the statistics pooled over every chain of the context (IDHMC_EPS_GLOBAL, IDHMC_METRIC_POOLED)
 * would mix posteriors and are refused with M > 1.  The diagnostics counters stay context-wide. */
enum {
    IDHMC_MODEL_ISO_GAUSSIAN = 0,   /* l(q) = -1/2 |q|^2                       */
    IDHMC_MODEL_DIAG_GAUSSIAN = 1,  /* l(q) = -1/2 sum tau_d (q_d - mu_d)^2    */
    IDHMC_MODEL_DENSE_MVN = 2,      /* l(q) = -1/2 (q-mu)' P (q-mu), P = Sigma^-1 (fp64 MFMA) */
    IDHMC_MODEL_CUSTOM = 3,         /* user HIP source, see above */
    IDHMC_MODEL_LOGISTIC_REGRESSION = 4,  /* Bayesian logistic regression, see above (fp64 MFMA) */
    IDHMC_MODEL_GLM = 5,                  /* a GLM with the user's observation source, see above (fp64 MFMA) */
    IDHMC_MODEL_GLM_AUX = 6               /* a GLM whose likelihood has sampled auxiliary parameters (scale, shape), see above */
};
typedef struct {
    int32_t kind;
    int32_t D;              /* dimension(model): 1 <= D <= 1024; ISO and DIAG up to 2048 in every metric mode, CUSTOM up to
                               2048 with a SHARED or POOLED metric */
    const double *mu;       /* host, D  (DIAG, DENSE; LOGISTIC_REGRESSION, GLM: prior mean, may be NULL) */
    const double *tau;      /* host, D  (DIAG; LOGISTIC_REGRESSION, GLM: prior precision, may be NULL) */
    const double *prec;     /* host, D*D row-major, symmetric (DENSE) */
    const char *source;     /* CUSTOM, GLM, GLM_AUX: NUL-terminated HIP device source */
    const double *params;   /* CUSTOM: host, nparams doubles copied to the device (may be NULL); LOGISTIC_REGRESSION: [X | y];
                               GLM: [K, nc, c | X | Y]; GLM_AUX: [K, nc, A, c | X | Y] */
    int64_t nparams;
} idhmc_model_desc;

/* ---- options: the reference's keyword structs, flattened ------------------
 * NUTS(max_depth, min_D)            src/NUTS.jl:214-219
 * DualAveraging(d, g, k, t0)        src/stepsize.jl:191-193
 * InitialStepsizeSearch(...)        src/stepsize.jl:29-37
 * default_warmup_stages(...)        src/warmup.jl:361-372                    */
enum { IDHMC_EPS_PER_CHAIN = 0, IDHMC_EPS_GLOBAL = 1, IDHMC_EPS_PER_RESPONSE = 2 };
enum { IDHMC_METRIC_PER_CHAIN = 0, IDHMC_METRIC_SHARED = 1, IDHMC_METRIC_POOLED = 2, IDHMC_METRIC_PER_RESPONSE = 3 };
typedef struct {
    int32_t max_depth;               /* 10 */
    double  min_delta;               /* -1000.0 */
    double  da_delta, da_gamma, da_kappa; /* 0.8, 0.05, 0.75 */
    int32_t da_t0;                   /* 10 */
    double  ss_a_min, ss_a_max, ss_eps0, ss_C; /* 0.25, 0.75, 1.0, 2.0 */
    int32_t ss_maxiter_crossing, ss_maxiter_bisect; /* 400, 400 */
    int32_t init_steps, middle_steps, doubling_stages, terminating_steps; /* 75, 25, 5, 50 */
    int32_t adapt_metric;            /* 1: TuningNUTS{Diagonal} in the doubling stages; 0: TuningNUTS{Nothing} */
    int32_t stepsize_search;         /* 1: InitialStepsizeSearch stage; 0: start from eps_init */
    double  eps_init;                /* initialization = (eps = ...), src/warmup.jl:87-92 */
    int32_t eps_mode;                /* IDHMC_EPS_PER_CHAIN = reference semantics (src/warmup.jl:284-303);
                                        IDHMC_EPS_GLOBAL = one dual-averaging state fed by the mean
                                        acceptance of all chains of all ranks (the RCCL all-reduce hook);
                                        IDHMC_EPS_PER_RESPONSE (idhmc_create_glm_responses only) = one dual-averaging state per
                                        response, fed by the mean acceptance of that response's chains_per_response chains: for
                                        every response the bits of a single-response context in IDHMC_EPS_GLOBAL on the same
                                        chains.  A context in this mode holds whole responses, so nothing is exchanged */
    int32_t metric_mode;             /* IDHMC_METRIC_PER_CHAIN = reference semantics (src/warmup.jl:309);
                                        IDHMC_METRIC_SHARED = one fixed M^-1 for all chains, never adapted;
                                        IDHMC_METRIC_POOLED = one M^-1 for all chains, adapted from the pooled windows of
                                        every chain (of every rank, through the idhmc_comm_* communicator: 2 all-reduces
                                        of D + 1 doubles per window) -- an addition for the many-chain regime, like the
                                        global stepsize; not reference semantics.  Rank-count-invariant like the stepsize:
                                        partial sums are formed per segment of IDHMC_POOL_SEGMENT GLOBAL chain ids and
                                        added in segment order on every rank (see idhmc_pool_partials);
                                        IDHMC_METRIC_PER_RESPONSE (idhmc_create_glm_responses only) = one M^-1 per response,
                                        adapted from the pooled windows of its chains with IDHMC_METRIC_POOLED's sums (the
                                        same segments of global chain ids, the same order), stored in the per-chain layout:
                                        D <= 512, whole responses per context, the bits of a single-response POOLED context */
    int32_t local_opt_iterations;    /* FindLocalOptimum stage of idhmc_mcmc_with_warmup (src/warmup.jl:137-150,
                                        362): 0 = skipped (default at this level), reference default 50 */
    int32_t leapfrog_grad_mode;      /* IDHMC_GRAD_RECOMPUTE (what idhmc_default_options sets): in idhmc_leapfrog(eps, 1) a
                                        separable density re-derives grad l(q) from q and does not write grad l(q') -- 4 D 8
                                        bytes per chain-step; idhmc_get_grad and every call that needs the array re-evaluate
                                        it first, results are bit-identical.  Every other density and n_steps > 1 ignore it;
                                        IDHMC_GRAD_STORE (= 0, what a zero-initialised struct holds): the sweep streams q, p,
                                        grad l in and out (6 D 8 bytes per chain-step, the reference's data movement) */
    double  local_opt_penalty;       /* magnitude_penalty, reference default 1e-4 */
} idhmc_options;

/* reference TreeStatisticsNUTS, src/NUTS.jl:229-242: exactly 32 bytes */
typedef struct {
    double  pi;                 /* logdensity(H, zeta) */
    double  acceptance_rate;
    int32_t term_left, term_right; /* InvalidTree (src/tree.jl:278-300): left==right divergence,
                                      (1,0) REACHED_MAX_DEPTH, otherwise turning */
    int32_t depth;
    int32_t steps;              /* leapfrog steps evaluated */
} idhmc_tree_stats;

enum { IDHMC_GRAD_STORE = 0, IDHMC_GRAD_RECOMPUTE = 1 };

typedef struct idhmc_ctx idhmc_ctx;

void idhmc_default_options(idhmc_options *opt);
const char *idhmc_last_error(void);
int idhmc_version(void);
/* 16 hex digits: SHA-256 prefix of the sources this library was built from (csrc/Makefile, `make print-digest` prints the tree's);
 * a build check compares the two, so a stale libidhmc.so next to edited sources does not pass for the current one */
const char *idhmc_build_digest(void);

/* Create the engine for `nchains` chains on HIP device `device`.  Chain c of
 * this context has global id first_chain_id + c.  Replaces the per-thread set-up
 * of threaded_mcmc / initialize_warmup_state (src/mcmc.jl:130-157,
 * src/warmup.jl:100-129): kappa = I, Tree arena, state vectors. */
int idhmc_create(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                 const idhmc_model_desc *model, const idhmc_options *opt, uint64_t seed);
/* A GLM handed over in parts is created by ONE function, idhmc_create_glm_model (declared behind the parts, below): zero-initialise an
 * idhmc_glm_model, set glm and the parts the model has, and leave the rest NULL; a later version appends its parts at the struct's end.
 * It behaves as idhmc_create_glm_multi does with the same parts.  (M, chains_per_response) = (1, 0), or the (0, 0) of a zeroed struct, is
 * one response, the context of idhmc_create_glm; anything else is the context of idhmc_create_glm_responses, with its refusals.  The
 * eleven functions idhmc_create_glm .. idhmc_create_glm_multi that follow, one per part in the order the parts were added, are it with
 * the later parts NULL: they stay, with their signatures and messages, and the text of each states what its part means and refuses. */
/* A GLM from an explicit descriptor: IDHMC_MODEL_GLM (A = 0) or IDHMC_MODEL_GLM_AUX (A > 0), optionally with H coefficient groups
 * (above).  X is n x Dx and Y n x K row-major, constants has nc entries (may be NULL when nc = 0), groups has Dx entries (NULL iff
 * H = 0), mu / tau have Dx + A + H entries or are NULL (0 and 1).  With H = 0 the context is the one idhmc_create makes of kinds 5
 * and 6 for the same data.  Refused with IDHMC_ERR_BAD_ARG before the device is touched: everything those kinds refuse, and H
 * outside 0..4, groups NULL with H > 0 (or given with H = 0), an id outside -1..H-1, a group that no column uses, Dx < 1. */
typedef struct {
    int64_t n;
    int32_t Dx, K, nc, A, H;
    const double *X, *Y, *constants;
    const int32_t *groups;
    const double *mu, *tau;
    const char *source;
} idhmc_glm_desc;
int idhmc_create_glm(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                     const idhmc_glm_desc *glm, const idhmc_options *opt, uint64_t seed);
/* The same GLM with M responses (above): glm->Y is M x n x K row-major, everything else in *glm is as for idhmc_create_glm, and the
 * chain of global id g samples response g / chains_per_response.  With M = 1 the context is bit for bit the one idhmc_create_glm
 * makes.  Refused with IDHMC_ERR_BAD_ARG before the device is touched: everything idhmc_create_glm refuses (a non-finite value in any
 * of the M planes of Y), M < 1, chains_per_response < 1, first_chain_id + nchains > M * chains_per_response (a chain without a
 * response), M * K * n_pad > 2^27 (Y on the device takes at most 1 GiB, as X does), M > 1 together with IDHMC_EPS_GLOBAL or
 * IDHMC_METRIC_POOLED, and, in IDHMC_EPS_PER_RESPONSE or IDHMC_METRIC_PER_RESPONSE, a first_chain_id or an nchains that is not a
 * multiple of chains_per_response (a context in these modes holds whole responses; every other mode takes any shard) and, for the
 * metric, D > 512.  Every other creation function refuses the two modes. */
int idhmc_create_glm_responses(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                               const idhmc_glm_desc *glm, int64_t M, int64_t chains_per_response,
                               const idhmc_options *opt, uint64_t seed);
/* M and chains_per_response of a context made by idhmc_create_glm_responses; 1 and 0 for every other context */
int idhmc_glm_responses(const idhmc_ctx *ctx, int64_t *M, int64_t *chains_per_response);
/* Priors beyond the Gaussian.  Each sampled coordinate c < D = Dx + A + H carries mu_c and tau_c (idhmc_glm_desc) and
 * here a kind_c and a nu_c.  With d = q_c - mu_c, T the partial that accumulates -2 log prior (up to a constant) and G_c the
 * likelihood's part of the gradient -- the kernels and the tests' C restatement follow this bit for bit: plain operations in the
 * association written, dfma, dexp and dlog1p those of idhmc_math.hpp --
 *
 *   kind                    meaning                                      contribution to T                         g_c
 *   0 NORMAL                q_c ~ N(mu, 1 / tau)                         T = dfma(tau d, d, T)                     dfma(-tau, d, G_c)
 *   1 STUDENT_T             q_c = mu + t_nu / sqrt(tau)                  a = tau d; s = a d;
 *                                                                        T = T + (nu + 1) dlog1p(s / nu)           G_c + (-((nu + 1) a) / (nu + s))
 *   2 LOG_HALF_NORMAL       exp(q_c) half-normal, scale exp(mu)          e = dexp(2 d);  T = T + (e - 2 d)         G_c + (1 - e)
 *   3 LOG_HALF_STUDENT_T    exp(q_c) half-t_nu, scale exp(mu)            e = dexp(2 d);
 *                           (half-Cauchy: nu = 1)                        T = T + ((nu + 1) dlog1p(e / nu) - 2 d)   G_c + (1 - ((nu + 1) e) / (nu + e))
 *   4 LOG_EXPONENTIAL       exp(q_c) exponential, mean exp(mu)           e = dexp(d);  T = T + 2 (e - d)           G_c + (1 - e)
 *
 * Everything behind T is unchanged: l(q) = -sum_i v_i - T_total / 2.  The log kinds are priors on sigma = exp(q_c) -- a group's
 * standard deviation exp(omega_g), a dispersion exp(a_j) -- and include the Jacobian of exp: the coordinate stays unconstrained.
 * Each kind is finite wherever its log density is, and that ends at: kind 1, tau d^2 finite (|d| < 1.3e154 / sqrt(tau)); kinds 2 and 3,
 * 2 d < 709.78 (dexp finite; every more negative d is fine: e = 0, T = -2 d); kind 4, d < 709.08 (2 exp(d) finite).  Past those ends T is +inf, which
 * the engine reads as l(q) = -inf: the ordinary rejected point.
 *
 * idhmc_create_glm_priors makes the context of idhmc_create_glm (M = 1, chains_per_response = 0) or of idhmc_create_glm_responses
 * (anything else) with these priors; kind and nu have Dx + A + H entries each, nu may be NULL if no kind takes one.  priors == NULL,
 * priors->kind == NULL or every kind 0 gives the existing context: the same kernels, the same bits.  Otherwise the GLM's kernels are
 * compiled with the table above in their last loop (no LDS is added: idhmc_glm_form is what it is for the same (L, A, metric) with
 * Gaussian priors).  Refused with IDHMC_ERR_BAD_ARG before the device is touched: a kind outside 0..4; nu not finite or <= 0 for
 * kinds 1 and 3 (or nu NULL with such a kind); nu != 0 for kinds 0, 2 and 4; tau != 1 for kinds 2..4 (their one scale is exp(mu));
 * kinds 2..4 on a coordinate c < Dx (a coefficient is not a logarithm); and everything the other two functions refuse. */
enum { IDHMC_PRIOR_NORMAL = 0, IDHMC_PRIOR_STUDENT_T = 1, IDHMC_PRIOR_LOG_HALF_NORMAL = 2, IDHMC_PRIOR_LOG_HALF_STUDENT_T = 3,
       IDHMC_PRIOR_LOG_EXPONENTIAL = 4 };
typedef struct { const int32_t *kind; const double *nu; } idhmc_glm_priors;   /* Dx + A + H entries each; nu may be NULL if no kind takes one */
int idhmc_create_glm_priors(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                            const idhmc_glm_desc *glm, const idhmc_glm_priors *priors,
                            int64_t M, int64_t chains_per_response, const idhmc_options *opt, uint64_t seed);
/* kind and nu as the context was given them, D entries each; all 0 for every other context */
int idhmc_glm_priors_get(const idhmc_ctx *ctx, int32_t *kind, double *nu);
/* Per-coefficient local scales: the horseshoe and its regularised form.  local[c] in {0, 1} per column of X; the J
 * flagged columns, in ascending column order, get local coordinates k = 0 .. J-1, and a chain's position is
 *   q = [u (Dx) | a (A) | omega (H) | lambda (J)],   D = Dx + A + H + J <= 1024,
 * lambda_k the LOGARITHM of the local scale of its column col(k).  slab_scale S > 0 is fixed, not sampled, inv2 = 1.0 / (S * S) computed
 * once on the host; S = 0: no slab.  Per gradient -- the kernels and the tests' C restatement follow this bit for bit: plain IEEE
 * operations in the association written, dfma and dexp those of idhmc_math.hpp, sqrt correctly rounded -- e_g = dexp(omega_g), and for a
 * column c < Dx with id = groups[c]:
 *   not flagged: b_c = id >= 0 ? u_c * e_id : u_c, as without local scales
 *   flagged, local coordinate k:
 *     f = dexp(lambda_k);  s = id >= 0 ? e_id * f : f
 *     without slab: st = s (h unused)
 *     with slab:    i = 1.0 / s;  nn = dfma(i, i, inv2);  st = 1.0 / sqrt(nn);  h = 1.0 - inv2 / nn
 *                   (st = s / sqrt(1 + s^2 / S^2), h = d log st / d log s; s = inf gives st = S, h = 0; s = 0 gives st = 0, h = 1)
 *     b_c = u_c * st
 * z_i, (r_i, v_i, s_ij), G_c, S_j and A[rho] are as without local scales, over the columns < Dx.  Then, for a flagged column,
 *   w_c = G_c * b_c;  wl_c = slab ? w_c * h : w_c;  G_{Dx+A+H+k} = wl_c (no reduction: one column feeds one coordinate);
 *   W_id[c & 127] takes wl_c where it took w_c (grouped);  G_c <- G_c * st (an unflagged grouped column: G_c * e_id)
 * W_g goes into G_{Dx+A+g} by the canonical tree and the prior runs over all D coordinates, unchanged: the lambdas are coordinates >= Dx, so
 * kinds 2..4 apply to them.  The horseshoe: u ~ N(0, 1), IDHMC_PRIOR_LOG_HALF_STUDENT_T with nu = 1 on every lambda, the same kind with
 * mu = log tau0 on the omega of the group that holds the shrunk columns, and optionally S.
 * Finite: with a slab at every finite q; without one s = inf (omega_g + lambda_k past 709.78) makes b_c infinite or NaN, l is not
 * finite and reads as -inf, the ordinary rejected point.  With a slab and s below about 1.5e-154, i * i overflows and st is 0 where it
 * should be s: an absolute error below 1.5e-154 |u_c| in b_c, not engineered around.
 *
 * idhmc_create_glm_local is idhmc_create_glm_priors with these; mu, tau, kind and nu have Dx + A + H + J entries.  local == NULL,
 * local->local == NULL or all zeros, with slab_scale == 0, gives the context of idhmc_create_glm_priors: the same kernels, the same bits.
 * No LDS is added: idhmc_glm_form is what it is for the same (L, A, metric), L counting the J lambdas.  Refused with
 * IDHMC_ERR_BAD_ARG before the device is touched: an entry of local other than 0 or 1; slab_scale negative or not finite; slab_scale > 0
 * with J = 0; D > 1024; and everything the other creation functions refuse (IDHMC_METRIC_PER_RESPONSE still needs D <= 512). */
typedef struct { const int32_t *local; double slab_scale; } idhmc_glm_local;   /* local: Dx entries, 0 or 1 */
int idhmc_create_glm_local(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                           const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                           int64_t M, int64_t chains_per_response, const idhmc_options *opt, uint64_t seed);
/* local (Dx entries) and slab_scale as the context was given them; zeros and 0 for every other context */
int idhmc_glm_local_get(const idhmc_ctx *ctx, int32_t *local, double *slab_scale);
/* Factor terms by level index instead of indicator columns: a random intercept per subject, site or item,
 * (1 | subject), without a dense column of X per level.  F factors, 0 <= F <= 4; factor f has N_f >= 1 levels and an index
 * lvl_f[i] in 0 .. N_f-1 per observation.  With Dd >= 1 dense columns, the columns of the model are
 *   c < Dd: dense, X[i][c] stored      off_f = Dd + N_0 + .. + N_{f-1}      c = off_f + k: level k of factor f, not stored
 *   Dx = Dd + sum N_f,   q = [u (Dx) | a (A) | omega (H) | lambda (J)],   D = Dx + A + H + J <= 1024   (unchanged)
 * b_c is as today for every c < Dx (group scale, local scale).  The arithmetic -- the kernels follow this bit for bit --
 *   z_i  = the dfma chain over c < Dd ascending of X[i][c] * b_c from +0,  then  z_i = z_i + b[off_f + lvl_f[i]]  for f = 0 .. F-1
 *          ascending (plain additions)
 *   (r_i, v_i, s_ij) as today; observations i >= n overwritten with 0 as today (the padding carries lvl = -1 and adds nothing to z)
 *   G_c, c < Dd: as today.   G_{off_f + k} = plain additions, from +0, of r_i over the observations i < n with lvl_f[i] = k, i ascending
 * and everything after G is untouched: auxiliary scores, group chain rule, local scales, prior loop, T, A[rho], P, l.
 * For finite b and r this is bit for bit the arithmetic of the same model with its factors written out as indicator columns of X
 * (n x Dx, column off_f + k holding 1.0 where lvl_f[i] = k and 0.0 elsewhere): adding +-0 changes nothing, because a chain from +0
 * never holds -0, and fma(1, x, y) is y + x rounded once.  The equivalence ends at the non-finite: a non-finite b of one level poisons
 * every z of the expanded model (0 * inf) and here only that level's observations; both are rejected points.  A level with no
 * observation is allowed: its G is +0 and the prior alone moves it.
 *
 * idhmc_create_glm_factors is idhmc_create_glm_local with these: glm->Dx counts dense and level columns (Dd = Dx - sum N_f), glm->X is
 * n x Dd, and groups, local, mu, tau, kind and nu have the lengths they have today.  factors == NULL or F == 0 gives the context of
 * idhmc_create_glm_local: the same kernels, the same bits.  On the device X is stored Lx = 128 ceil(Dd / 128) wide, not L, and the
 * limit on the observations is n_pad * Lx <= 2^27.  No LDS is added: idhmc_glm_form is what it is for the same (L, A, metric).
 * Refused with IDHMC_ERR_BAD_ARG before the device is touched: F outside 0..4; levels or index NULL with F > 0; N_f < 1; an index
 * outside 0 .. N_f-1; Dd < 1; and everything the other creation functions refuse. */
typedef struct { int32_t F; const int32_t *levels; const int32_t *index; } idhmc_glm_factors;   /* levels: F entries; index: F x n, row-major */
int idhmc_create_glm_factors(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                             const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                             const idhmc_glm_factors *factors, int64_t M, int64_t chains_per_response,
                             const idhmc_options *opt, uint64_t seed);
/* F, the levels (F entries; room for 4) and the indices (F x n, row-major) as the context was given them; F = 0 for every other
 * context.  levels and index may be NULL (F alone is wanted) */
int idhmc_glm_factors_get(const idhmc_ctx *ctx, int32_t *F, int32_t *levels, int32_t *index);
/* Random slopes: factor terms that carry a value per observation, (1 + x | subject).  A term f may carry w_f[i], a
 * finite double per observation, next to its level index.  Its columns are still off_f .. off_f + N_f - 1 of the model and are never
 * stored; coordinates, F <= 4, D <= 1024 and Dd >= 1 do not change.  Two terms may share one index array: (1 | s) and (x | s) are two
 * terms of N columns each.  The arithmetic -- the kernels follow this bit for bit --
 *   z_i = the dfma chain over c < Dd (as above), then for f = 0 .. F-1 ascending:
 *           term without values:  z_i = z_i + b[off_f + lvl_f[i]]                 (as above)
 *           term with values:     z_i = dfma(w_f[i], b[off_f + lvl_f[i]], z_i)
 *   G_{off_f + k}, term with values = the dfma chain from +0 of dfma(w_f[i], r_i, G) over the observations i < n with lvl_f[i] = k,
 *           i ascending
 * and everything after G is untouched.  An observation whose value is exactly 0.0 stays in its level's list: dfma(0, r, G) is
 * performed, as the expanded model performs it.  For finite b, r and w this is bit for bit the same model on the expanded matrix, whose
 * column off_f + k holds w_f[i] where lvl_f[i] = k and 0.0 elsewhere: fma(0, x, y) = y as long as y is not -0.  The one new edge, next
 * to the non-finite one above: a chain from +0 now can reach -0 -- fma(w, b, +0) with w b negative and below half the smallest subnormal
 * rounds to -0 -- and there the two models may differ in the sign of a zero.  Stated and not engineered around.
 *
 * idhmc_create_glm_slopes is idhmc_create_glm_factors with these: values is F x n row-major, has holds F flags, 0 or 1.  values == NULL
 * or every has[f] == 0 gives exactly the context of idhmc_create_glm_factors: the same kernels, the same bits.  Rows of unflagged terms
 * are not read.  With a flag set the device also holds the values twice, 16 F n_pad bytes, counted in idhmc_device_bytes.  Refused with
 * IDHMC_ERR_BAD_ARG before the device is touched: values given with factors == NULL or F == 0; has == NULL; a has entry other than 0 or
 * 1; values->values == NULL with a flag set; a non-finite value in a flagged row; and everything idhmc_create_glm_factors refuses. */
typedef struct { const double *values; /* F x n, row-major */ const int32_t *has; /* F flags, 0 or 1 */ } idhmc_glm_factor_values;
int idhmc_create_glm_slopes(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                            const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                            const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values,
                            int64_t M, int64_t chains_per_response, const idhmc_options *opt, uint64_t seed);
/* has (F entries; room for 4) and the values (F x n, row-major; rows of unflagged terms 0) as the context was given them; every has is 0
 * for a context without values, and values is then left alone.  values may be NULL (the flags alone are wanted) */
int idhmc_glm_factor_values_get(const idhmc_ctx *ctx, int32_t *has, double *values);
/* Correlated random effects: a sampled correlation per pair of factor terms -- the covariance of (1 + x | subject).
 * A model with factor terms may name P pairs of terms, 0 <= P <= 2.  Pair p is (first[p], second[p]), two distinct terms with equal
 * level counts N_p; a term belongs to at most one pair; either term may have values or not, and the two need not share an index array.
 * Level k of the first term is paired with level k of the second.  Each pair adds one sampled coordinate zeta_p = atanh rho_p at the end:
 *   q = [u (Dx) | a (A) | omega (H) | lambda (J) | zeta (P)],   D = Dx + A + H + J + P <= 1024.
 * Per gradient and pair -- the kernels and the tests' C restatement follow this bit for bit: plain IEEE operations in the association
 * written, dfma, dexp and dlog1p those of idhmc_math.hpp --
 *   s = dexp(-|zeta|);  t = s * s;  d = 1 + t;  rho = copysign((1 - t) / d, zeta);  c = (2 * s) / d
 * (c = sqrt(1 - rho^2) in exact arithmetic; zeta = +0 gives rho = +0, c = 1; past |zeta| of about 745 rho = +-1, c = 0, all finite).
 * Forward, for k < N_p with c1 = off_first + k and c2 = off_second + k:
 *   ut_c1 = u_c1;   ut_c2 = dfma(rho, u_c1, c * u_c2);   ut_c = u_c for every other coordinate,
 * and everything the sections above define runs on ut where it ran on u: b_c from group and local scales, z, (r, v, s), G_c, W_g, the
 * lambdas and the auxiliary scores.  With the two terms in groups g1 and g2 the effects of level k are
 *   (b_c1, b_c2) = (sigma_g1 u_c1, sigma_g2 (rho u_c1 + sqrt(1 - rho^2) u_c2)):  b = sigma .* (L u),  L = [[1, 0], [rho, sqrt(1 - rho^2)]].
 * No combination is refused: groups, local scales (also on paired columns), priors, several responses and values compose.
 * Backward, after the chain rules above have produced Gh_c = dl / dut_c for the columns and filled omega, lambda and a:
 *   m_k = Gh_c2 * (c * dfma(c, u_c1, -(rho * u_c2)));   G_c1 = dfma(rho, Gh_c2, Gh_c1);   G_c2 = c * Gh_c2
 *   M_p[c2 mod 128]: plain additions over chunks ascending, from +0, of the pair's m_k;   G_zeta_p = the canonical 128-residue tree over M_p.
 * The prior runs on the raw q (the prior of u is on u, not ut).  eta[p] > 0 puts LKJ(eta) on the 2 x 2 correlation, with the Jacobian
 * of tanh: log p(zeta) = eta log(1 - rho^2), so that (rho + 1) / 2 is Beta(eta, eta); in the prior loop's terms
 *   T = T + (4 eta) * ((|zeta| + dlog1p(t)) - ln 2);   g = dfma(-2 eta, rho, G)
 * and the entries of zeta_p in mu, tau, kind and nu must be the defaults (0, 1, 0, 0) and are not applied.  eta[p] == 0: those entries
 * apply as to any coordinate, kinds 0 and 1 (normal or Student-t on Fisher's z); the log kinds are refused, as on a coefficient.
 * A covariance among three or four terms is a correlation block (idhmc_create_glm_block below).
 *
 * idhmc_create_glm_corr is idhmc_create_glm_slopes with these; mu, tau, kind and nu have D entries, the zetas last.  pairs == NULL or
 * P == 0 gives exactly the context of idhmc_create_glm_slopes: the same kernels, bits and footprint.  No LDS is added.  Refused with
 * IDHMC_ERR_BAD_ARG before the device is touched: P outside 0..2; first, second or eta NULL with P > 0; a term index outside 0..F-1;
 * first == second; a term in two pairs; unequal level counts; eta negative or not finite; eta > 0 with a non-default prior entry on
 * that zeta; a log kind on a zeta; pairs without factors; D > 1024 counting P; and everything idhmc_create_glm_slopes refuses. */
typedef struct { int32_t P; const int32_t *first, *second; const double *eta; } idhmc_glm_pairs;
int idhmc_create_glm_corr(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                          const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                          const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                          int64_t M, int64_t chains_per_response, const idhmc_options *opt, uint64_t seed);
/* *P, and with non-NULL arrays first, second and eta (P entries each) as the context was given them; 0 for every other context */
int idhmc_glm_pairs_get(const idhmc_ctx *ctx, int32_t *P, int32_t *first, int32_t *second, double *eta);
/* Structured factor terms: AR(1) and first-order random-walk effects across a term's levels -- a week, age-band or
 * dose-step effect that is autocorrelated or smooth along its index.  A model with factor terms may name S structured terms, 0 <= S <= 2;
 * structure i is (term[i], kind[i], eta[i]) with kind IDHMC_STRUCT_AR1 or IDHMC_STRUCT_RW1.  Level k of the term is position k of the
 * sequence: the index order is the time order.  An AR(1) term adds one sampled coordinate zeta = atanh phi; a random walk adds none.
 * With Sz the AR(1) terms, their zetas in list order behind the pairs':
 *   q = [u (Dx) | a (A) | omega (H) | lambda (J) | zeta_pairs (P) | zeta_ar (Sz)],   D = Dx + A + H + J + P + Sz <= 1024.
 * Per gradient and AR(1) term (phi, c) come from zeta by the expressions of the section above, the same bits in every lane:
 *   s = dexp(-|zeta|);  t = s * s;  d = 1 + t;  phi = copysign((1 - t) / d, zeta);  c = (2 * s) / d;      a random walk has phi = c = 1.
 * The process is the stationary unit-variance one, ut_0 = u_0, ut_k = phi ut_{k-1} + c u_k, and its ARITHMETIC is this Kogge-Stone scan,
 * not the sequential recurrence -- the kernels and the tests' C restatement follow it bit for bit.  With o the term's first column and
 * N its levels:
 *   forward:  x_0 = u_o;  x_k = c * u_{o+k} (k >= 1);  p = phi;  h = 1;
 *             while h < N: every k >= h takes x_k = dfma(p, x_{k-h}, x_k), all from the values before the stage; then p = p * p; h = 2 h;
 *             ut_{o+k} = x_k, and ut = u on every other coordinate.
 * Everything the sections above define runs on ut where it ran on u: the group scale of the term, z, (r, v, s), G, W_g, the scores.  A
 * pair's mix and a term's scan touch disjoint columns.  After the chain rules above have left Gh_c = dl / dut_c:
 *   backward: y_k = Gh_{o+k};  p = phi;  h = 1;
 *             while h < N: every k with k + h < N takes y_k = dfma(p, y_{k+h}, y_k), from the values before the stage; p = p * p; h = 2 h;
 *             lambda_k = y_k;   G_{u_o} = lambda_0;   G_{u_{o+k}} = c * lambda_k (k >= 1);
 *   AR(1):    m_0 = +0;  m_k = lambda_k * (c * dfma(c, ut_{o+k-1}, -(phi * u_{o+k})))  (k >= 1; ut from the forward scan, run again);
 *             M[(o+k) mod 128]: plain additions over chunks ascending, from +0;   G_zeta = the canonical 128-residue tree over M.
 * zeta = +0 gives phi = +0, c = 1 and ut = u: the unstructured model's bits.  Past |zeta| of about 745 phi = +-1 and c = 0, every ut_k is
 * u_0 (up to sign) and G_zeta = 0, all finite.  The prior of zeta follows a pair's rules: eta > 0 puts Beta(eta, eta) on (phi + 1) / 2
 * with the Jacobian of tanh (the section above's T and g rows, the device's internal kind 5) and wants the defaults (0, 1, 0, 0) in zeta's
 * entries of mu, tau, kind and nu; eta == 0 lets those entries apply, kinds 0 and 1; the log kinds are refused.  The prior of u is on u.
 * Groups (a sampled scale on the term), local scales on other columns, priors, values on the structured term, several responses and pairs
 * among other terms compose.  Second-order walks (RW2), a sum-to-zero constraint, seasonal and spatial (ICAR) structures are GMRF terms
 * (idhmc_create_glm_gmrf below); out of scope: AR(p).  A random walk's level is not identified against an intercept; its u_0 has the prior the prior arrays give it.
 *
 * idhmc_create_glm_struct is idhmc_create_glm_corr with these.  structs == NULL or S == 0 gives exactly the context of
 * idhmc_create_glm_corr: the same kernels, bits and footprint.  No LDS is added.  Refused with IDHMC_ERR_BAD_ARG before the device is
 * touched: S outside 0..2; term, kind or eta NULL with S > 0; a term index outside 0..F-1; a term listed twice; a kind other than 1 or 2;
 * eta negative or not finite; eta != 0 on a random walk; a structured term with fewer than 2 levels; a structured term that is in a pair;
 * a local-scale flag on a column of a structured term; structures without factors; D > 1024 counting Sz; eta > 0 with a non-default prior
 * entry on that zeta; a log kind on a zeta; and everything idhmc_create_glm_corr refuses. */
#define IDHMC_STRUCT_AR1 1
#define IDHMC_STRUCT_RW1 2
typedef struct { int32_t S; const int32_t *term, *kind; const double *eta; } idhmc_glm_structs;
int idhmc_create_glm_struct(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                            const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                            const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                            const idhmc_glm_structs *structs, int64_t M, int64_t chains_per_response, const idhmc_options *opt, uint64_t seed);
/* *S, and with non-NULL arrays term, kind and eta (S entries each) as the context was given them; 0 for every other context */
int idhmc_glm_structs_get(const idhmc_ctx *ctx, int32_t *S, int32_t *term, int32_t *kind, double *eta);
/* Gaussian Markov random field priors on a factor term's levels: ICAR effects over regions, second-order random
 * walks, seasonal effects, difference penalties, or any "generic" term with a user's sparse precision.  A model with factor terms may
 * name G GMRF terms, 0 <= G <= 2; term i names factor term term[i] with N_i levels and first column o_i, a symmetric N_i x N_i
 * precision Q_i in CSR form and a fixed kappa[i] >= 0.  The rows of term 0 come first and then those of term 1: start has
 * sum N_i + 1 cumulative entries from 0, row k of term i is entries start[r + k] .. start[r + k + 1] - 1 of col and val with
 * r = 0 for term 0 and N_0 for term 1; col holds columns 0 .. N_i - 1 of the row's own term, strictly ascending within a row, the
 * diagonal present in every row and > 0, between 1 and 128 entries per row, Q_ij and Q_ji both present and bit-equal.
 * No coordinate is added.  The levels u of such a term get
 *   log p(u) = -1/2 u' Q u - 1/2 kappa (sum u)^2        (kappa > 0: a soft sum-to-zero constraint)
 * in place of the entries of the prior arrays, which must be the defaults (mu, tau, kind, nu = 0, 1, 0, 0) on its columns.  The scale of
 * the effect is the term's group scale, b = exp(omega_g) u, as for every term; BYM is two terms on one index array, one with a Q and one
 * without.  Per gradient, on the raw q (a member c = o + k, u_c = q_c; T and g are the prior loop's of the sections above):
 *   Sr per lane component: plain additions over chunks ascending, from +0, of the members' u_c;  S = the canonical 128-residue tree;
 *   s = kappa > 0 ? kappa * S : +0;   for e = start[k] .. start[k+1]-1 ascending:  s = dfma(val[e], u_{o + col[e]}, s);
 *   T = dfma(u_c, s, T);   g = G - s.
 * With Q = I and kappa = 0 these are the bits of the normal prior with mu = 0, tau = 1 for u and G that are not -0.  A Q that is only
 * positive semi-definite with kappa = 0 gives an improper prior along its null space (the likelihood has to identify it); the library
 * checks the table's form, not definiteness.  Groups, values on the term (a spatially varying slope), several responses, pairs and
 * structures on other terms and local scales on other columns compose.  Still out of scope: AR(p), a sampled CAR or Leroux
 * autocorrelation, the BYM2 mixing parameter, hard constraints.
 *
 * idhmc_create_glm_gmrf is idhmc_create_glm_struct with these.  gmrfs == NULL or G == 0 gives exactly the context of
 * idhmc_create_glm_struct: the same kernels, bits and footprint.  No LDS is added.  Refused with IDHMC_ERR_BAD_ARG before the device is
 * touched: G outside 0..2; term, start, col, val or kappa NULL with G > 0; GMRFs without factors; a term outside 0..F-1 or listed
 * twice; a GMRF term that is in a pair or structured; a local-scale flag on one of its columns; a non-default prior entry on one of its
 * columns; start not non-decreasing from 0; a row with 0 or more than 128 entries; columns not strictly ascending or outside 0..N-1; a
 * missing or non-positive diagonal; a non-finite value; Q_ij and Q_ji not bit-equal or one of them absent; kappa negative or not
 * finite; and everything idhmc_create_glm_struct refuses. */
typedef struct { int32_t G; const int32_t *term; const int64_t *start; const int32_t *col; const double *val; const double *kappa; } idhmc_glm_gmrfs;
int idhmc_create_glm_gmrf(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                          const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                          const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                          const idhmc_glm_structs *structs, const idhmc_glm_gmrfs *gmrfs, int64_t M, int64_t chains_per_response,
                          const idhmc_options *opt, uint64_t seed);
/* *G, and with non-NULL arrays term, kappa and nnz (the entries of each term's precision; G entries each) as the context was given
 * them; 0 for every other context */
int idhmc_glm_gmrfs_get(const idhmc_ctx *ctx, int32_t *G, int32_t *term, double *kappa, int64_t *nnz);
/* A correlation block of three or four factor terms: (1 + x1 + x2 | subject) with a sampled K x K correlation
 * matrix.  A model with factor terms may name ONE block of K in {2, 3, 4} distinct terms term[0 .. K-1], all of N levels, with values or
 * without, on one index array or several.  The order of term[] is the row order of L and is the caller's: level k of every term belongs
 * together, c_j = off_{term[j]} + k.  A model has pairs or a block, not both (K = 2 is the pair, bit for bit).  The block adds
 * K (K - 1) / 2 coordinates zeta_ji = atanh z_ji, 1 <= j < K, 0 <= i < j, where the pairs' zetas stand, row-major:
 *   q = [u (Dx) | a (A) | omega (H) | lambda (J) | zeta_block | zeta_ar (Sz)],   zeta_ji is coordinate cz0 + j (j - 1) / 2 + i,   D <= 1024.
 * z_ji are the canonical partial correlations of R = L L'.  Per gradient (plain IEEE operations in the association written):
 *   (z_ji, c_ji) from zeta_ji by the expressions of idhmc_create_glm_corr (rho and c there), the same bits in every lane;
 *   coef(j, m, .) for -1 <= m < j:  s = 1; for i = m+1 .. j-1: coef(j,m,i) = z_ji * s, then s = s * c_ji; coef(j,m,j) = s, and where s
 *   is still the initial 1 the other factor is taken itself (no multiplication);  L_ji = coef(j, -1, i), L_00 = 1;
 *   r_jm = c_j0 * .. * c_j,m-1 left to right, r_j0 = 1.
 *   mix:     ut_{c_0} = u_{c_0};  j >= 1: x = L_jj * u_{c_j}; for i = 0 .. j-1 ascending x = dfma(L_ji, u_{c_i}, x); ut_{c_j} = x.
 * Everything the sections above define runs on ut; the prior of u stays on u.  After the chain rules have left Gh = dl / dut:
 *   zeta_jm: w = coef(j,m,j) * u_{c_j} (u_{c_j} itself when j = m + 1); for i = m+1 .. j-1 ascending w = dfma(coef(j,m,i), u_{c_i}, w);
 *            e = c_jm * dfma(c_jm, u_{c_m}, -(z_jm * w));  m >= 1: e = r_jm * e;   m_k = Gh_{c_j} * e;
 *            M_jm[c_j mod 128]: plain additions over chunks ascending, from +0;  G_zeta_jm = the canonical 128-residue tree over M_jm;
 *   then, from the Gh before any is overwritten:  G_{c_i} = (i == 0 ? Gh_{c_0} : L_ii * Gh_{c_i});
 *            for j = i+1 .. K-1 ascending G_{c_i} = dfma(L_ji, Gh_{c_j}, G_{c_i}).
 * eta > 0 is LKJ(eta) on R, which is separable in the partial correlations: zeta_ji gets the LKJ row of idhmc_create_glm_corr with the
 * exponent beta_ji = eta + (K - 2 - i) / 2 (i the COLUMN), and the zetas' entries of mu, tau, kind and nu must be the defaults and are
 * not applied.  eta == 0: those entries apply (kinds 0 and 1; the log kinds are refused).  The reported correlations are
 *   R_j0 = z_j0;   i >= 1: x = L_ji * L_ii; for k = 0 .. i-1 ascending x = dfma(L_jk, L_ik, x); R_ji = x,
 * and the device summaries report [beta | a | sigma | exp lambda | R (row-major lower triangle) | phi].  Groups, local scales (also on
 * block columns), priors, values, several responses and an AR(1) or random-walk structure on a remaining term compose; a GMRF prior on a
 * remaining term is accepted too (the device tests cover no GMRF term next to a block).
 * Out of scope: more than one block, K > 4, a block next to pairs, a block term that is structured or a GMRF term.
 *
 * idhmc_create_glm_block is idhmc_create_glm_gmrf with these.  block == NULL or K == 0 gives exactly the context of
 * idhmc_create_glm_gmrf: the same kernels, bits and footprint.  No LDS is added.  Refused with IDHMC_ERR_BAD_ARG before the device is
 * touched: K not in {0, 2, 3, 4}; term NULL; a term outside 0..F-1 or listed twice; unequal level counts; eta negative or not finite;
 * eta > 0 with a non-default prior entry on one of the zetas; a log kind on a zeta; a block together with pairs; a block term that is
 * structured or a GMRF term; a block without factors; D > 1024 counting the zetas; and everything idhmc_create_glm_gmrf refuses. */
typedef struct { int32_t K; const int32_t *term; double eta; } idhmc_glm_block;
int idhmc_create_glm_block(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                           const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                           const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                           const idhmc_glm_structs *structs, const idhmc_glm_gmrfs *gmrfs, const idhmc_glm_block *block,
                           int64_t M, int64_t chains_per_response, const idhmc_options *opt, uint64_t seed);
/* *K, and with non-NULL term (K entries) and eta as the context was given them; 0 for every other context */
int idhmc_glm_block_get(const idhmc_ctx *ctx, int32_t *K, int32_t *term, double *eta);
/* Factor terms with several weighted levels per observation: penalised spline smooths s(x) -- a cubic B-spline
 * gives every observation four adjacent basis functions, and with an RW2 precision as the term's GMRF prior that is a P-spline --,
 * multi-membership effects (a pupil of two schools, weights summing to 1), a match between two teams (+1 / -1), any sparse block of the
 * design with a bounded number of entries per row.  Term f has a WIDTH M_f in 1..4: observation i has M_f entries
 * (lvl_{f,m}[i], w_{f,m}[i]), m < M_f.  The term's columns are still off_f .. off_f + N_f - 1 of the model and nothing is stored in X
 * for them; F <= 4 as before, and the planes P = sum M_f are limited to 8.  An entry may be absent (lvl = -1, its value ignored) when
 * an observation has fewer than M_f members: the present entries come first, and within a term their levels are STRICTLY ASCENDING,
 * hence distinct; an observation with no present entry in a term is allowed.  The arithmetic -- the kernels follow this bit for bit --
 *   z_i = the dfma chain over c < Dd (as above), then for f = 0 .. F-1 ascending and within f for m = 0 .. M_f-1 ascending:
 *           z_i = dfma(w_{f,m}[i], b[off_f + lvl_{f,m}[i]], z_i)   for every present entry (a term given without values: w = 1.0)
 *   G_{off_f + k} = the dfma chain from +0 of dfma(w, r_i, G) over the observations i < n that have level k in any plane of term f,
 *           i ascending (levels are distinct within an observation, so it appears at most once); a w of exactly 0.0 stays in its list
 * and everything after G is untouched.  Because the levels ascend, this is bit for bit the same model on the expanded matrix, whose
 * column off_f + k holds w_{f,m}[i] where lvl_{f,m}[i] = k and 0.0 elsewhere, under the conditions of idhmc_create_glm_slopes (finite b,
 * r, w; the -0 edge stated there).  A wide term may be grouped, carry local scales, be a GMRF term or be structured; many responses
 * compose.  Out of scope: width > 4, more than 8 planes, a wide term in a pair or a block.
 *
 * idhmc_create_glm_multi is idhmc_create_glm_block with these.  members == NULL gives exactly the context of idhmc_create_glm_block.
 * With members, factors gives F and levels and its index must be NULL, and values (the idhmc_glm_factor_values argument) must be NULL.
 * If every width is 1 (and then no entry may be absent) the context is the one idhmc_create_glm_block builds from those planes: the
 * same kernels, bits and footprint.  Otherwise the device holds the planes, 4 P n_pad + 16 P n_pad + P n_pad bytes plus the starts,
 * counted in idhmc_device_bytes.  No LDS is added.  Refused with IDHMC_ERR_BAD_ARG before the device is touched, each message naming the
 * term, plane and observation: a width outside 1..4 or P > 8; members without factors; both index sources or both value sources given;
 * a level outside -1 .. N_f-1; -1 in a term of width 1; a present entry behind an absent one; levels of an observation not strictly
 * ascending; a non-finite value on a present entry; a term of width > 1 named by a pair or a block; and everything
 * idhmc_create_glm_block refuses. */
typedef struct { const int32_t *width;   /* F entries, 1..4, sum <= 8 */
                 const int32_t *index;   /* P x n row-major, planes of term 0 first; -1 = absent */
                 const double  *values;  /* P x n row-major, or NULL: every present entry 1.0 */ } idhmc_glm_members;
int idhmc_create_glm_multi(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                           const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                           const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                           const idhmc_glm_structs *structs, const idhmc_glm_gmrfs *gmrfs, const idhmc_glm_block *block,
                           const idhmc_glm_members *members, int64_t M, int64_t chains_per_response, const idhmc_options *opt, uint64_t seed);
/* width (F entries; room for 4), and with non-NULL index and values the P x n planes as the context was given them (values: 1.0 on the
 * present entries of a table given without values, 0.0 on absent ones).  A context without a wide term reports its F terms as planes of
 * width 1.  With a wide term idhmc_glm_factors_get reports the first plane of every term. */
int idhmc_glm_members_get(const idhmc_ctx *ctx, int32_t *width, int32_t *index, double *values);
typedef struct {                             /* a GLM in parts, whole (the head of the GLM part, above) */
    const idhmc_glm_desc          *glm;      /* required */
    const idhmc_glm_priors        *priors;   /* each of the following: NULL = absent, exactly as the legacy argument */
    const idhmc_glm_local         *local;
    const idhmc_glm_factors       *factors;
    const idhmc_glm_factor_values *values;
    const idhmc_glm_pairs         *pairs;
    const idhmc_glm_structs       *structs;
    const idhmc_glm_gmrfs         *gmrfs;
    const idhmc_glm_block         *block;
    const idhmc_glm_members       *members;
    int64_t M, chains_per_response;          /* (1, 0) or (0, 0): one response, the context of idhmc_create_glm */
} idhmc_glm_model;
int idhmc_create_glm_model(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                           const idhmc_glm_model *model, const idhmc_options *opt, uint64_t seed);
int idhmc_destroy(idhmc_ctx *ctx);
/* run on a caller-owned hipStream_t (e.g. a torch.cuda.Stream); NULL = the library's own non-blocking stream.
 * NB the legacy default stream's handle IS NULL: it cannot be selected, and it does not order itself against the
 * library's stream -- hand over a created stream when other work must be ordered with the engine's. */
int idhmc_set_stream(idhmc_ctx *ctx, void *hip_stream);
int idhmc_synchronize(idhmc_ctx *ctx);
int64_t idhmc_nchains(const idhmc_ctx *ctx);
int32_t idhmc_dim(const idhmc_ctx *ctx);
int32_t idhmc_padded_dim(const idhmc_ctx *ctx);
/* the form of the NUTS kernel's gradient of a LOGISTIC_REGRESSION, GLM or GLM_AUX context: 0 one chain per wavefront, 1 the fp64
 * matrix cores (16 chains per workgroup); -1 for every other model.  Both forms compute the same bits. */
int idhmc_glm_form(const idhmc_ctx *ctx);
int64_t idhmc_device_bytes(const idhmc_ctx *ctx);
/* Contexts with state arrays of 64 MiB or more try several placements of q, p, grad l (and a per-chain M^-1) in HBM when they are
 * created and keep the one on which the single-step sweep's access pattern runs fastest (the same kernel differs by 10 % between
 * placements).  Reports the probe's rate on the placement kept (GB/s; 0 when nothing was probed) and how many
 * candidates were tried.  IDHMC_PLACEMENT_TRIES=1 in the environment takes the first placement. */
int idhmc_placement_info(const idhmc_ctx *ctx, double *probe_GBps, int32_t *candidates);
/* What that search cost and against what it judged: wall time of the search inside idhmc_create (ms), the most device bytes held at
 * one time while candidates were compared (the pair walk that comes first: spacers included, bounded by IDHMC_PLACEMENT_WALK_BYTES,
 * default 64 GiB, half of the free memory and 250 ms; the walk over whole sets: IDHMC_PLACEMENT_MAX_BYTES, default 16 GiB, and a quarter of it;
 * everything but the set kept is given back before idhmc_create returns),
 * the rate of ONE array alone in the same probe (GB/s; a candidate set is "good" at >= 1.10 x that), and the kind of placement
 * kept: 0 = separate allocations, 3 = separate allocations found by the pair walk (IDHMC_PLACEMENT_PAIRS=0 skips it).  Codes 1
 * and 2 belonged to placement kinds that were removed and are never returned.  Any pointer may be NULL. */
int idhmc_placement_cost(const idhmc_ctx *ctx, double *create_ms, int64_t *peak_transient_bytes, double *single_array_GBps, int32_t *kind);
/* The dense density's single-step sweep runs as up to four lanes of kernels on four streams (lane 0 = the context's stream); lanes
 * overlap only on different hardware queues, so the library picks streams that do (an idle-kernel test at the first such sweep).
 * Reports the lanes in use (0 before the first sweep or when the sweep is one kernel) and how many of them were found on
 * different hardware queues (fewer than `lanes` under a profiler that serialises streams). */
int idhmc_lanes_info(const idhmc_ctx *ctx, int32_t *lanes, int32_t *on_distinct_queues);
/* The single-step leapfrog of a separable density keeps every stride-th chain in the Infinity Cache from one sweep to the next
 * (default-policy loads and stores behind the other chains' non-temporal stream): the stride of the IDHMC_GRAD_STORE sweep
 * (three arrays, ceil(3 C L 8 / 192 MiB)) and of the IDHMC_GRAD_RECOMPUTE sweep (q and p only, ceil(2 C L 8 / 192 MiB));
 * 1 = the whole state fits.  Read-only. */
int idhmc_leapfrog_slice_info(const idhmc_ctx *ctx, int32_t *stride_store, int32_t *stride_recompute);

/* ---- state (PhasePoint / EvaluatedLogDensity, src/hamiltonian.jl:237-276) - */
/* q <- host[nchains*D]; evaluates l(q), grad l(q) (evaluate_l!, src/kinetic_energy.jl:72-85) */
int idhmc_set_q(idhmc_ctx *ctx, const double *q);
/* q ~ U[-2,2)^D per chain, then evaluate (random_position!, src/warmup.jl:73,119-124) */
int idhmc_random_position(idhmc_ctx *ctx);
int idhmc_set_p(idhmc_ctx *ctx, const double *p);
/* M^-1 <- host; per_chain = 0: D values shared by all chains, 1: nchains*D.
 * W = 1/sqrt(M^-1) (GaussianKineticEnergy, src/hamiltonian.jl:50-57) */
int idhmc_set_minv(idhmc_ctx *ctx, const double *minv, int per_chain);
int idhmc_set_eps(idhmc_ctx *ctx, double eps);                /* all chains */
int idhmc_set_eps_per_chain(idhmc_ctx *ctx, const double *eps);
int idhmc_get_q(idhmc_ctx *ctx, double *q);                   /* nchains*D */
int idhmc_get_p(idhmc_ctx *ctx, double *p);
int idhmc_get_grad(idhmc_ctx *ctx, double *g);   /* grad l(q) of the current state; re-evaluated first when the device copy is stale: a NUTS transition of a
                                                     separable density does not write it back (nothing on the sampling path reads it), nor does the
                                                     single-step leapfrog in its default mode, IDHMC_GRAD_RECOMPUTE */
int idhmc_get_minv(idhmc_ctx *ctx, double *minv);             /* nchains*D (shared metric is broadcast) */
int idhmc_get_lq(idhmc_ctx *ctx, double *lq);                 /* nchains: l(q) */
int idhmc_get_eps(idhmc_ctx *ctx, double *eps);               /* nchains */
/* pi = l(q) - K(p) per chain: logdensity(H, z), src/kinetic_energy.jl:107-112 (uses kinetic_energy :14-24) */
int idhmc_logdensity(idhmc_ctx *ctx, double *pi);

/* ---- hot path -------------------------------------------------------------- */
/* p <- W .* randn for transition number `iter` (rand_p!, src/kinetic_energy.jl:63; called
 * from src/NUTS.jl:254 and src/warmup.jl:195) */
int idhmc_refresh_momentum(idhmc_ctx *ctx, uint32_t iter);
/* n_steps fused leapfrog steps of size eps (eps < 0: backward, src/NUTS.jl:20) for every chain:
 * loop A, gradient, loop B (leapfrog, src/kinetic_energy.jl:126-163), leaving l(q') and
 * pi' = l(q') - K(p') per chain.  n_steps = 1 streams the state through HBM once.
 * Dense density, n_steps = 1, from 12 288 chains on, on the library's own stream: the sweep runs as several kernels on
 * up to four internal streams (ranges of chains; they fork from the context's stream and join it again inside the next
 * idhmc_* call of any other kind, so every call still sees the effects of all earlier ones).  With a caller-owned
 * stream (idhmc_set_stream) the sweep is one kernel on that stream, so that work the caller enqueues there is
 * ordered after it without going through the library. */
int idhmc_leapfrog(idhmc_ctx *ctx, double eps, int32_t n_steps);
/* the same with every chain's own eps (as set by idhmc_set_eps*, adaptation or the search) */
int idhmc_leapfrog_own_eps(idhmc_ctx *ctx, int32_t n_steps);
/* switch idhmc_options.leapfrog_grad_mode on a live context */
int idhmc_set_leapfrog_grad_mode(idhmc_ctx *ctx, int32_t mode);
/* one NUTS transition per chain with that chain's current eps: sample_tree (src/NUTS.jl:251-264)
 * = directions, rand_p!, sample_trajectory/adjacent_tree (src/tree.jl:321-444), leaf / turn /
 * acceptance / proposal bookkeeping (src/NUTS.jl:32-191).  iter >= 1 numbers the transition
 * (RNG address).  flags: see below.  Afterwards q, grad, l(q) hold the new draw; the momentum
 * array is unspecified until it is refreshed (the reference's next sample_tree overwrites it
 * first thing, src/NUTS.jl:254; no caller reads it in between). */
enum {
    IDHMC_T_ADAPT_EPS = 1,      /* adapt_stepsize after the transition (src/warmup.jl:303) */
    IDHMC_T_ACCUM_METRIC = 2,   /* add the new draw to the running metric window (src/warmup.jl:299,309) */
    IDHMC_T_ACCUM_MOMENTS = 4,  /* add the new draw to the running posterior mean / variance */
    IDHMC_T_KEEP_P = 8,         /* do not refresh p (reference kwarg p=..., src/NUTS.jl:251-258) */
    IDHMC_T_USE_DIRECTIONS = 16,/* use injected directions (reference kwarg directions=...) */
    IDHMC_T_ACCUM_DIAG = 32     /* add the transition to the device-side diagnostics (idhmc_diag_reset first) */
};
/* Any other bit of `flags` is refused with IDHMC_ERR_BAD_ARG before anything is launched (by idhmc_nuts_transitions too), and so
 * is IDHMC_T_ADAPT_EPS on a context in IDHMC_EPS_PER_RESPONSE (the per-response stepsize adapts between transitions, in the drivers).
 * (Bit 30 is the test suite's: accepted only on a context created with IDHMC_TEST_XCC_MISMATCH=1 in the environment.) */
int idhmc_nuts_transition(idhmc_ctx *ctx, uint32_t iter, uint32_t flags);
/* n transitions of every chain, numbered iter, iter + 1, ..., iter + n - 1, in ONE launch (src/warmup.jl:288-305 and :324-330 run
 * a chain's transitions back to back; chains are independent, src/mcmc.jl:150-157).  The state afterwards is bit for bit that of n
 * calls of idhmc_nuts_transition -- every random number is addressed by (seed, chain, transition) -- but the device hands out
 * (transition, chain) pairs from one queue, so a chain's next transition starts as soon as its previous one is done and a
 * wavefront is free, instead of when the slowest tree of the whole launch is: with few chains per resident wavefront (configs[3]:
 * four) the end of every single-transition launch is a quarter of its time.  Only the records of the last transition are kept
 * (idhmc_get_tree_stats); IDHMC_T_USE_DIRECTIONS and IDHMC_T_KEEP_P are not allowed, nor IDHMC_T_ADAPT_EPS with the global or the per-response stepsize (its exchange
 * sits between transitions).  If a chain raises the abort code no further transitions are started (nor any at all while the code
 * of an earlier launch is still set: the next driver call reports and clears it).
 * The library's own drivers (idhmc_tuning_stage, idhmc_mcmc) use it where no per-transition record leaves the device and the
 * chains are few per wavefront; IDHMC_FUSE=0 / 1 in the environment forbids / forces that. */
int idhmc_nuts_transitions(idhmc_ctx *ctx, uint32_t iter, int32_t n, uint32_t flags);
/* *possible: the device places workgroups b and b + 8 on one XCD (probed when the context was created), which the hand-over of a
 * chain inside a launch relies on -- otherwise idhmc_nuts_transitions makes n launches; *used_by_drivers: and IDHMC_FUSE does not forbid it */
int idhmc_fused_launch_info(idhmc_ctx *ctx, int32_t *possible, int32_t *used_by_drivers);
int idhmc_set_directions(idhmc_ctx *ctx, const uint32_t *directions); /* nchains, for IDHMC_T_USE_DIRECTIONS */
/* The reference aborts a warm-up the moment a chain's stepsize falls below 1e-10 (src/warmup.jl:291-296).  Every
 * transition launch is followed by an asynchronous copy of the device's abort word into pinned host memory;
 * idhmc_poll_abort waits for the word of the launch `lag` launches back (0 = the newest: a synchronisation) and
 * returns its code (0, IDHMC_ERR_EPS_UNDERFLOW, or IDHMC_ERR_HIP from a refused launch of several transitions) without touching the stream otherwise.  The library's own drivers
 * poll with lag 8, i.e. stop within 8 transitions of the underflow and then fail with the code. */
int idhmc_poll_abort(idhmc_ctx *ctx, int32_t lag, int32_t *code);
int idhmc_get_tree_stats(idhmc_ctx *ctx, idhmc_tree_stats *stats);    /* nchains records of the last transition */

/* ---- adaptation (callers of the hot path, src/warmup.jl:188-314) ----------- */
/* find_initial_stepsize per chain with the momentum now in p (src/stepsize.jl:111-164,
 * src/warmup.jl:188-200); result becomes each chain's eps.  Global mode: exp(mean of log eps over all chains of all
 * ranks), the IDHMC_XCHG_LOGEPS record all-reduced through the hook / communicator -- every rank gets the same bits */
int idhmc_find_initial_stepsize(idhmc_ctx *ctx);
/* the per-chain searches alone, in every mode: for a host that pools the stepsizes itself (idhmc_logeps_sum, its own
 * exchange of the record, idhmc_set_eps_from_logeps) */
int idhmc_find_initial_stepsize_per_chain(idhmc_ctx *ctx);
/* FindLocalOptimum (src/warmup.jl:137-187): per chain, maximise l(q) - magnitude_penalty/2 * sum(q^2) for at
 * most `iterations` quasi-Newton iterations from the current q; a non-finite result restarts from a new random
 * position with the penalty doubled, at most 100 times, else the call fails with IDHMC_ERR_OPTIMIZATION
 * (:162-172).  Leaves q, l(q), grad l(q) at the optimum.  The reference calls
 * QuasiNewtonMethods.proptimize! (external, source absent); the iteration here is the engine's own
 * L-BFGS (5 pairs, Armijo backtracking), identical in oracle/ and on the device. */
int idhmc_find_local_optimum(idhmc_ctx *ctx, double magnitude_penalty, int32_t iterations);
/* initial_adaptation_state from each chain's eps (src/stepsize.jl:208-212) */
int idhmc_da_init(idhmc_ctx *ctx);
/* eps <- final_eps = exp(logeps_bar) (src/stepsize.jl:241, src/warmup.jl:313) */
int idhmc_da_finalize(idhmc_ctx *ctx);
/* ---- the global-stepsize exchange (IDHMC_EPS_GLOBAL) --------------------------------------------------
 * The reference adapts eps per chain and has no exchange (src/warmup.jl:284-303); north_star adds ONE dual-averaging
 * state fed by the mean acceptance of all chains of all ranks.  For the result not to depend on how the chains are
 * sharded, the pooled statistic is carried as EXACT integers: every chain's value x is rounded to a fixed-point
 * integer v = rint(x * 2^S), split into two limbs hi = v >> B (arithmetic), lo = v & (2^B - 1), and the limbs are
 * summed as integers (in doubles: every partial sum stays below 2^53, so any SUM all-reduce of doubles -- RCCL, gloo,
 * MPI -- in any association is exact).  The mean is ((sum hi * 2^B + sum lo) * 2^-S) / count, evaluated from the
 * totals on every rank alike.  Two statistics use it:
 *   IDHMC_XCHG_ACCEPT  acceptance rates in [0, 1]:        S = 52, B = 26   (adapt_stepsize's `a`, src/stepsize.jl:220)
 *   IDHMC_XCHG_LOGEPS  log(eps) of the per-chain searches: S = 40, B = 25   (|log eps| clamped to 1024)
 * both exact for up to 2^26 chains per job.  The exchange buffer is IDHMC_XCHG_DOUBLES doubles in device memory:
 *   [0] sum of hi limbs  [1] sum of lo limbs  [2] number of chains  [3] number of chains with a pending error status
 * so eps is bit-identical for 1, 2, 4, 8 ... ranks. */
#define IDHMC_XCHG_DOUBLES 4
enum { IDHMC_XCHG_ACCEPT = 0, IDHMC_XCHG_LOGEPS = 1,
       IDHMC_XCHG_STATUS = 2 /* library-internal: a record whose sums are zero, only slots [2] and [3] carry data (error agreement) */ };
/* device: the exchange record of the last transition's acceptance rates / of the chains' current log(eps) */
int idhmc_accept_sum(idhmc_ctx *ctx, double *dev_xchg);
int idhmc_logeps_sum(idhmc_ctx *ctx, double *dev_xchg);
/* device: adapt_stepsize (src/stepsize.jl:220-229) with the pooled mean acceptance of an (all-reduced) record */
int idhmc_da_adapt_global(idhmc_ctx *ctx, const double *dev_xchg);
/* device: every chain's eps <- exp(pooled mean of log eps) of an (all-reduced) IDHMC_XCHG_LOGEPS record */
int idhmc_set_eps_from_logeps(idhmc_ctx *ctx, const double *dev_xchg);
/* host helpers of the same protocol (no device needed): add the record of n values to xchg4 (zero it first), and
 * the mean of a record; what a caller that exchanges by other means (MPI, files) or checks a run needs */
int idhmc_xchg_accumulate(int32_t kind, const double *values, int64_t n, double *xchg4);
int idhmc_xchg_mean(int32_t kind, const double *xchg4, double *mean);
/* Let the library's own drivers (idhmc_find_initial_stepsize, idhmc_tuning_stage, idhmc_mcmc_with_warmup) run the
 * exchange: after the record has been enqueued on the context's stream the library calls fn(dev_xchg, user); fn
 * must SUM-all-reduce the IDHMC_XCHG_DOUBLES doubles at dev_xchg over all ranks, ordered after the work already on
 * the stream and before what is enqueued next (RCCL on the same stream, or torch.distributed.all_reduce on a tensor
 * aliasing dev_xchg with the context on torch's stream).  dev_xchg is caller-owned device memory.
 * fn == NULL: single-rank (no exchange).
 * Errors are agreed on before they are returned: idhmc_find_initial_stepsize (both eps modes), idhmc_find_local_optimum and
 * idhmc_tuning_stage (so idhmc_mcmc_with_warmup's warm-up too) enqueue the exchange FIRST and then fail on every rank together
 * when the all-reduced slot [3] is non-zero (local code on the rank that owns the failing chain, IDHMC_ERR_PEER on the others);
 * idhmc_tuning_stage ends with one more such record (zeros but slot [3]) before its pooled-metric collectives.
 * idhmc_mcmc has no collective to leave a peer in and checks locally: only the rank that owns the failing chain fails.
 * idhmc_find_initial_stepsize_per_chain is the bare search for hosts that pool the stepsizes themselves: it checks locally too.
 * The hook carries ONLY this record.  IDHMC_METRIC_POOLED needs table-sized all-reduces, which go through the context's own
 * communicator (idhmc_comm_init); under a hook WITHOUT a communicator idhmc_metric_update pools the chains of this rank only
 * (rank-local metric) -- exchange the tables yourself with idhmc_pool_partials / idhmc_pool_consume for a job-wide one. */
typedef int (*idhmc_allreduce_fn)(double *dev_xchg, void *user);
int idhmc_set_allreduce_hook(idhmc_ctx *ctx, idhmc_allreduce_fn fn, void *user, double *dev_xchg);
/* Native exchange: an RCCL communicator owned by the context (one rank per GPU, xGMI inside a node).
 * Rank 0 obtains the 128-byte id with idhmc_comm_unique_id and distributes it by any host channel; every
 * rank then calls idhmc_comm_init (collective, on the context's device).  From then on the library's
 * drivers enqueue ncclAllReduce(SUM, IDHMC_XCHG_DOUBLES x fp64) on the context's stream between the record and its
 * consumer -- the only collective of the path (the reference has none: per-chain adaptation,
 * src/warmup.jl:284-303); a hook set with idhmc_set_allreduce_hook takes precedence.
 * RCCL is loaded with dlopen at the first of these calls; without it they return IDHMC_ERR_HIP. */
#define IDHMC_COMM_ID_BYTES 128
int idhmc_comm_unique_id(void *id128);
int idhmc_comm_init(idhmc_ctx *ctx, int32_t nranks, int32_t rank, const void *id128);
int idhmc_comm_destroy(idhmc_ctx *ctx);
/* for callers that drive the transitions themselves: SUM-all-reduce n doubles at dev_buf in place on the context's stream */
int idhmc_comm_allreduce(idhmc_ctx *ctx, double *dev_buf, int32_t n);
/* what the communicator has done: ranks, this rank, all-reduces enqueued since idhmc_comm_init (measurement: a
 * multi-GPU bench line reports these so that the record shows RCCL saw N ranks).  Without a communicator: 0, 0, 0. */
int idhmc_comm_info(idhmc_ctx *ctx, int32_t *nranks, int32_t *rank, int64_t *allreduces);
/* start / finish a metric window: GaussianKineticEnergy!(kappa, chain, lambda)
 * (src/hamiltonian.jl:117-189, src/warmup.jl:308-311), computed from running sums instead of a stored chain */
int idhmc_metric_begin(idhmc_ctx *ctx);
int idhmc_metric_update(idhmc_ctx *ctx, double lambda);
/* IDHMC_METRIC_POOLED by hand (what idhmc_metric_update does with the context's communicator): the column sums of a
 * pass are formed per segment of IDHMC_POOL_SEGMENT consecutive GLOBAL chain ids (ascending chain order inside) into a
 * table [seg_hi - seg_lo][padded_dim + 1] (last column: draw counts); segments this context holds no chain of are
 * written as zeros.  Tables of several contexts ADD (exact when every segment lies on one context: shards aligned to
 * the segment size); idhmc_pool_consume adds the table's rows in order -- pass 0 yields the pooled mean, pass 1 the
 * metric (reference regularisation, src/hamiltonian.jl:156-158 with the pooled count).  Call pass 0 partials, exchange,
 * consume, then the same for pass 1. */
#define IDHMC_POOL_SEGMENT 1024
int idhmc_pool_partials(idhmc_ctx *ctx, int32_t pass, double *dev_table, int64_t seg_lo, int64_t seg_hi);
int idhmc_pool_consume(idhmc_ctx *ctx, int32_t pass, const double *dev_table, int64_t nseg, double lambda);
/* running posterior moments over draws accumulated with IDHMC_T_ACCUM_MOMENTS */
int idhmc_moments_reset(idhmc_ctx *ctx);
int idhmc_get_moments(idhmc_ctx *ctx, double *mean, double *var, int64_t *count); /* nchains*D each */

/* ---- diagnostics reduced on the device (reference src/diagnostics.jl:28-32, 61-101) -----------------------
 * The reference computes EBFMI and summarize_tree_statistics from the stored TreeStatisticsNUTS records; at 65 536
 * chains the records of a run are N x 2 MiB, so the transition kernel reduces them as it goes (IDHMC_T_ACCUM_DIAG):
 * per chain the running sums EBFMI needs, and for all chains of the context integer counters -- every one an exact
 * integer, so counters of several contexts (ranks) simply add:
 *   [0] transitions  [1], [2] hi / lo limb sums of the acceptance rates (IDHMC_XCHG_ACCEPT fixed point)
 *   [3] REACHED_MAX_DEPTH  [4] divergent  [5] turning  (InvalidTree classes, src/tree.jl:278-300)
 *   [6 .. 6+32] trees of depth 0..32  [39 .. 39+1023] acceptance-rate histogram, 1024 equal bins on [0, 1]
 * idhmc_mcmc adds every draw once idhmc_diag_reset has been called. */
#define IDHMC_DIAG_COUNTERS (39 + 1024)
#define IDHMC_DIAG_ACC_BINS 1024
typedef struct {                    /* reference TreeStatisticsSummary, src/diagnostics.jl:44-55 */
    int64_t N;
    double  a_mean;                 /* exact to 2^-52 per record */
    double  a_quantiles[5];         /* 5/25/50/75/95 %, interpolated inside the histogram bin: within 1/1024 of the sample quantile */
    int64_t max_depth, divergence, turning;
    int64_t depth_counts[33];       /* first element is for depth 0 */
} idhmc_tree_summary;
int idhmc_diag_reset(idhmc_ctx *ctx);
int idhmc_get_diag_counters(idhmc_ctx *ctx, uint64_t *counters);            /* IDHMC_DIAG_COUNTERS values */
/* host only, no context: the summary of (summed) counters */
int idhmc_tree_summary_from_counters(const uint64_t *counters, idhmc_tree_summary *out);
/* EBFMI per chain = mean(abs2, diff(pi)) / var(pi) over the accumulated transitions (src/diagnostics.jl:28-32); NaN for a chain with
 * fewer than two of them (0 / 0, as the reference's formula gives on one record) */
int idhmc_get_ebfmi(idhmc_ctx *ctx, double *ebfmi);                          /* nchains */

/* ---- posterior summaries reduced on the device ------------------------------------------
 * With the draws kept, idhmc_mcmc is bound by the copy into the caller's array; a summary reduces the staged draws where they lie:
 * per group of chains and per reported parameter the pooled mean, variance, minimum, maximum, the number of positive values and a
 * histogram from which idhmc_summary_quantiles reads quantiles.
 *
 * Groups.  Chains are pooled in groups of chains_per_group consecutive GLOBAL chain ids; 0 means the default: chains_per_response of a
 * context of idhmc_create_glm_responses, nchains otherwise.  The context must hold whole groups: first_chain_id and nchains must be
 * multiples of chains_per_group.  Summaries are local to the context: nothing is exchanged between ranks.
 *
 * The reported vector theta has length D.  theta = q, except for a GLM with coefficient groups (H > 0), where
 * theta = [beta (Dx) | a (A, raw) | sigma (H)], sigma_g = exp(omega_g) and beta_c = u_c sigma_grp[c] (u_c itself for an ungrouped
 * column): the bits the density's own evaluation multiplies with X.
 *
 * Running statistics.  Each group's chains are cut into segments of IDHMC_SUMMARY_SEGMENT chains, counted from the group's first
 * chain.  Per (segment, d) the state (n, mean, m2, min, max, pos) starts at (0, 0, 0, +inf, -inf, 0); values are visited transition
 * by transition in the order the transitions happened, ascending chain id inside a transition, across blocks and calls:
 *   n += 1; inv = 1.0 / (double)n; dx = theta - mean; mean = fma(dx, inv, mean); m2 = fma(dx, theta - mean, m2)
 *   min = theta < min ? theta : min (likewise max); pos += theta > 0.0
 * The segments are folded in ascending order from segment 0; for the next segment b with nb > 0:
 *   n = na + nb; delta = mean_b - mean_a; f = (double)nb / (double)n; mean = fma(delta, f, mean_a)
 *   m2 = (m2_a + m2_b) + (delta delta) ((double)na f)
 * and var = m2 / (n - 1), 0.0 when n <= 1.  The bits depend on the segment size, which is why it is public.
 *
 * Histogram (bins > 0 interior bins, at most IDHMC_SUMMARY_BINS_MAX).  Values reduced while no range is set are not binned.
 * idhmc_summary_set_range takes host arrays lo, hi [groups][D] (finite, lo <= hi), or both NULL for the range of what has been
 * accumulated: sd = sqrt(var), lo = fma(-span, sd, mean), hi = fma(span, sd, mean) (needs two values in every group).
 * inv_w = hi > lo ? (double)bins / (hi - lo) : 0.0 is computed once and stored.  The call zeroes the histogram and its count; the moments
 * stay.  A binned value goes to bin 0 if theta < lo, to bin bins + 1 if theta >= hi, to 1 + min((int)((theta - lo) inv_w), bins - 1)
 * otherwise.  Counts are uint32: a call that could take a group's binned count past 2^32 - 1 is refused before it launches.
 *
 * Feeding.  While a summary is open idhmc_mcmc reduces every draw it makes, whether or not draws / stats are NULL; idhmc_tuning_stage
 * (and so the warm-up of idhmc_mcmc_with_warmup) never does.  When idhmc_mcmc fails the summary is invalid: idhmc_get_summary and
 * idhmc_summary_set_range refuse it until idhmc_summary_begin is called again.  idhmc_summary_add_draws reduces cnt host draws
 * [cnt][nchains][D] (draws saved earlier, or a test's) through the same staging buffers and the same kernel.
 *
 * Every refusal is IDHMC_ERR_BAD_ARG with the offending value in idhmc_last_error. */
#define IDHMC_SUMMARY_SEGMENT 256
#define IDHMC_SUMMARY_BINS_MAX 256
int idhmc_summary_begin(idhmc_ctx *ctx, int64_t chains_per_group, int32_t bins);   /* (re)opens: an open summary is discarded */
int idhmc_summary_set_range(idhmc_ctx *ctx, const double *lo, const double *hi, double span);
int idhmc_summary_add_draws(idhmc_ctx *ctx, const double *draws, int64_t cnt);
int idhmc_summary_dims(idhmc_ctx *ctx, int64_t *groups, int64_t *chains_per_group, int32_t *dim, int32_t *bins);
/* n, binned: [groups] values taken / binned per (group, parameter); mean ... inv_w: [groups][D]; counts: [groups][D][bins + 2] (untouched
 * when bins = 0).  lo, hi, inv_w are zero until a range is set.  Any pointer may be NULL. */
int idhmc_get_summary(idhmc_ctx *ctx, int64_t *n, int64_t *binned, double *mean, double *var, double *min, double *max, int64_t *pos,
                      double *lo, double *hi, double *inv_w, uint32_t *counts);
int idhmc_summary_end(idhmc_ctx *ctx);                                             /* frees everything; no summary open: nothing */
/* host only, no context: quantiles of one (group, parameter) from its bins + 2 counts.  With n_h = sum counts, k = clamp(ceil(p n_h), 1, n_h)
 * and j the smallest bin whose cumulative count reaches k: lo if j = 0, hi if j = bins + 1,
 * lo + (j - 1 + (k - cum_{j-1} - 0.5) / c_j) (hi - lo) / bins otherwise; NaN if n_h = 0.  The estimate lies in the bin that holds the
 * k-th order statistic: unless that is an end bin, its error is below one bin width. */
int idhmc_summary_quantiles(const uint32_t *counts, int32_t bins, double lo, double hi, const double *probs, int32_t nprobs, double *out);

/* ---- drivers: the reference's caller loops, run by the library -------------- */
/* warmup!(TuningNUTS) (src/warmup.jl:269-314): N transitions with dual averaging, optional
 * metric update at the end.  draws (host, N*nchains*D) / stats (host, N*nchains) may be NULL.
 * iter0 = number of transitions already made (RNG address continues at iter0+1). */
int idhmc_tuning_stage(idhmc_ctx *ctx, int32_t N, int32_t adapt_metric, uint32_t iter0,
                       double *draws, idhmc_tree_stats *stats);
/* mcmc! (src/warmup.jl:316-332): N transitions at fixed eps.  Fails with the code of any device-side error still pending when it
 * returns -- one raised before the call (a caller's own transition whose eps fell below 1e-10, a refused launch) included: a launch of
 * several transitions starts none while the abort code is set.  The error is reported once and cleared; the chains keep the state
 * they hold, and the next call goes on from it.  When the call fails the contents of draws / stats are unspecified. */
int idhmc_mcmc(idhmc_ctx *ctx, int32_t N, uint32_t iter0, double *draws, idhmc_tree_stats *stats);
/* mcmc_with_warmup! for all chains (src/mcmc.jl:94-105 under threaded_mcmc :130-159):
 * random start, [stepsize search], default_warmup_stages, then N draws.
 * draws: host N*nchains*D or NULL; stats: host N*nchains or NULL. */
int idhmc_mcmc_with_warmup(idhmc_ctx *ctx, int32_t N, double *draws, idhmc_tree_stats *stats);
/* total leapfrog steps taken by NUTS transitions since creation (sum of stats.steps) */
int idhmc_total_steps(idhmc_ctx *ctx, int64_t *steps);

/* ---- measurement helper ------------------------------------------------------
 * `sweeps` back-to-back idhmc_leapfrog(eps, 1) launches bracketed by HIP events on the
 * context's stream; returns the mean kernel+gap time per sweep in milliseconds. */
int idhmc_time_leapfrog(idhmc_ctx *ctx, double eps, int32_t sweeps, float *ms_per_sweep);
int idhmc_time_transitions(idhmc_ctx *ctx, int32_t n, uint32_t iter0, float *ms_total);      /* n idhmc_nuts_transition launches */
int idhmc_time_transitions_fused(idhmc_ctx *ctx, int32_t n, uint32_t iter0, float *ms_total); /* one idhmc_nuts_transitions(n) launch */
/* n times what the drivers enqueue between two adapting transitions to pool the acceptance and adapt the stepsize, bracketed by HIP
 * events: in IDHMC_EPS_GLOBAL the exchange sum, the all-reduce (hook or communicator, if any), the adaptation and the broadcast (three
 * launches), in IDHMC_EPS_PER_RESPONSE the one launch that does all of it per response; refused in IDHMC_EPS_PER_CHAIN, which adapts
 * inside the transition kernel.  It feeds the acceptance rates of the last transition n times: the stepsizes and the dual-averaging
 * state move as after n such transitions (call idhmc_da_init first; a measurement, not a step of any algorithm). */
int idhmc_time_eps_adapt(idhmc_ctx *ctx, int32_t n, float *ms_total);
/* 32 device counters: [0] = total leapfrog steps; [1] = pending abort code; [2..] = per-phase shader-cycle sums of the
 * NUTS kernel, filled only by the diagnostic build (-DIDHMC_STAMPS, tools/stamps.sh), zero otherwise. */
int idhmc_debug_counters(idhmc_ctx *ctx, uint64_t *out32);

#ifdef __cplusplus
}
#endif
#endif
