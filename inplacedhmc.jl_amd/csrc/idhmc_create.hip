// idhmc_create.hip -- a context's life: the argument checks of the creation entry points (every one answers before the
// device is looked for), set-up, idhmc_destroy, the default options and what a context can be asked about itself.
#include "idhmc_host.hpp"
#include "idhmc_members.hpp"

void idhmc_default_options(idhmc_options *o)
{
    if (!o) return;
    o->max_depth = 10;                    // DEFAULT_MAX_TREE_DEPTH, src/tree.jl:2
    o->min_delta = -1000.0;               // src/NUTS.jl:214
    o->da_delta = 0.8; o->da_gamma = 0.05; o->da_kappa = 0.75; o->da_t0 = 10;   // src/stepsize.jl:191
    o->ss_a_min = 0.25; o->ss_a_max = 0.75; o->ss_eps0 = 1.0; o->ss_C = 2.0;    // src/stepsize.jl:29
    o->ss_maxiter_crossing = 400; o->ss_maxiter_bisect = 400;
    o->init_steps = 75; o->middle_steps = 25; o->doubling_stages = 5; o->terminating_steps = 50;  // src/warmup.jl:366
    o->adapt_metric = 1;
    o->stepsize_search = 1;
    o->eps_init = 1.0;
    o->eps_mode = IDHMC_EPS_PER_CHAIN;
    o->metric_mode = IDHMC_METRIC_PER_CHAIN;
    o->local_opt_iterations = 0;          // the FindLocalOptimum stage is opt-in at this level (own optimiser)
    o->leapfrog_grad_mode = IDHMC_GRAD_RECOMPUTE;   // separable densities: 4 streams instead of 6, the same bits
    o->local_opt_penalty = 1e-4;          // src/warmup.jl:143
}

int idhmc_destroy(idhmc_ctx *c)
{
    if (!c) return IDHMC_OK;
    (void)hipSetDevice(c->device);
    for (int k = 1; k < idhmc_ctx::kLanes; ++k) if (c->lane[k]) (void)hipStreamSynchronize(c->lane[k]);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int k = 1; k < idhmc_ctx::kLanes; ++k) {
        if (c->lane[k]) (void)hipStreamDestroy(c->lane[k]);
        if (c->lane_ev[k]) (void)hipEventDestroy(c->lane_ev[k]);
    }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    for (void *p : c->allocs) (void)hipFree(p);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (int b = 0; b < 2; ++b) if (c->ev_packed[b]) (void)hipEventDestroy(c->ev_packed[b]);
    if (c->ring) (void)hipHostFree(c->ring);
    jit_destroy(c->jit);
    comm_destroy(c->comm);
    delete c;
    return IDHMC_OK;
}


// The data of a regression model -- a logistic regression ([X | y] in idhmc_model_desc::params), a GLM packed into params
// ([K, nc, c | X | Y]; with auxiliary coordinates [K, nc, A, c | X | Y]) or handed over in parts (idhmc_create_glm_model;
// a field's comment names the entry its part came with) -- as the one validation and the one upload below read it.  Any other model: the defaults.
struct GlmParts {
    const char *what = "";     // the model's name in messages
    int64_t n = 0;             // observations
    int32_t K = 1, nc = 0;     // data columns of Y, constants
    int32_t A = 0;             // auxiliary coordinates: X has Dx = D - A - H columns, the A coordinates after them are not coefficients
    int32_t H = 0;             // coefficient groups (idhmc_create_glm): the last H coordinates are their log scales
    const double *X = nullptr, *Y = nullptr, *c = nullptr;
    const int32_t *grp = nullptr;        // [Dx], H > 0
    bool responses = false;    // idhmc_create_glm_responses: Y is [M][n][K], global chain g samples response g / R
    int64_t M = 1, R = 0;      // (1, 0 otherwise)
    const int32_t *pkind = nullptr;      // [D] idhmc_create_glm_priors with some kind != 0: the priors' kinds and their nu (never null then)
    const double *pnu = nullptr;
    int32_t J = 0;             // idhmc_create_glm_local: flagged columns; the last J coordinates are the logarithms of their local scales
    const int32_t *local = nullptr;      // [Dx] 0 or 1, J > 0 (never null then)
    double slab = 0.0;         // the slab scale (0: none)
    int32_t F = 0;             // idhmc_create_glm_factors: factors; X holds the Dd = D - A - H - J - fcols dense columns only
    int32_t fcols = 0;         // their level columns, sum N_f
    const int32_t *levels = nullptr, *findex = nullptr;   // [F], [F][n], F > 0 (never null then; every index checked)
    const double *fvalues = nullptr;   // idhmc_create_glm_slopes with a flag set: [F][n] (rows of unflagged terms are not read) and
    const int32_t *fhas = nullptr;     // [F] 0 or 1; both null when no term has values
    int32_t P = 0;             // idhmc_create_glm_corr: pairs of terms; the last P coordinates are their zetas
    const int32_t *pfirst = nullptr, *psecond = nullptr;   // [P] the terms of each pair, P > 0 (never null then; every entry checked)
    const double *peta = nullptr;      // [P]
    const int32_t *pkind_pub = nullptr;    // P > 0 with some eta > 0: kind and nu as the caller gave them (pkind / pnu then hold the
    const double *pnu_pub = nullptr;       // device table, which marks those zetas); null: pkind / pnu are the caller's
    int32_t S = 0, SZ = 0;     // idhmc_create_glm_struct: structured terms, and those of them that are AR(1): the last SZ coordinates, behind
    const int32_t *sterm = nullptr, *skind = nullptr;      // the pairs' zetas, are theirs; [S] term and kind, S > 0 (every entry checked)
    const double *seta = nullptr;      // [S]
    int32_t G = 0;             // idhmc_create_glm_gmrf: GMRF terms; no coordinate is added
    const int32_t *gterm = nullptr, *gcol = nullptr;       // [G], and the entries' columns, G > 0 (never null then; every entry checked)
    const int64_t *gstart = nullptr;   // [sum N + 1]
    const double *gval = nullptr, *gkappa = nullptr;       // the entries' values, [G]
    int32_t BK = 0, BZ = 0;    // idhmc_create_glm_block: the block's terms K and its zetas K (K - 1) / 2, which stand where the pairs' would
    const int32_t *bterm = nullptr;    // [BK] the terms in row order, BK > 0 (never null then; every entry checked)
    double beta = 0.0;         // the block's eta
    int32_t MP = 0;            // idhmc_create_glm_multi with a wide term: the planes, sum of the widths (findex and fvalues are then unused)
    const int32_t *mwidth = nullptr, *mindex = nullptr;    // [F], [MP][n], MP > 0 (never null then; every entry checked)
    const double *mvalues = nullptr;   // [MP][n], or null: 1.0 on every present entry
};
// the padded width of the stored columns of X: L of the model, and with factors Lx = 128 ceil(Dd / 128)
static int64_t stored_width(const GlmParts &g, int D, int64_t *L_out = nullptr)
{
    int64_t L = 128;
    while (L < D) L *= 2;
    if (L_out) *L_out = L;
    return g.F > 0 ? ((int64_t)D - g.A - g.H - g.J - g.P - g.BZ - g.SZ - g.fcols + 127) / 128 * 128 : L;
}
// The head of a packed params array into *g: `head` = 0 (a logistic regression's [X | y]), 2 ([K, nc, c | X | Y]) or 3
// ([K, nc, A, c | X | Y]) doubles in front of the constants.  The entries are checked as doubles (integral, hence finite, and in
// range) before they are converted, and nothing at or past nparams is read: X, Y and c point at exactly the nparams - head doubles
// that follow the head.
static int unpack_params(const idhmc_model_desc *model, int head, GlmParts *g)
{
    const double *p = model->params;
    const int64_t np = model->nparams;
    const int D = model->D;
    const bool aux = head == 3;
    if (head == 0) {            // (K = 1 column, no constants: what follows holds, and fills *g, as for a GLM)
        if (np < 1 || np % (D + 1) != 0 || !p)
            return fail(IDHMC_ERR_BAD_ARG, "logistic regression: nparams = %lld must be a positive multiple of D + 1 = %d ([X | y])", (long long)np, D + 1);
    } else if (np < head || !p)
        return fail(IDHMC_ERR_BAD_ARG, "%s: params must begin with %s ([%s, c | X | Y])", g->what, aux ? "K, nc and A" : "K and nc", aux ? "K, nc, A" : "K, nc");
    static const struct { const char *name; double lo, hi; } kEntry[3] = {{"K", 1.0, 4.0}, {"nc", 0.0, 16.0}, {"A", 1.0, 4.0}};
    int32_t *const v[3] = {&g->K, &g->nc, &g->A};
    for (int i = 0; i < head; ++i) {
        if (!(p[i] >= kEntry[i].lo && p[i] <= kEntry[i].hi && p[i] == std::floor(p[i])))
            return fail(IDHMC_ERR_BAD_ARG, "%s: %s = %g must be an integer in %g..%g", g->what, kEntry[i].name, p[i], kEntry[i].lo, kEntry[i].hi);
        *v[i] = (int32_t)p[i];
    }
    const int64_t Dx = D - g->A;
    if (Dx < 1) return fail(IDHMC_ERR_BAD_ARG, "%s: Dx = D - A = %lld: at least one coefficient is needed", g->what, (long long)Dx);
    const int64_t rest = np - head - g->nc;
    if (rest < 1 || rest % (Dx + g->K) != 0)
        return fail(IDHMC_ERR_BAD_ARG, "%s: nparams - %d - nc = %lld must be a positive multiple of %s + K = %lld ([X | Y])",
                    g->what, head, (long long)rest, aux ? "Dx" : "D", (long long)(Dx + g->K));
    g->n = rest / (Dx + g->K);
    g->c = p + head;
    g->X = g->c + g->nc;
    g->Y = g->X + g->n * Dx;
    return IDHMC_OK;
}
// every check of a regression's data; `glm`: anything but a logistic regression
static int validate_regression(const GlmParts &g, bool glm, const idhmc_model_desc *model, const idhmc_options &opt, int64_t nchains, int64_t first_chain_id)
{
    const char *what = g.what;
    const int D = model->D;
    if (glm) {
        if (g.K < 1 || g.K > 4) return fail(IDHMC_ERR_BAD_ARG, "%s: K = %d must be an integer in 1..4", what, g.K);
        if (g.nc < 0 || g.nc > 16) return fail(IDHMC_ERR_BAD_ARG, "%s: nc = %d must be an integer in 0..16", what, g.nc);
        if (g.n < 1) return fail(IDHMC_ERR_BAD_ARG, "%s: n = %lld: at least one observation is needed", what, (long long)g.n);
        if (!g.X || !g.Y) return fail(IDHMC_ERR_BAD_ARG, "%s: X and Y are needed", what);
        if (g.nc > 0 && !g.c) return fail(IDHMC_ERR_BAD_ARG, "%s: nc = %d constants are needed", what, g.nc);
        for (int j = 0; j < g.nc; ++j)
            if (!std::isfinite(g.c[j])) return fail(IDHMC_ERR_BAD_ARG, "%s: constant c[%d] is not finite", what, j);
    }
    if (g.responses) {
        const int64_t M = g.M, R = g.R;
        if (M < 1) return fail(IDHMC_ERR_BAD_ARG, "%s: M = %lld: at least one response is needed", what, (long long)M);
        if (R < 1) return fail(IDHMC_ERR_BAD_ARG, "%s: chains_per_response = %lld: at least one chain per response is needed", what, (long long)R);
        if ((__int128)first_chain_id + nchains > (__int128)M * R)
            return fail(IDHMC_ERR_BAD_ARG, "%s: first_chain_id + nchains = %lld is past the M * chains_per_response = %lld * %lld chains of the model",
                        what, (long long)(first_chain_id + nchains), (long long)M, (long long)R);
        // both pool statistics over every chain of the context, and the chains of different responses sample different posteriors
        if (M > 1 && opt.eps_mode == IDHMC_EPS_GLOBAL)
            return fail(IDHMC_ERR_BAD_ARG, "%s: M = %lld responses with eps_mode = GLOBAL: the global stepsize pools the acceptance of chains "
                        "that sample different posteriors (use PER_CHAIN)", what, (long long)M);
        if (M > 1 && opt.metric_mode == IDHMC_METRIC_POOLED)
            return fail(IDHMC_ERR_BAD_ARG, "%s: M = %lld responses with metric_mode = POOLED: the pooled metric pools the windows of chains "
                        "that sample different posteriors (use PER_CHAIN or SHARED)", what, (long long)M);
        // pooled per response: rank-local and free of collectives because a context holds whole responses
        if (opt.eps_mode == IDHMC_EPS_PER_RESPONSE || opt.metric_mode == IDHMC_METRIC_PER_RESPONSE) {
            const char *mode = opt.eps_mode == IDHMC_EPS_PER_RESPONSE ? "eps_mode" : "metric_mode";
            if (first_chain_id % R != 0)
                return fail(IDHMC_ERR_BAD_ARG, "%s: first_chain_id = %lld is not a multiple of chains_per_response = %lld: a context with %s = "
                            "PER_RESPONSE holds whole responses", what, (long long)first_chain_id, (long long)R, mode);
            if (nchains % R != 0)
                return fail(IDHMC_ERR_BAD_ARG, "%s: nchains = %lld is not a multiple of chains_per_response = %lld: a context with %s = "
                            "PER_RESPONSE holds whole responses", what, (long long)nchains, (long long)R, mode);
        }
    }
    const int64_t n = g.n, K = g.K, M = g.M;
    const int64_t Dx = D - g.A - g.H - g.J - g.P - g.BZ - g.SZ - g.fcols;      // the columns of X (with factors: the dense ones)
    const int64_t L = stored_width(g, D);
    const int64_t npad = (n + 127) / 128 * 128;
    if (npad * L > ((int64_t)1 << 27))
        return fail(IDHMC_ERR_BAD_ARG, "%s: n = %lld observations at D = %d exceed n_pad * %s <= 2^27 (at most %lld)",
                    what, (long long)n, D, g.F > 0 ? "Lx" : "L", (long long)((((int64_t)1 << 27) / L) / 128 * 128));
    if (M > ((int64_t)1 << 27) || M * K * npad > ((int64_t)1 << 27))
        return fail(IDHMC_ERR_BAD_ARG, "%s: M = %lld responses of K = %lld columns and n = %lld observations exceed M * K * n_pad <= 2^27",
                    what, (long long)M, (long long)K, (long long)n);
    for (int64_t k = 0; k < n * Dx; ++k)
        if (!std::isfinite(g.X[k])) return fail(IDHMC_ERR_BAD_ARG, "%s: X[%lld, %lld] is not finite", what, (long long)(k / Dx), (long long)(k % Dx));
    if (glm) {
        for (int64_t k = 0; k < n * K; ++k)
            if (!std::isfinite(g.Y[k]))
                return fail(IDHMC_ERR_BAD_ARG, "%s: Y[%lld, %lld] is not finite", what, (long long)(k / K), (long long)(k % K));
        for (int64_t k = n * K; k < M * n * K; ++k)           // the further responses' planes
            if (!std::isfinite(g.Y[k]))
                return fail(IDHMC_ERR_BAD_ARG, "%s: Y[%lld, %lld, %lld] is not finite", what, (long long)(k / (n * K)),
                            (long long)(k / K % n), (long long)(k % K));
    } else {
        for (int64_t i = 0; i < n; ++i)
            if (g.Y[i] != 0.0 && g.Y[i] != 1.0) return fail(IDHMC_ERR_BAD_ARG, "logistic regression: y[%lld] = %g is neither 0 nor 1", (long long)i, g.Y[i]);
    }
    for (int k = 0; k < D; ++k) {
        if (model->tau && !(std::isfinite(model->tau[k]) && model->tau[k] > 0.0))
            return fail(IDHMC_ERR_BAD_ARG, "%s: prior precision tau[%d] = %g must be finite and > 0", what, k, model->tau[k]);
        if (model->mu && !std::isfinite(model->mu[k]))
            return fail(IDHMC_ERR_BAD_ARG, "%s: prior mean mu[%d] is not finite", what, k);
    }
    if (D > 512 && opt.metric_mode == IDHMC_METRIC_PER_CHAIN)
        return fail(IDHMC_ERR_BAD_ARG, "%s with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)", what);
    if (D > 512 && opt.metric_mode == IDHMC_METRIC_PER_RESPONSE)
        return fail(IDHMC_ERR_BAD_ARG, "%s with D = %d > 512 and metric_mode = PER_RESPONSE: the per-response metric is stored per chain and "
                    "shares the per-chain metric's LDS budget of the NUTS kernel (use SHARED)", what, D);
    return IDHMC_OK;
}
// X, X' and the K planes of Y zero-padded to [n_pad][L], [L][n_pad], [K][n_pad] (one set of planes per response, [M][K][n_pad]);
// a GLM's constants and groups
static int upload_regression(idhmc_ctx *c, const GlmParts &g, bool glm)
{
    DevState &s = c->s;
    const int64_t n = g.n, npad = (n + 127) / 128 * 128, L = s.L, Dm = s.D - g.A - g.H - g.J - g.P - g.BZ - g.SZ, K = g.K, M = g.M;    // Dm: the columns of the model
    const int64_t D = Dm - g.fcols, LX = stored_width(g, s.D);      // the columns X stores (with factors: the dense ones) and their padded width
    // The level lists of a model with factors, before anything is uploaded: per block of 128 observations its places sorted by factor,
    // level, place (a counting sort), and where each level's list starts
    const int64_t cols = g.fcols;
    Planes pl;                             // a plain term is one plane; a wide term (g.MP > 0) one per level an observation can have in it
    LevelLists ll;
    const bool fvalued = g.fhas || g.MP > 0;      // every plane reads a value
    if (g.F > 0) {
        for (int f = 0; f < g.F; ++f)
            for (int m = 0; m < (g.MP > 0 ? g.mwidth[f] : 1); ++m, ++pl.P) {
                pl.term[pl.P] = f;
                if (g.MP > 0) {
                    pl.idx[pl.P] = g.mindex + (int64_t)pl.P * n;
                    pl.val[pl.P] = g.mvalues ? g.mvalues + (int64_t)pl.P * n : nullptr;
                } else {
                    pl.idx[pl.P] = g.findex + (int64_t)f * n;
                    pl.val[pl.P] = g.fhas && g.fhas[f] ? g.fvalues + (int64_t)f * n : nullptr;
                }
            }
        // (a wide model's plane table, eight entries, stands behind the starts: filled in below, once the offsets are known)
        build_level_lists(pl, g.F, g.levels, n, fvalued, g.MP > 0 ? kMaxPlanes : 0, &ll);
    }
    std::vector<int32_t> &hfidx = ll.fidx, &hfstart = ll.fstart;
    std::vector<unsigned char> &hfpos = ll.fpos;
    std::vector<double> &hfval = ll.fval, &hfwl = ll.fwl;
    std::vector<double> hx((size_t)(npad * LX), 0.0), hxt((size_t)(npad * LX), 0.0), hy((size_t)(M * K * npad), 0.0);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 0; k < D; ++k) {
            const double v = g.X[i * D + k];
            hx[(size_t)(i * LX + k)] = v;
            hxt[(size_t)(k * npad + i)] = v;
        }
    for (int64_t m = 0; m < M; ++m)
        for (int64_t i = 0; i < n; ++i)
            for (int64_t k = 0; k < K; ++k) hy[(size_t)((m * K + k) * npad + i)] = g.Y[(m * n + i) * K + k];
    double *dx = nullptr, *dxt = nullptr, *dy = nullptr;
    if (int rc = dalloc(c, &dx, npad * LX)) return rc;
    if (int rc = dalloc(c, &dxt, npad * LX)) return rc;
    if (int rc = dalloc(c, &dy, M * K * npad)) return rc;
    if (glm) {
        double *dc = nullptr;
        if (int rc = dalloc(c, &dc, g.nc > 0 ? g.nc : 1)) return rc;
        if (g.nc > 0) HIPCHK(hipMemcpyAsync(dc, g.c, sizeof(double) * (size_t)g.nc, hipMemcpyHostToDevice, c->stream));
        s.user_params = dc;
        s.user_nparams = g.nc;
    }
    HIPCHK(hipMemcpyAsync(dx, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dxt, hxt.data(), sizeof(double) * hxt.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dy, hy.data(), sizeof(double) * hy.size(), hipMemcpyHostToDevice, c->stream));
    std::vector<int32_t> hg;
    if (g.H > 0) {
        // the group of every coordinate: -1 past the columns of X (auxiliary coordinates, log scales, padding)
        hg.assign((size_t)L, -1);
        for (int64_t k = 0; k < Dm; ++k) hg[(size_t)k] = g.grp[k];
        int32_t *dg = nullptr;
        if (int rc = dalloc(c, &dg, L)) return rc;
        HIPCHK(hipMemcpyAsync(dg, hg.data(), sizeof(int32_t) * hg.size(), hipMemcpyHostToDevice, c->stream));
        s.lr_grp = dg;
    }
    std::vector<int32_t> hk;
    std::vector<double> hnu;
    if (g.pkind) {
        // the prior of every coordinate: kind 0 (and nu 0) past the sampled ones
        const int64_t Dall = s.D;
        hk.assign((size_t)L, 0);
        hnu.assign((size_t)L, 0.0);
        for (int64_t k = 0; k < Dall; ++k) { hk[(size_t)k] = g.pkind[k]; hnu[(size_t)k] = g.pnu[k]; }
        int32_t *dk = nullptr;
        double *dnu = nullptr;
        if (int rc = dalloc(c, &dk, L)) return rc;
        if (int rc = dalloc(c, &dnu, L)) return rc;
        HIPCHK(hipMemcpyAsync(dk, hk.data(), sizeof(int32_t) * hk.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dnu, hnu.data(), sizeof(double) * hnu.size(), hipMemcpyHostToDevice, c->stream));
        s.lr_pkind = dk;
        s.lr_pnu = dnu;
        const int32_t *pk = g.pkind_pub ? g.pkind_pub : g.pkind;
        const double *pn = g.pkind_pub ? g.pnu_pub : g.pnu;
        c->prior_kind.assign(pk, pk + Dall);
        c->prior_nu.assign(pn, pn + Dall);
    }
    std::vector<int32_t> hp;
    if (g.J > 0) {
        // the partner of every coordinate: the k-th flagged column (ascending) and coordinate Dx + A + H + k name each other
        hp.assign((size_t)L, -1);
        int64_t k = s.D - g.SZ - g.P - g.BZ - g.J;
        for (int64_t col = 0; col < Dm; ++col)
            if (g.local[col]) { hp[(size_t)col] = (int32_t)k; hp[(size_t)k] = (int32_t)col; ++k; }
        int32_t *dp = nullptr;
        if (int rc = dalloc(c, &dp, L)) return rc;
        HIPCHK(hipMemcpyAsync(dp, hp.data(), sizeof(int32_t) * hp.size(), hipMemcpyHostToDevice, c->stream));
        s.lr_lpart = dp;
        s.lr_j = g.J;
        s.lr_inv2 = g.slab > 0.0 ? 1.0 / (g.slab * g.slab) : 0.0;
        c->glm_local.assign(g.local, g.local + Dm);
        c->slab_scale = g.slab;
    }
    if (g.F > 0) {
        int32_t *di = nullptr, *ds = nullptr;
        unsigned char *dp = nullptr;
        if (g.MP > 0) {
            // the first column of the term each plane belongs to (planes past the last repeat it: the table is read inside its eight entries)
            int32_t toff[4], o = (int32_t)D;
            for (int f = 0; f < g.F; o += g.levels[f], ++f) toff[f] = o;
            for (int p = 0; p < kMaxPlanes; ++p) hfstart[hfstart.size() - kMaxPlanes + p] = toff[pl.term[p < pl.P ? p : pl.P - 1]];
        }
        if (int rc = dalloc(c, &di, (int64_t)hfidx.size())) return rc;
        if (int rc = dalloc(c, &ds, (int64_t)hfstart.size())) return rc;
        if (int rc = dalloc(c, &dp, (int64_t)hfpos.size())) return rc;
        HIPCHK(hipMemcpyAsync(di, hfidx.data(), sizeof(int32_t) * hfidx.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(ds, hfstart.data(), sizeof(int32_t) * hfstart.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dp, hfpos.data(), hfpos.size(), hipMemcpyHostToDevice, c->stream));
        s.lr_f = g.F;
        s.lr_fidx = di; s.lr_fstart = ds; s.lr_fpos = dp;
        s.lr_dd = (int32_t)D; s.lr_lx = (int32_t)LX; s.lr_fcols = (int32_t)cols;
        int32_t off = (int32_t)D;
        for (int f = 0; f < 4; ++f) {
            s.lr_foff[f] = off;
            if (f < g.F) off += g.levels[f];
        }
        c->glm_flevels.assign(g.levels, g.levels + g.F);
        if (g.MP > 0) {
            // (idhmc_glm_factors_get reports the first plane of every term)
            s.lr_mp = g.MP;
            c->glm_mwidth.assign(g.mwidth, g.mwidth + g.F);
            c->glm_mindex.assign(g.mindex, g.mindex + (int64_t)g.MP * n);
            if (g.mvalues) c->glm_mvalues.assign(g.mvalues, g.mvalues + (int64_t)g.MP * n);
            for (int p = 0; p < pl.P; ++p)
                if (p == 0 || pl.term[p] != pl.term[p - 1]) c->glm_findex.insert(c->glm_findex.end(), pl.idx[p], pl.idx[p] + n);
            double *dv = nullptr, *dw = nullptr;
            if (int rc = dalloc(c, &dv, (int64_t)hfval.size())) return rc;
            if (int rc = dalloc(c, &dw, (int64_t)hfwl.size())) return rc;
            HIPCHK(hipMemcpyAsync(dv, hfval.data(), sizeof(double) * hfval.size(), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(dw, hfwl.data(), sizeof(double) * hfwl.size(), hipMemcpyHostToDevice, c->stream));
            s.lr_fval = dv; s.lr_fwl = dw;
        } else {
            c->glm_findex.assign(g.findex, g.findex + (int64_t)g.F * n);
        }
        if (g.fhas && g.MP == 0) {
            double *dv = nullptr, *dw = nullptr;
            if (int rc = dalloc(c, &dv, (int64_t)hfval.size())) return rc;
            if (int rc = dalloc(c, &dw, (int64_t)hfwl.size())) return rc;
            HIPCHK(hipMemcpyAsync(dv, hfval.data(), sizeof(double) * hfval.size(), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(dw, hfwl.data(), sizeof(double) * hfwl.size(), hipMemcpyHostToDevice, c->stream));
            s.lr_fval = dv; s.lr_fwl = dw;
            c->glm_fhas.assign(g.fhas, g.fhas + g.F);
            c->glm_fvalues.assign((size_t)((int64_t)g.F * n), 0.0);
            for (int f = 0; f < g.F; ++f) {
                if (!g.fhas[f]) continue;
                s.lr_fhas |= 1u << f;
                std::copy(g.fvalues + (int64_t)f * n, g.fvalues + (int64_t)(f + 1) * n, c->glm_fvalues.begin() + (int64_t)f * n);
            }
        }
    }
    std::vector<int32_t> hcp;
    if (g.P > 0) {
        // the partner of every paired column: level k of the first term and level k of the second name each other
        hcp.assign((size_t)L, -1);
        for (int p = 0; p < g.P; ++p) {
            const int32_t o1 = s.lr_foff[g.pfirst[p]], o2 = s.lr_foff[g.psecond[p]];
            for (int32_t k = 0; k < g.levels[g.pfirst[p]]; ++k) {
                hcp[(size_t)(o1 + k)] = (o2 + k) | (p << 10);
                hcp[(size_t)(o2 + k)] = (o1 + k) | (p << 10) | 2048;
            }
        }
        int32_t *dcp = nullptr;
        if (int rc = dalloc(c, &dcp, L)) return rc;
        HIPCHK(hipMemcpyAsync(dcp, hcp.data(), sizeof(int32_t) * hcp.size(), hipMemcpyHostToDevice, c->stream));
        s.lr_cpart = dcp;
        s.lr_cp = g.P;
        c->glm_pfirst.assign(g.pfirst, g.pfirst + g.P);
        c->glm_psecond.assign(g.psecond, g.psecond + g.P);
        c->glm_peta.assign(g.peta, g.peta + g.P);
    }
    std::vector<int32_t> hbp;
    if (g.BK > 0) {
        // the level and the row of every column of a block term; row r is term bterm[r]
        hbp.assign((size_t)L, -1);
        for (int r = 0; r < g.BK; ++r) {
            const int32_t o = s.lr_foff[g.bterm[r]];
            for (int32_t k = 0; k < g.levels[g.bterm[r]]; ++k) hbp[(size_t)(o + k)] = k | (r << 10);
            s.lr_boff[r] = o;
        }
        for (int r = g.BK; r < 4; ++r) s.lr_boff[r] = s.lr_boff[0];
        int32_t *dbp = nullptr;
        if (int rc = dalloc(c, &dbp, L)) return rc;
        HIPCHK(hipMemcpyAsync(dbp, hbp.data(), sizeof(int32_t) * hbp.size(), hipMemcpyHostToDevice, c->stream));
        s.lr_bpart = dbp;
        s.lr_bk = g.BK;
        c->glm_bterm.assign(g.bterm, g.bterm + g.BK);
        c->glm_beta = g.beta;
    }
    std::vector<int32_t> hsp;
    if (g.S > 0) {
        // the level of every column of a structured term and its slot; the AR(1) slots' zetas are the last coordinates, in list order
        hsp.assign((size_t)L, -1);
        int z = 0;
        for (int i = 0; i < g.S; ++i) {
            const int32_t o = s.lr_foff[g.sterm[i]], N = g.levels[g.sterm[i]];
            for (int32_t k = 0; k < N; ++k) hsp[(size_t)(o + k)] = k | (i << 10);
            s.lr_sn[i] = N;
            s.lr_skind[i] = g.skind[i];
            s.lr_scz[i] = g.skind[i] == IDHMC_STRUCT_AR1 ? (int32_t)(s.D - g.SZ + z++) : -1;
        }
        int32_t *dsp = nullptr;
        if (int rc = dalloc(c, &dsp, L)) return rc;
        HIPCHK(hipMemcpyAsync(dsp, hsp.data(), sizeof(int32_t) * hsp.size(), hipMemcpyHostToDevice, c->stream));
        s.lr_spart = dsp;
        s.lr_s = g.S;
        s.lr_sz = g.SZ;
        c->glm_sterm.assign(g.sterm, g.sterm + g.S);
        c->glm_skind.assign(g.skind, g.skind + g.S);
        c->glm_seta.assign(g.seta, g.seta + g.S);
    }
    std::vector<int32_t> hgp, hgs, hgc;
    if (g.G > 0) {
        // the level of every column of a GMRF term and its slot; the tables of the slots one behind the other, start as int32
        hgp.assign((size_t)L, -1);
        int64_t rows = 0;
        for (int i = 0; i < g.G; ++i) {
            const int32_t o = s.lr_foff[g.gterm[i]], N = g.levels[g.gterm[i]];
            for (int32_t k = 0; k < N; ++k) hgp[(size_t)(o + k)] = k | (i << 10);
            s.lr_go[i] = o;
            s.lr_gn[i] = N;
            s.lr_gkappa[i] = g.gkappa[i];
            s.lr_gnz[i] = (int32_t)(g.gstart[rows + N] - g.gstart[rows]);
            rows += N;
        }
        const int64_t nnz = g.gstart[rows];
        hgs.assign(g.gstart, g.gstart + rows + 1);           // (at most 2 * 1024 * 128 entries)
        hgc.assign(g.gcol, g.gcol + nnz);
        int32_t *dgp = nullptr, *dgs = nullptr, *dgc = nullptr;
        double *dgv = nullptr;
        if (int rc = dalloc(c, &dgp, L)) return rc;
        if (int rc = dalloc(c, &dgs, rows + 1)) return rc;
        if (int rc = dalloc(c, &dgc, nnz)) return rc;
        if (int rc = dalloc(c, &dgv, nnz)) return rc;
        HIPCHK(hipMemcpyAsync(dgp, hgp.data(), sizeof(int32_t) * hgp.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dgs, hgs.data(), sizeof(int32_t) * hgs.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dgc, hgc.data(), sizeof(int32_t) * hgc.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dgv, g.gval, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
        s.lr_gpart = dgp; s.lr_gstart = dgs; s.lr_gcol = dgc; s.lr_gval = dgv;
        s.lr_g = g.G;
        c->glm_gterm.assign(g.gterm, g.gterm + g.G);
        c->glm_gkappa.assign(g.gkappa, g.gkappa + g.G);
    }
    HIPCHK(hipStreamSynchronize(c->stream));     // the host copies go out of scope here
    s.lr_x = dx; s.lr_xt = dxt; s.lr_y = dy;
    s.lr_n = (int32_t)n; s.lr_npad = (int32_t)npad;
    return IDHMC_OK;
}
// every switch the library takes from the environment, read once per context (tests and measurements set them before they
// create one; nothing reads the environment on the launch path)
static void read_environment(idhmc_ctx *c)
{
    if (const char *w = getenv("IDHMC_FUSE")) c->fuse = atoi(w) != 0;
    if (const char *w = getenv("IDHMC_TEST_XCC_MISMATCH")) c->test_xcc = atoi(w) != 0;
    if (const char *w = getenv("IDHMC_DENSE_MFMA")) c->dense_mfma = w[0] != '0';
    if (const char *w = getenv("IDHMC_DENSE_LANES")) c->use_lanes = atoi(w) < idhmc_ctx::kLanes ? atoi(w) : idhmc_ctx::kLanes;
    if (const char *w = getenv("IDHMC_PLACEMENT_TRIES")) c->place.tries = atoi(w);
    if (const char *w = getenv("IDHMC_PLACEMENT_MAX_BYTES")) c->place.max_bytes = atoll(w);
    if (const char *w = getenv("IDHMC_PLACEMENT_WALK_BYTES")) c->place.walk_bytes = atoll(w);
    if (const char *w = getenv("IDHMC_PLACEMENT_PAIRS")) c->place.pairs = w[0] != '0';
    c->place.verbose = getenv("IDHMC_PLACEMENT_VERBOSE") != nullptr;
}
#define DALLOC(ptr, n)                                       \
    do {                                                     \
        if (int rc_ = dalloc(c, &(ptr), (n))) return rc_;    \
    } while (0)
// idhmc_create and idhmc_create_glm: one validation, one set-up.  `parts`: a GLM handed over in parts (else its data is in params)
static int create_context(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                          const idhmc_model_desc *model, const idhmc_options *opt_in, uint64_t seed, const GlmParts *parts)
{
    *out = nullptr;
    idhmc_options opt;
    if (opt_in) opt = *opt_in; else idhmc_default_options(&opt);
    if (nchains < 1 || nchains > (int64_t)0x7fffffff) return fail(IDHMC_ERR_BAD_ARG, "nchains = %lld out of range", (long long)nchains);
    if (first_chain_id < 0 || first_chain_id + nchains > (int64_t)0xffffffffll) return fail(IDHMC_ERR_BAD_ARG, "chain ids must fit 32 bits");
    if (model->D < 1 || model->D > 2048) return fail(IDHMC_ERR_BAD_ARG, "D = %d unsupported (1..2048)", model->D);
    // a GLM with auxiliary coordinates is a GLM to everything below but the parsing of its params and the choice of its kernels
    const bool glm_aux = model->kind == IDHMC_MODEL_GLM_AUX;
    const int kind = glm_aux ? (int)IDHMC_MODEL_GLM : model->kind;
    if (model->D > 1024) {
        // two register tiles per vector; the dense MVN's matrix (32 MB at D = 2048) has no kernel built for it
        if (kind == IDHMC_MODEL_DENSE_MVN)
            return fail(IDHMC_ERR_BAD_ARG, "D = %d: the dense density is limited to D <= 1024", model->D);
        if (kind == IDHMC_MODEL_LOGISTIC_REGRESSION)
            return fail(IDHMC_ERR_BAD_ARG, "D = %d: logistic regression is limited to D <= 1024", model->D);
        if (kind == IDHMC_MODEL_GLM)
            return fail(IDHMC_ERR_BAD_ARG, "D = %d: a GLM is limited to D <= 1024", model->D);
    }
    if (opt_in && (opt_in->metric_mode < 0 || opt_in->metric_mode > IDHMC_METRIC_PER_RESPONSE)) return fail(IDHMC_ERR_BAD_ARG, "unknown metric_mode %d", opt_in->metric_mode);
    // one stepsize / one metric per response: only a context with responses has any
    if (opt.eps_mode == IDHMC_EPS_PER_RESPONSE && !(parts && parts->responses))
        return fail(IDHMC_ERR_BAD_ARG, "eps_mode = %d (PER_RESPONSE) needs a context made by idhmc_create_glm_responses", opt.eps_mode);
    if (opt.metric_mode == IDHMC_METRIC_PER_RESPONSE && !(parts && parts->responses))
        return fail(IDHMC_ERR_BAD_ARG, "metric_mode = %d (PER_RESPONSE) needs a context made by idhmc_create_glm_responses", opt.metric_mode);
    if (kind < 0 || kind > IDHMC_MODEL_GLM_AUX) return fail(IDHMC_ERR_BAD_ARG, "unknown model kind %d", model->kind);
    if (kind == IDHMC_MODEL_CUSTOM) {
        if (!model->source || !model->source[0]) return fail(IDHMC_ERR_BAD_ARG, "custom model needs HIP source");
        if (model->nparams < 0 || (model->nparams > 0 && !model->params)) return fail(IDHMC_ERR_BAD_ARG, "custom model: bad params");
        if (model->D > 512 && opt.metric_mode == IDHMC_METRIC_PER_CHAIN)
            return fail(IDHMC_ERR_BAD_ARG, "custom model with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)");
    } else if (kind != IDHMC_MODEL_ISO_GAUSSIAN && kind != IDHMC_MODEL_LOGISTIC_REGRESSION && kind != IDHMC_MODEL_GLM &&
               !model->mu) {
        return fail(IDHMC_ERR_BAD_ARG, "model needs mu");
    }
    const bool glm = kind == IDHMC_MODEL_GLM, regression = glm || kind == IDHMC_MODEL_LOGISTIC_REGRESSION;
    GlmParts g = parts ? *parts : GlmParts{};
    if (regression) {
        g.what = glm_aux ? "GLM_AUX" : glm ? "GLM" : "logistic regression";
        if (glm && (!model->source || !model->source[0])) return fail(IDHMC_ERR_BAD_ARG, "GLM needs HIP source (glm_observation)");
        if (!parts) { if (int rc = unpack_params(model, glm_aux ? 3 : glm ? 2 : 0, &g)) return rc; }
        if (int rc = validate_regression(g, glm, model, opt, nchains, first_chain_id)) return rc;
    }
    if (kind == IDHMC_MODEL_DIAG_GAUSSIAN && !model->tau) return fail(IDHMC_ERR_BAD_ARG, "diagonal model needs tau");
    if (kind == IDHMC_MODEL_DENSE_MVN && !model->prec) return fail(IDHMC_ERR_BAD_ARG, "dense model needs prec");
    if (kind == IDHMC_MODEL_DENSE_MVN) {
        // the gradient kernel reads row c of P as column c (coalesced): P must be exactly symmetric
        const int D = model->D;
        for (int r = 0; r < D; ++r)
            for (int c2 = r + 1; c2 < D; ++c2)
                if (model->prec[(size_t)r * D + c2] != model->prec[(size_t)c2 * D + r])
                    return fail(IDHMC_ERR_BAD_ARG, "prec must be exactly symmetric (differs at [%d,%d]); pass (P+P')/2", r, c2);
        if (D > 512 && opt.metric_mode == IDHMC_METRIC_PER_CHAIN)
            return fail(IDHMC_ERR_BAD_ARG, "dense model with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)");
    }
    if (opt.max_depth < 1 || opt.max_depth > 15) return fail(IDHMC_ERR_BAD_ARG, "max_depth = %d unsupported (1..15)", opt.max_depth);
    if (!(opt.min_delta < 0)) return fail(IDHMC_ERR_BAD_ARG, "min_delta must be negative");
    if (!(opt.eps_init > 0)) return fail(IDHMC_ERR_BAD_ARG, "eps_init must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(IDHMC_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(IDHMC_ERR_BAD_ARG, "device %d out of range (%d visible)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));

    // the context is the guard's until it is the caller's: every return below frees it and all it has allocated
    struct Destroy { void operator()(idhmc_ctx *p) const { (void)idhmc_destroy(p); } };
    std::unique_ptr<idhmc_ctx, Destroy> guard(new (std::nothrow) idhmc_ctx());
    idhmc_ctx *c = guard.get();
    if (!c) return fail(IDHMC_ERR_ALLOC, "out of host memory");
    c->device = device;
    c->opt = opt;
    hipError_t se = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (se != hipSuccess) return fail(IDHMC_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(se));
    c->stream = c->own_stream;
    (void)hipEventCreate(&c->ev0);
    (void)hipEventCreate(&c->ev1);
    read_environment(c);

    DevState &s = c->s;
    s.C = nchains;
    s.D = model->D;
    // a vector is padded to the next multiple of 128 (the reference pads to its SIMD width, src/mcmc.jl:117); the
    // dense density's matrix kernels need a power-of-two number of 128-column chunks
    int nch = (model->D + 127) / 128;
    if (kind == IDHMC_MODEL_DENSE_MVN || regression) {
        nch = 1;
        while (nch * 128 < model->D) nch *= 2;
    }
    s.nch = nch;
    s.L = 128 * nch;
    s.model = kind;               // a GLM_AUX runs as a GLM with lr_a > 0
    s.lr_a = g.A;
    s.lr_h = g.H;
    s.lr_m = (int32_t)g.M;
    s.lr_r = g.responses ? (uint32_t)(g.R > (int64_t)0xffffffffll ? (int64_t)0xffffffffll : g.R) : 0u;
    c->glm_r = g.responses ? g.R : 0;
    s.k0 = (uint32_t)seed;
    s.k1 = (uint32_t)(seed >> 32);
    s.first_chain = (uint32_t)first_chain_id;
    s.max_depth = opt.max_depth;
    s.min_delta = opt.min_delta;
    s.da_delta = opt.da_delta; s.da_gamma = opt.da_gamma; s.da_kappa = opt.da_kappa; s.da_t0 = opt.da_t0;
    s.eps_mode = opt.eps_mode;
    s.ss_a_min = opt.ss_a_min; s.ss_a_max = opt.ss_a_max; s.ss_eps0 = opt.ss_eps0; s.ss_C = opt.ss_C;
    s.ss_maxiter_crossing = opt.ss_maxiter_crossing; s.ss_maxiter_bisect = opt.ss_maxiter_bisect;

    const int64_t CL = nchains * s.L;
    // the dense leapfrog's matrix-core kernel reads whole 32-chain tiles: rows past the last chain exist (zeros), see kRowPad
    const int64_t CLp = CL + (kind == IDHMC_MODEL_DENSE_MVN ? (int64_t)kRowPad * s.L : 0);
    // (the per-response metric lives in the per-chain layout: the R rows of a response hold the same values)
    const bool own_minv = opt.metric_mode == IDHMC_METRIC_PER_CHAIN || opt.metric_mode == IDHMC_METRIC_PER_RESPONSE;
    {
        double *sv[4] = {nullptr, nullptr, nullptr, nullptr};
        if (int rc = place_state(c, sv, own_minv ? 4 : 3, CLp, nchains, s.L)) return rc;
        s.q = sv[0]; s.p = sv[1]; s.g = sv[2];
        if (own_minv) s.minv = sv[3];
    }
    s.lf_stride = (3 * CL * (int64_t)sizeof(double) + kIcSliceBytes - 1) / kIcSliceBytes;
    if (s.lf_stride < 1) s.lf_stride = 1;
    s.lf_stride2 = (2 * CL * (int64_t)sizeof(double) + kIcSliceBytes - 1) / kIcSliceBytes;
    if (s.lf_stride2 < 1) s.lf_stride2 = 1;
    DALLOC(s.lq, nchains); DALLOC(s.pi, nchains); DALLOC(s.eps, nchains);
    if (own_minv) {
        DALLOC(s.w, CL);
        s.minv_stride = s.L;
        DALLOC(s.mw_x1, CL); DALLOC(s.mw_s1, CL); DALLOC(s.mw_s2, CL);
    } else {
        DALLOC(s.minv, s.L); DALLOC(s.w, s.L);
        s.minv_stride = 0;
        if (opt.metric_mode == IDHMC_METRIC_POOLED) {       // one M^-1, adapted from every chain's window
            DALLOC(s.mw_x1, CL); DALLOC(s.mw_s1, CL); DALLOC(s.mw_s2, CL);
            DALLOC(c->pool_scratch, (int64_t)pool_scratch_doubles(s.L));
        }
    }
    DALLOC(s.mw_n, nchains);
    DALLOC(s.stats, nchains);
    DALLOC(s.directions, nchains);
    DALLOC(s.queue, 16);
    DALLOC(s.iters_done, nchains);
    DALLOC(s.da.mu, nchains); DALLOC(s.da.Hbar, nchains); DALLOC(s.da.logeps, nchains);
    DALLOC(s.da.logeps_bar, nchains); DALLOC(s.da.m, nchains);
    DALLOC(s.da_global, 8);
    if (opt.eps_mode == IDHMC_EPS_PER_RESPONSE || opt.metric_mode == IDHMC_METRIC_PER_RESPONSE) c->resp_n = nchains / g.R;
    if (opt.eps_mode == IDHMC_EPS_PER_RESPONSE) DALLOC(c->resp_da, 6 * c->resp_n);
    DALLOC(s.xchg_acc, 3 * kXchgBlocks + 1);
    DALLOC(s.status, nchains);
    DALLOC(s.total_steps, 32);
    DALLOC(c->xchg, IDHMC_XCHG_DOUBLES);
    DALLOC(c->status_out, 1);
    {
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&c->ring), sizeof(unsigned long long) * idhmc_ctx::kRing * idhmc_ctx::kPulseWords,
                                     hipHostMallocDefault);
        if (e != hipSuccess) return fail(IDHMC_ERR_ALLOC, "pinned ring: %s", hipGetErrorString(e));
        for (int i = 0; i < idhmc_ctx::kRing * idhmc_ctx::kPulseWords; ++i) c->ring[i] = ~0ull;
        {   // several transitions per launch need workgroups b and b + 8 on one XCD (idhmc_nuts_kernel.hpp): look before relying on it
            const int g8 = prop.multiProcessorCount > 8 ? prop.multiProcessorCount : 8;
            uint32_t *dx = nullptr;
            std::vector<uint32_t> hx((size_t)g8, 0u);
            bool ok = hipMalloc(&dx, sizeof(uint32_t) * g8) == hipSuccess;
            ok = ok && launch_xcc_probe(dx, g8, c->stream) == hipSuccess;
            ok = ok && hipMemcpyAsync(hx.data(), dx, sizeof(uint32_t) * g8, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
            ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
            for (int b = 8; ok && b < g8; ++b) ok = hx[(size_t)b] == hx[(size_t)(b & 7)];
            if (dx) (void)hipFree(dx);
            c->fuse_ok = ok;
        }
    }
    // model parameters, padded with zeros
    {
        double *mu = nullptr, *tau = nullptr, *prec = nullptr;
        DALLOC(mu, s.L); DALLOC(tau, s.L);
        if (model->mu) HIPCHK(hipMemcpyAsync(mu, model->mu, sizeof(double) * s.D, hipMemcpyHostToDevice, c->stream));
        if (model->tau) HIPCHK(hipMemcpyAsync(tau, model->tau, sizeof(double) * s.D, hipMemcpyHostToDevice, c->stream));
        if (kind == IDHMC_MODEL_DENSE_MVN) {
            DALLOC(prec, (int64_t)s.L * s.L);
            HIPCHK(hipMemcpy2DAsync(prec, sizeof(double) * s.L, model->prec, sizeof(double) * s.D,
                                    sizeof(double) * s.D, s.D, hipMemcpyHostToDevice, c->stream));
        }
        s.mu = mu; s.tau = tau; s.prec = prec;
        if (regression) {
            // the prior's defaults (mu = 0 is the zeroed allocation), then the data
            if (!model->tau) HIPCHK(launch_fill(tau, 1.0, s.D, c->stream));
            if (int rc = upload_regression(c, g, glm)) return rc;
        }
    }
    // persistent NUTS waves and their tree arenas
    {
        // one workgroup of W wavefronts per CU (nuts_waves); slots in multiples of W
        const int W = nuts_waves_per_block(s.nch, s.model, !own_minv, s.lr_a);
        int64_t nslots = (int64_t)prop.multiProcessorCount * W;
        const int64_t need = (nchains + W - 1) / W * W;
        if (nslots > need) nslots = need;
        s.nslots = (int32_t)nslots;
        s.arena_stride = (int64_t)arena_vectors(opt.max_depth, model_is_separable(s.model), s.L) * s.L;
        DALLOC(s.arena, s.arena_stride * nslots);
    }
    // a user-supplied density: upload its parameters ...
    if (kind == IDHMC_MODEL_CUSTOM) {
        double *up = nullptr;
        DALLOC(up, model->nparams);
        if (model->nparams > 0) {
            hipError_t e = hipMemcpyAsync(up, model->params, sizeof(double) * (size_t)model->nparams, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) return fail(IDHMC_ERR_HIP, "params upload failed: %s", hipGetErrorString(e));
        }
        s.user_params = up;
        s.user_nparams = model->nparams;
    }
    // ... and compile it against the kernel templates; a GLM: its observation source compiled into the logistic regression's templates
    // (hipRTC); the data went up above
    if (kind == IDHMC_MODEL_CUSTOM || glm) {
        static thread_local char jlog[400];
        jlog[0] = 0;
        const int jrc = jit_build(s, model->source, &c->jit, jlog, sizeof jlog, glm ? g.K : 0, g.A, g.H);
        if (jrc != 0) return fail(IDHMC_ERR_BAD_ARG, "%s did not compile (%d): %s", glm ? "GLM observation source" : "custom density", jrc, jlog);
        s.jit = c->jit;
    }
    // kappa = I (GaussianKineticEnergy(sptr, Static{D}, 1.0), src/hamiltonian.jl:63-74)
    {
        const int64_t n = s.minv_stride ? CL : (int64_t)s.L;
        hipError_t e = launch_fill(s.minv, 1.0, n, c->stream);
        if (e == hipSuccess) e = launch_fill(s.w, 1.0, n, c->stream);
        if (e == hipSuccess) e = launch_fill(s.eps, opt.eps_init, nchains, c->stream);
        if (e != hipSuccess) return fail(IDHMC_ERR_HIP, "init kernels failed: %s", hipGetErrorString(e));
    }
    {
        hipError_t e = launch_eval(s, 0, c->stream);   // q = 0: consistent (lq, grad)
        if (e != hipSuccess && e != hipErrorNotSupported) return fail(IDHMC_ERR_HIP, "eval failed: %s", hipGetErrorString(e));
        e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(IDHMC_ERR_HIP, "init sync failed: %s", hipGetErrorString(e));
    }
    *out = guard.release();
    return IDHMC_OK;
}

int idhmc_create(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                 const idhmc_model_desc *model, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !model) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create: null argument");
    return create_context(out, device, nchains, first_chain_id, model, opt_in, seed, nullptr);
}

// What create_glm derives from an idhmc_glm_model as its validation proceeds: every validate_* below takes the model and these, reads
// the counts of the steps before it and sets its own (0, false: the part is absent and the context is the one without it).
struct GlmCounts {
    int64_t fcols = 0;         // the level columns, sum N_f
    bool valued = false;       // some term has values
    int J = 0, P = 0, S = 0, SZ = 0, G = 0, BK = 0, BZ = 0, MP = 0;   // local scales, pairs, structured terms (SZ: AR(1) ones), GMRF terms, block terms and zetas, planes of a wide table
};

// The priors of idhmc_create_glm_priors: every check of kind and nu over all D coordinates, so after every count is known.  *any: some
// kind is not 0 (none is: the context is the one without priors).  nu_out: nu with 0 wherever the caller passed none.
static int validate_priors(const idhmc_glm_model &m, const GlmCounts &n, std::vector<double> *nu_out, bool *any)
{
    const auto *glm = m.glm; const auto *pr = m.priors;
    *any = false;
    if (!pr || !pr->kind) {
        if (pr && pr->nu) return fail(IDHMC_ERR_BAD_ARG, "GLM: priors->nu without priors->kind");
        return IDHMC_OK;
    }
    const int D = glm->Dx + glm->A + glm->H + n.J + n.P + n.BZ + n.SZ;
    nu_out->assign((size_t)D, 0.0);
    for (int c = 0; c < D; ++c) {
        const int32_t k = pr->kind[c];
        const double nu = pr->nu ? pr->nu[c] : 0.0;
        if (k < IDHMC_PRIOR_NORMAL || k > IDHMC_PRIOR_LOG_EXPONENTIAL)
            return fail(IDHMC_ERR_BAD_ARG, "GLM: prior kind[%d] = %d is outside 0..4", c, k);
        const bool takes_nu = k == IDHMC_PRIOR_STUDENT_T || k == IDHMC_PRIOR_LOG_HALF_STUDENT_T;
        if (takes_nu && !pr->nu) return fail(IDHMC_ERR_BAD_ARG, "GLM: prior kind[%d] = %d needs nu (priors->nu is NULL)", c, k);
        if (takes_nu && !(std::isfinite(nu) && nu > 0.0))
            return fail(IDHMC_ERR_BAD_ARG, "GLM: prior nu[%d] = %g must be finite and > 0 (kind %d)", c, nu, k);
        if (!takes_nu && nu != 0.0) return fail(IDHMC_ERR_BAD_ARG, "GLM: prior nu[%d] = %g must be 0 (kind %d takes no nu)", c, nu, k);
        if (k >= IDHMC_PRIOR_LOG_HALF_NORMAL) {
            if (c < glm->Dx)
                return fail(IDHMC_ERR_BAD_ARG, "GLM: prior kind[%d] = %d is a prior on exp(q): coordinate %d is a coefficient, not a logarithm "
                            "(kinds 2..4 are for the coordinates behind the Dx = %d coefficients)", c, k, c, glm->Dx);
            if (glm->tau && glm->tau[c] != 1.0)
                return fail(IDHMC_ERR_BAD_ARG, "GLM: prior tau[%d] = %g must be 1 (kind %d: its one scale is exp(mu))", c, glm->tau[c], k);
        }
        (*nu_out)[(size_t)c] = nu;
        if (k != IDHMC_PRIOR_NORMAL) *any = true;
    }
    return IDHMC_OK;
}

// The local scales of idhmc_create_glm_local: every check of local and slab_scale.  J: the flagged columns
static int validate_local(const idhmc_glm_model &m, GlmCounts *n)
{
    const idhmc_glm_local *lc = m.local;
    if (!lc) return IDHMC_OK;
    if (!(std::isfinite(lc->slab_scale) && lc->slab_scale >= 0.0))
        return fail(IDHMC_ERR_BAD_ARG, "GLM: slab_scale = %g must be finite and >= 0 (0: no slab)", lc->slab_scale);
    int J = 0;
    if (lc->local)
        for (int c = 0; c < m.glm->Dx; ++c) {
            if (lc->local[c] != 0 && lc->local[c] != 1) return fail(IDHMC_ERR_BAD_ARG, "GLM: local[%d] = %d is neither 0 nor 1", c, lc->local[c]);
            J += lc->local[c];
        }
    if (lc->slab_scale > 0.0 && J == 0)
        return fail(IDHMC_ERR_BAD_ARG, "GLM: slab_scale = %g without a column that has a local scale (local is NULL or all zeros)", lc->slab_scale);
    n->J = J;
    return IDHMC_OK;
}

// The factors of idhmc_create_glm_factors: every check of F, levels and index (with members: of F and levels).  fcols: the level columns
static int validate_factors(const idhmc_glm_model &m, GlmCounts *n)
{
    const auto *glm = m.glm; const auto *fc = m.factors;
    if (!fc) return IDHMC_OK;
    if (fc->F < 0 || fc->F > 4) return fail(IDHMC_ERR_BAD_ARG, "GLM: F = %d factors must be an integer in 0..4", fc->F);
    if (fc->F == 0) return IDHMC_OK;
    if (m.members && fc->index)
        return fail(IDHMC_ERR_BAD_ARG, "GLM: members and factors->index are both given: with members the levels come from members->index (factors->index must be NULL)");
    if (!fc->levels || (!fc->index && !m.members)) return fail(IDHMC_ERR_BAD_ARG, "GLM: F = %d factors need levels and index (%s is NULL)", fc->F, fc->levels ? "index" : "levels");
    int64_t cols = 0;
    for (int f = 0; f < fc->F; ++f) {
        if (fc->levels[f] < 1) return fail(IDHMC_ERR_BAD_ARG, "GLM: factor %d has levels[%d] = %d: at least one level is needed", f, f, fc->levels[f]);
        cols += fc->levels[f];
    }
    if (glm->Dx - cols < 1)
        return fail(IDHMC_ERR_BAD_ARG, "GLM: Dd = Dx - sum of levels = %d - %lld = %lld: at least one dense column is needed",
                    glm->Dx, (long long)cols, (long long)(glm->Dx - cols));
    for (int f = 0; f < fc->F && !m.members; ++f)               // (a table of members is checked by check_members)
        for (int64_t i = 0; i < glm->n; ++i) {
            const int32_t v = fc->index[(int64_t)f * glm->n + i];
            if (v < 0 || v >= fc->levels[f])
                return fail(IDHMC_ERR_BAD_ARG, "GLM: index[%d][%lld] = %d is outside 0..%d (the levels of factor %d)", f, (long long)i, v, fc->levels[f] - 1, f);
        }
    n->fcols = cols;
    return IDHMC_OK;
}

// The values of idhmc_create_glm_slopes, after validate_factors: every check of has and values.  valued: some term has values
static int validate_factor_values(const idhmc_glm_model &m, GlmCounts *n)
{
    const auto *fc = m.factors; const auto *fv = m.values;
    if (!fv) return IDHMC_OK;
    if (!fc || n->fcols == 0) return fail(IDHMC_ERR_BAD_ARG, "GLM: factor values need factor terms (factors is %s)", fc ? "given with F = 0" : "NULL");
    if (!fv->has) return fail(IDHMC_ERR_BAD_ARG, "GLM: factor values need has, one flag per term (has is NULL)");
    bool any = false;
    for (int f = 0; f < fc->F; ++f) {
        if (fv->has[f] != 0 && fv->has[f] != 1) return fail(IDHMC_ERR_BAD_ARG, "GLM: has[%d] = %d must be 0 or 1", f, fv->has[f]);
        if (fv->has[f]) any = true;
    }
    if (!any) return IDHMC_OK;
    if (!fv->values) return fail(IDHMC_ERR_BAD_ARG, "GLM: a term is flagged in has and values is NULL");
    for (int f = 0; f < fc->F; ++f) {
        if (!fv->has[f]) continue;                         // rows of unflagged terms are not read
        for (int64_t i = 0; i < m.glm->n; ++i)
            if (!std::isfinite(fv->values[(int64_t)f * m.glm->n + i]))
                return fail(IDHMC_ERR_BAD_ARG, "GLM: values[%d][%lld] is not finite", f, (long long)i);
    }
    n->valued = true;
    return IDHMC_OK;
}

// The pairs of idhmc_create_glm_corr, after validate_factors and validate_local: every check of P, first, second and eta, and of the
// zetas' entries in the prior arrays.  P: the pairs
static int validate_pairs(const idhmc_glm_model &m, GlmCounts *n)
{
    const auto *glm = m.glm; const auto *pr = m.priors; const auto *fc = m.factors; const auto *pp = m.pairs;
    if (!pp) return IDHMC_OK;
    if (pp->P < 0 || pp->P > 2) return fail(IDHMC_ERR_BAD_ARG, "GLM: P = %d pairs must be an integer in 0..2", pp->P);
    if (pp->P == 0) return IDHMC_OK;
    if (!pp->first || !pp->second || !pp->eta)
        return fail(IDHMC_ERR_BAD_ARG, "GLM: P = %d pairs need first, second and eta (%s is NULL)", pp->P, !pp->first ? "first" : !pp->second ? "second" : "eta");
    if (!fc || n->fcols == 0) return fail(IDHMC_ERR_BAD_ARG, "GLM: pairs need factor terms (factors is %s)", fc ? "given with F = 0" : "NULL");
    bool used[4] = {false, false, false, false};
    const int cz0 = glm->Dx + glm->A + glm->H + n->J;
    for (int p = 0; p < pp->P; ++p) {
        const int32_t a = pp->first[p], b = pp->second[p];
        if (a < 0 || a >= fc->F) return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d: first = %d is outside 0..%d (the model's terms)", p, a, fc->F - 1);
        if (b < 0 || b >= fc->F) return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d: second = %d is outside 0..%d (the model's terms)", p, b, fc->F - 1);
        if (a == b) return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d: first = second = %d (a pair is two distinct terms)", p, a);
        if (used[a] || used[b]) return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d: term %d is in two pairs", p, used[a] ? a : b);
        used[a] = used[b] = true;
        if (fc->levels[a] != fc->levels[b])
            return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d: terms %d and %d have %d and %d levels (a pair needs equal level counts)", p, a, b,
                        fc->levels[a], fc->levels[b]);
        const double eta = pp->eta[p];
        if (!(std::isfinite(eta) && eta >= 0.0)) return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d: eta = %g must be finite and >= 0 (0: the prior arrays' entry applies)", p, eta);
        const int cz = cz0 + p;
        const int32_t k = pr && pr->kind ? pr->kind[cz] : 0;
        if (k >= IDHMC_PRIOR_LOG_HALF_NORMAL && k <= IDHMC_PRIOR_LOG_EXPONENTIAL)
            return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d: prior kind[%d] = %d is a prior on exp(q): coordinate %d is zeta = atanh rho, not a logarithm "
                        "(kinds 0 and 1 are for a zeta)", p, cz, k, cz);
        if (eta > 0.0) {
            const double nu = pr && pr->kind && pr->nu ? pr->nu[cz] : 0.0;
            if (k != 0 || nu != 0.0 || (glm->mu && glm->mu[cz] != 0.0) || (glm->tau && glm->tau[cz] != 1.0))
                return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d: eta = %g is the LKJ prior of zeta: the entry of coordinate %d in the prior arrays must "
                            "be the default (kind 0, mu 0, tau 1, nu 0) and is not applied", p, eta, cz);
        }
    }
    n->P = pp->P;
    return IDHMC_OK;
}

// The structures of idhmc_create_glm_struct, after validate_pairs: every check of S, term, kind and eta, of the terms against the pairs
// and the local flags, and of the AR(1) zetas' entries in the prior arrays (coordinate cz0 onwards: behind the pairs' zetas or, n->BZ,
// a block's).  S: the structured terms, SZ: those that are AR(1)
static int validate_structs(const idhmc_glm_model &m, GlmCounts *n)
{
    const auto *glm = m.glm; const auto *pr = m.priors; const auto *fc = m.factors; const auto *pp = m.pairs; const auto *st = m.structs;
    const int J = n->J, P = n->P, BZ = n->BZ;
    if (!st) return IDHMC_OK;
    if (st->S < 0 || st->S > 2) return fail(IDHMC_ERR_BAD_ARG, "GLM: S = %d structured terms must be an integer in 0..2", st->S);
    if (st->S == 0) return IDHMC_OK;
    if (!st->term || !st->kind || !st->eta)
        return fail(IDHMC_ERR_BAD_ARG, "GLM: S = %d structured terms need term, kind and eta (%s is NULL)", st->S, !st->term ? "term" : !st->kind ? "kind" : "eta");
    if (!fc || n->fcols == 0) return fail(IDHMC_ERR_BAD_ARG, "GLM: structured terms need factor terms (factors is %s)", fc ? "given with F = 0" : "NULL");
    int sz = 0;
    for (int i = 0; i < st->S; ++i) sz += st->kind[i] == IDHMC_STRUCT_AR1;
    if (glm->Dx + J + P + BZ + sz > 1024 - glm->A - glm->H)
        return fail(IDHMC_ERR_BAD_ARG, "D = Dx + A + H + J + P + Sz = %lld: a GLM is limited to D <= 1024 (Sz = %d AR(1) terms)",
                    (long long)glm->Dx + glm->A + glm->H + J + P + BZ + sz, sz);
    const int cz0 = glm->Dx + glm->A + glm->H + J + P + BZ;
    int z = 0;
    for (int i = 0; i < st->S; ++i) {
        const int32_t t = st->term[i], kd = st->kind[i];
        if (t < 0 || t >= fc->F) return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: term = %d is outside 0..%d (the model's terms)", i, t, fc->F - 1);
        if (i == 1 && st->term[0] == t) return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: term %d is listed twice", i, t);
        if (kd != IDHMC_STRUCT_AR1 && kd != IDHMC_STRUCT_RW1)
            return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: kind = %d must be IDHMC_STRUCT_AR1 (1) or IDHMC_STRUCT_RW1 (2)", i, kd);
        const double eta = st->eta[i];
        if (!(std::isfinite(eta) && eta >= 0.0))
            return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: eta = %g must be finite and >= 0 (0: the prior arrays' entry applies)", i, eta);
        if (kd == IDHMC_STRUCT_RW1 && eta != 0.0)
            return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: eta = %g on a random walk, which has no zeta (eta must be 0)", i, eta);
        if (fc->levels[t] < 2)
            return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: term %d has %d level (a structured term needs at least 2)", i, t, fc->levels[t]);
        for (int p = 0; p < P; ++p)
            if (pp->first[p] == t || pp->second[p] == t)
                return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: term %d is in pair %d (a term is structured or paired, not both)", i, t, p);
        if (J > 0) {
            int64_t o = glm->Dx - n->fcols;
            for (int f = 0; f < t; ++f) o += fc->levels[f];
            for (int32_t k = 0; k < fc->levels[t]; ++k)
                if (m.local->local[o + k])
                    return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: local[%lld] is set on level %d of term %d (a structured term takes no local scale)",
                                i, (long long)(o + k), k, t);
        }
        if (kd != IDHMC_STRUCT_AR1) continue;
        const int cz = cz0 + z++;
        const int32_t k = pr && pr->kind ? pr->kind[cz] : 0;
        if (k >= IDHMC_PRIOR_LOG_HALF_NORMAL && k <= IDHMC_PRIOR_LOG_EXPONENTIAL)
            return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: prior kind[%d] = %d is a prior on exp(q): coordinate %d is zeta = atanh phi, not a logarithm "
                        "(kinds 0 and 1 are for a zeta)", i, cz, k, cz);
        if (eta > 0.0) {
            const double nu = pr && pr->kind && pr->nu ? pr->nu[cz] : 0.0;
            if (k != 0 || nu != 0.0 || (glm->mu && glm->mu[cz] != 0.0) || (glm->tau && glm->tau[cz] != 1.0))
                return fail(IDHMC_ERR_BAD_ARG, "GLM: structure %d: eta = %g is the Beta(eta, eta) prior of zeta: the entry of coordinate %d in the prior arrays "
                            "must be the default (kind 0, mu 0, tau 1, nu 0) and is not applied", i, eta, cz);
        }
    }
    n->S = st->S;
    n->SZ = sz;
    return IDHMC_OK;
}

// The GMRF terms of idhmc_create_glm_gmrf, after validate_structs: every check of G, term and kappa, of the terms against the pairs, the
// structures, the local flags and the prior arrays, and of the precisions' tables.  G: the GMRF terms
static int validate_gmrfs(const idhmc_glm_model &m, GlmCounts *n)
{
    const auto *glm = m.glm; const auto *pr = m.priors; const auto *fc = m.factors; const auto *pp = m.pairs; const auto *st = m.structs;
    const auto *gm = m.gmrfs;
    const int J = n->J, P = n->P, S = n->S;
    if (!gm) return IDHMC_OK;
    if (gm->G < 0 || gm->G > 2) return fail(IDHMC_ERR_BAD_ARG, "GLM: G = %d GMRF terms must be an integer in 0..2", gm->G);
    if (gm->G == 0) return IDHMC_OK;
    if (!gm->term || !gm->start || !gm->col || !gm->val || !gm->kappa)
        return fail(IDHMC_ERR_BAD_ARG, "GLM: G = %d GMRF terms need term, start, col, val and kappa (%s is NULL)", gm->G,
                    !gm->term ? "term" : !gm->start ? "start" : !gm->col ? "col" : !gm->val ? "val" : "kappa");
    if (!fc || n->fcols == 0) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF terms need factor terms (factors is %s)", fc ? "given with F = 0" : "NULL");
    if (gm->start[0] != 0) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF start[0] = %lld must be 0", (long long)gm->start[0]);
    int64_t rows = 0;
    for (int i = 0; i < gm->G; ++i) {
        const int32_t t = gm->term[i];
        if (t < 0 || t >= fc->F) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: term = %d is outside 0..%d (the model's terms)", i, t, fc->F - 1);
        if (i == 1 && gm->term[0] == t) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: term %d is listed twice", i, t);
        const double kap = gm->kappa[i];
        if (!(std::isfinite(kap) && kap >= 0.0)) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: kappa = %g must be finite and >= 0", i, kap);
        for (int p = 0; p < P; ++p)
            if (pp->first[p] == t || pp->second[p] == t)
                return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: term %d is in pair %d (a GMRF term is in no pair)", i, t, p);
        for (int k = 0; k < S; ++k)
            if (st->term[k] == t) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: term %d is structure %d (a term is structured or a GMRF, not both)", i, t, k);
        const int32_t N = fc->levels[t];
        int64_t o = glm->Dx - n->fcols;
        for (int f = 0; f < t; ++f) o += fc->levels[f];
        for (int32_t k = 0; k < N; ++k) {
            const int64_t c = o + k;
            if (J > 0 && m.local->local[c])
                return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: local[%lld] is set on level %d of term %d (a GMRF term takes no local scale)", i, (long long)c, k, t);
            const int32_t kd = pr && pr->kind ? pr->kind[c] : 0;
            const double nu = pr && pr->kind && pr->nu ? pr->nu[c] : 0.0;
            if (kd != 0 || nu != 0.0 || (glm->mu && glm->mu[c] != 0.0) || (glm->tau && glm->tau[c] != 1.0))
                return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: the entry of coordinate %lld (level %d of term %d) in the prior arrays must be the default "
                            "(kind 0, mu 0, tau 1, nu 0): the precision is its prior", i, (long long)c, k, t);
        }
        // the table: rows rows .. rows + N - 1
        const int64_t *sp = gm->start + rows;
        for (int32_t k = 0; k < N; ++k) {
            const int64_t cnt = sp[k + 1] - sp[k];
            if (cnt < 0) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: start[%lld] = %lld is below start[%lld] = %lld (start must not decrease)", i,
                                     (long long)(rows + k + 1), (long long)sp[k + 1], (long long)(rows + k), (long long)sp[k]);
            if (cnt < 1 || cnt > 128)
                return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: row %d has %lld entries (1..128: the diagonal is always there)", i, k, (long long)cnt);
            bool diag = false;
            for (int64_t e = sp[k]; e < sp[k + 1]; ++e) {
                const int32_t cj = gm->col[e];
                if (cj < 0 || cj >= N) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: row %d: col[%lld] = %d is outside 0..%d", i, k, (long long)e, cj, N - 1);
                if (e > sp[k] && cj <= gm->col[e - 1])
                    return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: row %d: col[%lld] = %d is not above col[%lld] = %d (columns strictly ascending)", i, k,
                                (long long)e, cj, (long long)(e - 1), gm->col[e - 1]);
                if (!std::isfinite(gm->val[e])) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: row %d: val[%lld] = %g is not finite", i, k, (long long)e, gm->val[e]);
                if (cj == k) {
                    diag = true;
                    if (!(gm->val[e] > 0.0)) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: row %d: the diagonal val[%lld] = %g must be > 0", i, k, (long long)e, gm->val[e]);
                }
            }
            if (!diag) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: row %d has no diagonal entry", i, k);
        }
        // symmetry, once every row of the term is known to be inside the table: Q_kj and Q_jk both there and bit-equal
        for (int32_t k = 0; k < N; ++k)
            for (int64_t e = sp[k]; e < sp[k + 1]; ++e) {
                const int32_t cj = gm->col[e];
                const int32_t *b = gm->col + sp[cj], *en = gm->col + sp[cj + 1];
                const int32_t *it = std::lower_bound(b, en, k);
                if (it == en || *it != k) return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: Q[%d][%d] is given and Q[%d][%d] is absent (Q must be symmetric)", i, k, cj, cj, k);
                if (memcmp(&gm->val[it - gm->col], &gm->val[e], sizeof(double)) != 0)
                    return fail(IDHMC_ERR_BAD_ARG, "GLM: GMRF %d: Q[%d][%d] = %.17g and Q[%d][%d] = %.17g are not bit-equal (Q must be symmetric)", i, k, cj,
                                gm->val[e], cj, k, gm->val[it - gm->col]);
            }
        rows += N;
    }
    n->G = gm->G;
    return IDHMC_OK;
}

// The block of idhmc_create_glm_block, after validate_gmrfs: every check of K, term and eta, of the terms against the pairs, the
// structures and the GMRF terms, and of the zetas' entries in the prior arrays (coordinate Dx + A + H + J onwards).  BK: the block's
// terms (BZ, their zetas, is create_glm's: validate_structs needed it)
static int validate_block(const idhmc_glm_model &m, GlmCounts *n)
{
    const auto *glm = m.glm; const auto *pr = m.priors; const auto *fc = m.factors; const auto *st = m.structs; const auto *gm = m.gmrfs;
    const auto *bk = m.block;
    const int J = n->J, P = n->P, S = n->S, SZ = n->SZ, G = n->G;
    if (!bk) return IDHMC_OK;
    if (bk->K != 0 && (bk->K < 2 || bk->K > 4)) return fail(IDHMC_ERR_BAD_ARG, "GLM: a block of K = %d terms: K must be 0, 2, 3 or 4", bk->K);
    if (bk->K == 0) return IDHMC_OK;
    if (!bk->term) return fail(IDHMC_ERR_BAD_ARG, "GLM: a block of K = %d terms needs term (term is NULL)", bk->K);
    if (!fc || n->fcols == 0) return fail(IDHMC_ERR_BAD_ARG, "GLM: a block needs factor terms (factors is %s)", fc ? "given with F = 0" : "NULL");
    if (P > 0) return fail(IDHMC_ERR_BAD_ARG, "GLM: a block next to P = %d pairs (a model has pairs or a block, not both)", P);
    const int nz = (bk->K * (bk->K - 1)) / 2;
    if (glm->Dx + J + nz + SZ > 1024 - glm->A - glm->H)
        return fail(IDHMC_ERR_BAD_ARG, "D = Dx + A + H + J + K (K - 1) / 2 + Sz = %lld: a GLM is limited to D <= 1024 (a block of K = %d terms)",
                    (long long)glm->Dx + glm->A + glm->H + J + nz + SZ, bk->K);
    for (int r = 0; r < bk->K; ++r) {
        const int32_t t = bk->term[r];
        if (t < 0 || t >= fc->F) return fail(IDHMC_ERR_BAD_ARG, "GLM: block row %d: term = %d is outside 0..%d (the model's terms)", r, t, fc->F - 1);
        for (int q = 0; q < r; ++q)
            if (bk->term[q] == t) return fail(IDHMC_ERR_BAD_ARG, "GLM: block row %d: term %d is listed twice", r, t);
        if (fc->levels[t] != fc->levels[bk->term[0]])
            return fail(IDHMC_ERR_BAD_ARG, "GLM: block row %d: terms %d and %d have %d and %d levels (a block needs equal level counts)", r,
                        bk->term[0], t, fc->levels[bk->term[0]], fc->levels[t]);
        for (int i = 0; i < S; ++i)
            if (st->term[i] == t) return fail(IDHMC_ERR_BAD_ARG, "GLM: block row %d: term %d is structure %d (a block term is not structured)", r, t, i);
        for (int i = 0; i < G; ++i)
            if (gm->term[i] == t) return fail(IDHMC_ERR_BAD_ARG, "GLM: block row %d: term %d is GMRF %d (a block term is no GMRF term)", r, t, i);
    }
    const double eta = bk->eta;
    if (!(std::isfinite(eta) && eta >= 0.0)) return fail(IDHMC_ERR_BAD_ARG, "GLM: block: eta = %g must be finite and >= 0 (0: the prior arrays' entries apply)", eta);
    const int cz0 = glm->Dx + glm->A + glm->H + J;
    for (int e = 0; e < nz; ++e) {
        const int cz = cz0 + e;
        const int32_t k = pr && pr->kind ? pr->kind[cz] : 0;
        if (k >= IDHMC_PRIOR_LOG_HALF_NORMAL && k <= IDHMC_PRIOR_LOG_EXPONENTIAL)
            return fail(IDHMC_ERR_BAD_ARG, "GLM: block: prior kind[%d] = %d is a prior on exp(q): coordinate %d is a zeta = atanh z, not a logarithm "
                        "(kinds 0 and 1 are for a zeta)", cz, k, cz);
        if (eta > 0.0) {
            const double nu = pr && pr->kind && pr->nu ? pr->nu[cz] : 0.0;
            if (k != 0 || nu != 0.0 || (glm->mu && glm->mu[cz] != 0.0) || (glm->tau && glm->tau[cz] != 1.0))
                return fail(IDHMC_ERR_BAD_ARG, "GLM: block: eta = %g is the LKJ prior of the zetas: the entry of coordinate %d in the prior arrays must "
                            "be the default (kind 0, mu 0, tau 1, nu 0) and is not applied", eta, cz);
        }
    }
    n->BK = bk->K;
    return IDHMC_OK;
}

// The upload description of a validated model: every part the counts say is there (a part that is not keeps GlmParts' defaults)
static GlmParts glm_parts(const idhmc_glm_model &m, const GlmCounts &n, bool responses)
{
    const idhmc_glm_desc *glm = m.glm;
    GlmParts g{"", glm->n, glm->K, glm->nc, glm->A, glm->H, glm->X, glm->Y, glm->constants, glm->groups, responses, m.M, m.chains_per_response};
    if (n.J > 0) { g.J = n.J; g.local = m.local->local; g.slab = m.local->slab_scale; }
    if (n.fcols > 0) { g.F = m.factors->F; g.fcols = (int32_t)n.fcols; g.levels = m.factors->levels; g.findex = m.factors->index; }
    if (n.valued) { g.fvalues = m.values->values; g.fhas = m.values->has; }
    if (n.MP > 0) { g.MP = n.MP; g.mwidth = m.members->width; g.mindex = m.members->index; g.mvalues = m.members->values; }
    if (n.P > 0) { g.P = n.P; g.pfirst = m.pairs->first; g.psecond = m.pairs->second; g.peta = m.pairs->eta; }
    if (n.S > 0) { g.S = n.S; g.SZ = n.SZ; g.sterm = m.structs->term; g.skind = m.structs->kind; g.seta = m.structs->eta; }
    if (n.G > 0) { g.G = n.G; g.gterm = m.gmrfs->term; g.gstart = m.gmrfs->start; g.gcol = m.gmrfs->col; g.gval = m.gmrfs->val; g.gkappa = m.gmrfs->kappa; }
    if (n.BK > 0) { g.BK = n.BK; g.BZ = n.BZ; g.bterm = m.block->term; g.beta = m.block->eta; }
    return g;
}

// The one road of every GLM handed over in parts: idhmc_create_glm_model and the eleven entries that are it with the later parts NULL.
// `responses`: the context of idhmc_create_glm_responses whatever (M, chains_per_response) is; it is that for anything but (1, 0) anyway.
// The order of the checks is the order of the messages a doubly wrong call gets: DESIGN section 28.
static int create_glm(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id, const idhmc_glm_model &model, bool responses,
                      const idhmc_options *opt_in, uint64_t seed)
{
    *out = nullptr;
    idhmc_glm_model m = model;         // (the caller's is not written to: a table of members of width 1 is rewritten below)
    const idhmc_glm_desc *glm = m.glm;
    responses = responses || !(m.M == 1 && m.chains_per_response == 0);
    GlmCounts n;
    if (glm->Dx < 1) return fail(IDHMC_ERR_BAD_ARG, "GLM: Dx = %d: at least one coefficient is needed", glm->Dx);
    if (m.members && (!m.factors || m.factors->F == 0))
        return fail(IDHMC_ERR_BAD_ARG, "GLM: members need factor terms: factors gives F and levels (factors is %s)", m.factors ? "given with F = 0" : "NULL");
    if (m.members && m.values)
        return fail(IDHMC_ERR_BAD_ARG, "GLM: members and factor values are both given: with members the values come from members->values (values must be NULL)");
    if (int rc = validate_factors(m, &n)) return rc;
    // A table of members every term of which has width 1 is F plain index rows, with values where it gives some: from here on it IS
    // that model (the same context, kernels and footprint).  MP > 0: a wide term.
    idhmc_glm_factors plain_f;
    idhmc_glm_factor_values plain_v;
    const int32_t plain_has[4] = {1, 1, 1, 1};
    if (m.members) {
        char msg[320];
        bool wide = false;
        if (!check_members(m.factors->F, m.factors->levels, glm->n, m.members->width, m.members->index, m.members->values, &n.MP, &wide, msg, sizeof msg))
            return fail(IDHMC_ERR_BAD_ARG, "%s", msg);
        if (!wide) {
            plain_f = idhmc_glm_factors{m.factors->F, m.factors->levels, m.members->index};
            plain_v = idhmc_glm_factor_values{m.members->values, plain_has};
            m.factors = &plain_f;
            m.values = m.members->values ? &plain_v : nullptr;
            m.members = nullptr;
            n.MP = 0;
        }
    }
    if (int rc = validate_factor_values(m, &n)) return rc;
    if (glm->A < 0 || glm->A > 4) return fail(IDHMC_ERR_BAD_ARG, "GLM: A = %d must be an integer in 0..4", glm->A);
    if (glm->H < 0 || glm->H > 4) return fail(IDHMC_ERR_BAD_ARG, "GLM: H = %d must be an integer in 0..4", glm->H);
    if (glm->Dx > 1024 - glm->A - glm->H)
        return fail(IDHMC_ERR_BAD_ARG, "D = Dx + A + H = %lld: a GLM is limited to D <= 1024", (long long)glm->Dx + glm->A + glm->H);
    if (int rc = validate_local(m, &n)) return rc;
    if (glm->Dx + n.J > 1024 - glm->A - glm->H)
        return fail(IDHMC_ERR_BAD_ARG, "D = Dx + A + H + J = %lld: a GLM is limited to D <= 1024 (J = %d local scales)",
                    (long long)glm->Dx + glm->A + glm->H + n.J, n.J);
    if (m.pairs && m.pairs->P >= 0 && m.pairs->P <= 2 && glm->Dx + n.J + m.pairs->P > 1024 - glm->A - glm->H)
        return fail(IDHMC_ERR_BAD_ARG, "D = Dx + A + H + J + P = %lld: a GLM is limited to D <= 1024 (P = %d pairs)",
                    (long long)glm->Dx + glm->A + glm->H + n.J + m.pairs->P, m.pairs->P);
    if (int rc = validate_pairs(m, &n)) return rc;
    // (the AR(1) zetas stand behind the block's as behind the pairs': a well-formed block's count goes where P goes, and validate_block,
    // which needs S and G, then checks the block itself: it passes a block only with this count, and with none only when this is 0)
    if (n.P == 0 && m.block && m.block->K >= 2 && m.block->K <= 4) n.BZ = (m.block->K * (m.block->K - 1)) / 2;
    if (n.BZ > 0 && glm->Dx + n.J + n.BZ > 1024 - glm->A - glm->H)
        return fail(IDHMC_ERR_BAD_ARG, "D = Dx + A + H + J + K (K - 1) / 2 = %lld: a GLM is limited to D <= 1024 (a block of K = %d terms)",
                    (long long)glm->Dx + glm->A + glm->H + n.J + n.BZ, m.block->K);
    if (int rc = validate_structs(m, &n)) return rc;
    if (int rc = validate_gmrfs(m, &n)) return rc;
    if (int rc = validate_block(m, &n)) return rc;
    if (m.members) {
        // (a pair or a block takes level k of one term with level k of another, one level per observation each)
        for (int p = 0; p < n.P; ++p)
            for (const int32_t t : {m.pairs->first[p], m.pairs->second[p]})
                if (m.members->width[t] > 1)
                    return fail(IDHMC_ERR_BAD_ARG, "GLM: pair %d names term %d, which has width %d: a term with several levels per observation is in no pair", p, t, m.members->width[t]);
        for (int r = 0; r < n.BK; ++r)
            if (m.members->width[m.block->term[r]] > 1)
                return fail(IDHMC_ERR_BAD_ARG, "GLM: the block names term %d, which has width %d: a term with several levels per observation is in no block",
                            m.block->term[r], m.members->width[m.block->term[r]]);
    }
    if (glm->H > 0 && !glm->groups) return fail(IDHMC_ERR_BAD_ARG, "GLM: H = %d groups need the group of every column (groups is NULL)", glm->H);
    if (glm->H == 0 && glm->groups) return fail(IDHMC_ERR_BAD_ARG, "GLM: groups must be NULL with H = 0");
    if (glm->H > 0) {
        bool used[4] = {false, false, false, false};
        for (int c = 0; c < glm->Dx; ++c) {
            const int32_t g = glm->groups[c];
            if (g < -1 || g >= glm->H) return fail(IDHMC_ERR_BAD_ARG, "GLM: groups[%d] = %d is outside -1..%d", c, g, glm->H - 1);
            if (g >= 0) used[g] = true;
        }
        for (int g = 0; g < glm->H; ++g)
            if (!used[g]) return fail(IDHMC_ERR_BAD_ARG, "GLM: group %d has no column", g);
    }
    const int P = n.P, S = n.S, SZ = n.SZ, G = n.G, BK = n.BK, BZ = n.BZ;
    const idhmc_model_desc md = {.kind = glm->A > 0 ? IDHMC_MODEL_GLM_AUX : IDHMC_MODEL_GLM, .D = glm->Dx + glm->A + glm->H + n.J + P + BZ + SZ,
                                 .mu = glm->mu, .tau = glm->tau, .source = glm->source};
    std::vector<double> nu;
    bool any = false;
    if (int rc = validate_priors(m, n, &nu, &any)) return rc;
    GlmParts parts = glm_parts(m, n, responses);
    if (any) { parts.pkind = m.priors->kind; parts.pnu = nu.data(); }
    std::vector<int32_t> kdev, kpub;     // a zeta with eta > 0: the device table marks it (kPriorLkj of idhmc_glm_coords.hpp, eta in nu's place)
    std::vector<double> nudev, nupub;
    if (P > 0 || SZ > 0 || G > 0 || BK > 0) {
        bool lkj = G > 0 || (BK > 0 && m.block->eta > 0.0);      // (a GMRF term's members are marked too: kPriorGmrf)
        for (int p = 0; p < P; ++p) lkj = lkj || m.pairs->eta[p] > 0.0;
        for (int i = 0; i < S; ++i) lkj = lkj || m.structs->eta[i] > 0.0;
        if (lkj) {
            kpub.assign((size_t)md.D, 0);
            nupub.assign((size_t)md.D, 0.0);
            if (any) { kpub.assign(m.priors->kind, m.priors->kind + md.D); nupub = nu; }
            kdev = kpub;
            nudev = nupub;
            for (int p = 0; p < P; ++p)
                if (m.pairs->eta[p] > 0.0) { kdev[(size_t)(md.D - SZ - P + p)] = 5; nudev[(size_t)(md.D - SZ - P + p)] = m.pairs->eta[p]; }
            // LKJ(eta) on the block's K x K matrix: zeta_ji takes the row with beta_ji = eta + (K - 2 - i) / 2, i its column
            if (BK > 0 && m.block->eta > 0.0)
                for (int j = 1; j < BK; ++j)
                    for (int i = 0; i < j; ++i) {
                        const size_t cz = (size_t)(md.D - SZ - BZ + (j * (j - 1)) / 2 + i);
                        kdev[cz] = 5;
                        nudev[cz] = m.block->eta + 0.5 * (double)(BK - 2 - i);
                    }
            for (int i = 0, z = 0; i < S; ++i) {
                if (m.structs->kind[i] != IDHMC_STRUCT_AR1) continue;
                if (m.structs->eta[i] > 0.0) { kdev[(size_t)(md.D - SZ + z)] = 5; nudev[(size_t)(md.D - SZ + z)] = m.structs->eta[i]; }
                ++z;
            }
            for (int i = 0; i < G; ++i) {
                int64_t o = glm->Dx - n.fcols;
                for (int f = 0; f < m.gmrfs->term[i]; ++f) o += m.factors->levels[f];
                for (int32_t k = 0; k < m.factors->levels[m.gmrfs->term[i]]; ++k) kdev[(size_t)(o + k)] = 6;
            }
            parts.pkind = kdev.data(); parts.pnu = nudev.data();
            parts.pkind_pub = kpub.data(); parts.pnu_pub = nupub.data();
        }
    }
    return create_context(out, device, nchains, first_chain_id, &md, opt_in, seed, &parts);
}

int idhmc_create_glm_model(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                           const idhmc_glm_model *model, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !model || !model->glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_model: null argument");
    idhmc_glm_model m = *model;
    if (m.M == 0 && m.chains_per_response == 0) m.M = 1;          // a zero-initialised struct with glm set is a plain model
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

// The eleven entries from before idhmc_create_glm_model: each is it with the parts it has no argument for NULL and (M, chains_per_response)
// as given ((0, 0) is refused as it always was).  They differ in the fields they set; idhmc_create_glm_responses also forces its context.
int idhmc_create_glm(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                     const idhmc_glm_desc *glm, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm: null argument");
    const idhmc_glm_model m = {.glm = glm, .M = 1, .chains_per_response = 0};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_responses(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                               const idhmc_glm_desc *glm, int64_t M, int64_t chains_per_response,
                               const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_responses: null argument");
    const idhmc_glm_model m = {.glm = glm, .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, true, opt_in, seed);
}

int idhmc_create_glm_priors(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                            const idhmc_glm_desc *glm, const idhmc_glm_priors *priors,
                            int64_t M, int64_t chains_per_response, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_priors: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_local(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                           const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                           int64_t M, int64_t chains_per_response, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_local: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .local = local, .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_factors(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                             const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                             const idhmc_glm_factors *factors, int64_t M, int64_t chains_per_response,
                             const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_factors: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .local = local, .factors = factors, .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_slopes(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                            const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                            const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, int64_t M, int64_t chains_per_response,
                            const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_slopes: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .local = local, .factors = factors, .values = values,
                               .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_corr(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                          const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                          const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                          int64_t M, int64_t chains_per_response, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_corr: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .local = local, .factors = factors, .values = values, .pairs = pairs,
                               .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_struct(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                            const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                            const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                            const idhmc_glm_structs *structs, int64_t M, int64_t chains_per_response, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_struct: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .local = local, .factors = factors, .values = values, .pairs = pairs, .structs = structs,
                               .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_gmrf(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                          const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                          const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                          const idhmc_glm_structs *structs, const idhmc_glm_gmrfs *gmrfs, int64_t M, int64_t chains_per_response,
                          const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_gmrf: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .local = local, .factors = factors, .values = values,
                               .pairs = pairs, .structs = structs, .gmrfs = gmrfs,
                               .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_block(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                           const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                           const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                           const idhmc_glm_structs *structs, const idhmc_glm_gmrfs *gmrfs, const idhmc_glm_block *block,
                           int64_t M, int64_t chains_per_response, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_block: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .local = local, .factors = factors, .values = values,
                               .pairs = pairs, .structs = structs, .gmrfs = gmrfs, .block = block,
                               .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_create_glm_multi(idhmc_ctx **out, int device, int64_t nchains, int64_t first_chain_id,
                           const idhmc_glm_desc *glm, const idhmc_glm_priors *priors, const idhmc_glm_local *local,
                           const idhmc_glm_factors *factors, const idhmc_glm_factor_values *values, const idhmc_glm_pairs *pairs,
                           const idhmc_glm_structs *structs, const idhmc_glm_gmrfs *gmrfs, const idhmc_glm_block *block,
                           const idhmc_glm_members *members, int64_t M, int64_t chains_per_response, const idhmc_options *opt_in, uint64_t seed)
{
    if (!out || !glm) return fail(IDHMC_ERR_BAD_ARG, "idhmc_create_glm_multi: null argument");
    const idhmc_glm_model m = {.glm = glm, .priors = priors, .local = local, .factors = factors, .values = values,
                               .pairs = pairs, .structs = structs, .gmrfs = gmrfs, .block = block, .members = members,
                               .M = M, .chains_per_response = chains_per_response};
    return create_glm(out, device, nchains, first_chain_id, m, false, opt_in, seed);
}

int idhmc_glm_members_get(const idhmc_ctx *c, int32_t *width, int32_t *index, double *values)
{
    if (!c || !width) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_members_get: null argument");
    const int F = c->s.lr_f;
    const int64_t n = c->s.lr_n;
    if (c->s.lr_mp > 0) {
        std::copy(c->glm_mwidth.begin(), c->glm_mwidth.end(), width);
        if (index) std::copy(c->glm_mindex.begin(), c->glm_mindex.end(), index);
        if (values)
            for (size_t k = 0; k < c->glm_mindex.size(); ++k)
                values[k] = c->glm_mindex[k] < 0 ? 0.0 : c->glm_mvalues.empty() ? 1.0 : c->glm_mvalues[k];
        return IDHMC_OK;
    }
    // no wide term: F planes of width 1, the values of a term that has some and 1.0 elsewhere
    for (int f = 0; f < F; ++f) width[f] = 1;
    if (index) std::copy(c->glm_findex.begin(), c->glm_findex.end(), index);
    if (values)
        for (int f = 0; f < F; ++f)
            for (int64_t i = 0; i < n; ++i)
                values[f * n + i] = f < (int)c->glm_fhas.size() && c->glm_fhas[(size_t)f] ? c->glm_fvalues[(size_t)(f * n + i)] : 1.0;
    return IDHMC_OK;
}

int idhmc_glm_block_get(const idhmc_ctx *c, int32_t *K, int32_t *term, double *eta)
{
    if (!c || !K) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_block_get: null argument");
    *K = c->s.lr_bk;
    if (term) std::copy(c->glm_bterm.begin(), c->glm_bterm.end(), term);
    if (eta) *eta = c->glm_beta;
    return IDHMC_OK;
}

int idhmc_glm_gmrfs_get(const idhmc_ctx *c, int32_t *G, int32_t *term, double *kappa, int64_t *nnz)
{
    if (!c || !G) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_gmrfs_get: null argument");
    *G = c->s.lr_g;
    if (term) std::copy(c->glm_gterm.begin(), c->glm_gterm.end(), term);
    if (kappa) std::copy(c->glm_gkappa.begin(), c->glm_gkappa.end(), kappa);
    if (nnz) for (int i = 0; i < c->s.lr_g; ++i) nnz[i] = c->s.lr_gnz[i];
    return IDHMC_OK;
}

int idhmc_glm_structs_get(const idhmc_ctx *c, int32_t *S, int32_t *term, int32_t *kind, double *eta)
{
    if (!c || !S) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_structs_get: null argument");
    *S = c->s.lr_s;
    if (term) std::copy(c->glm_sterm.begin(), c->glm_sterm.end(), term);
    if (kind) std::copy(c->glm_skind.begin(), c->glm_skind.end(), kind);
    if (eta) std::copy(c->glm_seta.begin(), c->glm_seta.end(), eta);
    return IDHMC_OK;
}

int idhmc_glm_pairs_get(const idhmc_ctx *c, int32_t *P, int32_t *first, int32_t *second, double *eta)
{
    if (!c || !P) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_pairs_get: null argument");
    *P = c->s.lr_cp;
    if (first) std::copy(c->glm_pfirst.begin(), c->glm_pfirst.end(), first);
    if (second) std::copy(c->glm_psecond.begin(), c->glm_psecond.end(), second);
    if (eta) std::copy(c->glm_peta.begin(), c->glm_peta.end(), eta);
    return IDHMC_OK;
}

int idhmc_glm_factor_values_get(const idhmc_ctx *c, int32_t *has, double *values)
{
    if (!c || !has) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_factor_values_get: null argument");
    for (int f = 0; f < c->s.lr_f; ++f) has[f] = f < (int)c->glm_fhas.size() ? c->glm_fhas[(size_t)f] : 0;
    if (values) std::copy(c->glm_fvalues.begin(), c->glm_fvalues.end(), values);
    return IDHMC_OK;
}

int idhmc_glm_factors_get(const idhmc_ctx *c, int32_t *F, int32_t *levels, int32_t *index)
{
    if (!c || !F) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_factors_get: null argument");
    *F = c->s.lr_f;
    if (levels) std::copy(c->glm_flevels.begin(), c->glm_flevels.end(), levels);
    if (index) std::copy(c->glm_findex.begin(), c->glm_findex.end(), index);
    return IDHMC_OK;
}

int idhmc_glm_local_get(const idhmc_ctx *c, int32_t *local, double *slab_scale)
{
    if (!c || !local || !slab_scale) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_local_get: null argument");
    const int Dx = c->s.D - c->s.lr_a - c->s.lr_h - c->s.lr_j - c->s.lr_cp - block_zetas(c->s.lr_bk) - c->s.lr_sz;
    for (int k = 0; k < Dx; ++k) local[k] = c->glm_local.empty() ? 0 : c->glm_local[(size_t)k];
    *slab_scale = c->slab_scale;
    return IDHMC_OK;
}

int idhmc_glm_priors_get(const idhmc_ctx *c, int32_t *kind, double *nu)
{
    if (!c || !kind || !nu) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_priors_get: null argument");
    for (int k = 0; k < c->s.D; ++k) {
        kind[k] = c->prior_kind.empty() ? 0 : c->prior_kind[(size_t)k];
        nu[k] = c->prior_nu.empty() ? 0.0 : c->prior_nu[(size_t)k];
    }
    return IDHMC_OK;
}

int idhmc_glm_responses(const idhmc_ctx *c, int64_t *M, int64_t *chains_per_response)
{
    if (!c || !M || !chains_per_response) return fail(IDHMC_ERR_BAD_ARG, "idhmc_glm_responses: null argument");
    *M = c->glm_r > 0 ? c->s.lr_m : 1;
    *chains_per_response = c->glm_r;
    return IDHMC_OK;
}
int64_t idhmc_nchains(const idhmc_ctx *c) { return c ? c->s.C : 0; }
int32_t idhmc_dim(const idhmc_ctx *c) { return c ? c->s.D : 0; }
int32_t idhmc_padded_dim(const idhmc_ctx *c) { return c ? c->s.L : 0; }
int idhmc_glm_form(const idhmc_ctx *c)
{
    if (!c || (c->s.model != IDHMC_MODEL_LOGISTIC_REGRESSION && c->s.model != IDHMC_MODEL_GLM)) return -1;
    return glm_coop(c->s.nch, c->s.lr_a, c->s.minv_stride == 0) ? 1 : 0;
}
int64_t idhmc_device_bytes(const idhmc_ctx *c) { return c ? c->bytes : 0; }
int idhmc_placement_info(const idhmc_ctx *c, double *probe_GBps, int32_t *candidates)
{
    if (!c) return fail(IDHMC_ERR_BAD_ARG, "null context");
    if (probe_GBps) *probe_GBps = c->placement_GBps;
    if (candidates) *candidates = c->placement_tries;
    return IDHMC_OK;
}
int idhmc_leapfrog_slice_info(const idhmc_ctx *c, int32_t *stride_store, int32_t *stride_recompute)
{
    if (!c) return fail(IDHMC_ERR_BAD_ARG, "null context");
    if (stride_store) *stride_store = (int32_t)c->s.lf_stride;
    if (stride_recompute) *stride_recompute = (int32_t)c->s.lf_stride2;
    return IDHMC_OK;
}
int idhmc_lanes_info(const idhmc_ctx *c, int32_t *lanes, int32_t *on_distinct_queues)
{
    if (!c) return fail(IDHMC_ERR_BAD_ARG, "null context");
    int n = c->lane[1] ? 1 : 0;
    for (int k = 1; k < idhmc_ctx::kLanes; ++k) n += c->lane[k] != nullptr;
    if (lanes) *lanes = n;
    if (on_distinct_queues) *on_distinct_queues = c->lanes_distinct;
    return IDHMC_OK;
}
int idhmc_placement_cost(const idhmc_ctx *c, double *create_ms, int64_t *peak_transient_bytes, double *single_array_GBps, int32_t *kind)
{
    if (!c) return fail(IDHMC_ERR_BAD_ARG, "null context");
    if (create_ms) *create_ms = c->placement_ms;
    if (peak_transient_bytes) *peak_transient_bytes = c->placement_peak_bytes;
    if (single_array_GBps) *single_array_GBps = c->placement_single_GBps;
    if (kind) *kind = c->placement_kind;
    return IDHMC_OK;
}

