// idhmc_api.hip -- the C ABI (include/idhmc.h) of a context that exists: state transfer, the leapfrog and its lanes, transitions
// and their pulse, the exchange protocol and status, metric, moments and diagnostics.  Creation is idhmc_create.hip, the placement
// of the state arrays idhmc_place.hip, the reference's caller loops idhmc_drivers.hip.
#include <cstdarg>
#include "idhmc_host.hpp"

static thread_local char g_err[512] = "";
int idhmc::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
const char *idhmc_last_error(void) { return g_err; }
int idhmc_version(void) { return IDHMC_VERSION; }
#ifndef IDHMC_SOURCE_DIGEST
#define IDHMC_SOURCE_DIGEST "unknown"
#endif
const char *idhmc_build_digest(void) { return IDHMC_SOURCE_DIGEST; }

int idhmc::lanes_join(idhmc_ctx *c)
{
    if (!c->lanes_open) return IDHMC_OK;
    c->lanes_open = false;
    for (int k = 1; k < idhmc_ctx::kLanes; ++k) {
        if (!c->lane[k]) continue;
        HIPCHK(hipEventRecord(c->lane_ev[k], c->lane[k]));
        HIPCHK(hipStreamWaitEvent(c->stream, c->lane_ev[k], 0));
    }
    return IDHMC_OK;
}
// number of kernels a single-step sweep of this context is cut into (0: one kernel on the context's stream): ranges of at most
// 256 tiles, so that every kernel puts one workgroup on every CU; kernel j runs on lane j mod kLanes
static int lane_chunks(const idhmc_ctx *c, int n_steps)
{
    if (c->use_lanes < 2 || n_steps != 1 || c->s.model != IDHMC_MODEL_DENSE_MVN || c->s.nch > 2) return 0;
    if (c->stream != c->own_stream) return 0;     // a caller-owned stream is ordered by the caller's events, not by our entry points
    const int64_t ntiles = (c->s.C + 15) / 16;
    const int64_t n = (ntiles + 255) / 256;
    return n < 3 ? 0 : (int)n;
}
// Lanes only overlap when they sit on DIFFERENT hardware queues: the runtime multiplexes a process's streams onto four of them
// (least-used first at creation), and two streams on one queue run one after the other.  Which queue a new stream gets depends
// on every stream the process has made before (a context created after others, a runtime-internal stream ...: round 3's bench
// ran the lanes on three queues, 63 instead of 48 us per sweep), so the lanes are CHOSEN: candidates are created one by one and
// a candidate becomes a lane when an idle 60 us kernel on it runs concurrently with one on every lane chosen so far.
static bool streams_overlap(hipStream_t a, hipStream_t b)
{
    const long long ticks = 6000;                    // 60 us of the 100 MHz wall clock
    double best = 1e30;
    for (int r = 0; r < 2; ++r) {
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return false;
        const auto t0 = std::chrono::steady_clock::now();
        if (launch_spin(ticks, a) != hipSuccess || launch_spin(ticks, b) != hipSuccess) return false;
        (void)hipStreamSynchronize(a);
        (void)hipStreamSynchronize(b);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (us < best) best = us;
    }
    return best < 1.6 * 60.0;                        // one after the other: >= 120 us
}
static int pick_lane_streams(idhmc_ctx *c, int lanes)
{
    constexpr int kCand = 10;
    hipStream_t cand[kCand] = {};
    int ncand = 0, have = 1;                         // lane 0 is the context's stream
    for (int k = 1; k < lanes; ++k) if (c->lane[k]) ++have;
    while (have < lanes && ncand < kCand) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }   // what we have will do
        cand[ncand++] = s;
        bool ok = streams_overlap(c->stream, s);
        for (int k = 1; k < lanes && ok; ++k) if (c->lane[k]) ok = streams_overlap(c->lane[k], s);
        if (!ok) continue;
        for (int k = 1; k < lanes; ++k) if (!c->lane[k]) { c->lane[k] = s; cand[ncand - 1] = nullptr; ++have; break; }
    }
    // nothing overlaps with anything (a profiler that serialises the streams): take the candidates as they come, as round 2 did
    for (int k = 1, j = 0; k < lanes; ++k) {
        if (c->lane[k]) continue;
        while (j < ncand && !cand[j]) ++j;
        if (j < ncand) { c->lane[k] = cand[j]; cand[j] = nullptr; }
        else HIPCHK(hipStreamCreateWithFlags(&c->lane[k], hipStreamNonBlocking));
    }
    c->lanes_distinct = have;
    for (int j = 0; j < ncand; ++j) if (cand[j]) (void)hipStreamDestroy(cand[j]);
    for (int k = 1; k < lanes; ++k)
        if (!c->lane_ev[k]) HIPCHK(hipEventCreateWithFlags(&c->lane_ev[k], hipEventDisableTiming));
    return IDHMC_OK;
}
static int leapfrog_lanes(idhmc_ctx *c, double eps, int own, int chunks)
{
    const int lanes = chunks < c->use_lanes ? chunks : c->use_lanes;
    if (!c->fork_ev) HIPCHK(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
    {
        bool missing = false;
        for (int k = 1; k < lanes; ++k) missing |= !c->lane[k];
        if (missing) { if (int rc = pick_lane_streams(c, lanes)) return rc; }
    }
    if (!c->lanes_open) {
        HIPCHK(hipEventRecord(c->fork_ev, c->stream));
        for (int k = 1; k < lanes; ++k) HIPCHK(hipStreamWaitEvent(c->lane[k], c->fork_ev, 0));
        c->lanes_open = true;
    }
    const int64_t ntiles = (c->s.C + 15) / 16;
    for (int j = 0; j < chunks; ++j)
        HIPCHK(launch_leapfrog_dense_mfma_tiles(c->s, eps, own, 1, ntiles * j / chunks, ntiles * (j + 1) / chunks, 256,
                                                (j % lanes) ? c->lane[j % lanes] : c->stream));
    return IDHMC_OK;
}
// one fused leapfrog launch (or one per lane) for the entry points below
int idhmc::leapfrog_any(idhmc_ctx *c, double eps, int own, int n_steps, int regrad)
{
    const int chunks = c->dense_mfma ? lane_chunks(c, n_steps) : 0;
    if (chunks) return leapfrog_lanes(c, eps, own, chunks);
    if (int rc = lanes_join(c)) return rc;
    HIPCHK(launch_leapfrog(c->s, eps, own, n_steps, regrad, c->dense_mfma, c->stream));
    return IDHMC_OK;
}

// give one allocation of the context back early (staging buffers that are outgrown); `bytes` as it was counted by dalloc
void idhmc::dfree(idhmc_ctx *c, void *p, int64_t bytes)
{
    if (!p) return;
    for (size_t i = 0; i < c->allocs.size(); ++i)
        if (c->allocs[i] == p) { c->allocs.erase(c->allocs.begin() + (long)i); break; }
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(p);
    c->bytes -= bytes;
}

int idhmc_set_stream(idhmc_ctx *c, void *hip_stream)
{
    CTXCHK(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return IDHMC_OK;
}
int idhmc_synchronize(idhmc_ctx *c)
{
    CTXCHK(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    return IDHMC_OK;
}

// host [C][D] <-> device [C][L]
static int put_vec(idhmc_ctx *c, double *dst, const double *src, int64_t rows)
{
    const DevState &s = c->s;
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(double) * s.L, src, sizeof(double) * s.D, sizeof(double) * s.D,
                            (size_t)rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return IDHMC_OK;
}
static int get_vec(idhmc_ctx *c, double *dst, const double *src, int64_t rows)
{
    const DevState &s = c->s;
    HIPCHK(hipMemcpy2DAsync(dst, sizeof(double) * s.D, src, sizeof(double) * s.L, sizeof(double) * s.D,
                            (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return IDHMC_OK;
}

int idhmc_set_q(idhmc_ctx *c, const double *q)
{
    CTXCHK(c);
    if (!q) return fail(IDHMC_ERR_BAD_ARG, "null q");
    if (int rc = put_vec(c, c->s.q, q, c->s.C)) return rc;
    HIPCHK(launch_eval(c->s, 0, c->stream));
    c->grad_stale = false;
    return IDHMC_OK;
}
int idhmc_random_position(idhmc_ctx *c)
{
    CTXCHK(c);
    HIPCHK(launch_eval(c->s, 1, c->stream));
    c->grad_stale = false;
    return IDHMC_OK;
}
int idhmc_set_p(idhmc_ctx *c, const double *p)
{
    CTXCHK(c);
    if (!p) return fail(IDHMC_ERR_BAD_ARG, "null p");
    return put_vec(c, c->s.p, p, c->s.C);
}
int idhmc_set_minv(idhmc_ctx *c, const double *minv, int per_chain)
{
    CTXCHK(c);
    if (!minv) return fail(IDHMC_ERR_BAD_ARG, "null minv");
    DevState &s = c->s;
    const int64_t n = per_chain ? s.C * (int64_t)s.D : (int64_t)s.D;
    for (int64_t i = 0; i < n; ++i)
        if (!(minv[i] > 0.0) || !std::isfinite(minv[i])) return fail(IDHMC_ERR_BAD_ARG, "M^-1 must be positive and finite");
    if (s.minv_stride == 0) {
        if (per_chain) return fail(IDHMC_ERR_BAD_ARG, "context has a shared metric (metric_mode = SHARED)");
        if (int rc = put_vec(c, s.minv, minv, 1)) return rc;
    } else if (per_chain) {
        if (int rc = put_vec(c, s.minv, minv, s.C)) return rc;
    } else {
        // broadcast D values to every chain: row 0 from the host, the rest on the device
        if (int rc = put_vec(c, s.minv, minv, 1)) return rc;
        HIPCHK(launch_broadcast_row(s.minv, s.L, s.C, c->stream));
    }
    HIPCHK(launch_set_w(s, c->stream));
    return IDHMC_OK;
}
int idhmc_set_eps(idhmc_ctx *c, double eps)
{
    CTXCHK(c);
    if (!(eps > 0.0) || !std::isfinite(eps)) return fail(IDHMC_ERR_BAD_ARG, "eps must be positive and finite");
    HIPCHK(launch_fill(c->s.eps, eps, c->s.C, c->stream));
    return IDHMC_OK;
}
int idhmc_set_eps_per_chain(idhmc_ctx *c, const double *eps)
{
    CTXCHK(c);
    if (!eps) return fail(IDHMC_ERR_BAD_ARG, "null eps");
    HIPCHK(hipMemcpyAsync(c->s.eps, eps, sizeof(double) * c->s.C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return IDHMC_OK;
}
int idhmc_get_q(idhmc_ctx *c, double *q) { CTXCHK(c); return q ? get_vec(c, q, c->s.q, c->s.C) : fail(IDHMC_ERR_BAD_ARG, "null out"); }
int idhmc_get_p(idhmc_ctx *c, double *p) { CTXCHK(c); return p ? get_vec(c, p, c->s.p, c->s.C) : fail(IDHMC_ERR_BAD_ARG, "null out"); }
int idhmc_get_grad(idhmc_ctx *c, double *g)
{
    CTXCHK(c);
    if (!g) return fail(IDHMC_ERR_BAD_ARG, "null out");
    if (int rc = ensure_grad(c)) return rc;
    return get_vec(c, g, c->s.g, c->s.C);
}
int idhmc_get_minv(idhmc_ctx *c, double *m)
{
    CTXCHK(c);
    if (!m) return fail(IDHMC_ERR_BAD_ARG, "null out");
    const DevState &s = c->s;
    if (s.minv_stride) return get_vec(c, m, s.minv, s.C);
    if (int rc = get_vec(c, m, s.minv, 1)) return rc;
    for (int64_t ch = 1; ch < s.C; ++ch) memcpy(m + ch * s.D, m, sizeof(double) * s.D);
    return IDHMC_OK;
}
static int get_scalar(idhmc_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return IDHMC_OK;
}
int idhmc_get_lq(idhmc_ctx *c, double *lq) { CTXCHK(c); return lq ? get_scalar(c, lq, c->s.lq, sizeof(double) * c->s.C) : fail(IDHMC_ERR_BAD_ARG, "null out"); }
int idhmc_get_eps(idhmc_ctx *c, double *e) { CTXCHK(c); return e ? get_scalar(c, e, c->s.eps, sizeof(double) * c->s.C) : fail(IDHMC_ERR_BAD_ARG, "null out"); }
int idhmc_logdensity(idhmc_ctx *c, double *pi)
{
    CTXCHK(c);
    if (!pi) return fail(IDHMC_ERR_BAD_ARG, "null out");
    HIPCHK(launch_logdensity(c->s, c->stream));
    return get_scalar(c, pi, c->s.pi, sizeof(double) * c->s.C);
}

int idhmc_refresh_momentum(idhmc_ctx *c, uint32_t iter)
{
    CTXCHK(c);
    HIPCHK(launch_refresh(c->s, iter, c->stream));
    return IDHMC_OK;
}
// the stored gradient is needed: bring it up to date (evaluate_l! from q: the same bits every leapfrog would have stored)
int idhmc::ensure_grad(idhmc_ctx *c)
{
    if (c->grad_stale) {
        HIPCHK(launch_eval(c->s, 0, c->stream));
        c->grad_stale = false;
    }
    return IDHMC_OK;
}
int idhmc::leapfrog_regrad(const idhmc_ctx *c, int32_t n_steps)
{
    return (c->opt.leapfrog_grad_mode == IDHMC_GRAD_RECOMPUTE && model_is_separable(c->s.model) && n_steps == 1) ? 1 : 0;
}
int idhmc_set_leapfrog_grad_mode(idhmc_ctx *c, int32_t mode)
{
    CTXCHK(c);
    if (mode != IDHMC_GRAD_STORE && mode != IDHMC_GRAD_RECOMPUTE) return fail(IDHMC_ERR_BAD_ARG, "unknown gradient mode %d", mode);
    c->opt.leapfrog_grad_mode = mode;
    return IDHMC_OK;
}
// idhmc_leapfrog (own = 0) and idhmc_leapfrog_own_eps (own = 1)
static int leapfrog_steps(idhmc_ctx *c, double eps, int own, int32_t n_steps)
{
    CTXCHK_LANES(c);
    if (n_steps < 1) return fail(IDHMC_ERR_BAD_ARG, "n_steps must be >= 1");
    if (!own && !std::isfinite(eps)) return fail(IDHMC_ERR_BAD_ARG, "eps must be finite");
    const int regrad = leapfrog_regrad(c, n_steps);
    if (!regrad) { if (int rc = ensure_grad(c)) return rc; }
    if (int rc = leapfrog_any(c, eps, own, n_steps, regrad)) return rc;
    if (regrad) c->grad_stale = true;
    return IDHMC_OK;
}
int idhmc_leapfrog(idhmc_ctx *c, double eps, int32_t n_steps) { return leapfrog_steps(c, eps, 0, n_steps); }
int idhmc_leapfrog_own_eps(idhmc_ctx *c, int32_t n_steps) { return leapfrog_steps(c, 0.0, 1, n_steps); }
int idhmc::nuts_launch(idhmc_ctx *c, uint32_t iter, uint32_t flags, uint32_t n_iter, double *fz_q, idhmc_tree_stats *fz_st)
{
    if ((flags & IDHMC_T_ACCUM_METRIC) && !c->s.mw_x1) return fail(IDHMC_ERR_BAD_ARG, "shared-metric context cannot accumulate a metric window");
    if ((flags & IDHMC_T_ACCUM_MOMENTS) && !c->s.mom_mean) {
        if (int rc = idhmc_moments_reset(c)) return rc;
    }
    if ((flags & IDHMC_T_ACCUM_DIAG) && !c->s.diag.n) {
        if (int rc = idhmc_diag_reset(c)) return rc;
    }
    volatile unsigned long long *slot = c->ring + (c->launches % idhmc_ctx::kRing) * idhmc_ctx::kPulseWords;
    if (slot[0] == ~0ull && c->launches >= (uint64_t)idhmc_ctx::kRing) HIPCHK(hipStreamSynchronize(c->stream));   // slot still in flight
    slot[0] = ~0ull;
    HIPCHK(launch_nuts(c->s, iter, flags, c->stream, n_iter, fz_q, fz_st));
    // the transition of a separable density leaves grad l of the new state unwritten (8 KB per chain and transition that nothing on
    // the sampling path reads: the kernel re-derives the gradient from q); whoever needs the array re-evaluates first (ensure_grad)
    if (model_is_separable(c->s.model)) c->grad_stale = true;
    HIPCHK(hipMemcpyAsync(const_cast<unsigned long long *>(slot), c->s.total_steps + kPulseAt, sizeof(unsigned long long) * idhmc_ctx::kPulseWords,
                          hipMemcpyDeviceToHost, c->stream));
    ++c->launches;
    return IDHMC_OK;
}
// the public flags: the IDHMC_T_* set, and the XCD test's bit on a context that opted in at creation
static int check_flags(const idhmc_ctx *c, uint32_t flags)
{
    constexpr uint32_t kDocumented = IDHMC_T_ADAPT_EPS | IDHMC_T_ACCUM_METRIC | IDHMC_T_ACCUM_MOMENTS | IDHMC_T_KEEP_P |
                                     IDHMC_T_USE_DIRECTIONS | IDHMC_T_ACCUM_DIAG;
    const uint32_t unknown = flags & ~(kDocumented | (c->test_xcc ? kTestXccFlag : 0u));
    if (unknown) return fail(IDHMC_ERR_BAD_ARG, "unknown transition flags 0x%x", unknown);
    return IDHMC_OK;
}
int idhmc_nuts_transition(idhmc_ctx *c, uint32_t iter, uint32_t flags)
{
    CTXCHK(c);
    if (int rc = check_flags(c, flags)) return rc;
    if ((flags & IDHMC_T_ADAPT_EPS) && c->s.eps_mode == IDHMC_EPS_PER_RESPONSE) return fail(IDHMC_ERR_BAD_ARG, "the per-response stepsize adapts between transitions");
    return nuts_launch(c, iter, flags, 1);
}
int idhmc_nuts_transitions(idhmc_ctx *c, uint32_t iter, int32_t n, uint32_t flags)
{
    CTXCHK(c);
    if (int rc = check_flags(c, flags)) return rc;
    if (n < 1) return fail(IDHMC_ERR_BAD_ARG, "n must be >= 1");
    if ((uint64_t)c->s.C * (uint64_t)n >= (1ull << 31)) return fail(IDHMC_ERR_BAD_ARG, "nchains * n must be below 2^31");
    if (flags & (IDHMC_T_USE_DIRECTIONS | IDHMC_T_KEEP_P)) return fail(IDHMC_ERR_BAD_ARG, "injected directions / a kept momentum are one transition's");
    if ((flags & IDHMC_T_ADAPT_EPS) && c->s.eps_mode == IDHMC_EPS_GLOBAL) return fail(IDHMC_ERR_BAD_ARG, "the global stepsize adapts between transitions");
    if ((flags & IDHMC_T_ADAPT_EPS) && c->s.eps_mode == IDHMC_EPS_PER_RESPONSE) return fail(IDHMC_ERR_BAD_ARG, "the per-response stepsize adapts between transitions");
    if (!c->fuse_ok) {       // (a device whose workgroups b and b + 8 do not share an XCD: the same result from n launches)
        for (int32_t i = 0; i < n; ++i) { if (int rc = nuts_launch(c, iter + (uint32_t)i, flags, 1)) return rc; }
        return IDHMC_OK;
    }
    return nuts_launch(c, iter, flags, (uint32_t)n);
}
int idhmc_fused_launch_info(idhmc_ctx *c, int32_t *possible, int32_t *used_by_drivers)
{
    CTXCHK(c);
    if (possible) *possible = c->fuse_ok ? 1 : 0;
    if (used_by_drivers) *used_by_drivers = (c->fuse_ok && c->fuse != 0) ? 1 : 0;
    return IDHMC_OK;
}
// do the drivers make several transitions per launch (where nothing leaves the device per transition)?  Measured gains: dense
// configs[3] +29 % (3.5e8 against 2.7e8 leapfrog/s, 20 per launch), 1024-dim diagonal Gaussian at 65 536 chains +6-9 % (depth 4), +1.5 %
// (depth 7), D = 256 +22 %: the end of every launch and the gap to the next are paid once.  IDHMC_FUSE=0 restores one launch per transition.
bool idhmc::fuse_transitions(const idhmc_ctx *c)
{
    return c->fuse != 0 && c->fuse_ok;
}
// The abort code of the launch `lag` launches back (waiting for it to arrive: this is what bounds the drivers' run-ahead),
// 0 when there is none.  Used by the caller loops only; a caller driving idhmc_nuts_transition itself polls with
// idhmc_poll_abort.
int idhmc::pulse_abort(idhmc_ctx *c, int lag)
{
    if (c->launches < (uint64_t)lag + 1) return 0;
    volatile unsigned long long *slot = c->ring + ((c->launches - 1 - lag) % idhmc_ctx::kRing) * idhmc_ctx::kPulseWords;
    while (slot[0] == ~0ull) {
        if (hipStreamQuery(c->stream) == hipSuccess) break;       // everything has run (the copy included)
    }
    return slot[0] == ~0ull ? 0 : (int)slot[1];
}
int idhmc_poll_abort(idhmc_ctx *c, int32_t lag, int32_t *code)
{
    CTXCHK(c);
    if (lag < 0 || lag >= idhmc_ctx::kRing - 1 || !code) return fail(IDHMC_ERR_BAD_ARG, "lag must be in [0, %d)", idhmc_ctx::kRing - 1);
    *code = pulse_abort(c, lag);
    return IDHMC_OK;
}
int idhmc_set_directions(idhmc_ctx *c, const uint32_t *d)
{
    CTXCHK(c);
    if (!d) return fail(IDHMC_ERR_BAD_ARG, "null directions");
    HIPCHK(hipMemcpyAsync(c->s.directions, d, sizeof(uint32_t) * c->s.C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return IDHMC_OK;
}
int idhmc_get_tree_stats(idhmc_ctx *c, idhmc_tree_stats *st)
{
    CTXCHK(c);
    if (!st) return fail(IDHMC_ERR_BAD_ARG, "null out");
    return get_scalar(c, st, c->s.stats, sizeof(idhmc_tree_stats) * c->s.C);
}

int idhmc::check_status(idhmc_ctx *c, const char *what)
{
    HIPCHK(launch_status_max(c->s, c->status_out, c->stream));
    int32_t st = 0;
    if (int rc = get_scalar(c, &st, c->status_out, sizeof st)) return rc;
    if (st == 0) return IDHMC_OK;
    HIPCHK(hipMemsetAsync(c->s.status, 0, sizeof(int32_t) * c->s.C, c->stream));
    HIPCHK(hipMemsetAsync(c->s.total_steps + kPulseAt + 1, 0, sizeof(unsigned long long), c->stream));   // the abort word
    for (int i = 0; i < idhmc_ctx::kRing; ++i)       // ... and its copies (the stream is idle: get_scalar synchronised)
        if (c->ring[i * idhmc_ctx::kPulseWords] != ~0ull) c->ring[i * idhmc_ctx::kPulseWords + 1] = 0;
    switch (st) {
    case IDHMC_ERR_EPS_UNDERFLOW: return fail(st, "%s: a chain's stepsize fell below 1e-10 (reference src/warmup.jl:291-296)", what);
    case IDHMC_ERR_STEPSIZE_SEARCH: return fail(st, "%s: reached maximum number of iterations searching for eps (reference src/stepsize.jl:71,101)", what);
    case IDHMC_ERR_NONFINITE_START: return fail(st, "%s: starting point has non-finite density (reference src/stepsize.jl:152-153)", what);
    case IDHMC_ERR_OPTIMIZATION: return fail(st, "%s: Optimization failed to converge (reference src/warmup.jl:172)", what);
    case IDHMC_ERR_HIP: return fail(st, "%s: a launch of several transitions gave up (a chain range served from two XCDs, or a hand-over that never came)", what);
    default: return fail(st, "%s: device status %d", what, st);
    }
}

// the exchange record lives in the caller's buffer when a hook is set, else in the library's
double *idhmc::xchg_buf(idhmc_ctx *c) { return c->hook ? c->hook_buf : c->xchg; }
// SUM-all-reduce the record over the ranks, on the context's stream: hook > communicator > single rank (nothing)
int idhmc::exchange(idhmc_ctx *c, double *buf)
{
    if (c->hook) {
        if (int rc = c->hook(buf, c->hook_user)) return fail(IDHMC_ERR_BAD_ARG, "all-reduce hook returned %d", rc);
    } else if (c->comm) {
        char err[200];
        if (comm_allreduce_sum(c->comm, buf, IDHMC_XCHG_DOUBLES, c->stream, err, sizeof err)) return fail(IDHMC_ERR_HIP, "%s", err);
    }
    return IDHMC_OK;
}

int idhmc_find_local_optimum(idhmc_ctx *c, double magnitude_penalty, int32_t iterations)
{
    CTXCHK(c);
    if (!(magnitude_penalty >= 0.0) || iterations < 0) return fail(IDHMC_ERR_BAD_ARG, "penalty and iterations must be >= 0");
    if (int rc = ensure_grad(c)) return rc;
    HIPCHK(launch_local_optimum(c->s, magnitude_penalty, iterations, c->stream));
    return status_exchange(c, "find_local_optimum");     // sharded contexts agree on the outcome (one more 4-double exchange)
}
int idhmc_find_initial_stepsize_per_chain(idhmc_ctx *c)
{
    CTXCHK(c);
    if (int rc = ensure_grad(c)) return rc;
    HIPCHK(launch_stepsize_search(c->s, c->stream));
    return check_status(c, "find_initial_stepsize");
}
// A sharded stage fails on every rank or on none: `peers` is the all-reduced slot [3] of an exchange record (chains with a
// pending status, over all ranks).  The rank that owns such a chain returns its code, the others IDHMC_ERR_PEER.
static int status_agreed(idhmc_ctx *c, const char *what, double peers)
{
    if (int rc = check_status(c, what)) return rc;
    if (peers > 0.0) return fail(IDHMC_ERR_PEER, "%s: %.0f chain(s) of other rank(s) raised an error; the stage fails on every rank", what, peers);
    return IDHMC_OK;
}
// the same without a record at hand: one exchange of {0, 0, 0, local chains with a pending status}
static bool sharded(const idhmc_ctx *c) { return c->hook || c->comm; }
int idhmc::status_exchange(idhmc_ctx *c, const char *what)
{
    if (!sharded(c)) return check_status(c, what);
    double *buf = xchg_buf(c);
    HIPCHK(launch_xchg_sum(c->s, IDHMC_XCHG_STATUS, buf, c->stream));
    if (int rc = exchange(c, buf)) return rc;
    double rec[IDHMC_XCHG_DOUBLES];
    if (int rc = get_scalar(c, rec, buf, sizeof rec)) return rc;
    return status_agreed(c, what, rec[3]);
}
int idhmc_find_initial_stepsize(idhmc_ctx *c)
{
    CTXCHK(c);
    if (c->s.eps_mode == IDHMC_EPS_PER_RESPONSE) {
        // one eps per response: exp(mean log eps) over its searches.  The context holds whole responses, so nothing is exchanged but
        // the outcome, as for per-chain stepsizes
        if (int rc = ensure_grad(c)) return rc;
        HIPCHK(launch_stepsize_search(c->s, c->stream));
        HIPCHK(launch_resp_eps(c->s, IDHMC_XCHG_LOGEPS, c->resp_da, c->glm_r, c->resp_n, c->stream));
        return status_exchange(c, "find_initial_stepsize");
    }
    if (c->s.eps_mode != IDHMC_EPS_GLOBAL && !sharded(c)) return idhmc_find_initial_stepsize_per_chain(c);
    if (int rc = ensure_grad(c)) return rc;
    HIPCHK(launch_stepsize_search(c->s, c->stream));
    // per-chain stepsizes of a sharded run: nothing to pool, but the ranks agree on the outcome (a rank that failed alone would leave
    // the others in the next stage's collectives)
    if (c->s.eps_mode != IDHMC_EPS_GLOBAL) return status_exchange(c, "find_initial_stepsize");
    // one eps for everybody: exp(mean log eps) over the chains of ALL ranks -- the fixed-point record is exact under
    // any all-reduce order, and the engine's own dlog / dexp run on the device, so every rank holds the same bits.
    // The exchange is enqueued BEFORE any error is looked at: a rank whose search failed still takes part, and the record's
    // slot [3] tells every rank that the stage failed (a rank that returned early would leave the others in the all-reduce).
    double *buf = xchg_buf(c);
    HIPCHK(launch_xchg_sum(c->s, IDHMC_XCHG_LOGEPS, buf, c->stream));
    if (int rc = exchange(c, buf)) return rc;
    HIPCHK(launch_eps_from_logeps(c->s, buf, c->stream));
    double rec[IDHMC_XCHG_DOUBLES];
    if (int rc = get_scalar(c, rec, buf, sizeof rec)) return rc;
    return status_agreed(c, "find_initial_stepsize", rec[3]);
}
int idhmc_da_init(idhmc_ctx *c)
{
    CTXCHK(c);
    if (c->s.eps_mode == IDHMC_EPS_PER_RESPONSE) HIPCHK(launch_resp_da_init(c->s, c->resp_da, c->glm_r, c->resp_n, c->stream));
    else HIPCHK(launch_da_init(c->s, c->stream));
    return IDHMC_OK;
}
int idhmc_da_finalize(idhmc_ctx *c)
{
    CTXCHK(c);
    if (c->s.eps_mode == IDHMC_EPS_PER_RESPONSE) HIPCHK(launch_resp_da_finalize(c->s, c->resp_da, c->glm_r, c->stream));
    else HIPCHK(launch_da_finalize(c->s, c->stream));
    return IDHMC_OK;
}
static int xchg_sum(idhmc_ctx *c, int32_t kind, double *dev_xchg)
{
    CTXCHK(c);
    if (!dev_xchg) return fail(IDHMC_ERR_BAD_ARG, "null device buffer");
    HIPCHK(launch_xchg_sum(c->s, kind, dev_xchg, c->stream));
    return IDHMC_OK;
}
int idhmc_accept_sum(idhmc_ctx *c, double *dev_xchg) { return xchg_sum(c, IDHMC_XCHG_ACCEPT, dev_xchg); }
int idhmc_logeps_sum(idhmc_ctx *c, double *dev_xchg) { return xchg_sum(c, IDHMC_XCHG_LOGEPS, dev_xchg); }
int idhmc_da_adapt_global(idhmc_ctx *c, const double *dev_xchg)
{
    CTXCHK(c);
    if (!dev_xchg) return fail(IDHMC_ERR_BAD_ARG, "null device buffer");
    if (c->s.eps_mode != IDHMC_EPS_GLOBAL) return fail(IDHMC_ERR_BAD_ARG, "context is not in global-eps mode");
    HIPCHK(launch_da_adapt_global(c->s, dev_xchg, c->stream));
    return IDHMC_OK;
}
int idhmc_set_eps_from_logeps(idhmc_ctx *c, const double *dev_xchg)
{
    CTXCHK(c);
    if (!dev_xchg) return fail(IDHMC_ERR_BAD_ARG, "null device buffer");
    HIPCHK(launch_eps_from_logeps(c->s, dev_xchg, c->stream));
    return IDHMC_OK;
}
// host side of the same protocol (no device involved)
int idhmc_xchg_accumulate(int32_t kind, const double *values, int64_t n, double *xchg4)
{
    if (kind != IDHMC_XCHG_ACCEPT && kind != IDHMC_XCHG_LOGEPS) return fail(IDHMC_ERR_BAD_ARG, "unknown exchange kind %d", kind);
    if (n < 0 || (n > 0 && !values) || !xchg4) return fail(IDHMC_ERR_BAD_ARG, "bad arguments");
    long long hi = 0, lo = 0;
    for (int64_t i = 0; i < n; ++i) {
        long long h, l;
        xchg_limbs(kind, values[i], h, l);
        hi += h; lo += l;
    }
    xchg4[0] += (double)hi;
    xchg4[1] += (double)lo;
    xchg4[2] += (double)n;
    return IDHMC_OK;
}
int idhmc_xchg_mean(int32_t kind, const double *xchg4, double *mean)
{
    if (kind != IDHMC_XCHG_ACCEPT && kind != IDHMC_XCHG_LOGEPS) return fail(IDHMC_ERR_BAD_ARG, "unknown exchange kind %d", kind);
    if (!xchg4 || !mean) return fail(IDHMC_ERR_BAD_ARG, "bad arguments");
    *mean = xchg_mean(kind, xchg4[0], xchg4[1], xchg4[2]);
    return IDHMC_OK;
}
int idhmc_set_allreduce_hook(idhmc_ctx *c, idhmc_allreduce_fn fn, void *user, double *dev_xchg)
{
    CTXCHK(c);
    if (fn && !dev_xchg) return fail(IDHMC_ERR_BAD_ARG, "hook needs a device buffer");
    c->hook = fn; c->hook_user = user; c->hook_buf = dev_xchg;
    return IDHMC_OK;
}
int idhmc_comm_unique_id(void *id128)
{
    if (!id128) return fail(IDHMC_ERR_BAD_ARG, "null id buffer");
    char err[200];
    if (comm_unique_id(id128, err, sizeof err)) return fail(IDHMC_ERR_HIP, "%s", err);
    return IDHMC_OK;
}
int idhmc_comm_init(idhmc_ctx *c, int32_t nranks, int32_t rank, const void *id128)
{
    CTXCHK(c);
    if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(IDHMC_ERR_BAD_ARG, "bad communicator arguments");
    if (c->comm) return fail(IDHMC_ERR_BAD_ARG, "context already has a communicator");
    char err[200];
    c->comm = comm_create(nranks, rank, id128, err, sizeof err);
    if (!c->comm) return fail(IDHMC_ERR_HIP, "%s", err);
    return IDHMC_OK;
}
int idhmc_comm_destroy(idhmc_ctx *c)
{
    CTXCHK(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    comm_destroy(c->comm);
    c->comm = nullptr;
    return IDHMC_OK;
}
int idhmc_comm_allreduce(idhmc_ctx *c, double *dev_buf, int32_t n)
{
    CTXCHK(c);
    if (!dev_buf || n < 1) return fail(IDHMC_ERR_BAD_ARG, "bad buffer");
    if (!c->comm) return fail(IDHMC_ERR_BAD_ARG, "context has no communicator");
    char err[200];
    if (comm_allreduce_sum(c->comm, dev_buf, n, c->stream, err, sizeof err)) return fail(IDHMC_ERR_HIP, "%s", err);
    return IDHMC_OK;
}
int idhmc_comm_info(idhmc_ctx *c, int32_t *nranks, int32_t *rank, int64_t *allreduces)
{
    if (!c) return fail(IDHMC_ERR_BAD_ARG, "null context");
    int nr = 0, r = 0;
    long long n = 0;
    comm_info(c->comm, &nr, &r, &n);
    if (nranks) *nranks = nr;
    if (rank) *rank = r;
    if (allreduces) *allreduces = n;
    return IDHMC_OK;
}
static int pool_table_reserve(idhmc_ctx *c, long long nseg)
{
    if (nseg < 1 || nseg > 65535) return fail(IDHMC_ERR_BAD_ARG, "pooled metric: %lld segments of %d chains out of range", nseg, IDHMC_POOL_SEGMENT);
    if (nseg > c->pool_table_segs) {
        if (int rc = dalloc(c, &c->pool_table, nseg * (int64_t)(c->s.L + 1), false)) return rc;   // (the smaller one stays until destroy)
        c->pool_table_segs = nseg;
    }
    return IDHMC_OK;
}
// the pooled metric by hand (a host that exchanges the table itself), include/idhmc.h
int idhmc_pool_partials(idhmc_ctx *c, int32_t pass, double *dev_table, int64_t seg_lo, int64_t seg_hi)
{
    CTXCHK(c);
    if (c->s.minv_stride != 0 || !c->s.mw_x1) return fail(IDHMC_ERR_BAD_ARG, "context is not in pooled-metric mode");
    if (!dev_table || (pass != 0 && pass != 1) || seg_lo < 0 || seg_hi <= seg_lo) return fail(IDHMC_ERR_BAD_ARG, "bad arguments");
    HIPCHK(launch_pool_partials(c->s, pass, c->pool_scratch, dev_table, seg_lo, seg_hi, c->stream));
    return IDHMC_OK;
}
int idhmc_pool_consume(idhmc_ctx *c, int32_t pass, const double *dev_table, int64_t nseg, double lambda)
{
    CTXCHK(c);
    if (c->s.minv_stride != 0 || !c->s.mw_x1) return fail(IDHMC_ERR_BAD_ARG, "context is not in pooled-metric mode");
    if (!dev_table || (pass != 0 && pass != 1) || nseg < 1 || !(lambda >= 0.0)) return fail(IDHMC_ERR_BAD_ARG, "bad arguments");
    HIPCHK(launch_pool_consume(c->s, pass, c->pool_scratch, dev_table, nseg, lambda, c->stream));
    return IDHMC_OK;
}
int idhmc_metric_begin(idhmc_ctx *c)
{
    CTXCHK(c);
    HIPCHK(hipMemsetAsync(c->s.mw_n, 0, sizeof(int32_t) * c->s.C, c->stream));
    return IDHMC_OK;
}
int idhmc_metric_update(idhmc_ctx *c, double lambda)
{
    CTXCHK(c);
    if (!c->s.mw_x1) return fail(IDHMC_ERR_BAD_ARG, "shared-metric context has no metric window");
    if (!(lambda >= 0.0)) return fail(IDHMC_ERR_BAD_ARG, "lambda must be >= 0");
    if (c->opt.metric_mode == IDHMC_METRIC_PER_RESPONSE) {      // the pooled sums with one instance per response, no collective
        HIPCHK(launch_resp_metric(c->s, lambda, c->glm_r, c->resp_n, c->stream));
        return IDHMC_OK;
    }
    if (c->s.minv_stride == 0) {
        // pooled: every chain's window, on every rank when the context has a communicator.  The table of per-segment
        // partials covers the global segments [0, ceil(total / IDHMC_POOL_SEGMENT)); the total comes from an exact all-reduce
        // of the chain counts (shards tile [0, total)), a lone context covers just its own segments.
        const DevState &s = c->s;
        long long seg_lo = (long long)s.first_chain / IDHMC_POOL_SEGMENT;
        long long seg_hi = ((long long)s.first_chain + s.C + IDHMC_POOL_SEGMENT - 1) / IDHMC_POOL_SEGMENT;
        char err[200];
        if (c->comm) {
            double cnt[IDHMC_XCHG_DOUBLES] = {0.0, 0.0, (double)s.C, 0.0};
            HIPCHK(hipMemcpyAsync(c->xchg, cnt, sizeof cnt, hipMemcpyHostToDevice, c->stream));
            if (comm_allreduce_sum(c->comm, c->xchg, IDHMC_XCHG_DOUBLES, c->stream, err, sizeof err)) return fail(IDHMC_ERR_HIP, "%s", err);
            if (int rc = get_scalar(c, cnt, c->xchg, sizeof cnt)) return rc;
            seg_lo = 0;
            seg_hi = ((long long)cnt[2] + IDHMC_POOL_SEGMENT - 1) / IDHMC_POOL_SEGMENT;
        }
        const long long nseg = seg_hi - seg_lo;
        if (int rc = pool_table_reserve(c, nseg)) return rc;
        for (int pass = 0; pass < 2; ++pass) {
            HIPCHK(launch_pool_partials(s, pass, c->pool_scratch, c->pool_table, seg_lo, seg_hi, c->stream));
            if (c->comm && comm_allreduce_sum(c->comm, c->pool_table, (int)(nseg * (s.L + 1)), c->stream, err, sizeof err))
                return fail(IDHMC_ERR_HIP, "%s", err);
            HIPCHK(launch_pool_consume(s, pass, c->pool_scratch, c->pool_table, nseg, lambda, c->stream));
        }
        return IDHMC_OK;
    }
    HIPCHK(launch_metric_update(c->s, lambda, c->stream));
    return IDHMC_OK;
}
int idhmc_moments_reset(idhmc_ctx *c)
{
    CTXCHK(c);
    DevState &s = c->s;
    const int64_t CL = s.C * s.L;
    if (!s.mom_mean) {
        if (int rc = dalloc(c, &s.mom_mean, CL)) return rc;
        if (int rc = dalloc(c, &s.mom_m2, CL)) return rc;
        if (int rc = dalloc(c, &s.mom_n, s.C)) return rc;
    } else {
        HIPCHK(hipMemsetAsync(s.mom_mean, 0, sizeof(double) * CL, c->stream));
        HIPCHK(hipMemsetAsync(s.mom_m2, 0, sizeof(double) * CL, c->stream));
        HIPCHK(hipMemsetAsync(s.mom_n, 0, sizeof(int64_t) * s.C, c->stream));
    }
    return IDHMC_OK;
}
int idhmc_get_moments(idhmc_ctx *c, double *mean, double *var, int64_t *count)
{
    CTXCHK(c);
    DevState &s = c->s;
    if (!s.mom_mean) return fail(IDHMC_ERR_BAD_ARG, "no moments accumulated");
    const int64_t CL = s.C * s.L;
    if (!c->scratch) { if (int rc = dalloc(c, &c->scratch, 2 * CL)) return rc; }
    HIPCHK(launch_moments_get(s, c->scratch, c->scratch + CL, c->stream));
    if (mean) { if (int rc = get_vec(c, mean, c->scratch, s.C)) return rc; }
    if (var) { if (int rc = get_vec(c, var, c->scratch + CL, s.C)) return rc; }
    if (count) { if (int rc = get_scalar(c, count, s.mom_n, sizeof(int64_t) * s.C)) return rc; }
    return IDHMC_OK;
}
// ---- diagnostics reduced on the device (src/diagnostics.jl:28-32, 61-101) -----------------------------------
int idhmc_diag_reset(idhmc_ctx *c)
{
    CTXCHK(c);
    DevState &s = c->s;
    if (!s.diag.n) {
        if (int rc = dalloc(c, &s.diag.n, s.C)) return rc;
        if (int rc = dalloc(c, &s.diag.pi1, s.C)) return rc;
        if (int rc = dalloc(c, &s.diag.prev, s.C)) return rc;
        if (int rc = dalloc(c, &s.diag.s1, s.C)) return rc;
        if (int rc = dalloc(c, &s.diag.s2, s.C)) return rc;
        if (int rc = dalloc(c, &s.diag.d2, s.C)) return rc;
        if (int rc = dalloc(c, &s.diag.counters, (int64_t)IDHMC_DIAG_COUNTERS)) return rc;
        if (int rc = dalloc(c, &c->ebfmi_out, s.C)) return rc;
    } else {
        HIPCHK(hipMemsetAsync(s.diag.n, 0, sizeof(int32_t) * s.C, c->stream));
        // (the sums too: the kernel writes them with a window's first record, and idhmc_get_ebfmi on an empty window must find what a
        // fresh context has -- zeros, hence NaN -- not the previous window's)
        HIPCHK(hipMemsetAsync(s.diag.s1, 0, sizeof(double) * s.C, c->stream));
        HIPCHK(hipMemsetAsync(s.diag.s2, 0, sizeof(double) * s.C, c->stream));
        HIPCHK(hipMemsetAsync(s.diag.d2, 0, sizeof(double) * s.C, c->stream));
        HIPCHK(hipMemsetAsync(s.diag.counters, 0, sizeof(unsigned long long) * IDHMC_DIAG_COUNTERS, c->stream));
    }
    return IDHMC_OK;
}
int idhmc_get_diag_counters(idhmc_ctx *c, uint64_t *counters)
{
    CTXCHK(c);
    if (!counters) return fail(IDHMC_ERR_BAD_ARG, "null out");
    if (!c->s.diag.n) return fail(IDHMC_ERR_BAD_ARG, "no diagnostics accumulated (idhmc_diag_reset first)");
    return get_scalar(c, counters, c->s.diag.counters, sizeof(uint64_t) * IDHMC_DIAG_COUNTERS);
}
int idhmc_tree_summary_from_counters(const uint64_t *cn, idhmc_tree_summary *out)
{
    if (!cn || !out) return fail(IDHMC_ERR_BAD_ARG, "null argument");
    memset(out, 0, sizeof *out);
    const uint64_t N = cn[0];
    out->N = (int64_t)N;
    out->max_depth = (int64_t)cn[3]; out->divergence = (int64_t)cn[4]; out->turning = (int64_t)cn[5];
    for (int d = 0; d < 33; ++d) out->depth_counts[d] = (int64_t)cn[6 + d];
    if (N == 0) return IDHMC_OK;
    out->a_mean = xchg_mean(IDHMC_XCHG_ACCEPT, (double)(int64_t)cn[1], (double)cn[2], (double)N);
    // sample quantile (linear interpolation between the order statistics on either side of position q (N - 1)), each order statistic
    // located in the histogram and taken as equally spaced inside its bin: both are within a bin's width of the sample's, so their
    // interpolation is too -- also when they lie in different bins with empty ones between them
    auto order_statistic = [cn](uint64_t i) {
        uint64_t below = 0;
        for (int b = 0; b < IDHMC_DIAG_ACC_BINS; ++b) {
            const uint64_t nb = cn[39 + b];
            if (i < below + nb) return ((double)b + ((double)(i - below) + 0.5) / (double)nb) / (double)IDHMC_DIAG_ACC_BINS;
            below += nb;
        }
        return 1.0;
    };
    static const double qs[5] = {0.05, 0.25, 0.5, 0.75, 0.95};       // ACCEPTANCE_QUANTILES, src/diagnostics.jl:35
    for (int k = 0; k < 5; ++k) {
        const double pos = qs[k] * (double)(N - 1);
        const uint64_t i = (uint64_t)pos;
        const double lo = order_statistic(i), frac = pos - (double)i;
        out->a_quantiles[k] = frac > 0.0 && i + 1 < N ? lo + frac * (order_statistic(i + 1) - lo) : lo;
    }
    return IDHMC_OK;
}
int idhmc_get_ebfmi(idhmc_ctx *c, double *ebfmi)
{
    CTXCHK(c);
    if (!ebfmi) return fail(IDHMC_ERR_BAD_ARG, "null out");
    if (!c->s.diag.n) return fail(IDHMC_ERR_BAD_ARG, "no diagnostics accumulated (idhmc_diag_reset first)");
    HIPCHK(launch_ebfmi(c->s, c->ebfmi_out, c->stream));
    return get_scalar(c, ebfmi, c->ebfmi_out, sizeof(double) * c->s.C);
}

int idhmc_total_steps(idhmc_ctx *c, int64_t *steps)
{
    CTXCHK(c);
    if (!steps) return fail(IDHMC_ERR_BAD_ARG, "null out");
    unsigned long long v = 0;
    if (int rc = get_scalar(c, &v, c->s.total_steps, sizeof v)) return rc;
    *steps = (int64_t)v;
    return IDHMC_OK;
}

int idhmc_debug_counters(idhmc_ctx *c, uint64_t *out32)
{
    CTXCHK(c);
    if (!out32) return fail(IDHMC_ERR_BAD_ARG, "null out");
    return get_scalar(c, out32, c->s.total_steps, sizeof(uint64_t) * 32);
}
