// idhmc_drivers.hip -- the reference's caller loops (warmup!(TuningNUTS), mcmc!, mcmc_with_warmup!, src/warmup.jl:269-332,
// src/mcmc.jl:94-105) run for all chains of a context, the pipeline that takes their draws and records to the host, and the
// measurement helpers.
#include "idhmc_host.hpp"


// ---- the reference's caller loops --------------------------------------------------------------------
// what sits between two adapting transitions where the stepsize is not a chain's own: the acceptance is pooled and the stepsize adapted
// behind the transition (global: the exchange record, the ranks' all-reduce, the adaptation; per response: one launch, nothing to exchange)
static int adapt_pooled_eps(idhmc_ctx *c)
{
    if (c->s.eps_mode == IDHMC_EPS_GLOBAL) {
        double *buf = xchg_buf(c);
        HIPCHK(launch_xchg_sum(c->s, IDHMC_XCHG_ACCEPT, buf, c->stream));
        if (int rc = exchange(c, buf)) return rc;
        HIPCHK(launch_da_adapt_global(c->s, buf, c->stream));
    } else if (c->s.eps_mode == IDHMC_EPS_PER_RESPONSE) {
        HIPCHK(launch_resp_eps(c->s, IDHMC_XCHG_ACCEPT, c->resp_da, c->glm_r, c->resp_n, c->stream));
    }
    return IDHMC_OK;
}
// one transition by a launch of its own; `adapt` with a global or per-response stepsize: adapt_pooled_eps behind it
static int one_transition(idhmc_ctx *c, uint32_t iter, uint32_t flags, bool adapt)
{
    if (int rc = idhmc_nuts_transition(c, iter, flags)) return rc;
    return adapt ? adapt_pooled_eps(c) : IDHMC_OK;
}
// ---- draws and records to the host, overlapped with the next transition ------------------------------------------------
// fetch_pack(n) is enqueued right behind transition n: the device packs the draw (padded rows -> contiguous) and the records
// into staging buffer n & 1.  stage_copy(n, 1, n & 1) is called AFTER transition n + 1 has been enqueued: it waits for the pack and
// copies to the caller's (pageable) arrays on a second stream -- the host blocks in that copy while the device computes.
// Buffer n & 1 is reused by pack(n + 2), which is enqueued after the copy of n has returned.
// stage_reserve: the staging buffers hold K transitions (grow-only; every path uses the same buffers)
int idhmc::stage_reserve(idhmc_ctx *c, int32_t K, bool draws, bool stats)
{
    const DevState &s = c->s;
    if (!c->copy_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) HIPCHK(hipEventCreateWithFlags(&c->ev_packed[b], hipEventDisableTiming));
    }
    for (int b = 0; b < 2; ++b) {
        if (draws && (!c->stage_q[b] || c->stage_kq < K)) {
            dfree(c, c->stage_q[b], (int64_t)sizeof(double) * c->stage_kq * s.C * s.D);
            c->stage_q[b] = nullptr;
            if (int rc = dalloc(c, &c->stage_q[b], (int64_t)K * s.C * s.D, false)) return rc;
        }
        if (stats && (!c->stage_st[b] || c->stage_kst < K)) {
            dfree(c, c->stage_st[b], (int64_t)sizeof(idhmc_tree_stats) * c->stage_kst * s.C);
            c->stage_st[b] = nullptr;
            if (int rc = dalloc(c, &c->stage_st[b], (int64_t)K * s.C, false)) return rc;
        }
    }
    if (draws && c->stage_kq < K) c->stage_kq = K;
    if (stats && c->stage_kst < K) c->stage_kst = K;
    return IDHMC_OK;
}
// `sum`: an open summary reduces the packed draw where it lies, right behind the pack (the host copy needs the pack alone)
static int fetch_pack(idhmc_ctx *c, int32_t n, bool draws, bool stats, bool sum)
{
    if (!draws && !stats) return IDHMC_OK;
    const int b = n & 1;
    HIPCHK(launch_pack_draw(c->s, draws ? c->stage_q[b] : nullptr, stats ? c->stage_st[b] : nullptr, c->stream));
    HIPCHK(hipEventRecord(c->ev_packed[b], c->stream));
    return sum ? summary_feed(c, c->stage_q[b], 1) : IDHMC_OK;
}
// transitions n0 .. n0 + cnt - 1 from staging buffer b to the caller's arrays
static int stage_copy(idhmc_ctx *c, int32_t n0, int32_t cnt, int b, double *draws, idhmc_tree_stats *stats)
{
    if (!draws && !stats) return IDHMC_OK;
    const DevState &s = c->s;
    const int64_t CD = s.C * (int64_t)s.D;
    HIPCHK(hipStreamWaitEvent(c->copy_stream, c->ev_packed[b], 0));
    if (draws) HIPCHK(hipMemcpyAsync(draws + (int64_t)n0 * CD, c->stage_q[b], sizeof(double) * (size_t)(cnt * CD), hipMemcpyDeviceToHost, c->copy_stream));
    if (stats) HIPCHK(hipMemcpyAsync(stats + (int64_t)n0 * s.C, c->stage_st[b], sizeof(idhmc_tree_stats) * (size_t)(cnt * s.C), hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(hipStreamSynchronize(c->copy_stream));
    return IDHMC_OK;
}

// Draws and records for the host with several transitions per launch: the kernel writes every transition's draw and record into a
// staging block of K transitions; block j is copied out (second stream, the host blocks in that copy) while block j + 1 computes, two
// blocks alternating.  K = what fits 256 MiB per block (at most 64; larger blocks gain nothing: with the draws kept the loop is bound
// by the copy into the caller's pageable array, 10-22 GB/s); a draw of more than half a block keeps the per-transition path (K = 0).
static int32_t block_transitions(const idhmc_ctx *c, int32_t N)
{
    if (N < 2) return 0;
    const int64_t per = c->s.C * (int64_t)c->s.D * (int64_t)sizeof(double) + c->s.C * (int64_t)sizeof(idhmc_tree_stats);
    const int64_t k = ((int64_t)256 << 20) / per;
    int32_t K = (int32_t)(k > N ? N : k);
    if (K > 64) K = 64;
    if (K < 2 || (uint64_t)c->s.C * (uint64_t)K >= (1ull << 31)) K = 0;
    return K;
}
// `sum`: the draws are staged for an open summary too (also when the host wants none), and each block is reduced behind its launch
static int run_blocks(idhmc_ctx *c, uint32_t iter_first, int32_t N, uint32_t fl, int32_t K, double *draws, idhmc_tree_stats *stats, bool sum)
{
    int32_t prev_n0 = -1, prev_cnt = 0;
    int blk = 0;
    for (int32_t n0 = 0; n0 < N; n0 += K, ++blk) {
        const int32_t cnt = N - n0 < K ? N - n0 : K;
        const int b = blk & 1;
        if (int rc = nuts_launch(c, iter_first + (uint32_t)n0, fl, (uint32_t)cnt, draws || sum ? c->stage_q[b] : nullptr, stats ? c->stage_st[b] : nullptr)) return rc;
        HIPCHK(hipEventRecord(c->ev_packed[b], c->stream));
        if (sum) { if (int rc = summary_feed(c, c->stage_q[b], cnt)) return rc; }
        if (prev_n0 >= 0) { if (int rc = stage_copy(c, prev_n0, prev_cnt, b ^ 1, draws, stats)) return rc; }      // ... while block blk computes
        prev_n0 = n0; prev_cnt = cnt;
    }
    if (prev_n0 >= 0) { if (int rc = stage_copy(c, prev_n0, prev_cnt, (blk - 1) & 1, draws, stats)) return rc; }
    HIPCHK(hipStreamSynchronize(c->stream));
    return IDHMC_OK;
}
// N transitions, the first one `iter_first`, for idhmc_tuning_stage (`adapt`: the stepsize adapts; `stop_on_abort`) and idhmc_mcmc:
// in blocks of K transitions, in one launch, or one launch per transition.  `feed` (idhmc_mcmc): an open summary takes every draw, so
// the draws are staged on the device whether or not the host wants them; the host copies stay the non-null pointers' alone
static int run_transitions(idhmc_ctx *c, uint32_t iter_first, int32_t N, uint32_t flags, bool adapt, bool stop_on_abort,
                           double *draws, idhmc_tree_stats *stats, bool feed)
{
    const bool sum = feed && c->sum.open;
    const bool stage_q = draws || sum;
    const bool any = stage_q || stats;
    // the global and the per-response stepsize adapt between transitions: one launch each
    const bool fusable = fuse_transitions(c) && !(adapt && (c->s.eps_mode == IDHMC_EPS_GLOBAL || c->s.eps_mode == IDHMC_EPS_PER_RESPONSE));
    const int32_t K = any && fusable ? block_transitions(c, N) : 0;
    if (any) { if (int rc = stage_reserve(c, K ? K : 1, stage_q, stats != nullptr)) return rc; }
    if (adapt && c->s.eps_mode == IDHMC_EPS_PER_CHAIN) flags |= IDHMC_T_ADAPT_EPS;
    if (K) return run_blocks(c, iter_first, N, flags, K, draws, stats, sum);     // the draws / records leave in blocks of K transitions
    if (!any && fusable && N > 1) {
        // nothing leaves the device per transition: one launch (the kernel itself stops handing out
        // transitions once a chain has raised the abort code)
        if (int rc = idhmc_nuts_transitions(c, iter_first, N, flags)) return rc;
        if (stop_on_abort) (void)pulse_abort(c, 0);        // (waits for the launch: the stage's verdict is agreed on below)
        return IDHMC_OK;
    }
    int32_t done = 0;
    for (int32_t n = 0; n < N; ++n) {                                            // src/warmup.jl:288-305, :324-330
        // the reference throws as soon as eps < 1e-10 (:291-296): stop within kLag transitions of the one that set it
        if (stop_on_abort && pulse_abort(c, idhmc_ctx::kLag)) break;
        if (int rc = one_transition(c, iter_first + (uint32_t)n, flags, adapt)) return rc;
        if (int rc = fetch_pack(c, n, stage_q, stats != nullptr, sum)) return rc;
        if (n > 0) { if (int rc = stage_copy(c, n - 1, 1, (n - 1) & 1, draws, stats)) return rc; }   // ... while transition n computes
        done = n + 1;
    }
    if (done > 0) { if (int rc = stage_copy(c, done - 1, 1, (done - 1) & 1, draws, stats)) return rc; }
    return IDHMC_OK;
}
int idhmc_tuning_stage(idhmc_ctx *c, int32_t N, int32_t adapt_metric, uint32_t iter0, double *draws, idhmc_tree_stats *stats)
{
    CTXCHK(c);
    if (N < 1) return fail(IDHMC_ERR_BAD_ARG, "N must be >= 1");
    if (adapt_metric && !c->s.mw_x1) return fail(IDHMC_ERR_BAD_ARG, "shared-metric context cannot adapt the metric");
    if (adapt_metric && N < 2) return fail(IDHMC_ERR_BAD_ARG, "metric window needs N >= 2");
    if (int rc = idhmc_da_init(c)) return rc;                                    // src/warmup.jl:284
    if (adapt_metric) { if (int rc = idhmc_metric_begin(c)) return rc; }
    const double lambda = 5.0 / (double)N;                                       // src/warmup.jl:229
    if (int rc = run_transitions(c, iter0 + 1u, N, adapt_metric ? IDHMC_T_ACCUM_METRIC : 0u, true, true, draws, stats, false)) return rc;
    // sharded: agree on the outcome first -- a rank that failed alone would leave the others in the pooled metric's all-reduces
    if (int rc = status_exchange(c, "warmup")) return rc;
    if (adapt_metric) { if (int rc = idhmc_metric_update(c, lambda)) return rc; } // :308-311
    return idhmc_da_finalize(c);                                                 // :313
}
int idhmc_mcmc(idhmc_ctx *c, int32_t N, uint32_t iter0, double *draws, idhmc_tree_stats *stats)
{
    CTXCHK(c);
    if (N < 0) return fail(IDHMC_ERR_BAD_ARG, "N must be >= 0");
    const uint32_t fl = (c->s.mom_mean ? IDHMC_T_ACCUM_MOMENTS : 0u) | (c->s.diag.n ? IDHMC_T_ACCUM_DIAG : 0u);
    if (int rc = summary_admit(c, N)) return rc;
    int rc = run_transitions(c, iter0 + 1u, N, fl, false, false, draws, stats, true);
    // A status still pending (a refused launch, a caller's own transition that underflowed) must not pass as success: a launch of
    // several transitions hands out none while the abort word is set, and the staging blocks are not zeroed.  A local check (it
    // also waits for the stream): sampling has no collective that a rank failing alone could leave the others waiting in.
    // An open summary has then reduced staging rows that may never have been written: it is invalid until idhmc_summary_begin.
    if (!rc) rc = check_status(c, "mcmc");
    if (rc && c->sum.open) c->sum.valid = false;
    return rc;
}
int idhmc_mcmc_with_warmup(idhmc_ctx *c, int32_t N, double *draws, idhmc_tree_stats *stats)
{
    CTXCHK(c);
    const idhmc_options &o = c->opt;
    uint32_t iter = 0;
    if (int rc = idhmc_random_position(c)) return rc;                            // initialize_warmup_state, src/warmup.jl:100-129
    if (o.local_opt_iterations > 0) {                                            // FindLocalOptimum, src/warmup.jl:152-186
        if (int rc = idhmc_find_local_optimum(c, o.local_opt_penalty, o.local_opt_iterations)) return rc;
    }
    if (int rc = idhmc_set_eps(c, o.eps_init)) return rc;
    if (o.stepsize_search) {                                                     // src/warmup.jl:188-200
        if (int rc = idhmc_refresh_momentum(c, 0)) return rc;
        if (int rc = idhmc_find_initial_stepsize(c)) return rc;
    }
    const int adapt = o.adapt_metric && c->s.mw_x1;
    if (int rc = idhmc_tuning_stage(c, o.init_steps, 0, iter, nullptr, nullptr)) return rc;           // src/warmup.jl:369
    iter += (uint32_t)o.init_steps;
    for (int d = 0; d < o.doubling_stages; ++d) {                                                     // :341-344
        const int32_t n = o.middle_steps << d;
        if (int rc = idhmc_tuning_stage(c, n, adapt, iter, nullptr, nullptr)) return rc;
        iter += (uint32_t)n;
    }
    if (int rc = idhmc_tuning_stage(c, o.terminating_steps, 0, iter, nullptr, nullptr)) return rc;    // :371
    iter += (uint32_t)o.terminating_steps;
    return idhmc_mcmc(c, N, iter, draws, stats);                                                      // src/mcmc.jl:104
}

// ---- measurement helpers ----------------------------------------------------------------------------
// the events ev0, ev1 around what `enqueue` puts on the context's stream: the milliseconds between them
template <class F>
static int time_bracket(idhmc_ctx *c, float *ms, F enqueue)
{
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if (int rc = enqueue()) return rc;
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev1));
    HIPCHK(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return IDHMC_OK;
}
int idhmc_time_leapfrog(idhmc_ctx *c, double eps, int32_t sweeps, float *ms_per_sweep)
{
    CTXCHK(c);
    if (sweeps < 1 || !ms_per_sweep) return fail(IDHMC_ERR_BAD_ARG, "bad arguments");
    const int regrad = leapfrog_regrad(c, 1);
    if (!regrad) { if (int rc = ensure_grad(c)) return rc; }     // (before the first event: the pair brackets the sweeps alone)
    float ms = 0.f;
    if (int rc = time_bracket(c, &ms, [&]() -> int {
            for (int i = 0; i < sweeps; ++i) { if (int rc = leapfrog_any(c, eps, 0, 1, regrad)) return rc; }
            if (regrad) c->grad_stale = true;
            return lanes_join(c);
        })) return rc;
    *ms_per_sweep = ms / (float)sweeps;
    return IDHMC_OK;
}
int idhmc_time_transitions(idhmc_ctx *c, int32_t n, uint32_t iter0, float *ms_total)
{
    CTXCHK(c);
    if (n < 1 || !ms_total) return fail(IDHMC_ERR_BAD_ARG, "bad arguments");
    return time_bracket(c, ms_total, [&]() -> int {
        for (int i = 0; i < n; ++i) { if (int rc = idhmc_nuts_transition(c, iter0 + 1u + (uint32_t)i, 0u)) return rc; }
        return IDHMC_OK;
    });
}
int idhmc_time_transitions_fused(idhmc_ctx *c, int32_t n, uint32_t iter0, float *ms_total)
{
    CTXCHK(c);
    if (n < 1 || !ms_total) return fail(IDHMC_ERR_BAD_ARG, "bad arguments");
    return time_bracket(c, ms_total, [&]() -> int { return idhmc_nuts_transitions(c, iter0 + 1u, n, 0u); });
}
int idhmc_time_eps_adapt(idhmc_ctx *c, int32_t n, float *ms_total)
{
    CTXCHK(c);
    if (n < 1 || !ms_total) return fail(IDHMC_ERR_BAD_ARG, "bad arguments");
    if (c->s.eps_mode != IDHMC_EPS_GLOBAL && c->s.eps_mode != IDHMC_EPS_PER_RESPONSE)
        return fail(IDHMC_ERR_BAD_ARG, "the per-chain stepsize adapts inside the transition kernel");
    return time_bracket(c, ms_total, [&]() -> int {
        for (int i = 0; i < n; ++i) { if (int rc = adapt_pooled_eps(c)) return rc; }
        return IDHMC_OK;
    });
}
