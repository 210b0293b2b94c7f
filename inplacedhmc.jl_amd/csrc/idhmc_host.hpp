// idhmc_host.hpp -- what the host units of the C ABI share (idhmc_api.hip, idhmc_create.hip, idhmc_place.hip, idhmc_drivers.hip): the
// context, the error text and the helpers that cross their boundaries.  Host only: nothing that hipRTC or a kernel unit includes
// may include this file.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <new>
#include <vector>
#include <algorithm>
#include <chrono>
#include <memory>
#include "idhmc_internal.hpp"
#include "idhmc_xchg.hpp"

namespace idhmc {
// sets the text of idhmc_last_error (one per thread) and returns `code`
int fail(int code, const char *fmt, ...);
}
using namespace idhmc;

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(IDHMC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
// every entry point starts here; CTXCHK_LANES is for the ones that may leave the dense leapfrog's lanes open (see idhmc_ctx)
#define CTXCHK_LANES(ctx)                                                    \
    do {                                                                     \
        if (!(ctx)) return fail(IDHMC_ERR_BAD_ARG, "null context");          \
        HIPCHK(hipSetDevice((ctx)->device));                                 \
    } while (0)
#define CTXCHK(ctx)                                                          \
    do {                                                                     \
        CTXCHK_LANES(ctx);                                                   \
        if (int rc_lanes_ = lanes_join(ctx)) return rc_lanes_;               \
    } while (0)

// an open posterior summary (idhmc_summary_begin; idhmc_summary.hip): the tables are the reduction's own arguments,
// DevState knows nothing of them
struct Summary {
    bool open = false, valid = false;     // valid: no idhmc_mcmc that fed it has failed
    bool ranged = false;                  // a histogram range is set: values reduced from now on are binned
    int64_t G = 0, groups = 0;            // chains per group, groups of this context
    int32_t spg = 0, bins = 0;            // segments of IDHMC_SUMMARY_SEGMENT chains per group, interior bins
    double *part = nullptr;               // [6][groups spg D] per-segment running state
    double *fin = nullptr;                // [6][groups D] the fold of the segments (k_summary_finish)
    double *rng = nullptr;                // [3][groups D] lo, hi, inv_w
    uint32_t *hist = nullptr;             // [groups][D][bins + 2]
    double *scales = nullptr;             // [scales_rows][H] group scales of a staged block's rows (GLM with coefficient groups)
    int64_t scales_rows = 0;
    uint64_t fed_t = 0, binned_t = 0;     // transitions reduced / binned since begin / set_range: times G, a group's counts
};

struct idhmc_ctx {
    int device = 0;
    DevState s{};
    idhmc_options opt{};
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    std::vector<void *> allocs;
    int64_t bytes = 0;
    int64_t glm_r = 0;             // idhmc_create_glm_responses: chains per response as given (0: any other context)
    std::vector<int32_t> prior_kind;   // idhmc_create_glm_priors with some kind != 0: kind and nu as given, D entries each (empty otherwise)
    std::vector<double> prior_nu;
    std::vector<int32_t> glm_local;    // idhmc_create_glm_local with some column flagged: local as given, Dx entries (empty otherwise)
    double slab_scale = 0.0;           // and its slab scale (0: none)
    std::vector<int32_t> glm_flevels;  // idhmc_create_glm_factors with F > 0: levels (F entries) and index (F x n) as given (empty otherwise)
    std::vector<int32_t> glm_findex;
    std::vector<int32_t> glm_fhas;     // idhmc_create_glm_slopes with a flag set: has (F entries) and values (F x n, rows of unflagged terms 0) (empty otherwise)
    std::vector<double> glm_fvalues;
    std::vector<int32_t> glm_pfirst, glm_psecond;   // idhmc_create_glm_corr with P > 0: the pairs' terms and eta as given (empty otherwise)
    std::vector<double> glm_peta;
    std::vector<int32_t> glm_sterm, glm_skind;      // idhmc_create_glm_struct with S > 0: the structured terms, their kinds and eta as given
    std::vector<double> glm_seta;
    std::vector<int32_t> glm_gterm;                 // idhmc_create_glm_gmrf with G > 0: the GMRF terms and their kappa as given
    std::vector<double> glm_gkappa;
    std::vector<int32_t> glm_bterm;                 // idhmc_create_glm_block with K > 0: the block's terms in row order and eta as given
    double glm_beta = 0.0;
    std::vector<int32_t> glm_mwidth, glm_mindex;    // idhmc_create_glm_multi with a wide term: width (F entries), index (P x n) and, where
    std::vector<double> glm_mvalues;                // given, values (P x n) as given (empty otherwise)
    // IDHMC_EPS_PER_RESPONSE / IDHMC_METRIC_PER_RESPONSE: the context holds resp_n = C / glm_r whole responses (0 in every other mode)
    int64_t resp_n = 0;
    double *resp_da = nullptr;     // [resp_n][6] dual-averaging states of IDHMC_EPS_PER_RESPONSE: mu, m, Hbar, logeps, logeps_bar, eps
    double *xchg = nullptr;        // library-owned exchange record (IDHMC_XCHG_DOUBLES)
    int32_t *status_out = nullptr; // device scalar
    double *scratch = nullptr;     // [C][L] staging for broadcasts / moments
    idhmc_allreduce_fn hook = nullptr;
    void *hook_user = nullptr;
    double *hook_buf = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    JitModule *jit = nullptr;      // hipRTC module of a custom density
    Comm *comm = nullptr;          // RCCL communicator of the global-eps exchange (idhmc_comm_init)
    // Pulse of the transition kernel: after every launch the device words {total leapfrog steps, abort code} are
    // copied asynchronously into a pinned ring, one slot per launch.  The drivers read it without ever synchronising
    // the stream: (1) the reference aborts the moment a chain's stepsize falls below 1e-10 (src/warmup.jl:291-296) --
    // the drivers keep at most kLag launches in flight and stop at the first slot that carries the code; (2)
    // measurement.
    static constexpr int kRing = 64, kLag = 8, kPulseWords = 2;
    unsigned long long *ring = nullptr;   // pinned host memory, kRing x kPulseWords; word 0 == ~0: not yet written
    uint64_t launches = 0;
    // switches from the environment, read once in idhmc_create
    int fuse = -1;                        // IDHMC_FUSE = 0 / 1: the drivers never / always make several transitions per launch (-1: yes)
    bool fuse_ok = false;                 // workgroups b and b + 8 share an XCD on this device (probed at creation): fused launches are possible
    bool test_xcc = false;                // IDHMC_TEST_XCC_MISMATCH=1: the transition flags may carry kTestXccFlag (test suite only)
    bool dense_mfma = true;               // IDHMC_DENSE_MFMA=0: the dense single-step leapfrog runs the per-wave GEMV kernel (tests)
    int use_lanes = kLanes;               // IDHMC_DENSE_LANES = 0 switches the dense leapfrog's lanes off, n caps their number (measurements)
    struct {                              // place_state's search, IDHMC_PLACEMENT_{TRIES, MAX_BYTES, WALK_BYTES, PAIRS, VERBOSE}
        int tries = 32;
        int64_t max_bytes = (int64_t)16 << 30, walk_bytes = (int64_t)64 << 30;
        bool pairs = true, verbose = false;
    } place;
    // The device copy of grad l lags behind q after (a) the single-step leapfrog of a separable density in its default mode,
    // IDHMC_GRAD_RECOMPUTE, and (b) every NUTS transition of a separable density: neither writes the array.  Every host entry
    // point whose kernel reads s.g goes through ensure_grad first -- idhmc_get_grad, both stepsize searches, find_local_optimum,
    // the n-step leapfrog, the IDHMC_GRAD_STORE single step and idhmc_time_leapfrog in that mode; set_q and random_position
    // evaluate and clear the flag.  The other readers of s.g (dense, JIT / GLM, logistic kernels, k_nuts of a non-separable
    // density) are unreachable for a separable model, and nothing else ever sets the flag (the list is in DESIGN 3.1)
    bool grad_stale = false;
    double *pool_scratch = nullptr;       // IDHMC_METRIC_POOLED: {acc0, acc1, mean}
    double *pool_table = nullptr;         // [segments][L + 1] partial sums (grown on demand)
    int64_t pool_table_segs = 0;
    double *ebfmi_out = nullptr;          // [C], idhmc_get_ebfmi
    // draws / records that the caller wants on the host leave through two staging buffers: the device packs transition n,
    // the host copies it out (a blocking pageable copy on its own stream) while transition n + 1 computes
    double *stage_q[2] = {nullptr, nullptr};
    idhmc_tree_stats *stage_st[2] = {nullptr, nullptr};
    int32_t stage_kq = 1, stage_kst = 1;  // transitions the staging buffers hold (idhmc_mcmc's launches of several transitions: more than one)
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_packed[2] = {nullptr, nullptr};
    Summary sum;                          // fed by idhmc_mcmc and idhmc_summary_add_draws while open
    // Lanes of the dense single-step leapfrog (configs[3]).  One sweep of its matrix-core kernel is a load phase, a matrix
    // phase and a store phase that every CU goes through at the same time, so HBM idles while the matrix cores work and vice
    // versa.  Chains are independent, so the context cuts them into up to kLanes contiguous ranges of tiles, each
    // swept on its own stream by a kernel of one workgroup per CU: three such kernels are resident per CU, in different phases,
    // and back-to-back sweeps pipeline across the lanes (lane k's sweep n + 1 waits only for lane k's sweep n).  Lane 0 is the
    // context's stream (the runtime spreads a process's streams over four hardware queues; two lanes on one queue run one
    // after the other); the others fork from it at the first such call and join it at the next entry point of any other kind.
    static constexpr int kLanes = 4;
    hipStream_t lane[kLanes] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t lane_ev[kLanes] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork_ev = nullptr;
    bool lanes_open = false;
    int lanes_distinct = 0;               // lanes (the context's stream included) found on different hardware queues
    double placement_GBps = 0.0;          // place_state: probe rate of the placement kept, candidates tried
    int placement_tries = 0;
    int placement_kind = 0;               // 0 separate allocations, 3 separate allocations found by the pair walk (1, 2: kinds no longer built)
    double placement_single_GBps = 0.0;   // one array alone (the yardstick of "good")
    double placement_ms = 0.0;            // wall time of place_state
    int64_t placement_peak_bytes = 0;     // most device bytes held at one time during the search
};

template <class T>
static int dalloc(idhmc_ctx *c, T **out, int64_t n, bool zero = true)
{
    void *p = nullptr;
    const size_t bytes = (size_t)(n > 0 ? n : 1) * sizeof(T);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(IDHMC_ERR_ALLOC, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    if (zero) {
        e = hipMemsetAsync(p, 0, bytes, c->stream);
        if (e != hipSuccess) return fail(IDHMC_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e));
    }
    c->allocs.push_back(p);
    c->bytes += (int64_t)bytes;
    *out = (T *)p;
    return IDHMC_OK;
}
namespace idhmc {
int lanes_join(idhmc_ctx *c);
void dfree(idhmc_ctx *c, void *p, int64_t bytes);                                          // idhmc_api.hip
int place_state(idhmc_ctx *c, double **out, int nvec, int64_t n, int64_t C, int L);       // idhmc_place.hip
// idhmc_api.hip, for the caller loops and the measurement helpers of idhmc_drivers.hip
int ensure_grad(idhmc_ctx *c);
int leapfrog_regrad(const idhmc_ctx *c, int32_t n_steps);
int leapfrog_any(idhmc_ctx *c, double eps, int own, int n_steps, int regrad);
int nuts_launch(idhmc_ctx *c, uint32_t iter, uint32_t flags, uint32_t n_iter, double *fz_q = nullptr, idhmc_tree_stats *fz_st = nullptr);
bool fuse_transitions(const idhmc_ctx *c);
int pulse_abort(idhmc_ctx *c, int lag);
int check_status(idhmc_ctx *c, const char *what);
int status_exchange(idhmc_ctx *c, const char *what);
double *xchg_buf(idhmc_ctx *c);
int stage_reserve(idhmc_ctx *c, int32_t K, bool draws, bool stats);                        // idhmc_drivers.hip
// idhmc_summary.hip, for idhmc_mcmc: may cnt more transitions be reduced; reduce the staged block [cnt][C][D] on the context's stream
int summary_admit(idhmc_ctx *c, int64_t cnt);
int summary_feed(idhmc_ctx *c, const double *stage, int32_t cnt);
int exchange(idhmc_ctx *c, double *buf);
}
