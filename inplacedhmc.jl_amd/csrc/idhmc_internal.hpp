// idhmc_internal.hpp -- host/device shared descriptors and launcher prototypes (not part of the ABI).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "../../include/idhmc.h"

namespace idhmc {

// dual-averaging state, reference DualAveragingState (src/stepsize.jl:196-202), SoA over chains
struct DaArrays {
    double *mu, *Hbar, *logeps, *logeps_bar;
    int64_t *m;
};

// device-side diagnostics (IDHMC_T_ACCUM_DIAG): per chain the running sums of EBFMI, shifted by the first pi; per
// context the integer counters of include/idhmc.h
struct DiagArrays {
    int32_t *n;                                // [C] transitions accumulated
    double *pi1, *prev, *s1, *s2, *d2;         // [C] first pi, previous pi, sum(pi - pi1), sum (pi - pi1)^2, sum (diff pi)^2
    unsigned long long *counters;              // [IDHMC_DIAG_COUNTERS]
};

// everything a kernel needs, passed by value
struct DevState {
    int64_t C;            // chains in this context
    int32_t L, D, nch;    // padded length, dimension, L/128
    int32_t model;        // IDHMC_MODEL_*
    uint32_t k0, k1;      // Philox key = seed
    uint32_t first_chain; // global id of chain 0
    // A GLM with several responses (idhmc_create_glm_responses): lr_y is [lr_m][K][lr_npad] and the chain of GLOBAL id
    // g = first_chain + c samples response g / lr_r (chains_per_response, capped at 2^32 - 1: chain ids fit 32 bits, so a larger one is one
    // response all the same).  lr_m = 1, lr_r = 0 for every other context.  Both sit where the struct had alignment padding: its size and
    // every other offset are what they were, so no ahead-of-time kernel changes (tools/kres.py, profiles/r09_kres_*.txt).
    uint32_t lr_r;
    double *q, *p, *g;    // [C][L]
    double *lq, *pi;      // [C]  l(q),  pi = l(q) - K(p)
    double *eps;          // [C]
    double *minv, *w;     // [C][L] (minv_stride = L) or [L] shared (minv_stride = 0)
    int64_t minv_stride;
    int64_t lf_stride;        // k_leapfrog1: chains c % lf_stride == 0 are the Infinity-Cache slice (idhmc_create, kIcSliceBytes)
    int64_t lf_stride2;       // the same for the REGRAD variants, which touch q and p only: a slice of two arrays
    const double *mu, *tau;   // [L]
    const double *prec;       // [L][L]
    const double *lr_x, *lr_xt, *lr_y;   // IDHMC_MODEL_LOGISTIC_REGRESSION, _GLM: X [lr_npad][L], X' [L][lr_npad], Y [lr_m][K][lr_npad], zero-padded
    int32_t lr_n, lr_npad;               // observations, and rounded up to a multiple of 128
    int32_t lr_a;                        // a GLM's auxiliary coordinates: X has D - lr_a - lr_h columns, lr_a coordinates after them are theirs (0: none)
    int32_t lr_h;                        // a GLM's coefficient groups: the last lr_h coordinates are their log scales (0: none)
    const double *user_params;   // IDHMC_MODEL_CUSTOM: the user's parameter blob; IDHMC_MODEL_GLM: its constants
    int64_t user_nparams;
    const void *jit;             // host only: the hipRTC module of a custom density or a GLM
    // NUTS
    int32_t max_depth;
    int32_t lr_m;             // responses of a GLM (see lr_r)
    double min_delta;
    idhmc_tree_stats *stats;  // [C]
    uint32_t *directions;     // [C] injected directions
    double *arena;            // per wave slot tree storage
    int64_t arena_stride;     // doubles per slot
    int32_t nslots;           // persistent waves
    uint32_t *queue;          // chain work counter
    uint32_t n_iter;          // transitions per chain of the launch being made (launch_nuts sets it in its copy of the state; 0 / 1: one)
    uint32_t *iters_done;     // [C] n_iter > 1: transitions of this launch each chain has completed (zeroed by launch_nuts)
    double *fz_q;             // this launch's draws leave here, [n_iter][C][D] contiguous rows (null: nobody wants them); set per launch
    idhmc_tree_stats *fz_st;  // and its records, [n_iter][C]
    // adaptation
    DaArrays da;
    double da_delta, da_gamma, da_kappa;
    int32_t da_t0;
    int32_t eps_mode;
    double *da_global;        // [8] global dual-averaging state: mu, m, Hbar, logeps, logeps_bar, eps
    unsigned long long *xchg_acc;   // [3 * kXchgBlocks + 1] per-workgroup integer partials + ticket of the exchange sum (k_xchg_sum)
    // metric window: x1, sum delta, sum delta^2 ([C][L] each), draws in the window [C]
    double *mw_x1, *mw_s1, *mw_s2;
    int32_t *mw_n;
    // running moments: mean, M2 ([C][L]), count [C]
    double *mom_mean, *mom_m2;
    int64_t *mom_n;
    // stepsize search
    double ss_a_min, ss_a_max, ss_eps0, ss_C;
    int32_t ss_maxiter_crossing, ss_maxiter_bisect;
    int32_t *status;          // [C] per-chain error codes from the search / eps underflow
    DiagArrays diag;          // all null until idhmc_diag_reset
    unsigned long long *total_steps;  // [32]: the pulse the host polls = {[0] leapfrog steps, [1] abort code (an IDHMC_ERR_* a
                                      // chain raised: eps underflow)}; [2..9] cycle stamps of the diagnostic build (-DIDHMC_STAMPS)
    const int32_t *lr_grp;    // [L] a GLM with lr_h > 0: the group of every coordinate, -1 for ungrouped and padded ones (null otherwise)
    // a GLM with a non-Gaussian prior on some coordinate (idhmc_create_glm_priors; both null otherwise)
    const int32_t *lr_pkind;  // [L] IDHMC_PRIOR_* of every coordinate, 0 for padded ones
    const double *lr_pnu;     // [L] degrees of freedom of the kinds that take them, 0 elsewhere
    // a GLM with per-coefficient local scales (idhmc_create_glm_local; null, 0, 0 otherwise): the last lr_j coordinates
    // are their logarithms, X has D - lr_a - lr_h - lr_j columns
    const int32_t *lr_lpart;  // [L] the partner of every coordinate: a flagged column's lambda, a lambda's column, -1 elsewhere
    double lr_inv2;           // 1 / slab_scale^2 (0: no slab)
    int32_t lr_j;
    // a GLM with factor terms (idhmc_create_glm_factors; 0 and null otherwise, and then lr_x is [lr_npad][L] as above).
    // Appended: every other offset is what it was, so no kernel of a model without factors changes (profiles/r17_glm_factors_kres_*.txt).
    int32_t lr_f;             // factors, 0..4
    const int32_t *lr_fidx;   // [lr_f][lr_npad] the level of every observation, -1 in the padding
    const int32_t *lr_fstart; // [lr_npad / 128][lr_fcols + 1] per block of 128 observations: where each level's list starts in the block's bytes
    const unsigned char *lr_fpos;   // [lr_npad / 128][128 lr_f] per block: its observations (place in the block) sorted by factor, level, place
    int32_t lr_dd, lr_lx;     // dense (stored) columns; Lx = 128 ceil(lr_dd / 128): lr_x is [lr_npad][lr_lx], lr_xt [lr_lx][lr_npad]
    int32_t lr_fcols;         // level columns, sum N_f
    int32_t lr_foff[4];       // the column of level 0 of factor f
    // factor terms that carry a value per observation (idhmc_create_glm_slopes; null and 0 unless some term has values).
    // Appended again: no kernel of a model without values changes (profiles/r18_glm_slopes_kres_*.txt).
    const double *lr_fval;    // [lr_f][lr_npad] w of every observation: the values of a valued term, 1.0 for a plain term, 0.0 in the padding
    const double *lr_fwl;     // [lr_npad / 128][128 lr_f] the same values in the order of lr_fpos: entry t is the value of the observation byte t names
    uint32_t lr_fhas;         // bit f: term f has values
    // correlated pairs of factor terms (idhmc_create_glm_corr; null and 0 without a pair): the last lr_cp coordinates are
    // the zetas.  Appended again, and not lr_lpart: no kernel of a model without pairs changes (profiles/r19_glm_corr_kres_*.txt).
    const int32_t *lr_cpart;  // [L] -1, or for a paired column: partner | pair << 10 | (second of its pair ? 2048 : 0)
    int32_t lr_cp;            // pairs, 0..2
    // structured factor terms (idhmc_create_glm_struct; null and 0 without one): the last lr_sz coordinates, behind the
    // pairs' zetas, are the zetas of the AR(1) terms.  Appended again: no kernel of a model without a structure changes
    // (profiles/r20_glm_struct_kres_*.txt).
    const int32_t *lr_spart;  // [L] -1, or for a column of a structured term: k | slot << 10, k its level
    int32_t lr_s, lr_sz;      // structured terms (slots), 0..2, and those of them that are AR(1)
    int32_t lr_sn[2];         // the levels of slot i
    int32_t lr_skind[2];      // IDHMC_STRUCT_AR1 or IDHMC_STRUCT_RW1
    int32_t lr_scz[2];        // the coordinate of the slot's zeta (AR(1)), -1 for a random walk
    // Gaussian Markov random field priors on factor terms (idhmc_create_glm_gmrf; null and 0 without one): no
    // coordinate is added.  Appended again: the kernels of a model without a GMRF term keep their instructions but for the offsets of the
    // kernel arguments behind DevState -- and, in the kStruct kernels, which read the fields just above, the grouping of the scalar loads
    // next to them (profiles/r22_glm_gmrf_asm_diff.txt).
    const int32_t *lr_gpart;  // [L] -1, or for a column of a GMRF term: k | slot << 10, k its level
    const int32_t *lr_gstart; // [sum N + 1] where each row's entries start: the rows of slot 0, then those of slot 1, cumulative
    const int32_t *lr_gcol;   // the entries' columns, 0 .. N-1 of their slot, ascending within a row
    const double *lr_gval;    // and their values
    double lr_gkappa[2];      // the slot's kappa (0: no sum-to-zero term)
    int32_t lr_g;             // GMRF terms (slots), 0..2
    int32_t lr_go[2];         // the first column of slot i
    int32_t lr_gn[2];         // its levels
    int32_t lr_gnz[2];        // its entries
    // a correlation block of K = 2..4 factor terms (idhmc_create_glm_block; null and 0 without one): the
    // K (K - 1) / 2 zetas stand where the pairs' stand (a model has pairs or a block), in front of the AR(1) zetas.  Appended again.
    const int32_t *lr_bpart;  // [L] -1, or for a column of a block term: k | row << 10, k its level, row its row of L
    int32_t lr_bk;            // K, 0 without a block
    int32_t lr_boff[4];       // the first column of the term in row r
    // factor terms with several weighted levels per observation (idhmc_create_glm_multi; 0 without a wide term).  With
    // lr_mp > 0 the arrays above are laid out by PLANE: lr_fidx and lr_fval [lr_mp][lr_npad], lr_fpos and lr_fwl 128 lr_mp entries per
    // block, and eight more int32 stand behind the last row of lr_fstart: the first column of the term each plane belongs to.  The one
    // field takes the four bytes the struct ended on: its size, and with it every kernel argument's offset, is what it was.
    int32_t lr_mp;            // planes, sum of the terms' widths, 2..8
};
static_assert(sizeof(DevState) == 864, "DevState keeps its size: the kernel arguments behind it keep their offsets");
// A density whose data depend on the chain (Model::kBindsChain: a GLM with several responses) is told the GLOBAL id of the chain a
// kernel is about to evaluate, wherever a kernel takes a chain; for every other density nothing is compiled.
template <class Model, class = void>
struct BindsChain { static constexpr bool value = false; };
template <class Model>
struct BindsChain<Model, decltype(void(Model::kBindsChain))> { static constexpr bool value = Model::kBindsChain; };
template <class Model>
__device__ __forceinline__ void bind_chain(Model &mdl, const DevState &s, uint32_t global_chain)
{
    if constexpr (BindsChain<Model>::value) mdl.bind_chain(s, global_chain);
}
constexpr int kPulseAt = 0;
constexpr int kStreamWaves = 4;         // wavefronts, i.e. chains, per workgroup of the streaming kernels (idhmc_stream.hpp, idhmc_optimum.hpp)
constexpr int kLdsBytes = 160 * 1024;   // LDS of a CU
// transition flag of the test suite only (see the XCD check in k_nuts); idhmc_nuts_transition(s) accept it on a context created
// with IDHMC_TEST_XCC_MISMATCH=1 in the environment, and refuse it, like every other bit outside the IDHMC_T_* set, otherwise
constexpr uint32_t kTestXccFlag = 1u << 30;
constexpr int kRespBlocks = 1024;   // most workgroups of k_resp_eps / k_resp_da_init (four wavefronts each, strided beyond)
constexpr int kXchgBlocks = 64;   // workgroups of k_xchg_sum; DevState::xchg_acc holds 3 * kXchgBlocks partials + 1 ticket
// the most q, p, grad bytes the single-step leapfrog keeps in the 256 MiB Infinity Cache across sweeps: every lf_stride-th chain, with
// lf_stride = ceil(C L 3 8 / kIcSliceBytes), 1 when the whole state fits (tools/ubench/ic_slice.hip: 192 MiB stays resident behind a
// 2.6 GiB nt stream, 219 MiB only in part); the sweep that re-derives the gradient touches q and p only and sizes its slice for
// those: lf_stride2 = ceil(C L 2 8 / kIcSliceBytes) (profiles/r05_ic_slice_two_arrays.log)
constexpr int64_t kIcSliceBytes = (int64_t)192 << 20;

#ifndef __HIPCC_RTC__   // host side only (the header is also compiled by hipRTC for custom densities)
// ---- dispatch over the padded length: NCH = L / 128 = ceil(D / 128), every value 1..16 for the separable densities
// (a vector is padded to the next multiple of 128, like the reference pads to the SIMD width, src/mcmc.jl:117);
// the dense density's matrix kernels need a power of two (D <= 1024)
#define IDHMC_NCH_CASE(N, ...) case N: { constexpr int NCH = N; __VA_ARGS__; } break;
#define IDHMC_DISPATCH_NCH(NCHV, ...)                                                                              \
    switch (NCHV) {                                                                                                \
        IDHMC_NCH_CASE(1, __VA_ARGS__) IDHMC_NCH_CASE(2, __VA_ARGS__) IDHMC_NCH_CASE(3, __VA_ARGS__) IDHMC_NCH_CASE(4, __VA_ARGS__)    \
        IDHMC_NCH_CASE(5, __VA_ARGS__) IDHMC_NCH_CASE(6, __VA_ARGS__) IDHMC_NCH_CASE(7, __VA_ARGS__) IDHMC_NCH_CASE(8, __VA_ARGS__)    \
        IDHMC_NCH_CASE(9, __VA_ARGS__) IDHMC_NCH_CASE(10, __VA_ARGS__) IDHMC_NCH_CASE(11, __VA_ARGS__) IDHMC_NCH_CASE(12, __VA_ARGS__) \
        IDHMC_NCH_CASE(13, __VA_ARGS__) IDHMC_NCH_CASE(14, __VA_ARGS__) IDHMC_NCH_CASE(15, __VA_ARGS__) IDHMC_NCH_CASE(16, __VA_ARGS__) \
    default: return hipErrorInvalidValue;                                                                          \
    }
#define IDHMC_DISPATCH_NCH_POW2(NCHV, ...)                                                                         \
    switch (NCHV) {                                                                                                \
        IDHMC_NCH_CASE(1, __VA_ARGS__) IDHMC_NCH_CASE(2, __VA_ARGS__) IDHMC_NCH_CASE(4, __VA_ARGS__) IDHMC_NCH_CASE(8, __VA_ARGS__)    \
    default: return hipErrorInvalidValue;                                                                          \
    }
// ---- custom densities and GLMs through hipRTC (idhmc_jit.hip) -------------------------------------------
struct JitModule;
// compiles `source` against the kernel templates for this state's shape; on failure returns non-zero and
// fills `log` (compiler output, truncated)
// K, A and H of a GLM; s.lr_m > 1 makes its policy one of several responses (kResponses), s.lr_pkind one with priors (kPriors),
// s.lr_lpart one with local scales (kLocal), s.lr_f > 0 one with factor terms (kFactors), s.lr_fval one whose terms read a value (kSlopes),
// s.lr_cp > 0 one with correlated pairs (kCorr), s.lr_s > 0 one with structured terms (kStruct), s.lr_g > 0 one with GMRF terms (kGmrf),
// s.lr_bk > 0 one with a correlation block (kBlock), s.lr_mp > 0 one with a wide term (kMulti)
int jit_build(const DevState &s, const char *source, JitModule **out, char *log, size_t log_cap, int glm_k = 0, int glm_a = 0, int glm_h = 0);
void jit_destroy(JitModule *m);

// ---- RCCL communicator for the global-eps exchange (idhmc_comm.hip; RCCL bound with dlopen) ----------
struct Comm;
int comm_unique_id(void *out128, char *err, size_t cap);
Comm *comm_create(int nranks, int rank, const void *id128, char *err, size_t cap);   // on the current device
int comm_allreduce_sum(Comm *c, double *dev_buf, int n, hipStream_t st, char *err, size_t cap);
void comm_destroy(Comm *c);
void comm_info(const Comm *c, int *nranks, int *rank, long long *allreduces);

// ---- the backends: who evaluates a density -------------------------------------------------------------
// One row per backend, defined by the translation unit that owns it; the launchers below go through backend(model).
struct Backend {
    hipError_t (*eval)(const DevState &s, int random_q, hipStream_t st);
    // regrad, dense_mfma: as for launch_leapfrog; a backend they do not concern ignores them
    hipError_t (*leapfrog)(const DevState &s, double eps, int own, int n_steps, int regrad, int dense_mfma, hipStream_t st);
    hipError_t (*stepsize_search)(const DevState &s, hipStream_t st);
    hipError_t (*local_optimum)(const DevState &s, double penalty, int iterations, hipStream_t st);
    hipError_t (*nuts)(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
};
// (functions, not variables: a constant at namespace scope would be emitted for the device as well, host pointers and all)
const Backend &separable_backend();   // idhmc_kernels.hip: the Gaussians
const Backend &dense_backend();       // idhmc_dense.hip
const Backend &logistic_backend();    // idhmc_logistic.hip
const Backend &jit_backend();         // idhmc_jit.hip: a custom density or a GLM, compiled at run time
// the zetas of a correlation block of K terms (DevState::lr_bk; 0 without a block)
inline int block_zetas(int K) { return (K * (K - 1)) >> 1; }
inline bool model_is_separable(int model) { return model == IDHMC_MODEL_ISO_GAUSSIAN || model == IDHMC_MODEL_DIAG_GAUSSIAN; }
inline const Backend *backend(int model)
{
    if (model_is_separable(model)) return &separable_backend();
    if (model == IDHMC_MODEL_DENSE_MVN) return &dense_backend();
    if (model == IDHMC_MODEL_LOGISTIC_REGRESSION) return &logistic_backend();
    if (model == IDHMC_MODEL_CUSTOM || model == IDHMC_MODEL_GLM) return &jit_backend();
    return nullptr;
}
// entries of a row that another translation unit defines, so that the parallel build stays as it is: the separable densities'
// search and optimum stage and every k_nuts of the separable and dense rows (idhmc_nuts.hip, idhmc_nuts_sep{1,2,3,4}.hip), the
// dense density's matrix-core leapfrog (idhmc_dense_mfma.hip)
hipError_t launch_stepsize_search_separable(const DevState &s, hipStream_t st);
hipError_t launch_local_optimum_separable(const DevState &s, double penalty, int iterations, hipStream_t st);
hipError_t launch_nuts_separable(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_nuts_sep_from1(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_nuts_sep_from5(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_nuts_sep_from9(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_nuts_sep_from13(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_nuts_dense(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_leapfrog_dense_mfma(const DevState &s, double eps, int own, int n_steps, hipStream_t st);
// The grid of a streaming kernel: kStreamWaves chains per workgroup, capped so that every CU keeps several workgroups
// (k_leapfrog1 is uncapped, the optimum stage bounded by the arena slots: every launched wavefront owns one, >= 2 kLbfgsR vectors)
constexpr int kSeparableBlocks = 256 * 16, kGeneralBlocks = 256 * 8;
inline int stream_grid(int64_t C, int64_t max_blocks)
{
    int64_t b = (C + kStreamWaves - 1) / kStreamWaves;
    if (b > max_blocks) b = max_blocks;
    return (int)(b < 1 ? 1 : b);
}
inline int optimum_grid(const DevState &s) { return stream_grid(s.C, s.nslots / kStreamWaves); }

// ---- GLM shapes (idhmc_logistic.hip) ---------------------------------------------------------------
// NUTS gradients on the matrix cores (GlmCoop: logistic regression, GLM) at this padded length, with `aux` auxiliary coordinates
// and a shared (or pooled) metric or a per-chain one
bool glm_coop(int nch, int aux, bool shared);
size_t glm_nuts_lds_bytes(int nch, bool shared, int aux);   // dynamic LDS of a GLM's NUTS kernel

// ---- launchers (idhmc_kernels.hip / idhmc_nuts.hip) ------------------------------------------------
hipError_t launch_eval(const DevState &s, int random_q, hipStream_t st);   // lq, grad from q; random_q: q ~ U[-2,2)^D first
hipError_t launch_refresh(const DevState &s, uint32_t iter, hipStream_t st);   // p = W randn; pi
hipError_t launch_logdensity(const DevState &s, hipStream_t st);               // pi from (lq, p)
// regrad != 0 (separable densities, single step): the gradient array is neither read nor written and goes stale;
// dense_mfma == 0 (dense density): the per-wave GEMV kernel instead of the matrix-core one
hipError_t launch_leapfrog(const DevState &s, double eps, int use_own_eps, int n_steps, int regrad, int dense_mfma, hipStream_t st);
constexpr int kRowPad = 32;   // rows of slack after q, p, g and a per-chain M^-1 of a dense context (ragged last tile, never stored)
// dense density, matrix-core kernel over the 16-chain tiles [tile_begin, tile_end) with at most max_grid workgroups (0: as many
// as are resident); hipErrorNotSupported outside the kernel's range (idhmc_dense_mfma.hip)
hipError_t launch_leapfrog_dense_mfma_tiles(const DevState &s, double eps, int own, int n_steps, int64_t tile_begin,
                                            int64_t tile_end, int64_t max_grid, hipStream_t st);
hipError_t launch_set_w(const DevState &s, hipStream_t st);                    // W = 1/sqrt(M^-1)
hipError_t launch_fill(double *p, double v, int64_t n, hipStream_t st);
hipError_t launch_xcc_probe(uint32_t *out, int grid, hipStream_t st);   // out[b] = XCD id of workgroup b
hipError_t launch_spin(long long ticks_100MHz, hipStream_t st);   // an idle wavefront for that long (hardware-queue discovery)
hipError_t launch_placement_probe(double *const *v, int nvec, int64_t C, int L, hipStream_t st);   // reads and rewrites v[k][0 .. C L)
hipError_t launch_pack_draw(const DevState &s, double *q_out, idhmc_tree_stats *st_out, hipStream_t st);
hipError_t launch_broadcast_row(double *a, int L, int64_t C, hipStream_t st);
// the NUTS kernel's shape decisions (idhmc_nuts.hip): arena vectors per wavefront, wavefronts per workgroup, dynamic LDS of a custom density
int arena_vectors(int max_depth, bool separable, int L);
int nuts_waves_per_block(int nch, int model, int shared_metric, int glm_aux);
size_t nuts_lds_bytes(int nch, bool shared_metric);
hipError_t launch_nuts(const DevState &s, uint32_t iter, uint32_t flags, hipStream_t st, uint32_t n_iter = 1,
                       double *fz_q = nullptr, idhmc_tree_stats *fz_st = nullptr);
hipError_t launch_stepsize_search(const DevState &s, hipStream_t st);
hipError_t launch_local_optimum(const DevState &s, double penalty, int iterations, hipStream_t st);
hipError_t launch_da_init(const DevState &s, hipStream_t st);
hipError_t launch_da_finalize(const DevState &s, hipStream_t st);
hipError_t launch_xchg_sum(const DevState &s, int kind, double *dev_xchg, hipStream_t st);   // IDHMC_XCHG_* record
hipError_t launch_da_adapt_global(const DevState &s, const double *dev_xchg, hipStream_t st);
hipError_t launch_eps_from_logeps(const DevState &s, const double *dev_xchg, hipStream_t st);
hipError_t launch_metric_update(const DevState &s, double lambda, hipStream_t st);
hipError_t launch_moments_get(const DevState &s, double *mean_out, double *var_out, hipStream_t st);
// pooled metric (IDHMC_METRIC_POOLED): partial sums per segment of global chain ids, added in segment order (idhmc_kernels.hip)
size_t pool_scratch_doubles(int L);
hipError_t launch_pool_partials(const DevState &s, int pass, const double *scratch, double *table, long long seg_lo, long long seg_hi,
                                hipStream_t st);
hipError_t launch_pool_consume(const DevState &s, int pass, double *scratch, const double *table, long long nseg, double lambda,
                               hipStream_t st);
// per-response stepsize and metric (IDHMC_EPS_PER_RESPONSE, IDHMC_METRIC_PER_RESPONSE): the context's chains are nresp whole responses
// of R chains; resp_da is the context's [nresp][6] dual-averaging states (idhmc_kernels.hip)
hipError_t launch_resp_eps(const DevState &s, int kind, double *resp_da, long long R, long long nresp, hipStream_t st);
hipError_t launch_resp_da_init(const DevState &s, double *resp_da, long long R, long long nresp, hipStream_t st);
hipError_t launch_resp_da_finalize(const DevState &s, const double *resp_da, long long R, hipStream_t st);
hipError_t launch_resp_metric(const DevState &s, double lambda, long long R, long long nresp, hipStream_t st);
hipError_t launch_status_max(const DevState &s, int32_t *dev_out, hipStream_t st);
hipError_t launch_ebfmi(const DevState &s, double *out, hipStream_t st);
#endif  // !__HIPCC_RTC__

}  // namespace idhmc
