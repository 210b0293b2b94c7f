// idhmc_kernels.hip -- the separable densities' streaming kernels (idhmc_stream.hpp) and their single-step leapfrog, the momentum
// refresh, dual-averaging / metric / moment bookkeeping, and the launchers that go through the table of backends.  One chain per
// wavefront (see idhmc_device.hpp).
#include "idhmc_stream.hpp"
#include "idhmc_xchg.hpp"

namespace idhmc {

// rand_p! (reference src/kinetic_energy.jl:63) + pi = logdensity(H, z) (:107-112)
template <int NCH>
__global__ __launch_bounds__(256) void k_refresh(DevState s, uint32_t iter, int draw)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t c = wave; c < s.C; c += nw) {
        const Vec<NCH> minv = vload<NCH>(s.minv + c * s.minv_stride, lane);
        Vec<NCH> p;
        if (draw) {
            const RngKey key{s.k0, s.k1, s.first_chain + (uint32_t)c};
            const Vec<NCH> w = vload<NCH>(s.w + c * s.minv_stride, lane);
            p = rand_momentum<NCH>(key, iter, w, lane, s.D);
            vstore<NCH>(s.p + c * s.L, lane, p);
        } else {
            p = vload<NCH>(s.p + c * s.L, lane);
        }
        const double K = kinetic_energy<NCH>(minv, p);
        if (lane == 0) s.pi[c] = phase_logdensity(s.lq[c], K);
    }
}

// Single-step form of k_leapfrog (idhmc_stream.hpp), the HBM-bound headline path (BASELINE.json configs[1]).
// VAR bit 0: issue every load of the chain (q, p, grad: 3 KiB per chunk from HBM; a per-chain M^-1 likewise)
//            before the first store, so one wave keeps 24 KiB of HBM reads in flight (2 waves/SIMD);
//            otherwise chunk-by-chunk at 4 waves/SIMD.
// VAR bit 1: non-temporal loads/stores for the streamed state.
// With bit 0, the chains c % s.lf_stride == 0 (a slice of at most kIcSliceBytes of q, p, grad, spread through the sweep) use
// default-policy loads and stores instead: behind the other chains' nt stream that slice stays in the Infinity Cache from one sweep to
// the next, so its bytes are served on die while the rest streams from HBM (tools/ubench/ic_slice.hip).  The REGRAD
// variants never touch grad: their slice is sized for q and p alone (s.lf_stride2).
typedef double v2d __attribute__((ext_vector_type(2)));
template <bool NT> IDHMC_DEV v2d ld2(const v2d *p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT> IDHMC_DEV void st2(v2d *p, v2d v) { if (NT) __builtin_nontemporal_store(v, p); else *p = v; }

// The parameters every chain of a launch shares -- M^-1 of a shared metric, mu and tau of the density -- live in LDS: rows kLf1M, kLf1Mu,
// kLf1Tau of NCH chunks, one v2d per lane per chunk (one ds_read_b128 per read), staged by the workgroup's four waves in every launch
// (nothing outlives a launch: set_minv, a metric update or new model parameters are seen by the next one).  Read from global memory by
// every chain they were 24 KiB of L2 requests per 32 KiB of state.
constexpr int kLf1M = 0, kLf1Mu = 1, kLf1Tau = 2;
template <class Model> constexpr int lf1_param_rows() { return Model::kHasParams ? 3 : 1; }

// this wave's share of the staging (chunks wv, wv + 4, ... of every staged row), then the workgroup's barrier: every wave of the
// workgroup comes here exactly once, with or without a chain.  The call is inlined into each form of the chain body and into the
// kernel's tail, so the waves of one workgroup may arrive at different s_barrier instructions (one per policy branch, one for a wave
// without a chain): this relies on the hardware barrier counting the workgroup's arrivals wherever their program counters are.
template <int NCH, class Model>
IDHMC_DEV void leapfrog1_stage(const DevState &s, v2d *prm, int lane)
{
    constexpr int kPer = (NCH + kStreamWaves - 1) / kStreamWaves;
    const int wv = (int)(threadIdx.x >> 6);
    const bool shared_m = s.minv_stride == 0;
    const v2d *src[3] = {reinterpret_cast<const v2d *>(s.minv) + lane, reinterpret_cast<const v2d *>(s.mu) + lane,
                         reinterpret_cast<const v2d *>(s.tau) + lane};
    v2d t[3][kPer];
    // every load before the first LDS store; a chunk index past the row is clamped for the load and not stored
#pragma unroll
    for (int k = 0; k < lf1_param_rows<Model>(); ++k) {
        if (k == kLf1M && !shared_m) continue;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int j = wv + i * kStreamWaves;
            t[k][i] = src[k][(j < NCH ? j : NCH - 1) * 64];
        }
    }
#pragma unroll
    for (int k = 0; k < lf1_param_rows<Model>(); ++k) {
        if (k == kLf1M && !shared_m) continue;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int j = wv + i * kStreamWaves;
            if (j < NCH) prm[(k * NCH + j) * 64 + lane] = t[k][i];
        }
    }
    __syncthreads();
}

// one chain of k_leapfrog1; NT: the policy of this chain's q, p, grad loads and stores; MSH: the metric is shared (M^-1 from LDS),
// otherwise this chain's own row streams from global memory.  stage: the wave's first chain, which fills the LDS rows once its own
// q, p (grad) loads are on their way, so the fill's L2 latency runs under their HBM latency.
template <int NCH, class Model, bool PRE, bool NT, bool REGRAD, bool MSH>
IDHMC_DEV void leapfrog1_chain(const DevState &s, v2d *prm, bool stage, int64_t c, int lane, double eps_arg, int own_eps)
{
    const v2d *mL = prm + kLf1M * NCH * 64 + lane, *muL = nullptr, *tauL = nullptr;
    if constexpr (Model::kHasParams) { muL = prm + kLf1Mu * NCH * 64 + lane; tauL = prm + kLf1Tau * NCH * 64 + lane; }
    const int64_t off = c * s.L;
    v2d *__restrict__ q2 = reinterpret_cast<v2d *>(s.q + off) + lane;
    v2d *__restrict__ p2 = reinterpret_cast<v2d *>(s.p + off) + lane;
    v2d *__restrict__ g2 = reinterpret_cast<v2d *>(s.g + off) + lane;
    const v2d *__restrict__ m2 = reinterpret_cast<const v2d *>(s.minv + c * s.minv_stride) + lane;
    const double eps = own_eps ? s.eps[c] : eps_arg;
    const double eh = 0.5 * eps;
    double l0 = 0.0, l1 = 0.0, k0 = 0.0, k1 = 0.0;
    // PRE: the whole chain; otherwise chunk 0 only, the rest chunk by chunk below
    constexpr int NPRE = PRE ? NCH : 1;
    v2d qv[NPRE], pv[NPRE], gv[NPRE], mvv[NPRE];
#pragma unroll
    for (int j = 0; j < NPRE; ++j) {
        qv[j] = ld2<NT>(q2 + j * 64);
        pv[j] = ld2<NT>(p2 + j * 64);
        if (!REGRAD) gv[j] = ld2<NT>(g2 + j * 64);
    }
    if (!MSH) {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) mvv[j] = m2[j * 64];
    }
    if (stage) leapfrog1_stage<NCH, Model>(s, prm, lane);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        v2d q, p, g, mv, mu = {0.0, 0.0}, tau = {1.0, 1.0};
        if (j < NPRE) {
            q = qv[j]; p = pv[j];
            if (!REGRAD) g = gv[j];
            if (!MSH) mv = mvv[j];
        } else {
            q = ld2<NT>(q2 + j * 64); p = ld2<NT>(p2 + j * 64);
            if (!REGRAD) g = ld2<NT>(g2 + j * 64);
            if (!MSH) mv = m2[j * 64];
        }
        if (MSH) mv = mL[j * 64];
        if (Model::kHasParams) { mu = muL[j * 64]; tau = tauL[j * 64]; }
        if (REGRAD) g = v2d{-(tau.x * (q.x - mu.x)), -(tau.y * (q.y - mu.y))};
        const double pmx = dfma(eh, g.x, p.x), pmy = dfma(eh, g.y, p.y);
        const double qx = dfma(eps * mv.x, pmx, q.x), qy = dfma(eps * mv.y, pmy, q.y);
        const double dx = qx - mu.x, dy = qy - mu.y;
        const double tx = tau.x * dx, ty = tau.y * dy;
        l0 = dfma(tx, dx, l0);
        l1 = dfma(ty, dy, l1);
        const double px = dfma(eh, -tx, pmx), py = dfma(eh, -ty, pmy);
        k0 = dfma(px * mv.x, px, k0);
        k1 = dfma(py * mv.y, py, k1);
        st2<NT>(q2 + j * 64, v2d{qx, qy});
        st2<NT>(p2 + j * 64, v2d{px, py});
        if (!REGRAD) st2<NT>(g2 + j * 64, v2d{-tx, -ty});
        if (!PRE) sched_fence();      // chunk by chunk: the LDS reads of all chunks, hoisted to the top, would spill at 4 waves/SIMD
    }
    double sl, sk;
    wave_sum2(l0, l1, k0, k1, sl, sk);
    double lq = -0.5 * sl;
    lq = dfinite(lq) ? lq : -kInf;
    if (lane == 0) {
        s.lq[c] = lq;
        s.pi[c] = phase_logdensity(lq, 0.5 * sk);
    }
}

// waves per SIMD, at least: 2 with the whole chain preloaded; chunk by chunk 4 -- 3 where four workgroups' staged rows (42 KiB and up)
// exceed a CU's LDS.  At most: what the registers admit, as ever, except for the preload variants at NCH = 8, which stay at the two
// they have always run: without the preloaded parameters the registers would admit a third, which measured slower.
template <int NCH, class Model, int VAR>
constexpr int lf1_waves() { return (VAR & 1) ? 2 : (4 * lf1_param_rows<Model>() * NCH * 1024 > kLdsBytes ? 3 : 4); }
template <int NCH, int VAR>
constexpr int lf1_max_waves() { return ((VAR & 1) && NCH == 8) ? 2 : 8; }

template <int NCH, class Model, int VAR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(lf1_waves<NCH, Model, VAR>(), lf1_max_waves<NCH, VAR>())))
void k_leapfrog1(DevState s, double eps_arg, int own_eps)
{
    // VAR bit 2 (REGRAD): the gradient stream is dropped -- grad l(q) is re-derived from q (2 flops per element, the
    // very bits the previous step would have stored) and grad l(q') is not written: 4 D 8 bytes per step instead of 6 D 8
    constexpr bool PRE = (VAR & 1) != 0, NT = (VAR & 2) != 0, REGRAD = (VAR & 4) != 0;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t stride = REGRAD ? s.lf_stride2 : s.lf_stride;
    __shared__ v2d prm[lf1_param_rows<Model>() * NCH * 64];
    bool stage = true;
    if (s.minv_stride == 0) {
        for (int64_t c = wave; c < s.C; c += nw, stage = false) {
            if (PRE && NT && c % stride == 0) leapfrog1_chain<NCH, Model, PRE, false, REGRAD, true>(s, prm, stage, c, lane, eps_arg, own_eps);
            else leapfrog1_chain<NCH, Model, PRE, NT, REGRAD, true>(s, prm, stage, c, lane, eps_arg, own_eps);
        }
    } else {
        for (int64_t c = wave; c < s.C; c += nw, stage = false) {
            if (PRE && NT && c % stride == 0) leapfrog1_chain<NCH, Model, PRE, false, REGRAD, false>(s, prm, stage, c, lane, eps_arg, own_eps);
            else leapfrog1_chain<NCH, Model, PRE, NT, REGRAD, false>(s, prm, stage, c, lane, eps_arg, own_eps);
        }
    }
    if (stage) leapfrog1_stage<NCH, Model>(s, prm, lane);      // a wave without a chain: its share of the fill, and the barrier
}

// W = 1/sqrt(M^-1) (GaussianKineticEnergy, reference src/hamiltonian.jl:50-57)
__global__ void k_set_w(double *w, const double *minv, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = 1.0 / __builtin_sqrt(minv[i]);
}
// copy row 0 of a [C][L] array into rows 1..C-1
__global__ void k_broadcast_row(double *a, int L, int64_t C)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (C - 1) * L) return;
    a[L + i] = a[i % L];
}
// the draw of every chain ([C][L] padded rows -> [C][D] contiguous) and its record into a staging buffer: the host copy of
// transition n then runs while transition n + 1 computes (idhmc_api.hip, fetch pipeline)
__global__ void k_pack_draw(DevState s, double *q_out, idhmc_tree_stats *st_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = s.C * s.D;
    if (q_out && i < n) {
        const int64_t c = i / s.D;
        q_out[i] = s.q[c * s.L + (i - c * s.D)];
    }
    if (st_out && i < s.C) st_out[i] = s.stats[i];
}
__global__ void k_fill(double *p, double v, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// initial_adaptation_state (reference src/stepsize.jl:208-212); eps <- current_eps = exp(log eps) (:235)
__global__ void k_da_init(DevState s)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= s.C) return;
    const double le = dlog(s.eps[c]);
    s.da.mu[c] = dlog(10.0) + le;
    s.da.m[c] = 0;
    s.da.Hbar[c] = 0.0;
    s.da.logeps[c] = le;
    s.da.logeps_bar[c] = 0.0;
    s.eps[c] = dexp(le);
}
// global mode: one state for all chains, started from chain 0's eps (all chains hold the same value)
__global__ void k_da_init_global(DevState s)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double le = dlog(s.eps[0]);
        s.da_global[0] = dlog(10.0) + le;
        s.da_global[1] = 0.0;
        s.da_global[2] = 0.0;
        s.da_global[3] = le;
        s.da_global[4] = 0.0;
        s.da_global[5] = dexp(le);
    }
}
// final_eps = exp(logeps_bar) (reference src/stepsize.jl:241)
__global__ void k_da_finalize(DevState s)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= s.C) return;
    s.eps[c] = (s.eps_mode == IDHMC_EPS_GLOBAL) ? dexp(s.da_global[4]) : dexp(s.da.logeps_bar[c]);
}

// The exchange record of a per-chain statistic (include/idhmc.h, idhmc_xchg.hpp): fixed-point limbs summed as INTEGERS,
// so neither the order of this reduction nor that of the all-reduce behind it can change a bit of the result.
// KIND = IDHMC_XCHG_ACCEPT: the last transition's acceptance rates; IDHMC_XCHG_LOGEPS: log of each chain's eps.
template <int KIND>
__global__ __launch_bounds__(1024) void k_xchg_sum(DevState s, double *out4)
{
    // Up to kXchgBlocks workgroups of 1024 threads (one chain per thread at configs[1]), integer partial sums: inside a workgroup
    // through LDS, across workgroups through a table of per-workgroup partials in s.xchg_acc -- the workgroup that draws the last
    // ticket (ONE atomic per workgroup: contended atomics on one address cost ~15 ns each, 1024 of them were the whole 17 us of
    // the first multi-block form) adds the table in index order and writes the record.  Integer addition is associative, so the
    // record is exact and the same in any order anyway.  xchg_acc = [3 * kXchgBlocks partials][ticket], ticket left at zero.
    __shared__ long long sh[3][16];
    long long v[3] = {0, 0, 0};                      // hi, lo, chains with a pending status
    for (int64_t c = (int64_t)blockIdx.x * 1024 + threadIdx.x; c < s.C; c += (int64_t)gridDim.x * 1024) {
        if (KIND != IDHMC_XCHG_STATUS) {
            const double x = (KIND == IDHMC_XCHG_ACCEPT) ? s.stats[c].acceptance_rate : dlog(s.eps[c]);
            long long h, l;
            xchg_limbs(KIND, x, h, l);
            v[0] += h; v[1] += l;
        }
        v[2] += s.status[c] != 0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < 3; ++k) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
        if (lane == 0) sh[k][wave] = v[k];
    }
    __syncthreads();
    if (wave != 0) return;                           // the rest is one wavefront's work
    for (int k = 0; k < 3; ++k) {
        v[k] = lane < 16 ? sh[k][lane] : 0;
        for (int o = 8; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    }
    unsigned long long *acc = s.xchg_acc;
    int last = 0;
    if (lane == 0) {
        for (int k = 0; k < 3; ++k) __hip_atomic_store(acc + 3 * blockIdx.x + k, (unsigned long long)v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = atomicAdd(acc + 3 * kXchgBlocks, 1ull) == (unsigned long long)gridDim.x - 1ull;
    }
    if (!__shfl(last, 0)) return;
    __threadfence();
    // the last workgroup: lane b reads workgroup b's partials (kXchgBlocks <= 64: one load per lane and value, all in flight together)
    for (int k = 0; k < 3; ++k) {
        v[k] = (unsigned)lane < gridDim.x ? (long long)__hip_atomic_load(acc + 3 * lane + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    }
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    if (lane == 0) {
        out4[0] = (double)v[0];
        out4[1] = (double)v[1];
        out4[2] = (double)s.C;
        out4[3] = (double)v[2];
        __hip_atomic_store(acc + 3 * kXchgBlocks, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
static_assert(kXchgBlocks <= 64, "the finisher reads one workgroup's partials per lane");
// adapt_stepsize (reference src/stepsize.jl:220-229) on the pooled mean acceptance
__global__ void k_da_adapt_global(DevState s, const double *xchg)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double a = xchg_mean(IDHMC_XCHG_ACCEPT, xchg[0], xchg[1], xchg[2]);
        double mu = s.da_global[0], m = s.da_global[1], Hbar = s.da_global[2], lb = s.da_global[4];
        m += 1.0;
        Hbar += (s.da_delta - a - Hbar) / (m + (double)s.da_t0);
        const double le = mu - __builtin_sqrt(m) / s.da_gamma * Hbar;
        lb += dexp(-s.da_kappa * dlog(m)) * (le - lb);
        s.da_global[1] = m;
        s.da_global[2] = Hbar;
        s.da_global[3] = le;
        s.da_global[4] = lb;
        s.da_global[5] = dexp(le);
    }
}
// global mode after the per-chain searches: one eps for everybody, exp(pooled mean of log eps)
__global__ void k_eps_from_logeps(DevState s, const double *xchg)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= s.C) return;
    s.eps[c] = dexp(xchg_mean(IDHMC_XCHG_LOGEPS, xchg[0], xchg[1], xchg[2]));
}
__global__ void k_eps_from_global(DevState s)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= s.C) return;
    const double e = s.da_global[5];
    s.eps[c] = e;
    if (e < 1e-10) {
        s.status[c] = IDHMC_ERR_EPS_UNDERFLOW;
        if (c == 0) atomicMax(s.total_steps + 1, (unsigned long long)IDHMC_ERR_EPS_UNDERFLOW);   // the host's pulse
    }
}

// GaussianKineticEnergy!(kappa, chain, lambda) (reference src/hamiltonian.jl:119-189) from the running
// window sums {x1, sum(x-x1), sum(x-x1)^2} kept by the transition kernel
__global__ void k_metric_update(DevState s, double lambda)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.C * s.L) return;
    const int64_t c = i / s.L;
    const int d = (int)(i - c * s.L);
    double mv = 1.0, wv = 1.0;
    if (d < s.D) {
        const double N = (double)s.mw_n[c];
        const double Ninv = 1.0 / N;                                  // :156
        const double mulreg = N / ((N + lambda) * (N - 1.0));         // :157
        const double addreg = 1e-3 * lambda / (N + lambda);           // :158
        const double s1 = s.mw_s1[i], s2 = s.mw_s2[i];
        const double s2nm1 = dfma(-(s1 * s1), Ninv, s2);              // :94-95
        mv = dfma(s2nm1, mulreg, addreg);                             // :96
        wv = 1.0 / __builtin_sqrt(mv);                                // :97
    }
    s.minv[i] = mv;
    s.w[i] = wv;
}
// ---- pooled metric (IDHMC_METRIC_POOLED): one M^-1 for all chains, estimated from every chain's window --------------
// Many chains sample the same posterior, so their windows are pooled: two passes over the per-chain running sums
// {n, x1, sum(x - x1), sum(x - x1)^2}:
//   pass 0: N = sum n_c,  A_d = sum_c (n_c x1 + s1)                      -> mean_d = A_d / N
//   pass 1: S_d = sum_c [ (s2 - s1^2 / n_c) + n_c (m_c - mean_d)^2 ],  m_c = x1 + s1 / n_c
// then the reference's regularisation with the pooled count (src/hamiltonian.jl:156-158,94-97).
// So that the result does not depend on how the chains are sharded, the column sums are taken over SEGMENTS OF GLOBAL CHAIN
// IDS (IDHMC_POOL_SEGMENT chains each): a segment's partial sum runs over its chains in ascending id, and the partials are
// added in ascending segment order.  Ranks exchange the [segments][L + 1] table of partials with a SUM all-reduce in which
// every entry is non-zero on one rank only (shards aligned to the segment size) -- adding zeros is exact in any order -- and
// every rank then adds the same table in the same order.
__global__ void k_pool_partial(DevState s, int pass, const double *mean, double *table, long long seg_lo, long long seg_hi)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    const long long seg = seg_lo + blockIdx.y;
    if (d > s.L || seg >= seg_hi) return;
    const long long g0 = seg * IDHMC_POOL_SEGMENT, g1 = g0 + IDHMC_POOL_SEGMENT;         // global chain ids of the segment
    long long c0 = g0 - (long long)s.first_chain, c1 = g1 - (long long)s.first_chain;    // local indices, clipped to this context
    c0 = c0 < 0 ? 0 : c0;
    c1 = c1 > s.C ? s.C : c1;
    double acc = 0.0;
    if (d < s.L) {
        const double mu = pass ? mean[d] : 0.0;
        for (long long c = c0; c < c1; ++c) {
            const double n = (double)s.mw_n[c];
            if (!(n > 0.0)) continue;
            const int64_t i = c * s.L + d;
            const double x1 = s.mw_x1[i], s1 = s.mw_s1[i], s2 = s.mw_s2[i];
            if (pass == 0) {
                acc += dfma(n, x1, s1);
            } else {
                const double m = x1 + s1 / n, dm = m - mu;
                acc += dfma(-(s1 * s1), 1.0 / n, s2) + n * (dm * dm);
            }
        }
    } else {                                    // column L: the number of draws (an integer: exact)
        for (long long c = c0; c < c1; ++c) acc += (double)s.mw_n[c];
    }
    table[(seg - seg_lo) * (s.L + 1) + d] = acc;
}
// out[0..L] = column sums of the table in ascending segment order
__global__ void k_pool_finish(DevState s, const double *table, long long nseg, double *out)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d > s.L) return;
    double acc = 0.0;
    for (long long g = 0; g < nseg; ++g) acc += table[g * (s.L + 1) + d];
    out[d] = acc;
}
__global__ void k_pool_mean(DevState s, const double *acc0, double *mean)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < s.L) mean[d] = acc0[d] / acc0[s.L];
}
__global__ void k_pool_apply(DevState s, const double *acc0, const double *acc1, double lambda)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= s.L) return;
    double mv = 1.0, wv = 1.0;
    if (d < s.D) {
        const double N = acc0[s.L];
        const double mulreg = N / ((N + lambda) * (N - 1.0));         // src/hamiltonian.jl:157
        const double addreg = 1e-3 * lambda / (N + lambda);           // :158
        mv = dfma(acc1[d], mulreg, addreg);                           // :96
        wv = 1.0 / __builtin_sqrt(mv);                                // :97
    }
    s.minv[d] = mv;
    s.w[d] = wv;
}
// ---- per-response stepsize and metric (IDHMC_EPS_PER_RESPONSE, IDHMC_METRIC_PER_RESPONSE) -----------------
// A context of a GLM with several responses holds whole responses: response r of the context is its chains [r R, (r + 1) R).  What
// follows is the global stepsize and the pooled metric with one instance per response, and for every response bit for bit what a
// single-response context on the same chains computes with k_xchg_sum / k_da_adapt_global / k_eps_from_global and k_pool_*: the
// same integer record, the same expression sequences.  resp_da is [responses][6]: mu, m, Hbar, logeps, logeps_bar, eps.
// Lanes by response: a response of R <= 32 chains takes the smallest power of two of lanes that holds it, so a wavefront serves
// 64 / resp_lanes(R) responses side by side (at R = 16 four: k_resp_eps over 4096 responses takes 10.4-11.0 us where one response per
// wavefront took 13.7-14.6, profiles/r10_glm_pooling.log); a larger one has the wavefront to itself
__host__ __device__ inline int resp_lanes(long long R)
{
    int g = 64;
    while (g > 1 && (g >> 1) >= R) g >>= 1;
    return g;
}
// eps of every chain of a response (lane l of its `lanes`), k_eps_from_global's underflow rule for that response
__device__ __forceinline__ void resp_set_eps(const DevState &s, long long c0, long long c1, int l, int lanes, double e)
{
    for (long long c = c0 + l; c < c1; c += lanes) {
        s.eps[c] = e;
        if (e < 1e-10) s.status[c] = IDHMC_ERR_EPS_UNDERFLOW;
    }
    if (e < 1e-10 && l == 0) atomicMax(s.total_steps + 1, (unsigned long long)IDHMC_ERR_EPS_UNDERFLOW);   // the host's pulse
}
// One launch per call.  A response is reduced inside one wavefront, its lanes striding over its chains (any R), the grid striding
// over the responses: the limbs are integers, so the order of the reduction cannot change a bit, and nothing needs LDS, an atomic or
// a ticket.  KIND = IDHMC_XCHG_ACCEPT: adapt_stepsize on the response's mean acceptance, then its eps to its chains;
// IDHMC_XCHG_LOGEPS: eps = exp(mean log eps).
template <int KIND>
__global__ __launch_bounds__(256) void k_resp_eps(DevState s, double *resp_da, long long R, long long nresp)
{
    const int lane = threadIdx.x & 63;
    const int lanes = resp_lanes(R), per = 64 / lanes, sub = lane / lanes, l = lane - sub * lanes;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long nunits = (nresp + per - 1) / per;            // wavefronts' worth of responses
    for (long long u = wave; u < nunits; u += nw) {
        const long long r = u * per + sub;
        const bool live = r < nresp;                             // (the last wavefront may have lanes without a response: they add zeros)
        const long long c0 = r * R, c1 = live ? c0 + R : c0;
        long long hi = 0, lo = 0;
        for (long long c = c0 + l; c < c1; c += lanes) {
            const double x = (KIND == IDHMC_XCHG_ACCEPT) ? s.stats[c].acceptance_rate : dlog(s.eps[c]);
            long long h, w;
            xchg_limbs(KIND, x, h, w);
            hi += h; lo += w;
        }
        for (int o = lanes >> 1; o > 0; o >>= 1) {               // (xor with o < lanes stays inside the response's lanes)
            hi += __shfl_xor(hi, o);
            lo += __shfl_xor(lo, o);
        }
        if (!live) continue;
        const double mean = xchg_mean(KIND, (double)hi, (double)lo, (double)R);
        double e;
        if (KIND == IDHMC_XCHG_ACCEPT) {             // k_da_adapt_global's sequence (every lane computes, lane 0 of the response keeps the state)
            double *da = resp_da + 6 * r;
            double mu = da[0], m = da[1], Hbar = da[2], lb = da[4];
            m += 1.0;
            Hbar += (s.da_delta - mean - Hbar) / (m + (double)s.da_t0);
            const double le = mu - __builtin_sqrt(m) / s.da_gamma * Hbar;
            lb += dexp(-s.da_kappa * dlog(m)) * (le - lb);
            e = dexp(le);
            if (l == 0) {
                da[1] = m;
                da[2] = Hbar;
                da[3] = le;
                da[4] = lb;
                da[5] = e;
            }
        } else {
            e = dexp(mean);
        }
        resp_set_eps(s, c0, c1, l, lanes, e);
    }
}
// k_da_init_global per response: the state starts from the eps of the response's first chain (all of them hold the same value)
__global__ __launch_bounds__(256) void k_resp_da_init(DevState s, double *resp_da, long long R, long long nresp)
{
    const int lane = threadIdx.x & 63;
    const int lanes = resp_lanes(R), per = 64 / lanes, sub = lane / lanes, l = lane - sub * lanes;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long nunits = (nresp + per - 1) / per;
    for (long long u = wave; u < nunits; u += nw) {
        const long long r = u * per + sub;
        if (r >= nresp) continue;
        const double le = dlog(s.eps[r * R]);
        const double e = dexp(le);
        if (l == 0) {
            double *da = resp_da + 6 * r;
            da[0] = dlog(10.0) + le;
            da[1] = 0.0;
            da[2] = 0.0;
            da[3] = le;
            da[4] = 0.0;
            da[5] = e;
        }
        resp_set_eps(s, r * R, r * R + R, l, lanes, e);
    }
}
// final_eps = exp(logeps_bar) of the chain's response (k_da_finalize's global branch)
__global__ void k_resp_da_finalize(DevState s, const double *resp_da, long long R)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= s.C) return;
    s.eps[c] = dexp(resp_da[6 * (c / R) + 4]);
}
// The pooled metric of every response: one thread per (response, d), d fastest, so the loads of the windows and the stores of the
// rows are coalesced.  The sums are k_pool_partial's and k_pool_finish's restricted to the response: a partial per
// IDHMC_POOL_SEGMENT-aligned segment of GLOBAL chain ids in ascending id, chains with an empty window skipped, the partials added to
// 0.0 in ascending segment order (a response that straddles a multiple of the segment size has two); then k_pool_mean, the second
// pass and k_pool_apply.  M^-1 and W go to the rows of all R chains; pads stay 1.
__global__ __launch_bounds__(256) void k_resp_metric(DevState s, double lambda, long long R, long long nresp)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nresp * s.L) return;
    const long long r = i / s.L;
    const int d = (int)(i - r * s.L);
    const long long c0 = r * R, c1 = c0 + R;
    double mv = 1.0, wv = 1.0;
    if (d < s.D) {
        const long long first = (long long)s.first_chain;
        const long long g0 = first + c0, g1 = first + c1;
        const long long seg_lo = g0 / IDHMC_POOL_SEGMENT, seg_hi = (g1 + IDHMC_POOL_SEGMENT - 1) / IDHMC_POOL_SEGMENT;
        double N = 0.0, A = 0.0;                      // pass 0: the count column and sum_c (n_c x1 + s1)
        for (long long seg = seg_lo; seg < seg_hi; ++seg) {
            long long a = seg * IDHMC_POOL_SEGMENT, b = a + IDHMC_POOL_SEGMENT;
            a = (a < g0 ? g0 : a) - first;
            b = (b > g1 ? g1 : b) - first;
            double pn = 0.0, pa = 0.0;
            for (long long c = a; c < b; ++c) {
                const double n = (double)s.mw_n[c];
                pn += n;
                if (!(n > 0.0)) continue;
                const int64_t k = c * s.L + d;
                pa += dfma(n, s.mw_x1[k], s.mw_s1[k]);
            }
            N += pn;
            A += pa;
        }
        const double mu = A / N;                      // k_pool_mean
        double S = 0.0;                               // pass 1
        for (long long seg = seg_lo; seg < seg_hi; ++seg) {
            long long a = seg * IDHMC_POOL_SEGMENT, b = a + IDHMC_POOL_SEGMENT;
            a = (a < g0 ? g0 : a) - first;
            b = (b > g1 ? g1 : b) - first;
            double ps = 0.0;
            for (long long c = a; c < b; ++c) {
                const double n = (double)s.mw_n[c];
                if (!(n > 0.0)) continue;
                const int64_t k = c * s.L + d;
                const double x1 = s.mw_x1[k], s1 = s.mw_s1[k], s2 = s.mw_s2[k];
                const double m = x1 + s1 / n, dm = m - mu;
                ps += dfma(-(s1 * s1), 1.0 / n, s2) + n * (dm * dm);
            }
            S += ps;
        }
        const double mulreg = N / ((N + lambda) * (N - 1.0));         // src/hamiltonian.jl:157
        const double addreg = 1e-3 * lambda / (N + lambda);           // :158
        mv = dfma(S, mulreg, addreg);                                 // :96
        wv = 1.0 / __builtin_sqrt(mv);                                // :97
    }
    for (long long c = c0; c < c1; ++c) {
        s.minv[c * s.L + d] = mv;
        s.w[c * s.L + d] = wv;
    }
}
__global__ void k_moments_get(DevState s, double *mean, double *var)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.C * s.L) return;
    const int64_t c = i / s.L;
    const double n = (double)s.mom_n[c];
    mean[i] = s.mom_mean[i];
    var[i] = n > 1.0 ? s.mom_m2[i] / (n - 1.0) : 0.0;
}
// EBFMI per chain from the running sums (reference src/diagnostics.jl:28-32): mean(abs2, diff(pi)) / var(pi)
__global__ void k_ebfmi(DevState s, double *out)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= s.C) return;
    const double n = (double)s.diag.n[c];
    const double s1 = s.diag.s1[c];
    const double var = dfma(-(s1 * s1), 1.0 / n, s.diag.s2[c]) / (n - 1.0);
    out[c] = (s.diag.d2[c] / (n - 1.0)) / var;
}
__global__ void k_status_max(DevState s, int32_t *out)
{
    __shared__ int sh[256];
    int m = 0;
    for (int64_t c = threadIdx.x; c < s.C; c += 256) m = max(m, s.status[c]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// ---- launchers ---------------------------------------------------------------------------------------

static hipError_t launch_eval_separable(const DevState &s, int random_q, hipStream_t st)
{
    return IDHMC_SEPARABLE(launch_eval_t, s, random_q, st);
}
static hipError_t launch_leapfrog_separable(const DevState &s, double eps, int own, int n_steps, int regrad, int, hipStream_t st)
{
    if (n_steps == 1) {
        const int grid = stream_grid(s.C, 1 << 30);       // one block per four chains, uncapped
        // measured on MI355X (65 536 chains x 1024): diag 6.03 TB/s with 3, iso 5.89 TB/s with 2
        int var = (s.model == IDHMC_MODEL_ISO_GAUSSIAN) ? 2 : 3;
        if (regrad) var = 7;
        if (s.nch > 8) var = regrad ? 6 : 2;      // L = 2048: preloading the whole chain would spill, chunk by chunk instead
        // only the forms the choice above can reach are built: the preload variants up to NCH 8, variant 6 past it
#define IDHMC_LF1(V)                                                                                          \
    IDHMC_DISPATCH_NCH(s.nch, {                                                                               \
        if constexpr (((V) & 1) ? NCH <= 8 : ((V) == 2 || NCH > 8)) {                                         \
            if (s.model == IDHMC_MODEL_ISO_GAUSSIAN)                                                          \
                hipLaunchKernelGGL((k_leapfrog1<NCH, IsoGaussian<NCH>, V>), dim3(grid), dim3(256), 0, st, s, eps, own); \
            else                                                                                              \
                hipLaunchKernelGGL((k_leapfrog1<NCH, DiagGaussian<NCH>, V>), dim3(grid), dim3(256), 0, st, s, eps, own); \
        } else {                                                                                              \
            return hipErrorInvalidValue;                                                                      \
        }                                                                                                     \
    })
        switch (var) {      // (variants 0 and 1, temporal loads, lost the round-1 sweep and are no longer built)
        case 2: IDHMC_LF1(2); break;
        case 6: IDHMC_LF1(6); break;
        case 7: IDHMC_LF1(7); break;
        default: IDHMC_LF1(3); break;
        }
        return hipGetLastError();
    }
    return IDHMC_SEPARABLE(launch_leapfrog_t, s, eps, own, n_steps, st);
}
const Backend &separable_backend()
{
    static const Backend row = {launch_eval_separable, launch_leapfrog_separable, launch_stepsize_search_separable,
                                launch_local_optimum_separable, launch_nuts_separable};
    return row;
}

// each: the common prologue, then the model's backend
hipError_t launch_eval(const DevState &s, int random_q, hipStream_t st)
{
    const Backend *b = backend(s.model);
    return b ? b->eval(s, random_q, st) : hipErrorNotSupported;
}
hipError_t launch_leapfrog(const DevState &s, double eps, int own, int n_steps, int regrad, int dense_mfma, hipStream_t st)
{
    const Backend *b = backend(s.model);
    return b ? b->leapfrog(s, eps, own, n_steps, regrad, dense_mfma, st) : hipErrorNotSupported;
}
hipError_t launch_stepsize_search(const DevState &s, hipStream_t st)
{
    const Backend *b = backend(s.model);
    return b ? b->stepsize_search(s, st) : hipErrorNotSupported;
}
// FindLocalOptimum (src/warmup.jl:137-187), idhmc_optimum.hpp
hipError_t launch_local_optimum(const DevState &s, double penalty, int iterations, hipStream_t st)
{
    const Backend *b = backend(s.model);
    return b ? b->local_optimum(s, penalty, iterations, st) : hipErrorNotSupported;
}
hipError_t launch_refresh(const DevState &s, uint32_t iter, hipStream_t st)
{
    const int grid = stream_grid(s.C, kSeparableBlocks);
    IDHMC_DISPATCH_NCH(s.nch, hipLaunchKernelGGL((k_refresh<NCH>), dim3(grid), dim3(256), 0, st, s, iter, 1));
    return hipGetLastError();
}
hipError_t launch_logdensity(const DevState &s, hipStream_t st)
{
    const int grid = stream_grid(s.C, kSeparableBlocks);
    IDHMC_DISPATCH_NCH(s.nch, hipLaunchKernelGGL((k_refresh<NCH>), dim3(grid), dim3(256), 0, st, s, 0u, 0));
    return hipGetLastError();
}
hipError_t launch_set_w(const DevState &s, hipStream_t st)
{
    const int64_t n = s.minv_stride ? s.C * s.L : (int64_t)s.L;
    hipLaunchKernelGGL(k_set_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s.w, s.minv, n);
    return hipGetLastError();
}
hipError_t launch_broadcast_row(double *a, int L, int64_t C, hipStream_t st)
{
    const int64_t n = (C - 1) * L;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_broadcast_row, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, L, C);
    return hipGetLastError();
}
hipError_t launch_pack_draw(const DevState &s, double *q_out, idhmc_tree_stats *st_out, hipStream_t st)
{
    const int64_t n = q_out ? s.C * s.D : s.C;
    hipLaunchKernelGGL(k_pack_draw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s, q_out, st_out);
    return hipGetLastError();
}
// Placement probe (idhmc_create): the access pattern of the single-step leapfrog on nvec state arrays -- one chain of L doubles per
// wavefront, 16 bytes per lane and chunk, every array read and written in place, element i of all of them at the same time.
__global__ __launch_bounds__(256) void k_placement_probe(double *a0, double *a1, double *a2, double *a3, int nvec, int64_t C, int L)
{
    const int lane = threadIdx.x & 63;
    const int64_t chain = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (chain >= C) return;
    double *v[4] = {a0, a1, a2, a3};
    for (int j = 0; j < L / 128; ++j) {
        double2 x[4];
        for (int k = 0; k < nvec; ++k) x[k] = reinterpret_cast<const double2 *>(v[k] + chain * L)[j * 64 + lane];
        for (int k = 0; k < nvec; ++k) reinterpret_cast<double2 *>(v[k] + chain * L)[j * 64 + lane] = x[k];
    }
}
hipError_t launch_placement_probe(double *const *v, int nvec, int64_t C, int L, hipStream_t st)
{
    hipLaunchKernelGGL(k_placement_probe, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, st, v[0], v[1], nvec > 2 ? v[2] : nullptr,
                       nvec > 3 ? v[3] : nullptr, nvec, C, L);
    return hipGetLastError();
}
// one wavefront that does nothing for `ticks` of the 100 MHz wall clock: two of these on two streams take once or twice that,
// which tells whether the streams share a hardware queue (idhmc_api.hip, pick_lane_streams)
__global__ void k_spin(long long ticks, unsigned long long *sink)
{
    const long long t0 = wall_clock64();
    long long t = t0;
    while (t - t0 < ticks) t = wall_clock64();
    if (ticks < 0) *sink = (unsigned long long)t;
}
// which XCD each workgroup of a grid of that size runs on (HW_REG_XCC_ID); several transitions per launch (idhmc_nuts_kernel.hpp) hand a
// chain's state from one workgroup to another through the L2 that workgroups b and b + 8 share -- idhmc_create verifies that they do
__global__ void k_xcc_probe(uint32_t *out)
{
    if (threadIdx.x == 0) out[blockIdx.x] = (uint32_t)__builtin_amdgcn_s_getreg(6164) & 15u;      // hwreg(HW_REG_XCC_ID, 0, 4)
}
hipError_t launch_xcc_probe(uint32_t *out, int grid, hipStream_t st)
{
    hipLaunchKernelGGL(k_xcc_probe, dim3(grid), dim3(64), 0, st, out);
    return hipGetLastError();
}
hipError_t launch_spin(long long ticks, hipStream_t st)
{
    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st, ticks, (unsigned long long *)nullptr);
    return hipGetLastError();
}
hipError_t launch_fill(double *p, double v, int64_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, v, n);
    return hipGetLastError();
}
hipError_t launch_da_init(const DevState &s, hipStream_t st)
{
    if (s.eps_mode == IDHMC_EPS_GLOBAL) {
        hipLaunchKernelGGL(k_da_init_global, dim3(1), dim3(64), 0, st, s);
        hipLaunchKernelGGL(k_eps_from_global, dim3((unsigned)((s.C + 255) / 256)), dim3(256), 0, st, s);
    } else {
        hipLaunchKernelGGL(k_da_init, dim3((unsigned)((s.C + 255) / 256)), dim3(256), 0, st, s);
    }
    return hipGetLastError();
}
hipError_t launch_da_finalize(const DevState &s, hipStream_t st)
{
    hipLaunchKernelGGL(k_da_finalize, dim3((unsigned)((s.C + 255) / 256)), dim3(256), 0, st, s);
    return hipGetLastError();
}
hipError_t launch_xchg_sum(const DevState &s, int kind, double *dev_xchg, hipStream_t st)
{
    const int64_t nb = (s.C + 1023) / 1024;
    const dim3 grid((unsigned)(nb < kXchgBlocks ? nb : kXchgBlocks));
    if (kind == IDHMC_XCHG_ACCEPT) hipLaunchKernelGGL(k_xchg_sum<IDHMC_XCHG_ACCEPT>, grid, dim3(1024), 0, st, s, dev_xchg);
    else if (kind == IDHMC_XCHG_LOGEPS) hipLaunchKernelGGL(k_xchg_sum<IDHMC_XCHG_LOGEPS>, grid, dim3(1024), 0, st, s, dev_xchg);
    else hipLaunchKernelGGL(k_xchg_sum<IDHMC_XCHG_STATUS>, grid, dim3(1024), 0, st, s, dev_xchg);
    return hipGetLastError();
}
hipError_t launch_da_adapt_global(const DevState &s, const double *dev_xchg, hipStream_t st)
{
    hipLaunchKernelGGL(k_da_adapt_global, dim3(1), dim3(64), 0, st, s, dev_xchg);
    hipLaunchKernelGGL(k_eps_from_global, dim3((unsigned)((s.C + 255) / 256)), dim3(256), 0, st, s);
    return hipGetLastError();
}
hipError_t launch_eps_from_logeps(const DevState &s, const double *dev_xchg, hipStream_t st)
{
    hipLaunchKernelGGL(k_eps_from_logeps, dim3((unsigned)((s.C + 255) / 256)), dim3(256), 0, st, s, dev_xchg);
    return hipGetLastError();
}
hipError_t launch_metric_update(const DevState &s, double lambda, hipStream_t st)
{
    const int64_t n = s.C * s.L;
    hipLaunchKernelGGL(k_metric_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s, lambda);
    return hipGetLastError();
}
// small scratch of the pooled metric: [L + 1 acc0][L + 1 acc1][L mean]
size_t pool_scratch_doubles(int L) { return 2 * (size_t)(L + 1) + L; }
hipError_t launch_pool_partials(const DevState &s, int pass, const double *scratch, double *table, long long seg_lo, long long seg_hi,
                                hipStream_t st)
{
    const double *mean = scratch + 2 * (size_t)(s.L + 1);
    const long long nseg = seg_hi - seg_lo;
    if (nseg < 1 || nseg > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_partial, dim3((unsigned)((s.L + 256) / 256), (unsigned)nseg), dim3(256), 0, st, s, pass, mean, table, seg_lo, seg_hi);
    return hipGetLastError();
}
// pass 0: acc0 and the mean; pass 1: acc1 and the metric
hipError_t launch_pool_consume(const DevState &s, int pass, double *scratch, const double *table, long long nseg, double lambda,
                               hipStream_t st)
{
    double *acc0 = scratch, *acc1 = scratch + (s.L + 1), *mean = scratch + 2 * (size_t)(s.L + 1);
    const unsigned g1 = (unsigned)((s.L + 256) / 256), g0 = (unsigned)((s.L + 255) / 256);
    hipLaunchKernelGGL(k_pool_finish, dim3(g1), dim3(256), 0, st, s, table, nseg, pass ? acc1 : acc0);
    if (pass == 0) hipLaunchKernelGGL(k_pool_mean, dim3(g0), dim3(256), 0, st, s, acc0, mean);
    else hipLaunchKernelGGL(k_pool_apply, dim3(g0), dim3(256), 0, st, s, acc0, acc1, lambda);
    return hipGetLastError();
}
// per-response stepsize and metric: R chains per response, nresp = C / R responses in this context
static dim3 resp_grid(long long R, long long nresp)
{
    const long long per = 64 / resp_lanes(R);         // responses per wavefront, four wavefronts per workgroup
    const long long b = ((nresp + per - 1) / per + 3) / 4;
    return dim3((unsigned)(b > kRespBlocks ? kRespBlocks : b));
}
hipError_t launch_resp_eps(const DevState &s, int kind, double *resp_da, long long R, long long nresp, hipStream_t st)
{
    if (kind == IDHMC_XCHG_ACCEPT) hipLaunchKernelGGL(k_resp_eps<IDHMC_XCHG_ACCEPT>, resp_grid(R, nresp), dim3(256), 0, st, s, resp_da, R, nresp);
    else hipLaunchKernelGGL(k_resp_eps<IDHMC_XCHG_LOGEPS>, resp_grid(R, nresp), dim3(256), 0, st, s, resp_da, R, nresp);
    return hipGetLastError();
}
hipError_t launch_resp_da_init(const DevState &s, double *resp_da, long long R, long long nresp, hipStream_t st)
{
    hipLaunchKernelGGL(k_resp_da_init, resp_grid(R, nresp), dim3(256), 0, st, s, resp_da, R, nresp);
    return hipGetLastError();
}
hipError_t launch_resp_da_finalize(const DevState &s, const double *resp_da, long long R, hipStream_t st)
{
    hipLaunchKernelGGL(k_resp_da_finalize, dim3((unsigned)((s.C + 255) / 256)), dim3(256), 0, st, s, resp_da, R);
    return hipGetLastError();
}
hipError_t launch_resp_metric(const DevState &s, double lambda, long long R, long long nresp, hipStream_t st)
{
    const long long n = nresp * s.L;
    hipLaunchKernelGGL(k_resp_metric, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s, lambda, R, nresp);
    return hipGetLastError();
}
hipError_t launch_moments_get(const DevState &s, double *mean_out, double *var_out, hipStream_t st)
{
    const int64_t n = s.C * s.L;
    hipLaunchKernelGGL(k_moments_get, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s, mean_out, var_out);
    return hipGetLastError();
}
hipError_t launch_ebfmi(const DevState &s, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_ebfmi, dim3((unsigned)((s.C + 255) / 256)), dim3(256), 0, st, s, out);
    return hipGetLastError();
}
hipError_t launch_status_max(const DevState &s, int32_t *dev_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_status_max, dim3(1), dim3(256), 0, st, s, dev_out);
    return hipGetLastError();
}

}  // namespace idhmc
