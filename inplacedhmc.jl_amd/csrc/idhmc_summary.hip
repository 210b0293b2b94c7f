// idhmc_summary.hip -- posterior summaries reduced on the device (include/idhmc.h "posterior summaries"): the
// streaming reduction over a staged block of draws [cnt][C][D], the fold of its segments, the histogram range, and the C ABI around
// them.  The draws are reduced where idhmc_mcmc's drivers (idhmc_drivers.hip) staged them; nothing here touches k_nuts or DevState.
#include "idhmc_host.hpp"
#include "idhmc_math.hpp"

namespace idhmc {

constexpr int kSumBlock = 256;              // lanes of a workgroup of k_summary
// 16-bit counters of one histogram bin for the workgroup's lanes, padded to an odd number of dwords: a lane's increments and the
// flush (64 lanes read 64 consecutive bins of ONE lane's row) both spread over the LDS banks
constexpr int kSumRow = kSumBlock + 2;
constexpr int kSumFields = 6;               // n, mean, m2, min, max, pos: partials [kSumFields][lanes], finished [kSumFields][groups D]
static_assert((IDHMC_SUMMARY_BINS_MAX + 2) * kSumRow * 2 <= kLdsBytes, "the lane-owned histogram rows must fit the LDS of a CU");
static_assert(64 * IDHMC_SUMMARY_SEGMENT < 65536, "a lane's count of one block must fit 16 bits");

struct SumArgs {
    const double *stage;     // [cnt][C][D]
    const double *scales;    // [cnt][C][H] dexp(omega_g) of every row (k_summary_scales); null without coefficient groups
    const int32_t *grp;      // DevState::lr_grp
    double *part;            // [kSumFields][lanes]
    const double *rng;       // [3][groups D]: lo, hi, inv_w
    uint32_t *hist;          // [groups][D][bins + 2]
    int64_t C, G, lanes;     // chains, chains per group, (segment, d) pairs = groups spg D
    int32_t D, cnt, spg;     // dimension, transitions of the block, segments per group
    int32_t bins, Dx, A, H;
    // a GLM with local scales: theta = [beta | a raw | sigma | exp(lambda)], a row of scales is [e (H) | f (J) | st (J)]
    const int32_t *lpart;    // DevState::lr_lpart
    int32_t J, W;            // local scales; doubles per row of scales = H + 2 J
};

// one value into a lane's running state: the expressions of k_nuts at IDHMC_T_ACCUM_MOMENTS, then min / max / sign
struct SumState {
    int64_t n, pos;
    double mean, m2, mn, mx;
};
IDHMC_DEV void sum_update(SumState &w, double x)
{
    w.n += 1;
    const double inv = 1.0 / (double)w.n;
    const double dx = x - w.mean;
    w.mean = dfma(dx, inv, w.mean);
    w.m2 = dfma(dx, x - w.mean, w.m2);
    w.mn = x < w.mn ? x : w.mn;
    w.mx = x > w.mx ? x : w.mx;
    w.pos += x > 0.0 ? 1 : 0;
}
// bin of a value: 0 below lo, bins + 1 from hi on, 1 + min((int)((x - lo) inv_w), bins - 1) between.  No division; a NaN (which
// only a draw that was never written can be) fails both comparisons and converts to 0: no index leaves the table for any input.
IDHMC_DEV int sum_bin(double x, double lo, double hi, double inv_w, int bins)
{
    if (x < lo) return 0;
    if (x >= hi) return bins + 1;
    int j = (int)((x - lo) * inv_w);
    j = j < 0 ? 0 : j;
    return 1 + (j < bins - 1 ? j : bins - 1);
}

// dexp(omega_g) of every (transition, chain) row of the block, once per row: the D values of the row share them
__global__ void k_summary_scales(const double *stage, double *scales, int64_t rows, int32_t D, int32_t H)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * H) return;
    const int64_t r = i / H;
    const int32_t g = (int32_t)(i - r * H);
    scales[i] = dexp(stage[r * D + (D - H) + g]);
}

// The same for a GLM with local scales, one thread per (row, group or local coordinate): e_g = dexp(omega_g) as above; for local
// coordinate k, column col(k) with id = grp[col(k)], f = dexp(lambda_k) and st by the expressions of idhmc_glm_coords.hpp (glm_local_scale):
//   s = id >= 0 ? e_id * f : f;  no slab: st = s;  slab: i = 1 / s, nn = dfma(i, i, inv2), st = 1 / sqrt(nn)
// A row of scales is [e (H) | f (J) | st (J)].
__global__ void k_summary_local_scales(const double *stage, double *scales, int64_t rows, int32_t D, int32_t H, int32_t J, const int32_t *grp,
                                       const int32_t *lpart, double inv2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t T = H + J, W = H + 2 * J;
    if (i >= rows * T) return;
    const int64_t r = i / T;
    const int32_t t = (int32_t)(i - r * T);
    const double *q = stage + r * D;
    if (t < H) {
        scales[r * W + t] = dexp(q[(D - J - H) + t]);
        return;
    }
    const int32_t k = t - H;
    const double f = dexp(q[(D - J) + k]);
    const int32_t id = H > 0 ? grp[lpart[(D - J) + k]] : -1;
    const double s = id >= 0 ? dexp(q[(D - J - H) + id]) * f : f;
    double st = s;
    if (inv2 != 0.0) {
        const double iv = 1.0 / s;
        const double nn = dfma(iv, iv, inv2);
        st = 1.0 / __builtin_sqrt(nn);
    }
    scales[r * W + H + k] = f;
    scales[r * W + H + J + k] = st;
}

// A correlation block as the theta kernels take it: K = 0 without one.  cz0: the coordinate of zeta_10
struct SumBlock {
    const int32_t *bpart;
    int32_t K, cz0;
    int32_t off[4];
};
// (z, c) of the block's zeta at index e of row q (glm_corr_factors)
__device__ __forceinline__ void sum_block_zc(const double *q, const SumBlock &b, int e, double &z, double &c)
{
    const double x = q[b.cz0 + e];
    const double s = dexp(-__builtin_fabs(x));
    const double t = s * s, d = 1.0 + t;
    z = __builtin_copysign((1.0 - t) / d, x);
    c = (2.0 * s) / d;
}
// L_ji, i <= j, of row q by the header comment of idhmc_glm_coords.hpp: coef(j, -1, i)
__device__ __forceinline__ double sum_block_l(const double *q, const SumBlock &b, int j, int i)
{
    double s = 1.0, z, c;
    bool one = true;
    for (int k = 0; k < i; ++k) {
        sum_block_zc(q, b, ((j * (j - 1)) >> 1) + k, z, c);
        s = one ? c : s * c;
        one = false;
    }
    if (i == j) return s;
    sum_block_zc(q, b, ((j * (j - 1)) >> 1) + i, z, c);
    return one ? z : z * s;
}
// What a block makes of coordinate d of row q, x its value so far (u for a column): ut for a column of the rows >= 1 (stage 2 of the
// header comment of idhmc_glm_coords.hpp), R_ji for the zeta at index j (j - 1) / 2 + i; x itself elsewhere.  Used by both theta kernels.
__device__ double sum_block_theta(const double *q, const SumBlock &b, int32_t d, int32_t Dx, double x)
{
    if (b.K == 0) return x;
    const int nz = (b.K * (b.K - 1)) >> 1;
    if (d < Dx) {
        const int32_t e = b.bpart[d];
        if (e < 1024) return x;
        const int j = e >> 10, k = e & 1023;
        double y = sum_block_l(q, b, j, j) * x;
        for (int i = 0; i < j; ++i) y = dfma(sum_block_l(q, b, j, i), q[b.off[i] + k], y);
        return y;
    }
    if (d < b.cz0 || d >= b.cz0 + nz) return x;
    const int e = d - b.cz0;
    const int j = e < 1 ? 1 : e < 3 ? 2 : 3, i = e - ((j * (j - 1)) >> 1);
    if (i == 0) return sum_block_l(q, b, j, 0);
    double y = sum_block_l(q, b, j, i) * sum_block_l(q, b, i, i);
    for (int k = 0; k < i; ++k) y = dfma(sum_block_l(q, b, j, k), sum_block_l(q, b, i, k), y);
    return y;
}

// A GLM with correlated pairs: theta = [beta | a raw | sigma | exp(lambda) | rho], beta taken from ut.  One thread per
// (row, coordinate) writes the whole reported vector of the row, by the expressions of idhmc_glm_coords.hpp (glm_corr_factors, glm_corr_mix,
// glm_scaled, glm_local_scale); the reduction then runs on it as it runs on raw draws (MODE 3).  A row of "scales" is theta, D doubles.
__global__ void k_summary_corr_theta(const double *stage, double *theta, int64_t rows, int32_t D, int32_t Dx, int32_t A, int32_t H, int32_t J,
                                     int32_t P, const int32_t *grp, const int32_t *lpart, const int32_t *cpart, double inv2, SumBlock blk)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * D) return;
    const int64_t r = i / D;
    const int32_t d = (int32_t)(i - r * D);
    const double *q = stage + r * D;
    double x = q[d];
    if (d >= D - P) {
        // (P counts a block's zetas where there is one: their entries report R, the correlations, not tanh zeta)
        if (blk.K > 0) {
            x = sum_block_theta(q, blk, d, Dx, x);
        } else {
            const double s = dexp(-__builtin_fabs(x));
            const double t = s * s;
            x = __builtin_copysign((1.0 - t) / (1.0 + t), x);
        }
    } else if (d >= Dx + A) {
        x = dexp(x);
    } else if (d < Dx) {
        x = sum_block_theta(q, blk, d, Dx, x);
        const int32_t p = blk.K > 0 ? -1 : cpart[d];
        if (p >= 0 && (p & 2048)) {
            const double z = q[D - P + ((p >> 10) & 1)];
            const double s = dexp(-__builtin_fabs(z));
            const double t = s * s, dd = 1.0 + t;
            const double rho = __builtin_copysign((1.0 - t) / dd, z), c = (2.0 * s) / dd;
            x = dfma(rho, q[p & 1023], c * x);
        }
        const int32_t id = H > 0 ? grp[d] : -1;
        const int32_t lp = J > 0 ? lpart[d] : -1;
        if (lp >= 0) {
            const double f = dexp(q[lp]);
            const double s = id >= 0 ? dexp(q[Dx + A + id]) * f : f;
            double st = s;
            if (inv2 != 0.0) {
                const double iv = 1.0 / s;
                const double nn = dfma(iv, iv, inv2);
                st = 1.0 / __builtin_sqrt(nn);
            }
            x = x * st;
        } else if (id >= 0) {
            x = x * dexp(q[Dx + A + id]);
        }
    }
    theta[i] = x;
}

// A GLM with structured terms: theta = [beta | a raw | sigma | exp(lambda) | rho | phi], beta taken from ut.  The scan
// needs a row's neighbours, so a wavefront owns a row: it stages x (u, c u in the levels k >= 1 of a structured term) in its own LDS
// vector and runs the forward stages of glm_struct_scan between two vectors, lane by lane over the coordinates; then each coordinate
// takes the pair's mix (P > 0), the scales and the transforms as k_summary_corr_theta does.  Every wavefront of the workgroup runs the
// same stages (nm is the model's), so the barriers between them are uniform; a wavefront past the last row works on row 0 and writes
// nothing.  The reduction then runs on theta as on raw draws (MODE 3).
constexpr int kStructThetaWaves = 2;
__global__ void __launch_bounds__(64 * kStructThetaWaves)
k_summary_struct_theta(const double *stage, double *theta, int64_t rows, int32_t D, int32_t Dx, int32_t A, int32_t H, int32_t J, int32_t P,
                       int32_t Sz, const int32_t *grp, const int32_t *lpart, const int32_t *cpart, const int32_t *spart, int32_t n0, int32_t n1,
                       int32_t cz0, int32_t cz1, double inv2, SumBlock blk)
{
    __shared__ double vecs[kStructThetaWaves][2][1024];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kStructThetaWaves + w;
    const bool live = r0 < rows;
    const double *q = stage + (live ? r0 : 0) * D;
    double f0 = 1.0, c0 = 1.0, f1 = 1.0, c1 = 1.0;
    if (cz0 >= 0) {
        const double z = q[cz0], s = dexp(-__builtin_fabs(z)), t = s * s, d = 1.0 + t;
        f0 = __builtin_copysign((1.0 - t) / d, z);
        c0 = (2.0 * s) / d;
    }
    if (cz1 >= 0) {
        const double z = q[cz1], s = dexp(-__builtin_fabs(z)), t = s * s, d = 1.0 + t;
        f1 = __builtin_copysign((1.0 - t) / d, z);
        c1 = (2.0 * s) / d;
    }
    double *va = vecs[w][0], *vb = vecs[w][1];
    for (int c = lane; c < Dx; c += 64) {
        const int32_t e = spart[c];
        va[c] = e >= 0 && (e & 1023) >= 1 ? ((e & 1024) ? c1 : c0) * q[c] : q[c];
    }
    __syncthreads();
    const int nm = n0 > n1 ? n0 : n1;
    double p0 = f0, p1 = f1;
    for (int h = 1; h < nm; h <<= 1) {
        for (int c = lane; c < Dx; c += 64) {
            const int32_t e = spart[c];
            const bool act = e >= 0 && (e & 1023) >= h;
            vb[c] = act ? dfma((e & 1024) ? p1 : p0, va[c - h], va[c]) : va[c];
        }
        __syncthreads();
        double *tmp = va; va = vb; vb = tmp;
        p0 = p0 * p0;
        p1 = p1 * p1;
    }
    if (!live) return;
    for (int d = lane; d < D; d += 64) {
        double x = q[d];
        if (d >= D - P - Sz) {
            if (blk.K > 0 && d < D - Sz) {
                x = sum_block_theta(q, blk, d, Dx, x);
            } else {
                const double s = dexp(-__builtin_fabs(x));
                const double t = s * s;
                x = __builtin_copysign((1.0 - t) / (1.0 + t), x);
            }
        } else if (d >= Dx + A) {
            x = dexp(x);
        } else if (d < Dx) {
            // (a block's columns and a structured term's are disjoint: the scan left u in them)
            x = sum_block_theta(q, blk, d, Dx, va[d]);
            const int32_t p = P > 0 && blk.K == 0 ? cpart[d] : -1;
            if (p >= 0 && (p & 2048)) {
                const double z = q[D - Sz - P + ((p >> 10) & 1)];
                const double s = dexp(-__builtin_fabs(z));
                const double t = s * s, dd = 1.0 + t;
                const double rho = __builtin_copysign((1.0 - t) / dd, z), c = (2.0 * s) / dd;
                x = dfma(rho, q[p & 1023], c * x);
            }
            const int32_t id = H > 0 ? grp[d] : -1;
            const int32_t lp = J > 0 ? lpart[d] : -1;
            if (lp >= 0) {
                const double f = dexp(q[lp]);
                const double s = id >= 0 ? dexp(q[Dx + A + id]) * f : f;
                double st = s;
                if (inv2 != 0.0) {
                    const double iv = 1.0 / s;
                    const double nn = dfma(iv, iv, inv2);
                    st = 1.0 / __builtin_sqrt(nn);
                }
                x = x * st;
            } else if (id >= 0) {
                x = x * dexp(q[Dx + A + id]);
            }
        }
        theta[r0 * D + d] = x;
    }
}

// The reduction.  Lane i owns (segment, d) = (i / D, i % D): consecutive lanes take consecutive d, so a wavefront reads contiguous
// runs of a row.  The lane visits its segment's chains transition by transition, ascending chain id inside, with its state in
// registers; HIST: it counts its values' bins in its own LDS row and the workgroup adds the rows to the table at the end.
// MODE: 0 theta = q; 1 coefficient groups; 2 local scales (with or without groups); 3, correlated pairs and structured terms, is MODE 0
// on the theta that k_summary_corr_theta or k_summary_struct_theta wrote
template <bool HIST, int MODE>
IDHMC_DEV void summary_body(const SumArgs &a, uint16_t *lds_cnt)
{
    constexpr bool SCALED = MODE == 1;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kSumBlock + tid;
    if constexpr (HIST) {
        uint32_t *z = reinterpret_cast<uint32_t *>(lds_cnt);
        const int nz = (a.bins + 2) * (kSumRow / 2);
        for (int j = tid; j < nz; j += kSumBlock) z[j] = 0u;
        __syncthreads();
    }
    if (i < a.lanes) {
        const int64_t slot = i / a.D;
        const int32_t d = (int32_t)(i - slot * a.D);
        const int64_t g = slot / a.spg;
        const int64_t c0 = g * a.G + (slot - g * a.spg) * IDHMC_SUMMARY_SEGMENT;
        const int64_t rest = (g + 1) * a.G - c0;
        const int nc = (int)(rest < IDHMC_SUMMARY_SEGMENT ? rest : IDHMC_SUMMARY_SEGMENT);
        SumState w;
        w.n = (int64_t)d2u(a.part[i]);
        w.mean = a.part[a.lanes + i];
        w.m2 = a.part[2 * a.lanes + i];
        w.mn = a.part[3 * a.lanes + i];
        w.mx = a.part[4 * a.lanes + i];
        w.pos = (int64_t)d2u(a.part[5 * a.lanes + i]);
        double lo = 0.0, hi = 0.0, iw = 0.0;
        if constexpr (HIST) {
            const int64_t gd = g * a.D + d, GD = a.lanes / a.spg;
            lo = a.rng[gd]; hi = a.rng[GD + gd]; iw = a.rng[2 * GD + gd];
        }
        // theta of a GLM with coefficient groups: [beta = u e_grp | a raw | sigma = e]; which scale this lane's coordinate takes
        int sidx = -1;
        bool sigma = false;
        if constexpr (SCALED) {
            if (d < a.Dx) sidx = a.grp[d];
            else if (d >= a.Dx + a.A) { sidx = d - a.Dx - a.A; sigma = true; }
        }
        // with local scales: the column of the row of scales this lane's coordinate takes (-1: raw), and whether the value is the scale itself
        if constexpr (MODE == 2) {
            if (d < a.Dx) {
                const int32_t p = a.lpart[d];
                sidx = p >= 0 ? a.H + a.J + (p - (a.D - a.J)) : (a.H > 0 ? a.grp[d] : -1);
            } else if (d >= a.Dx + a.A) {
                sidx = d - a.Dx - a.A;          // e_g, then f_k: the row of scales continues as theta does
                sigma = true;
            }
        }
        auto value = [&](double u, int64_t row) -> double {
            if constexpr (MODE == 2) {
                if (sidx < 0) return u;
                const double e = a.scales[row * a.W + sidx];
                return sigma ? e : u * e;
            } else if constexpr (SCALED) {
                if (sidx < 0) return u;
                const double e = a.scales[row * a.H + sidx];
                return sigma ? e : u * e;
            } else {
                return u;
            }
        };
        auto take = [&](double x) {
            sum_update(w, x);
            if constexpr (HIST) {
                uint16_t *cell = lds_cnt + sum_bin(x, lo, hi, iw, a.bins) * kSumRow + tid;
                *cell = (uint16_t)(*cell + 1);
            }
        };
        for (int t = 0; t < a.cnt; ++t) {
            const int64_t row0 = (int64_t)t * a.C + c0;
            const double *src = a.stage + row0 * a.D + d;
            int c = 0;
            for (; c + 8 <= nc; c += 8) {          // eight loads in flight ahead of the serial updates
                double u[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) u[k] = value(src[(int64_t)(c + k) * a.D], row0 + c + k);
#pragma unroll
                for (int k = 0; k < 8; ++k) take(u[k]);
            }
            for (; c < nc; ++c) take(value(src[(int64_t)c * a.D], row0 + c));
        }
        a.part[i] = u2d((uint64_t)w.n);
        a.part[a.lanes + i] = w.mean;
        a.part[2 * a.lanes + i] = w.m2;
        a.part[3 * a.lanes + i] = w.mn;
        a.part[4 * a.lanes + i] = w.mx;
        a.part[5 * a.lanes + i] = u2d((uint64_t)w.pos);
    }
    if constexpr (HIST) {
        // the flush: a wavefront adds the rows of its own 64 lanes one after the other, 64 consecutive bins per instruction -- contiguous
        // uint32 adds.  A group of one segment owns its table rows (plain adds); several segments share them (integer atomics: exact in
        // any order).  One global atomic per VALUE would put 64 lanes in 64 rows, the shape float atomics run 17x below their full rate in;
        // integer atomics of either shape have not been measured on their own (DESIGN section 17 has the flush's cost as part of the kernel).
        __syncthreads();
        const int lane = tid & 63, r0 = tid - lane;
        const int nb = a.bins + 2;
        for (int r = r0; r < r0 + 64; ++r) {
            const int64_t ir = (int64_t)blockIdx.x * kSumBlock + r;
            if (ir >= a.lanes) break;
            const int64_t slot = ir / a.D;
            uint32_t *dst = a.hist + ((slot / a.spg) * a.D + (ir - slot * a.D)) * nb;
            for (int j = lane; j < nb; j += 64) {
                const uint32_t v = lds_cnt[j * kSumRow + r];
                if (v == 0u) continue;
                if (a.spg > 1) atomicAdd(dst + j, v);
                else dst[j] += v;
            }
        }
    }
}

template <bool HIST, bool SCALED>
__global__ __launch_bounds__(kSumBlock) void k_summary(SumArgs a)
{
    extern __shared__ __align__(16) uint16_t lds_cnt[];   // [bins + 2][kSumRow]
    summary_body<HIST, SCALED ? 1 : 0>(a, lds_cnt);
}
template <bool HIST>
__global__ __launch_bounds__(kSumBlock) void k_summary_local(SumArgs a)
{
    extern __shared__ __align__(16) uint16_t lds_cnt[];
    summary_body<HIST, 2>(a, lds_cnt);
}

__global__ void k_summary_init(double *part, int64_t lanes)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lanes) return;
    part[i] = u2d(0ull);
    part[lanes + i] = 0.0;
    part[2 * lanes + i] = 0.0;
    part[3 * lanes + i] = kInf;
    part[4 * lanes + i] = -kInf;
    part[5 * lanes + i] = u2d(0ull);
}

// the fold: one thread per (group, d), the group's segments in ascending order from segment 0; fin = [n, mean, var, min, max, pos][GD]
__global__ void k_summary_finish(const double *part, double *fin, int64_t GD, int32_t D, int32_t spg)
{
    const int64_t gd = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gd >= GD) return;
    const int64_t lanes = GD * spg;
    const int64_t g = gd / D, d = gd - g * D;
    int64_t i = (g * spg) * D + d;
    int64_t n = (int64_t)d2u(part[i]), pos = (int64_t)d2u(part[5 * lanes + i]);
    double mean = part[lanes + i], m2 = part[2 * lanes + i], mn = part[3 * lanes + i], mx = part[4 * lanes + i];
    for (int k = 1; k < spg; ++k) {
        i += D;
        const int64_t nb = (int64_t)d2u(part[i]);
        if (nb <= 0) continue;
        const int64_t na = n;
        n = na + nb;
        const double mean_b = part[lanes + i], m2_b = part[2 * lanes + i];
        const double delta = mean_b - mean;
        const double f = (double)nb / (double)n;
        mean = dfma(delta, f, mean);
        m2 = (m2 + m2_b) + (delta * delta) * ((double)na * f);
        const double mn_b = part[3 * lanes + i], mx_b = part[4 * lanes + i];
        mn = mn_b < mn ? mn_b : mn;
        mx = mx_b > mx ? mx_b : mx;
        pos += (int64_t)d2u(part[5 * lanes + i]);
    }
    fin[gd] = u2d((uint64_t)n);
    fin[GD + gd] = mean;
    fin[2 * GD + gd] = n > 1 ? m2 / (double)(n - 1) : 0.0;
    fin[3 * GD + gd] = mn;
    fin[4 * GD + gd] = mx;
    fin[5 * GD + gd] = u2d((uint64_t)pos);
}

// the histogram's range: from the finished moments (from_moments: lo, hi = mean -+ span sd) or as uploaded; inv_w in one place
__global__ void k_summary_range(const double *fin, double *rng, int64_t GD, int32_t bins, double span, int from_moments)
{
    const int64_t gd = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gd >= GD) return;
    double lo = rng[gd], hi = rng[GD + gd];
    if (from_moments) {
        const double mean = fin[GD + gd], sd = __builtin_sqrt(fin[2 * GD + gd]);
        lo = dfma(-span, sd, mean);
        hi = dfma(span, sd, mean);
        rng[gd] = lo;
        rng[GD + gd] = hi;
    }
    rng[2 * GD + gd] = hi > lo ? (double)bins / (hi - lo) : 0.0;
}

static unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// MODE as summary_body's
template <bool HIST, int MODE>
static hipError_t launch_summary(const SumArgs &a, hipStream_t st)
{
    void (*const kernel)(SumArgs) = [] {
        if constexpr (MODE == 2) return &k_summary_local<HIST>;
        else return &k_summary<HIST, MODE == 1>;
    }();
    const size_t lds = HIST ? (size_t)(a.bins + 2) * kSumRow * sizeof(uint16_t) : 0;
    if constexpr (HIST) {
        static bool attr_done[64] = {};  // per instantiation and device (the attribute is per device), as launch_nuts_t does
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (!attr_done[dev & 63]) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (IDHMC_SUMMARY_BINS_MAX + 2) * kSumRow * (int)sizeof(uint16_t));
            if (e != hipSuccess) return e;
            attr_done[dev & 63] = true;
        }
    }
    hipLaunchKernelGGL(kernel, dim3(blocks_for(a.lanes, kSumBlock)), dim3(kSumBlock), lds, st, a);
    return hipGetLastError();
}

}  // namespace idhmc

// ---- host side -------------------------------------------------------------------------------------------------------------------
static bool scaled_theta(const idhmc_ctx *c) { return c->s.model == IDHMC_MODEL_GLM && (c->s.lr_h > 0 || c->s.lr_j > 0 || c->s.lr_cp > 0 || c->s.lr_s > 0 || c->s.lr_bk > 0); }
// doubles per row of Summary::scales: e_g, and with local scales f_k and st_k; with correlated pairs or structured terms the whole theta
static int64_t scales_width(const idhmc_ctx *c) { return c->s.lr_cp > 0 || c->s.lr_s > 0 || c->s.lr_bk > 0 ? (int64_t)c->s.D : c->s.lr_h + 2 * (int64_t)c->s.lr_j; }
static int64_t sum_gd(const idhmc_ctx *c) { return c->sum.groups * (int64_t)c->s.D; }

static void summary_release(idhmc_ctx *c)
{
    Summary &m = c->sum;
    const int64_t GD = sum_gd(c);
    dfree(c, m.part, (int64_t)sizeof(double) * kSumFields * GD * m.spg);
    dfree(c, m.fin, (int64_t)sizeof(double) * kSumFields * GD);
    dfree(c, m.rng, (int64_t)sizeof(double) * 3 * GD);
    dfree(c, m.hist, (int64_t)sizeof(uint32_t) * (m.bins > 0 ? GD * (m.bins + 2) : 1));
    dfree(c, m.scales, (int64_t)sizeof(double) * (m.scales_rows > 0 ? m.scales_rows * scales_width(c) : 1));
    m = Summary{};
}

int idhmc_summary_begin(idhmc_ctx *c, int64_t chains_per_group, int32_t bins)
{
    CTXCHK(c);
    const DevState &s = c->s;
    if (chains_per_group < 0) return fail(IDHMC_ERR_BAD_ARG, "summary: chains_per_group = %lld is negative", (long long)chains_per_group);
    const int64_t G = chains_per_group > 0 ? chains_per_group : (c->glm_r > 0 ? c->glm_r : s.C);
    if (s.C % G != 0 || (int64_t)s.first_chain % G != 0)
        return fail(IDHMC_ERR_BAD_ARG, "summary: chains_per_group = %lld does not divide first_chain_id = %u and nchains = %lld: the context must hold whole groups",
                    (long long)G, s.first_chain, (long long)s.C);
    if (bins < 0 || bins > IDHMC_SUMMARY_BINS_MAX) return fail(IDHMC_ERR_BAD_ARG, "summary: bins = %d outside 0 ... %d", bins, IDHMC_SUMMARY_BINS_MAX);
    const int64_t groups = s.C / G, GD = groups * s.D;
    const int64_t hist_bytes = bins > 0 ? GD * (bins + 2) * (int64_t)sizeof(uint32_t) : 0;
    if (hist_bytes > ((int64_t)2 << 30))
        return fail(IDHMC_ERR_BAD_ARG, "summary: the histogram table [%lld][%d][%d] takes %lld bytes, above 2 GiB", (long long)groups, s.D, bins + 2, (long long)hist_bytes);
    if (c->sum.open) summary_release(c);
    Summary &m = c->sum;
    m.G = G; m.groups = groups; m.bins = bins;
    m.spg = (int32_t)((G + IDHMC_SUMMARY_SEGMENT - 1) / IDHMC_SUMMARY_SEGMENT);
    const int64_t lanes = GD * m.spg;
    int rc = dalloc(c, &m.part, kSumFields * lanes, false);
    if (!rc) rc = dalloc(c, &m.fin, kSumFields * GD);
    if (!rc) rc = dalloc(c, &m.rng, 3 * GD);
    if (!rc && bins > 0) rc = dalloc(c, &m.hist, GD * (bins + 2));
    if (rc) { summary_release(c); return rc; }
    hipLaunchKernelGGL(k_summary_init, dim3(blocks_for(lanes, 256)), dim3(256), 0, c->stream, m.part, lanes);
    HIPCHK(hipGetLastError());
    m.open = true;
    m.valid = true;
    return IDHMC_OK;
}
int idhmc_summary_end(idhmc_ctx *c)
{
    CTXCHK(c);
    if (c->sum.open) summary_release(c);
    return IDHMC_OK;
}
int idhmc_summary_dims(idhmc_ctx *c, int64_t *groups, int64_t *chains_per_group, int32_t *dim, int32_t *bins)
{
    CTXCHK(c);
    if (!c->sum.open) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_dims: no summary is open (idhmc_summary_begin first)");
    if (groups) *groups = c->sum.groups;
    if (chains_per_group) *chains_per_group = c->sum.G;
    if (dim) *dim = c->s.D;
    if (bins) *bins = c->sum.bins;
    return IDHMC_OK;
}
// may `cnt` more transitions be reduced?  A group's binned count is a uint32
int idhmc::summary_admit(idhmc_ctx *c, int64_t cnt)
{
    const Summary &m = c->sum;
    if (!m.open || !m.ranged || cnt <= 0) return IDHMC_OK;
    const uint64_t room = 0xffffffffull / (uint64_t)m.G;      // transitions a group's count can hold
    if (m.binned_t > room || (uint64_t)cnt > room - m.binned_t)
        return fail(IDHMC_ERR_BAD_ARG, "summary: %lld more transitions of %lld chains would take a group's binned count (%llu now) past 2^32 - 1",
                    (long long)cnt, (long long)m.G, (unsigned long long)(m.binned_t * (uint64_t)m.G));
    return IDHMC_OK;
}
// the reduction of the staged block [cnt][C][D] at `stage`, enqueued on the context's stream
int idhmc::summary_feed(idhmc_ctx *c, const double *stage, int32_t cnt)
{
    Summary &m = c->sum;
    const DevState &s = c->s;
    const bool strct = s.lr_s > 0, corr = s.lr_cp > 0 || s.lr_bk > 0 || strct, scaled = scaled_theta(c), local = s.lr_j > 0 && !corr;
    // the zetas in the pairs' place: the pairs' or a block's (a model has one or the other)
    const int32_t pz = s.lr_cp + block_zetas(s.lr_bk);
    SumBlock blk{s.lr_bpart, s.lr_bk, s.D - s.lr_sz - pz, {s.lr_boff[0], s.lr_boff[1], s.lr_boff[2], s.lr_boff[3]}};
    if (scaled) {
        const int64_t rows = (int64_t)cnt * s.C;
        if (m.scales_rows < rows) {
            dfree(c, m.scales, (int64_t)sizeof(double) * m.scales_rows * scales_width(c));
            m.scales = nullptr; m.scales_rows = 0;
            if (int rc = dalloc(c, &m.scales, rows * scales_width(c), false)) return rc;
            m.scales_rows = rows;
        }
        if (strct)
            hipLaunchKernelGGL(k_summary_struct_theta, dim3(blocks_for(rows, kStructThetaWaves)), dim3(64 * kStructThetaWaves), 0, c->stream, stage,
                               m.scales, rows, s.D, s.D - s.lr_a - s.lr_h - s.lr_j - pz - s.lr_sz, s.lr_a, s.lr_h, s.lr_j, pz, s.lr_sz,
                               s.lr_grp, s.lr_lpart, s.lr_cpart, s.lr_spart, s.lr_sn[0], s.lr_s > 1 ? s.lr_sn[1] : 0, s.lr_scz[0],
                               s.lr_s > 1 ? s.lr_scz[1] : -1, s.lr_inv2, blk);
        else if (corr)
            hipLaunchKernelGGL(k_summary_corr_theta, dim3(blocks_for(rows * s.D, 256)), dim3(256), 0, c->stream, stage, m.scales, rows, s.D,
                               s.D - s.lr_a - s.lr_h - s.lr_j - pz, s.lr_a, s.lr_h, s.lr_j, pz, s.lr_grp, s.lr_lpart, s.lr_cpart, s.lr_inv2, blk);
        else if (local)
            hipLaunchKernelGGL(k_summary_local_scales, dim3(blocks_for(rows * (s.lr_h + s.lr_j), 256)), dim3(256), 0, c->stream, stage, m.scales, rows,
                               s.D, s.lr_h, s.lr_j, s.lr_grp, s.lr_lpart, s.lr_inv2);
        else
            hipLaunchKernelGGL(k_summary_scales, dim3(blocks_for(rows * s.lr_h, 256)), dim3(256), 0, c->stream, stage, m.scales, rows, s.D, s.lr_h);
        HIPCHK(hipGetLastError());
    }
    SumArgs a{};
    a.stage = stage; a.scales = m.scales; a.grp = s.lr_grp; a.part = m.part; a.rng = m.rng; a.hist = m.hist;
    a.C = s.C; a.G = m.G; a.lanes = sum_gd(c) * m.spg;
    a.D = s.D; a.cnt = cnt; a.spg = m.spg;
    a.bins = m.bins; a.Dx = s.D - s.lr_a - s.lr_h - s.lr_j; a.A = s.lr_a; a.H = s.lr_h;
    a.lpart = s.lr_lpart; a.J = s.lr_j; a.W = (int32_t)scales_width(c);
    if (corr) a.stage = m.scales;       // MODE 3: the theta written above, reduced as raw draws are
    const bool hist = m.ranged && m.bins > 0;
    const bool plain = corr || !scaled;
    hipError_t e = plain ? (hist ? launch_summary<true, 0>(a, c->stream) : launch_summary<false, 0>(a, c->stream)) :
                   hist ? (local ? launch_summary<true, 2>(a, c->stream) : scaled ? launch_summary<true, 1>(a, c->stream) : launch_summary<true, 0>(a, c->stream))
                        : (local ? launch_summary<false, 2>(a, c->stream) : scaled ? launch_summary<false, 1>(a, c->stream) : launch_summary<false, 0>(a, c->stream));
    HIPCHK(e);
    m.fed_t += (uint64_t)cnt;
    if (hist) m.binned_t += (uint64_t)cnt;
    return IDHMC_OK;
}
static int summary_usable(const idhmc_ctx *c, const char *what)
{
    if (!c->sum.open) return fail(IDHMC_ERR_BAD_ARG, "%s: no summary is open (idhmc_summary_begin first)", what);
    if (!c->sum.valid)
        return fail(IDHMC_ERR_BAD_ARG, "%s: the summary is invalid: an idhmc_mcmc that fed it ended with an error (idhmc_summary_begin again)", what);
    return IDHMC_OK;
}
static int summary_finish(idhmc_ctx *c)
{
    const int64_t GD = sum_gd(c);
    hipLaunchKernelGGL(k_summary_finish, dim3(blocks_for(GD, 256)), dim3(256), 0, c->stream, c->sum.part, c->sum.fin, GD, c->s.D, c->sum.spg);
    HIPCHK(hipGetLastError());
    return IDHMC_OK;
}
int idhmc_summary_add_draws(idhmc_ctx *c, const double *draws, int64_t cnt)
{
    CTXCHK(c);
    if (!c->sum.open) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_add_draws: no summary is open (idhmc_summary_begin first)");
    if (cnt < 1) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_add_draws: cnt = %lld must be >= 1", (long long)cnt);
    if (!draws) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_add_draws: null draws");
    if (int rc = summary_admit(c, cnt)) return rc;
    const int64_t CD = c->s.C * (int64_t)c->s.D;
    int64_t K = ((int64_t)256 << 20) / (CD * (int64_t)sizeof(double));       // the drivers' block: what fits 256 MiB, at most 64
    K = K < 1 ? 1 : (K > 64 ? 64 : K);
    K = K > cnt ? cnt : K;
    if (int rc = stage_reserve(c, (int32_t)K, true, false)) return rc;
    int b = 0;
    for (int64_t n0 = 0; n0 < cnt; n0 += K, b ^= 1) {
        const int64_t k = cnt - n0 < K ? cnt - n0 : K;
        HIPCHK(hipMemcpyAsync(c->stage_q[b], draws + n0 * CD, sizeof(double) * (size_t)(k * CD), hipMemcpyHostToDevice, c->stream));
        if (int rc = summary_feed(c, c->stage_q[b], (int32_t)k)) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return IDHMC_OK;
}
int idhmc_summary_set_range(idhmc_ctx *c, const double *lo, const double *hi, double span)
{
    CTXCHK(c);
    if (int rc = summary_usable(c, "idhmc_summary_set_range")) return rc;
    Summary &m = c->sum;
    if (m.bins == 0) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_set_range: the summary was opened with bins = 0: it has no histogram");
    if ((lo == nullptr) != (hi == nullptr)) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_set_range: lo and hi must both be given or both be NULL");
    const int64_t GD = sum_gd(c);
    if (lo) {
        for (int64_t i = 0; i < GD; ++i)
            if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || !(lo[i] <= hi[i]))
                return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_set_range: range [%g, %g] of group %lld, parameter %lld is not finite with lo <= hi",
                            lo[i], hi[i], (long long)(i / c->s.D), (long long)(i % c->s.D));
        HIPCHK(hipMemcpyAsync(m.rng, lo, sizeof(double) * (size_t)GD, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(m.rng + GD, hi, sizeof(double) * (size_t)GD, hipMemcpyHostToDevice, c->stream));
    } else {
        if (!std::isfinite(span) || span < 0.0) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_set_range: span = %g must be finite and >= 0", span);
        const unsigned long long n = (unsigned long long)m.fed_t * (unsigned long long)m.G;
        if (n < 2) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_set_range: a range from the moments needs two values in every group, each holds %llu", n);
        if (int rc = summary_finish(c)) return rc;
    }
    hipLaunchKernelGGL(k_summary_range, dim3(blocks_for(GD, 256)), dim3(256), 0, c->stream, m.fin, m.rng, GD, m.bins, span, lo ? 0 : 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(m.hist, 0, sizeof(uint32_t) * (size_t)(GD * (m.bins + 2)), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));      // (the host arrays are the caller's again)
    m.ranged = true;
    m.binned_t = 0;
    return IDHMC_OK;
}
int idhmc_get_summary(idhmc_ctx *c, int64_t *n, int64_t *binned, double *mean, double *var, double *min, double *max, int64_t *pos,
                      double *lo, double *hi, double *inv_w, uint32_t *counts)
{
    CTXCHK(c);
    if (int rc = summary_usable(c, "idhmc_get_summary")) return rc;
    const Summary &m = c->sum;
    const int64_t GD = sum_gd(c);
    if (int rc = summary_finish(c)) return rc;
    auto fetch = [&](void *dst, const void *src, size_t bytes) -> int {
        if (!dst) return IDHMC_OK;
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
        return IDHMC_OK;
    };
    const size_t row = sizeof(double) * (size_t)GD;
    if (int rc = fetch(mean, m.fin + GD, row)) return rc;
    if (int rc = fetch(var, m.fin + 2 * GD, row)) return rc;
    if (int rc = fetch(min, m.fin + 3 * GD, row)) return rc;
    if (int rc = fetch(max, m.fin + 4 * GD, row)) return rc;
    if (int rc = fetch(pos, m.fin + 5 * GD, row)) return rc;
    if (int rc = fetch(lo, m.rng, row)) return rc;
    if (int rc = fetch(hi, m.rng + GD, row)) return rc;
    if (int rc = fetch(inv_w, m.rng + 2 * GD, row)) return rc;
    if (m.bins > 0) { if (int rc = fetch(counts, m.hist, sizeof(uint32_t) * (size_t)(GD * (m.bins + 2)))) return rc; }
    HIPCHK(hipStreamSynchronize(c->stream));
    // every group has taken the same number of values: the chains of a group times the transitions fed (binned)
    for (int64_t g = 0; g < m.groups; ++g) {
        if (n) n[g] = (int64_t)(m.fed_t * (uint64_t)m.G);
        if (binned) binned[g] = (int64_t)(m.binned_t * (uint64_t)m.G);
    }
    return IDHMC_OK;
}

// host only, no context: quantiles from one (group, parameter)'s histogram
int idhmc_summary_quantiles(const uint32_t *counts, int32_t bins, double lo, double hi, const double *probs, int32_t nprobs, double *out)
{
    if (!counts || !probs || !out) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_quantiles: null argument");
    if (bins < 1 || bins > IDHMC_SUMMARY_BINS_MAX) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_quantiles: bins = %d outside 1 ... %d", bins, IDHMC_SUMMARY_BINS_MAX);
    if (nprobs < 0) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_quantiles: nprobs = %d is negative", nprobs);
    uint64_t nh = 0;
    for (int j = 0; j < bins + 2; ++j) nh += counts[j];
    for (int32_t i = 0; i < nprobs; ++i) {
        const double p = probs[i];
        if (!(p >= 0.0 && p <= 1.0)) return fail(IDHMC_ERR_BAD_ARG, "idhmc_summary_quantiles: probability %g outside [0, 1]", p);
        if (nh == 0) { out[i] = std::nan(""); continue; }
        const double kd = std::ceil(p * (double)nh);
        const uint64_t k = kd < 1.0 ? 1 : (kd > (double)nh ? nh : (uint64_t)kd);
        uint64_t below = 0;                 // cum_{j - 1}
        int j = 0;
        while (below + counts[j] < k) below += counts[j++];
        if (j == 0) out[i] = lo;
        else if (j == bins + 1) out[i] = hi;
        else out[i] = lo + ((double)(j - 1) + ((double)(k - below) - 0.5) / (double)counts[j]) * (hi - lo) / (double)bins;
    }
    return IDHMC_OK;
}
