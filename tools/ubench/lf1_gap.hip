// lf1_gap.hip -- where does k_leapfrog1<8, DiagGaussian<8>, 7> lose its time against a copy of the same bytes?  (tools/ubench, GPU box)
// The copy is cell ST of `ic_slice two`: 65 536 chains x 1024 doubles in two arrays (placement classes A B), one chain per wavefront,
// all 16 loads before the first store, chains c % 6 == 0 with the default policy (the Infinity-Cache slice), the others non-temporal,
// at least 2 waves per SIMD, one workgroup per four chains.  On top of it, one ingredient of the kernel at a time, cumulatively:
//   a   M^-1, mu, tau (3 x 8 KiB, the same for every chain) loaded from global memory by every chain and folded into what is stored
//   b   the kernel's arithmetic (the gradient-recompute step, ~14 fp64 operations per element)
//   c   the wave reduction and lane 0's two 8-byte stores (lq, pi)
//   d   per-lane 64-bit global addressing instead of buffer instructions with a scalar base
//   a'  as a, the rows served from LDS: staged once per workgroup by its four waves after their own loads are issued, one barrier
// a'bcd is the kernel with its parameters in LDS; the last cells run it with the grid capped at 2 and at 3 workgroups per CU (each
// wavefront then loops over its chains and the staging happens once per workgroup per launch).  Each line: microseconds per sweep (3
// warm-up + 20 timed sweeps back to back), the ratio to the copy, and the registers and LDS the compiler gave the cell.  Passes 1 and 2
// sweep zero-filled arrays as ic_slice.hip does, passes 3 and 4 the same arrays filled with non-trivial values.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/ubench/lf1_gap tools/ubench/lf1_gap.hip
#include "../../inplacedhmc.jl_amd/csrc/idhmc_device.hpp"
#include <cstdio>
#include <vector>

using namespace idhmc;

constexpr int NCH = 8, L = 128 * NCH, kWaves = 4;
constexpr int kParG = 1, kParL = 2, kArith = 4, kRed = 8, kGaddr = 16;

template <bool G, bool NT>
IDHMC_DEV Vec<NCH> load_row(double *row, int lane)
{
    if (!G) return bload<NCH, NT ? 2 : 0>(row, lane);
    Vec<NCH> v;
    const v2d *b = reinterpret_cast<const v2d *>(row) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) v.c[j] = __builtin_bit_cast(double2, NT ? __builtin_nontemporal_load(b + j * 64) : b[j * 64]);
    return v;
}
template <bool G, bool NT>
IDHMC_DEV void store_row(double *row, int lane, const Vec<NCH> &v)
{
    if (!G) { bstore<NCH, NT ? 2 : 0>(row, lane, v); return; }
    v2d *b = reinterpret_cast<v2d *>(row) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const v2d x = __builtin_bit_cast(v2d, v.c[j]);
        if (NT) __builtin_nontemporal_store(x, b + j * 64); else b[j * 64] = x;
    }
}
// the three rows into LDS: wave wv takes chunks wv, wv + 4 of each, every load before the first LDS store; then the barrier
IDHMC_DEV void stage_rows(const double *par, double2 *prm, int lane)
{
    constexpr int kPer = NCH / kWaves;
    const int wv = (int)(threadIdx.x >> 6);
    double2 t[3][kPer];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < kPer; ++i) t[k][i] = reinterpret_cast<const double2 *>(par + k * L)[(wv + i * kWaves) * 64 + lane];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < kPer; ++i) prm[(k * NCH + wv + i * kWaves) * 64 + lane] = t[k][i];
    __syncthreads();
}

template <int ING, bool NT>
IDHMC_DEV void chain_pass(double *a0, double *a1, const double *par, double2 *prm, bool stage, double *lq_out, double *pi_out,
                          long long c, int lane, double eps)
{
    constexpr bool G = (ING & kGaddr) != 0;
    // two passes that differ in nothing but the policy of plain loads and stores are merged by the compiler, which drops the policy:
    // the marker keeps them apart (the buffer instructions carry the policy as an operand and need none)
    if (G && !NT) asm volatile("; default-policy chain" ::: "memory");
    Vec<NCH> q = load_row<G, NT>(a0 + c * L, lane), p = load_row<G, NT>(a1 + c * L, lane);
    Vec<NCH> mvv, muv, tav;
    if (ING & kParG) { mvv = vload<NCH>(par, lane); muv = vload<NCH>(par + L, lane); tav = vload<NCH>(par + 2 * L, lane); }
    if ((ING & kParL) && stage) stage_rows(par, prm, lane);
    const double eh = 0.5 * eps;
    double l0 = 0.0, l1 = 0.0, k0 = 0.0, k1 = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        double2 mv = make_double2(1.0, 1.0), mu = make_double2(0.0, 0.0), tau = make_double2(1.0, 1.0);
        if (ING & kParG) { mv = mvv.c[j]; mu = muv.c[j]; tau = tav.c[j]; }
        if (ING & kParL) { mv = prm[j * 64 + lane]; mu = prm[(NCH + j) * 64 + lane]; tau = prm[(2 * NCH + j) * 64 + lane]; }
        if (ING & kArith) {
            const double2 qq = q.c[j], pp = p.c[j];
            const double gx = -(tau.x * (qq.x - mu.x)), gy = -(tau.y * (qq.y - mu.y));
            const double pmx = dfma(eh, gx, pp.x), pmy = dfma(eh, gy, pp.y);
            const double qx = dfma(eps * mv.x, pmx, qq.x), qy = dfma(eps * mv.y, pmy, qq.y);
            const double dx = qx - mu.x, dy = qy - mu.y;
            const double tx = tau.x * dx, ty = tau.y * dy;
            l0 = dfma(tx, dx, l0);
            l1 = dfma(ty, dy, l1);
            const double px = dfma(eh, -tx, pmx), py = dfma(eh, -ty, pmy);
            k0 = dfma(px * mv.x, px, k0);
            k1 = dfma(py * mv.y, py, k1);
            q.c[j] = make_double2(qx, qy);
            p.c[j] = make_double2(px, py);
        } else if (ING & (kParG | kParL)) {
            // folded into the stored values, so that no load is dropped
            q.c[j].x += mv.x * mu.x; q.c[j].y += mv.y * mu.y;
            p.c[j].x += tau.x * mu.x; p.c[j].y += tau.y * mu.y;
        }
    }
    store_row<G, NT>(a0 + c * L, lane, q);
    store_row<G, NT>(a1 + c * L, lane, p);
    if (ING & kRed) {
        double sl, sk;
        wave_sum2(l0, l1, k0, k1, sl, sk);
        double lq = -0.5 * sl;
        lq = dfinite(lq) ? lq : -kInf;
        if (lane == 0) {
            lq_out[c] = lq;
            pi_out[c] = phase_logdensity(lq, 0.5 * sk);
        }
    } else if (ING & kArith) {
        asm volatile("" ::"v"(l0), "v"(l1), "v"(k0), "v"(k1));      // the accumulations stay, the reduction does not
    }
    if (G && !NT) asm volatile("; default-policy chain ends" ::: "memory");
}

// MAXW: at most that many waves per SIMD (the copy alone needs 80 VGPRs and would otherwise run six, the kernel's 200 allow two)
template <int ING, int MAXW = 8>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, MAXW))) void sweep(double *a0, double *a1, const double *par,
                                                                                           double *lq, double *pi, long long C,
                                                                                           int stride, double eps)
{
    __shared__ double2 prm[(ING & kParL) ? 3 * NCH * 64 : 1];
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
    bool stage = true;
    for (long long c = wave; c < C; c += nw, stage = false) {
        if (c % stride == 0) chain_pass<ING, false>(a0, a1, par, prm, stage, lq, pi, c, lane, eps);
        else chain_pass<ING, true>(a0, a1, par, prm, stage, lq, pi, c, lane, eps);
    }
    if ((ING & kParL) && stage) stage_rows(par, prm, lane);      // a wave without a chain still fills and meets the barrier
}
// the placement probe: nvec arrays read and written in place with plain policy (as in ic_slice.hip)
__global__ __launch_bounds__(256) void probe(double *a0, double *a1, int nvec, long long C)
{
    const int lane = threadIdx.x & 63;
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (c >= C) return;
    double *v[2] = {a0, a1};
    for (int j = 0; j < NCH; ++j) {
        double2 x[2];
        for (int k = 0; k < nvec; ++k) x[k] = reinterpret_cast<const double2 *>(v[k] + c * L)[j * 64 + lane];
        for (int k = 0; k < nvec; ++k) reinterpret_cast<double2 *>(v[k] + c * L)[j * 64 + lane] = x[k];
    }
}

// non-trivial values in [-0.5, 0.5): ic_slice.hip sweeps zero-filled arrays, the kernel does not
__global__ void fill_hash(double *a, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (double)(((unsigned long long)i * 0x9E3779B97F4A7C15ull) >> 40) * (1.0 / 16777216.0) - 0.5;
}

typedef void (*SweepFn)(double *, double *, const double *, double *, double *, long long, int, double);
struct Cell { const char *name; SweepFn fn; int blocks_per_cu; };      // blocks_per_cu 0: one workgroup per four chains
static const long long C = 65536;
static const int kStride = 6, kWarm = 3, kRuns = 20, kCus = 256;

static double us_sweep(const Cell &cell, double *a0, double *a1, const double *par, double *lq, double *pi)
{
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const dim3 grid(cell.blocks_per_cu ? (unsigned)(kCus * cell.blocks_per_cu) : (unsigned)((C + kWaves - 1) / kWaves));
    for (int i = 0; i < kWarm; ++i) hipLaunchKernelGGL(cell.fn, grid, dim3(256), 0, 0, a0, a1, par, lq, pi, C, kStride, 0.1);
    (void)hipEventRecord(e0);
    for (int i = 0; i < kRuns; ++i) hipLaunchKernelGGL(cell.fn, grid, dim3(256), 0, 0, a0, a1, par, lq, pi, C, kStride, 0.1);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 1e3 * ms / kRuns;
}
static double probe_gbps(double *a0, double *a1, int nvec)
{
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const dim3 grid((unsigned)((C + 3) / 4));
    for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(probe, grid, dim3(256), 0, 0, a0, a1, nvec, C);
    (void)hipEventRecord(e0);
    for (int i = 0; i < 8; ++i) hipLaunchKernelGGL(probe, grid, dim3(256), 0, 0, a0, a1, nvec, C);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 8.0 * nvec * 2.0 * C * L * 8 / (ms * 1e-3) / 1e9;
}

int main()
{
    constexpr int A = kParG, Ap = kParL, B = kArith, Cc = kRed, Dd = kGaddr;
    const Cell cells[] = {
        {"copy (ST of ic_slice two)", sweep<0>, 0},
        {"copy, at most 2 waves per SIMD", sweep<0, 2>, 0},
        {"copy, at most 3 waves per SIMD", sweep<0, 3>, 0},
        {"+ a    parameters from global", sweep<A>, 0},
        {"+ a b  arithmetic", sweep<A | B>, 0},
        {"+ a b c  reduction, lq and pi stores", sweep<A | B | Cc>, 0},
        {"+ a b c d  global addressing (the kernel)", sweep<A | B | Cc | Dd>, 0},
        {"+ a'   parameters from LDS", sweep<Ap>, 0},
        {"+ a' b c d  (the kernel, parameters in LDS)", sweep<Ap | B | Cc | Dd>, 0},
        {"+ a' b c d  at most 2 waves per SIMD", sweep<Ap | B | Cc | Dd, 2>, 0},
        {"+ a' b c d  grid capped at 2 workgroups per CU", sweep<Ap | B | Cc | Dd>, 2},
        {"+ a' b c d  grid capped at 3 workgroups per CU", sweep<Ap | B | Cc | Dd>, 3},
    };
    const size_t bytes = sizeof(double) * C * L;
    // arrays of both placement classes, found as in ic_slice.hip: a pair streams well when it mixes them
    std::vector<double *> a, b;
    double *ref = nullptr;
    if (hipMalloc(&ref, bytes) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    (void)hipMemset(ref, 0, bytes); (void)hipDeviceSynchronize();
    a.push_back(ref);
    const double single = probe_gbps(ref, nullptr, 1);
    std::vector<void *> spacers;
    for (int i = 0; i < 60 && b.size() < 1; ++i) {
        if (i >= 3) { void *s = nullptr; if (hipMalloc(&s, (size_t)1 << 30) == hipSuccess) spacers.push_back(s); }
        double *x = nullptr; if (hipMalloc(&x, bytes) != hipSuccess) break;
        (void)hipMemset(x, 0, bytes); (void)hipDeviceSynchronize();
        const double r = probe_gbps(ref, x, 2) / single;
        (r >= 1.10 ? b : a).push_back(x);
    }
    if (b.size() < 1) { printf("no array pair of both placement classes found (one array: %.0f GB/s)\n", single); return 0; }
    double *q = a[0], *p = b[0], *par = nullptr, *lq = nullptr, *pi = nullptr;
    if (hipMalloc(&par, 3 * L * sizeof(double)) != hipSuccess || hipMalloc(&lq, C * sizeof(double)) != hipSuccess ||
        hipMalloc(&pi, C * sizeof(double)) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    std::vector<double> hpar(3 * L);
    for (int i = 0; i < L; ++i) { hpar[i] = 1.0; hpar[L + i] = 0.0; hpar[2 * L + i] = 1.0; }      // M^-1 = 1, mu = 0, tau = 1
    (void)hipMemcpy(par, hpar.data(), hpar.size() * sizeof(double), hipMemcpyHostToDevice);
    printf("one array in place: %.0f GB/s; pair A B: %.0f GB/s = %.3f x\n", single, probe_gbps(q, p, 2), probe_gbps(q, p, 2) / single);
    printf("%lld chains x %d doubles x 2 arrays = %.0f MiB; slice c %% %d == 0 default policy, stream nt; %d warm-up + %d timed sweeps per cell\n\n",
           C, L, 2.0 * bytes / 1048576.0, kStride, kWarm, kRuns);
    for (int rep = 0; rep < 4; ++rep) {
        if (rep == 2) {
            const long long n = C * L;
            hipLaunchKernelGGL(fill_hash, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, q, n);
            hipLaunchKernelGGL(fill_hash, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, p, n);
            (void)hipDeviceSynchronize();
            printf("passes 3 and 4: the same arrays filled with values in [-0.5, 0.5) instead of zeros\n\n");
        }
        double copy_us = 0.0;
        for (const Cell &cell : cells) {
            hipFuncAttributes fa;
            (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(cell.fn));
            const double us = us_sweep(cell, q, p, par, lq, pi);
            if (copy_us == 0.0) copy_us = us;
            printf("pass %d  %-50s %7.1f us = %.3f x copy   (%3d VGPRs, %5zu B LDS)\n", rep + 1, cell.name, us, us / copy_us, fa.numRegs,
                   fa.sharedSizeBytes);
        }
        printf("\n");
    }
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) { printf("device error\n"); return 1; }
    return 0;
}
