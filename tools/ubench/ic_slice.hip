// ic_slice.hip -- can a fixed slice of the chains stay in the Infinity Cache from one sweep to the next while the rest of the state
// streams past it?  (tools/ubench, GPU box)  The sweep of k_leapfrog1<8, ., 3>: 65 536 chains x 1024 doubles in three arrays, one
// chain per wavefront, each wave loads its 3 x 8 KiB rows (16 B per lane, all 24 loads before the first store) and stores them back in
// place.  Chains with c % stride == 0 form the TABLE (spread through the sweep), the others the STREAM; each side has its own
// cache-policy bits on every load and store (the buffer AUX of bload / bstore).  For every (table policy, stream policy) pair and
// table size it times, back to back:
//   S   the stream chains alone (table waves exit at once),
//   ST  stream + table, each with its own policy,
//   H   stream + table both with the stream policy (the table's bytes at the stream's rate; for the nt stream: today's sweep).
// The table is resident when ST <= 1.02 x S.  Arrays: one set of three that streams in the good placement mode (pair probe as in
// placement_pingpong.hip).
// `ic_slice two`: the sweep of the REGRAD variants, which touch q and p only -- a0 and a1 (classes A B) are swept, a2 is left alone, with
// the one policy pair the kernel uses (nt stream, default-policy table) at strides 8, 6 and 5: 128, 170.7 and 204.8 MiB of table.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/ubench/ic_slice tools/ubench/ic_slice.hip
#include "../../inplacedhmc.jl_amd/csrc/idhmc_device.hpp"
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

using namespace idhmc;

constexpr int NCH = 8, L = 128 * NCH;
// gfx950 buffer AUX bits: sc0 = 1, nt = 2, sc1 = 16 (the compiler emits sc1 + nt as plain nt, so that pair is not listed);
// a policy is (load AUX) | (store AUX) << 8
constexpr int kPol[8] = {0, 2 | 2 << 8, 1 | 1 << 8, 16 | 16 << 8, 3 | 3 << 8, 17 | 17 << 8, 2, 2 << 8};
static const char *kPolName[8] = {"default", "nt", "sc0", "sc1", "sc0 nt", "sc0 sc1", "ld nt", "st nt"};

template <int POL>
IDHMC_DEV void chain_pass(double *a0, double *a1, double *a2, int lane)
{
    constexpr int LD = POL & 255, ST = POL >> 8;
    Vec<NCH> x0 = bload<NCH, LD>(a0, lane), x1 = bload<NCH, LD>(a1, lane), x2 = bload<NCH, LD>(a2, lane);
    bstore<NCH, ST>(a0, lane, x0);
    bstore<NCH, ST>(a1, lane, x1);
    bstore<NCH, ST>(a2, lane, x2);
}
template <int POL>
IDHMC_DEV void chain_pass2(double *a0, double *a1, int lane)
{
    constexpr int LD = POL & 255, ST = POL >> 8;
    Vec<NCH> x0 = bload<NCH, LD>(a0, lane), x1 = bload<NCH, LD>(a1, lane);
    bstore<NCH, ST>(a0, lane, x0);
    bstore<NCH, ST>(a1, lane, x1);
}
// mode 0: stream chains only; 1: every chain; 2: table chains only
template <int TPOL, int SPOL>
__global__ __launch_bounds__(256, 2) void sweep2(double *a0, double *a1, double *, long long C, int stride, int mode)
{
    const int lane = threadIdx.x & 63;
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (c >= C) return;
    const bool table = (c % stride) == 0;
    if ((mode == 0 && table) || (mode == 2 && !table)) return;
    const long long off = c * L;
    if (table) chain_pass2<TPOL>(a0 + off, a1 + off, lane);
    else chain_pass2<SPOL>(a0 + off, a1 + off, lane);
}
template <int TPOL, int SPOL>
__global__ __launch_bounds__(256, 2) void sweep(double *a0, double *a1, double *a2, long long C, int stride, int mode)
{
    const int lane = threadIdx.x & 63;
    const long long c = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (c >= C) return;
    const bool table = (c % stride) == 0;
    if ((mode == 0 && table) || (mode == 2 && !table)) return;
    const long long off = c * L;
    if (table) chain_pass<TPOL>(a0 + off, a1 + off, a2 + off, lane);
    else chain_pass<SPOL>(a0 + off, a1 + off, a2 + off, lane);
}
// the placement probe: nvec arrays read and written in place with plain policy
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

typedef void (*SweepFn)(double *, double *, double *, long long, int, int);
static SweepFn g_fn[8][8];
template <size_t I> static void fill_one() { g_fn[I / 8][I % 8] = sweep<kPol[I / 8], kPol[I % 8]>; }
template <size_t... I> static void fill_all(std::index_sequence<I...>) { (fill_one<I>(), ...); }

static SweepFn g_fn2[2][2];      // two-array mode: [table policy][stream policy] over {default, nt}
static bool g_two = false;
static const long long C = 65536;
static const int kWarm = 3, kRuns = 20;

// mean microseconds per sweep over kRuns back-to-back launches after kWarm
static double us_sweep(int ti, int si, double *a0, double *a1, double *a2, int stride, int mode)
{
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const dim3 grid((unsigned)((C + 3) / 4));
    const SweepFn fn = g_two ? g_fn2[ti][si] : g_fn[ti][si];
    for (int i = 0; i < kWarm; ++i) hipLaunchKernelGGL(fn, grid, dim3(256), 0, 0, a0, a1, a2, C, stride, mode);
    (void)hipEventRecord(e0);
    for (int i = 0; i < kRuns; ++i) hipLaunchKernelGGL(fn, grid, dim3(256), 0, 0, a0, a1, a2, C, stride, mode);
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

int main(int argc, char **argv)
{
    fill_all(std::make_index_sequence<64>{});
    g_fn2[0][0] = sweep2<kPol[0], kPol[0]>; g_fn2[0][1] = sweep2<kPol[0], kPol[1]>;
    g_fn2[1][0] = sweep2<kPol[1], kPol[0]>; g_fn2[1][1] = sweep2<kPol[1], kPol[1]>;
    g_two = argc > 1 && std::string(argv[1]) == "two";
    const size_t A = sizeof(double) * C * L;
    // arrays of both placement classes (a set streams well when it mixes them); the sweep uses classes A B A like place_state
    std::vector<double *> a, b;
    double *ref = nullptr;
    if (hipMalloc(&ref, A) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    (void)hipMemset(ref, 0, A); (void)hipDeviceSynchronize();
    a.push_back(ref);
    const double single = probe_gbps(ref, nullptr, 1);
    std::vector<void *> spacers;
    for (int i = 0; i < 60 && (a.size() < 2 || b.size() < 1); ++i) {
        if (i >= 3) { void *s = nullptr; if (hipMalloc(&s, (size_t)1 << 30) == hipSuccess) spacers.push_back(s); }
        double *x = nullptr; if (hipMalloc(&x, A) != hipSuccess) break;
        (void)hipMemset(x, 0, A); (void)hipDeviceSynchronize();
        const double r = probe_gbps(ref, x, 2) / single;
        (r >= 1.10 ? b : a).push_back(x);
    }
    if (a.size() < 2 || b.size() < 1) { printf("no array set of both placement classes found (one array: %.0f GB/s)\n", single); return 0; }
    double *q = a[0], *p = b[0], *g = a[1];
    printf("one array in place: %.0f GB/s; pair A B: %.0f GB/s; sweep on arrays of classes A B A\n", single, probe_gbps(q, p, 2));
    printf("state: %lld chains x %d doubles x 3 arrays = %.0f MiB; %d warm-up + %d timed sweeps back to back per cell (mean)\n\n",
           C, L, 3.0 * A / 1048576.0, kWarm, kRuns);

    if (g_two) {
        printf("two-array mode: a0 (class A) and a1 (class B) are swept, %.0f MiB; stream policy nt, table policy default\n\n", 2.0 * A / 1048576.0);
        const int strides2[] = {8, 6, 5};
        for (int rep = 0; rep < 2; ++rep)
            for (int stride : strides2) {
                const long long nt = (C + stride - 1) / stride;
                const double tab_mib = nt * 2.0 * L * 8 / 1048576.0, str_gib = (C - nt) * 4.0 * L * 8 / 1073741824.0;
                const double S = us_sweep(1, 1, q, p, g, stride, 0), H = us_sweep(1, 1, q, p, g, stride, 1);
                const double T = us_sweep(0, 0, q, p, g, stride, 2), ST = us_sweep(0, 1, q, p, g, stride, 1);
                printf("stride %d: table %lld chains = %.1f MiB held; stream %.2f GiB moved per sweep\n", stride, nt, tab_mib, str_gib);
                printf("   S  stream alone (nt)            %7.1f us\n   ST stream nt + table default    %7.1f us = %.3f x S%s\n"
                       "   H  stream + table both nt       %7.1f us = %.3f x S\n   T  table alone (default)        %7.1f us\n"
                       "   ST / H = %.3f: %s by the criterion ST <= 1.02 S\n",
                       S, ST, ST / S, ST <= 1.02 * S ? " *" : "", H, H / S, T, ST / H, ST <= 1.02 * S ? "RESIDENT" : "not resident");
            }
        return 0;
    }
    const int strides[] = {24, 12, 8, 7};
    for (int stride : strides) {
        const long long nt = (C + stride - 1) / stride;
        const double tab_mib = nt * 3.0 * L * 8 / 1048576.0, str_gib = (C - nt) * 6.0 * L * 8 / 1073741824.0;
        printf("=== stride %d: table %lld chains = %.0f MiB held (%.0f MiB moved per sweep); stream %.2f GiB moved per sweep ===\n",
               stride, nt, tab_mib, 2 * tab_mib, str_gib);
        double S[8], H[8], T[8], ST[8][8];
        for (int si = 0; si < 8; ++si) {
            S[si] = us_sweep(si, si, q, p, g, stride, 0);
            H[si] = us_sweep(si, si, q, p, g, stride, 1);
        }
        for (int ti = 0; ti < 8; ++ti) T[ti] = us_sweep(ti, ti, q, p, g, stride, 2);
        for (int ti = 0; ti < 8; ++ti)
            for (int si = 0; si < 8; ++si) ST[ti][si] = us_sweep(ti, si, q, p, g, stride, 1);
        printf("stream policy:        ");
        for (int si = 0; si < 8; ++si) printf(" %10s", kPolName[si]);
        printf("\nS  stream alone (us): ");
        for (int si = 0; si < 8; ++si) printf(" %10.1f", S[si]);
        printf("\nH  table at stream policy (us):");
        for (int si = 0; si < 8; ++si) printf(" %10.1f", H[si]);
        printf("\n   H / S:             ");
        for (int si = 0; si < 8; ++si) printf(" %10.3f", H[si] / S[si]);
        printf("\nST / S (rows: table policy; table alone in us at the right):\n");
        for (int ti = 0; ti < 8; ++ti) {
            printf("   %-18s ", kPolName[ti]);
            for (int si = 0; si < 8; ++si) printf(" %9.3f%s", ST[ti][si] / S[si], ST[ti][si] <= 1.02 * S[si] ? "*" : " ");
            printf("   | %7.1f\n", T[ti]);
        }
        printf("resident (* = ST <= 1.02 S); best ST per stream policy vs nt-everywhere H[nt] = %.1f us:\n", H[1]);
        for (int si = 0; si < 8; ++si) {
            int best = 0;
            for (int ti = 1; ti < 8; ++ti) if (ST[ti][si] < ST[best][si]) best = ti;
            printf("   stream %-11s table %-11s ST %7.1f us = %.3f x H[nt]\n", kPolName[si], kPolName[best], ST[best][si], ST[best][si] / H[1]);
        }
        printf("\n");
    }
    (void)argc; (void)argv;
    return 0;
}
