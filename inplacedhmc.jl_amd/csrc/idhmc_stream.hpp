// idhmc_stream.hpp -- the streaming kernels, one per reference function and for every density: evaluation (with the random start),
// fused leapfrog, initial-stepsize search; one chain per wavefront, kStreamWaves chains per workgroup.  A density is either
//   separable (Model::kSeparable: the Gaussians)  load(mu, tau, lane) puts its parameters in registers, mu(j) / tau(j) give them; or
//   general  a type with
//     template <class State> __device__ void init(const State &s, double *lds_vec, int lane);
//     __device__ double grad(const Vec<NCH> &q, Vec<NCH> &g) const;     // returns l(q), fills grad l(q)
//   -- the device form of the reference's logdensity_and_gradient!(grad, model, q, sptr) (src/kinetic_energy.jl:73) -- which owns
//   one LDS vector per wavefront.
// The three places where the two differ are the compile-time choices below; everything else is stated once.  Instantiated ahead
// of time by the translation unit that owns a density (idhmc_kernels.hip, idhmc_dense.hip, idhmc_logistic.hip) and at run time
// through hipRTC for a user-supplied density (idhmc_jit.hip).
#pragma once
#include "idhmc_device.hpp"
#include "idhmc_internal.hpp"

namespace idhmc {

// random_position! (src/warmup.jl:73): q ~ U[-2,2)^D, pads zero; `attempt` addresses the draw (0: the start, n + 1: the n-th
// restart of the FindLocalOptimum stage)
template <int NCH>
IDHMC_DEV Vec<NCH> uniform_position(const RngKey &key, uint32_t attempt, int lane, int D)
{
    const auto spread = [](double u) { return dfma(4.0, u, -2.0); };     // [0,1) -> [-2,2)
    Vec<NCH> q;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int pair = j * 64 + lane;
        const u32x4 x = rng_draw(key, attempt, kStreamInitQ, (uint32_t)pair);
        q.c[j].x = (2 * pair < D) ? spread(u01(x.x, x.y)) : 0.0;
        q.c[j].y = (2 * pair + 1 < D) ? spread(u01(x.z, x.w)) : 0.0;
    }
    return q;
}

// ---- separable or general: set-up, evaluation, one leapfrog step --------------------------------------------------------------
template <class Model>
IDHMC_DEV void density_setup(Model &mdl, const DevState &s, double *lds_vec, int lane)
{
    if constexpr (Model::kSeparable) mdl.load(s.mu, s.tau, lane);
    else mdl.init(s, lds_vec, lane);
}
template <int NCH, class Model>
IDHMC_DEV double density_eval(const Model &mdl, const Vec<NCH> &q, Vec<NCH> &g)
{
    double lq;
    if constexpr (Model::kSeparable) lq = eval_density<NCH>(mdl, q, g);
    else lq = mdl.grad(q, g);
    return dfinite(lq) ? lq : -kInf;                    // evaluate_l!, src/kinetic_energy.jl:80-84
}
template <int NCH, class Model>
IDHMC_DEV void density_step(const Model &mdl, const Vec<NCH> &minv, double eps, Vec<NCH> &q, Vec<NCH> &p, Vec<NCH> &g,
                            double &lq, double &K)
{
    if constexpr (Model::kSeparable) leapfrog_step<NCH>(mdl, minv, eps, q, p, g, lq, K);
    else leapfrog_step_general<NCH>(mdl, minv, eps, q, p, g, lq, K);
}
// The third choice is the kernel's: a general density's owns one LDS vector per wavefront, PTR; a separable one's declares none
// (0 bytes of LDS) and PTR is null.  For use inside a kernel template: reads the enclosing template's `Model` and `NCH`.
#define IDHMC_WAVE_LDS_VECTOR(PTR)                                                          \
    double *PTR = nullptr;                                                                  \
    if constexpr (!Model::kSeparable) {                                                     \
        __shared__ __attribute__((aligned(16))) double dshare[kStreamWaves][128 * NCH];     \
        PTR = dshare[threadIdx.x >> 6];                                                     \
    }
// (The kernels compute their wavefront's index themselves: only inside a __global__ function does the compiler fold blockDim.x to
// the launch bound.)

// evaluate_l! (src/kinetic_energy.jl:72-85); random_q = 1: q ~ U[-2,2) first (random_position!, src/warmup.jl:73)
template <int NCH, class Model>
__global__ __launch_bounds__(kStreamWaves * 64) void k_eval(DevState s, int random_q)
{
    IDHMC_WAVE_LDS_VECTOR(lds_vec);
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    Model mdl;
    density_setup(mdl, s, lds_vec, lane);
    for (int64_t c = wave; c < s.C; c += nw) {
        const RngKey key{s.k0, s.k1, s.first_chain + (uint32_t)c};
        bind_chain(mdl, s, key.chain);                         // a GLM with several responses: this chain's Y
        Vec<NCH> q, g;
        if (random_q) {
            q = uniform_position<NCH>(key, 0u, lane, s.D);
            vstore<NCH>(s.q + c * s.L, lane, q);
        } else {
            q = vload<NCH>(s.q + c * s.L, lane);
        }
        const double lq = density_eval<NCH>(mdl, q, g);
        vstore<NCH>(s.g + c * s.L, lane, g);
        if (lane == 0) s.lq[c] = lq;
    }
}

// leapfrog (src/kinetic_energy.jl:126-163), n_steps per launch, state in registers.
// HBM traffic per chain and launch: read q, p, grad, write q', p', grad' = 6*L*8 bytes
// (M^-1, and a separable density's mu, tau, are L2-resident: L*8 bytes each, shared by all chains).
template <int NCH, class Model>
__global__ __launch_bounds__(kStreamWaves * 64) void k_leapfrog(DevState s, double eps_arg, int own_eps, int n_steps)
{
    IDHMC_WAVE_LDS_VECTOR(lds_vec);
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    Model mdl;
    density_setup(mdl, s, lds_vec, lane);
    for (int64_t c = wave; c < s.C; c += nw) {
        bind_chain(mdl, s, s.first_chain + (uint32_t)c);       // a GLM with several responses: this chain's Y
        const int64_t off = c * s.L;
        Vec<NCH> q = vload<NCH>(s.q + off, lane);
        Vec<NCH> p = vload<NCH>(s.p + off, lane);
        Vec<NCH> g = vload<NCH>(s.g + off, lane);
        const Vec<NCH> minv = vload<NCH>(s.minv + c * s.minv_stride, lane);
        const double eps = own_eps ? s.eps[c] : eps_arg;
        double lq = 0.0, K = 0.0;
        for (int it = 0; it < n_steps; ++it) density_step<NCH>(mdl, minv, eps, q, p, g, lq, K);
        vstore<NCH>(s.q + off, lane, q);
        vstore<NCH>(s.p + off, lane, p);
        vstore<NCH>(s.g + off, lane, g);
        if (lane == 0) {
            s.lq[c] = lq;
            s.pi[c] = phase_logdensity(lq, K);
        }
    }
}

// A(eps) of find_initial_stepsize (src/stepsize.jl:150-154): exp(logdensity(H, leapfrog(z, eps)) - logdensity(H, z)); only
// scalars leave the registers
template <int NCH, class Model>
IDHMC_DEV double local_ratio(const Model &mdl, const Vec<NCH> &minv, const Vec<NCH> &q, const Vec<NCH> &p,
                             const Vec<NCH> &g, double eps, double target)
{
    Vec<NCH> q1 = q, p1 = p, g1 = g;
    double lq, K;
    density_step<NCH>(mdl, minv, eps, q1, p1, g1, lq, K);
    return dexp(phase_logdensity(lq, K) - target);
}

// find_initial_stepsize (src/stepsize.jl:111-164) per chain.  The one streaming kernel whose chain loop is a function of its own,
// because it is the one at the edge of its registers: a general density's search holds 7 vectors and sits at the SGPR limit, and
// with the state taken by reference (State = const DevState &) the compiler keeps it inside two wavefronts per SIMD at L = 1024
// (255 VGPRs; used in place as the kernel's parameter: 254 + 2 AGPRs, one wavefront).  The Gaussians take it by value (State =
// DevState), which leaves their register, scratch and LDS figures what they are in the kernel itself.
template <int NCH, class Model, class State>
IDHMC_DEV void stepsize_search_chains(State s, double *lds_vec, int lane, int64_t wave, int64_t nw)
{
    Model mdl;
    density_setup(mdl, s, lds_vec, lane);
    for (int64_t c = wave; c < s.C; c += nw) {
        bind_chain(mdl, s, s.first_chain + (uint32_t)c);       // a GLM with several responses: this chain's Y
        const int64_t off = c * s.L;
        const Vec<NCH> q = vload<NCH>(s.q + off, lane);
        const Vec<NCH> p = vload<NCH>(s.p + off, lane);
        const Vec<NCH> g = vload<NCH>(s.g + off, lane);
        const Vec<NCH> minv = vload<NCH>(s.minv + c * s.minv_stride, lane);
        const double target = phase_logdensity(s.lq[c], kinetic_energy<NCH>(minv, p));     // :151
        int rc = 0;
        double e0 = s.ss_eps0, result = s.ss_eps0;
        if (!dfinite(target)) {
            rc = IDHMC_ERR_NONFINITE_START;                                                // :152-153
        } else {
            double A0 = local_ratio<NCH>(mdl, minv, q, p, g, e0, target);                  // :113
            if (!(s.ss_a_min <= A0 && A0 <= s.ss_a_max)) {                                 // :114
                const double sg = A0 > s.ss_a_max ? 1.0 : -1.0;                            // find_crossing_stepsize :51-72
                const double a = A0 > s.ss_a_max ? s.ss_a_max : s.ss_a_min;
                const double Cf = sg < 0.0 ? 1.0 / s.ss_C : s.ss_C;
                double e1 = e0, A1 = A0;
                bool found = false;
                for (int it = 0; it < s.ss_maxiter_crossing; ++it) {
                    const double e = e0 * Cf;
                    const double Ae = local_ratio<NCH>(mdl, minv, q, p, g, e, target);
                    if (sg * (Ae - a) <= 0.0) { e1 = e; A1 = Ae; found = true; break; }
                    e0 = e; A0 = Ae;
                }
                if (!found) {
                    rc = IDHMC_ERR_STEPSIZE_SEARCH;                                        // :71
                } else if (s.ss_a_min <= A1 && A1 <= s.ss_a_max) {
                    result = e1;                                                           // :118
                } else {
                    double lo = e0, hi = e1;                                               // :120-124
                    if (!(e0 < e1)) { lo = e1; hi = e0; }
                    found = false;
                    for (int it = 0; it < s.ss_maxiter_bisect; ++it) {                     // bisect_stepsize :83-102
                        const double em = 0.5 * (lo + hi);
                        const double Am = local_ratio<NCH>(mdl, minv, q, p, g, em, target);
                        if (s.ss_a_min <= Am && Am <= s.ss_a_max) { result = em; found = true; break; }
                        else if (Am < s.ss_a_min) hi = em;
                        else lo = em;
                    }
                    if (!found) rc = IDHMC_ERR_STEPSIZE_SEARCH;                            // :101
                }
            }
        }
        if (lane == 0) {
            s.eps[c] = result;
            if (rc) s.status[c] = rc;
        }
    }
}
template <int NCH, class Model>
__global__ __launch_bounds__(kStreamWaves * 64) void k_stepsize_search(DevState s)
{
    IDHMC_WAVE_LDS_VECTOR(lds_vec);
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if constexpr (Model::kSeparable) stepsize_search_chains<NCH, Model, DevState>(s, lds_vec, lane, wave, nw);
    else stepsize_search_chains<NCH, Model, const DevState &>(s, lds_vec, lane, wave, nw);
}

#ifndef __HIPCC_RTC__
// ---- host: one launcher per kernel, instantiated by the translation unit that owns the density --------------------------------
// The padded lengths a density is built for: every NCH in 1..16 for a separable one, the powers of two up to 8 for a general one.
// f is called with IntC<NCH>.
template <int N> struct IntC { static constexpr int value = N; };
template <template <int> class Model, class F>
static hipError_t dispatch_nch(int nch, F &&f)
{
    if constexpr (Model<1>::kSeparable) { IDHMC_DISPATCH_NCH(nch, return f(IntC<NCH>{})); }
    else { IDHMC_DISPATCH_NCH_POW2(nch, return f(IntC<NCH>{})); }
}
// the separable row is two densities, one model id each.  Reads the caller's `s`; the caller is an entry of the separable row, which
// backend(model) hands out for these two model ids only (idhmc_internal.hpp), so "not iso" is diag here
#define IDHMC_SEPARABLE(LAUNCHER, ...) \
    (s.model == IDHMC_MODEL_ISO_GAUSSIAN ? LAUNCHER<IsoGaussian>(__VA_ARGS__) : LAUNCHER<DiagGaussian>(__VA_ARGS__))
template <template <int> class Model>
static int stream_grid_of(int64_t C) { return stream_grid(C, Model<1>::kSeparable ? kSeparableBlocks : kGeneralBlocks); }

template <template <int> class Model>
static hipError_t launch_eval_t(const DevState &s, int random_q, hipStream_t st)
{
    return dispatch_nch<Model>(s.nch, [&](auto n) {
        constexpr int NCH = decltype(n)::value;
        hipLaunchKernelGGL((k_eval<NCH, Model<NCH>>), dim3(stream_grid_of<Model>(s.C)), dim3(kStreamWaves * 64), 0, st, s, random_q);
        return hipGetLastError();
    });
}
template <template <int> class Model>
static hipError_t launch_leapfrog_t(const DevState &s, double eps, int own, int n_steps, hipStream_t st)
{
    return dispatch_nch<Model>(s.nch, [&](auto n) {
        constexpr int NCH = decltype(n)::value;
        hipLaunchKernelGGL((k_leapfrog<NCH, Model<NCH>>), dim3(stream_grid_of<Model>(s.C)), dim3(kStreamWaves * 64), 0, st, s, eps, own,
                           n_steps);
        return hipGetLastError();
    });
}
template <template <int> class Model>
static hipError_t launch_stepsize_search_t(const DevState &s, hipStream_t st)
{
    return dispatch_nch<Model>(s.nch, [&](auto n) {
        constexpr int NCH = decltype(n)::value;
        hipLaunchKernelGGL((k_stepsize_search<NCH, Model<NCH>>), dim3(stream_grid_of<Model>(s.C)), dim3(kStreamWaves * 64), 0, st, s);
        return hipGetLastError();
    });
}
#endif

}  // namespace idhmc
