// idhmc_optimum.hpp -- the FindLocalOptimum warm-up stage (reference src/warmup.jl:137-187), one chain per
// wavefront, for separable and general densities alike.
//
// Contract of the reference stage: maximise l(q) - 1/2 * magnitude_penalty * sum(q^2) for at most `iterations`
// quasi-Newton iterations; a non-finite result draws a new random position, doubles the penalty and tries
// again, at most 100 times (:162-171), else the stage fails (:172); on success the chain's (q, l(q), grad l(q))
// is the optimum.  The reference's optimiser is QuasiNewtonMethods.proptimize! (:163) -- an external package
// whose source is not in the reference tree -- so the iteration is this engine's own: L-BFGS with kLbfgsM
// pairs and Armijo backtracking, stated once in oracle/idhmc_oracle.c (orc_find_local_optimum) and once here,
// operation for operation, with every reduction in the canonical order: the two agree bit for bit.
//
// Where the state lives: x, grad l, G = grad F, the search direction, the trial point and its gradient in
// VGPRs (6 vectors); the (s, y) history as a ring of kLbfgsM + 1 slots in the wavefront's tree arena (L2) --
// one slot is always free, so a new pair is formed in place and simply not committed when it fails the
// curvature test; rho, alpha and the loop state in SGPR-uniform scalars.
#pragma once
#include "idhmc_stream.hpp"

namespace idhmc {

constexpr int kLbfgsM = 5, kLbfgsR = kLbfgsM + 1;

template <int NCH>
IDHMC_DEV double vdot(const Vec<NCH> &a, const Vec<NCH> &b)
{
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        a0 = dfma(a.c[j].x, b.c[j].x, a0);
        a1 = dfma(a.c[j].y, b.c[j].y, a1);
    }
    return wave_sum(a0, a1);
}
// r = fma(a, y, r) elementwise
template <int NCH>
IDHMC_DEV void vaxpy(double a, const Vec<NCH> &y, Vec<NCH> &r)
{
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        r.c[j].x = dfma(a, y.c[j].x, r.c[j].x);
        r.c[j].y = dfma(a, y.c[j].y, r.c[j].y);
    }
}
template <int NCH>
IDHMC_DEV Vec<NCH> vscale(double a, const Vec<NCH> &v)
{
    Vec<NCH> r;
#pragma unroll
    for (int j = 0; j < NCH; ++j) r.c[j] = make_double2(a * v.c[j].x, a * v.c[j].y);
    return r;
}
template <int NCH>
IDHMC_DEV Vec<NCH> vsub(const Vec<NCH> &a, const Vec<NCH> &b)
{
    Vec<NCH> r;
#pragma unroll
    for (int j = 0; j < NCH; ++j) r.c[j] = make_double2(a.c[j].x - b.c[j].x, a.c[j].y - b.c[j].y);
    return r;
}
// small wave-uniform arrays indexed by a run-time slot number: selects instead of scratch memory
IDHMC_DEV double ring_get(const double (&a)[kLbfgsR], int i)
{
    double v = a[0];
#pragma unroll
    for (int u = 1; u < kLbfgsR; ++u) v = (i == u) ? a[u] : v;
    return v;
}
IDHMC_DEV void ring_set(double (&a)[kLbfgsR], int i, double v)
{
#pragma unroll
    for (int u = 0; u < kLbfgsR; ++u) a[u] = (i == u) ? v : a[u];
}

template <int NCH, class Model>
IDHMC_DEV void local_optimum_body(const DevState &s, Model &mdl, double penalty, int iterations, double *hist)
{
    constexpr int L = 128 * NCH, M = kLbfgsM, R = kLbfgsR;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    double *const S = hist, *const Y = hist + (size_t)R * L;
    for (int64_t c = wave; c < s.C; c += nw) {
        const int64_t off = c * L;
        const RngKey key{s.k0, s.k1, s.first_chain + (uint32_t)c};
        bind_chain(mdl, s, key.chain);                         // a GLM with several responses: this chain's Y
        Vec<NCH> x = vload<NCH>(s.q + off, lane);
        Vec<NCH> gl = vload<NCH>(s.g + off, lane);
        double lq = s.lq[c];
        double lam = penalty;
        int rc = IDHMC_ERR_OPTIMIZATION;
        for (uint32_t attempt = 0; attempt < 100u; ++attempt) {                      // :162
            double xx = vdot<NCH>(x, x);
            double F = dfma(0.5 * lam, xx, -lq);
            Vec<NCH> G;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                G.c[j] = make_double2(dfma(lam, x.c[j].x, -gl.c[j].x), dfma(lam, x.c[j].y, -gl.c[j].y));
            double rho[R], alpha[R], gamma = 1.0;
#pragma unroll
            for (int u = 0; u < R; ++u) { rho[u] = 0.0; alpha[u] = 0.0; }
            int k = 0, head = 0;
            for (int it = 0; it < iterations; ++it) {
                const double gg = vdot<NCH>(G, G);
                if (!(gg > 1e-16 * (xx > 1.0 ? xx : 1.0))) break;                     // converged (or not a number)
                Vec<NCH> r = G;
                for (int j = 0; j < k; ++j) {                                         // two-loop recursion, newest first
                    const int i = (head + R - 1 - j) % R;
                    const double al = ring_get(rho, i) * vdot<NCH>(vload<NCH>(S + (size_t)i * L, lane), r);
                    ring_set(alpha, i, al);
                    vaxpy<NCH>(-al, vload<NCH>(Y + (size_t)i * L, lane), r);
                }
                r = vscale<NCH>(k > 0 ? gamma : 1.0 / __builtin_sqrt(gg), r);
                for (int j = k - 1; j >= 0; --j) {                                    // oldest first
                    const int i = (head + R - 1 - j) % R;
                    const double beta = ring_get(rho, i) * vdot<NCH>(vload<NCH>(Y + (size_t)i * L, lane), r);
                    vaxpy<NCH>(ring_get(alpha, i) - beta, vload<NCH>(S + (size_t)i * L, lane), r);
                }
                double gd = -vdot<NCH>(G, r);                                         // direction d = -r
                if (!(gd < 0.0)) {                                                    // not a descent direction: restart
                    k = 0;
                    r = vscale<NCH>(1.0 / __builtin_sqrt(gg), G);
                    gd = -vdot<NCH>(G, r);
                }
                double t = 1.0, lqn = 0.0, xxn = 0.0, Fn = 0.0;
                bool accepted = false;
                Vec<NCH> xn, gln;
                for (int ls = 0; ls < 30; ++ls) {                                     // Armijo backtracking
#pragma unroll
                    for (int j = 0; j < NCH; ++j)
                        xn.c[j] = make_double2(dfma(-t, r.c[j].x, x.c[j].x), dfma(-t, r.c[j].y, x.c[j].y));
                    lqn = density_eval<NCH>(mdl, xn, gln);
                    xxn = vdot<NCH>(xn, xn);
                    Fn = dfma(0.5 * lam, xxn, -lqn);
                    if (dfinite(Fn) && Fn <= dfma(1e-4 * t, gd, F)) { accepted = true; break; }
                    t *= 0.5;
                }
                if (!accepted) break;
                Vec<NCH> Gn;
#pragma unroll
                for (int j = 0; j < NCH; ++j)
                    Gn.c[j] = make_double2(dfma(lam, xn.c[j].x, -gln.c[j].x), dfma(lam, xn.c[j].y, -gln.c[j].y));
                const Vec<NCH> sv = vsub<NCH>(xn, x), yv = vsub<NCH>(Gn, G);
                vstore<NCH>(S + (size_t)head * L, lane, sv);                          // the ring's free slot
                vstore<NCH>(Y + (size_t)head * L, lane, yv);
                const double sy = vdot<NCH>(sv, yv), yy = vdot<NCH>(yv, yv);
                if (sy > 1e-10 * yy) {                                                // curvature condition: commit the pair
                    ring_set(rho, head, 1.0 / sy);
                    gamma = sy / yy;
                    head = (head + 1) % R;
                    if (k < M) ++k;
                }
                x = xn; gl = gln; G = Gn;
                lq = lqn; F = Fn; xx = xxn;
            }
            if (dfinite(lq)) { rc = 0; break; }                                       // :168
            // random_position! with this attempt's draws, evaluate, double the penalty (:169-171)
            x = uniform_position<NCH>(key, attempt + 1u, lane, s.D);
            lq = density_eval<NCH>(mdl, x, gl);
            lam += lam;
        }
        vstore<NCH>(s.q + off, lane, x);
        vstore<NCH>(s.g + off, lane, gl);
        if (lane == 0) {
            s.lq[c] = lq;
            if (rc) s.status[c] = rc;                                                 // "Optimization failed to converge", :172
        }
    }
}

// a separable density's parameters in registers, a general density's LDS vector per wavefront (idhmc_stream.hpp)
template <int NCH, class Model>
__global__ __launch_bounds__(kStreamWaves * 64) void k_local_optimum(DevState s, double penalty, int iterations)
{
    IDHMC_WAVE_LDS_VECTOR(lds_vec);
    Model mdl;
    density_setup(mdl, s, lds_vec, threadIdx.x & 63);
    double *hist = s.arena + ((int64_t)blockIdx.x * kStreamWaves + (threadIdx.x >> 6)) * s.arena_stride;
    local_optimum_body<NCH, Model>(s, mdl, penalty, iterations, hist);
}

#ifndef __HIPCC_RTC__
template <template <int> class Model>
static hipError_t launch_local_optimum_t(const DevState &s, double penalty, int iterations, hipStream_t st)
{
    return dispatch_nch<Model>(s.nch, [&](auto n) {
        constexpr int NCH = decltype(n)::value;
        hipLaunchKernelGGL((k_local_optimum<NCH, Model<NCH>>), dim3(optimum_grid(s)), dim3(kStreamWaves * 64), 0, st, s, penalty,
                           iterations);
        return hipGetLastError();
    });
}
#endif

}  // namespace idhmc
