// jit_rehearsal.hip -- the source idhmc_jit.hip hands to hipRTC, compiled ahead of time: the same #include lines, a user's
// density and a user's GLM, and explicit instantiations of exactly the five name expressions jit_build asks for, once for a
// custom density (tests/test_gpu_custom.py's, L = 1024) and once for a GLM with A = 1 (glm.GAUSSIAN_IDENTITY_LOGSIGMA as
// tools/bench_glm.py runs it, L = 256: the matrix-core form in the NUTS kernel), both with a shared metric.  `make` never
// compiles the hipRTC source; this does, and gives tools/kres.py the resource figures of those kernels:
//     tools/kres.py tools/jit_rehearsal.hip "" -Iinplacedhmc.jl_amd/csrc
// Not part of the library.
#define IDHMC_JIT_USER_DENSITY 1
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"
namespace idhmc {

template <int NCH>
__device__ double logdensity_and_gradient(const Vec<NCH> &q, Vec<NCH> &grad, const UserCtx &ctx)
{
    const double a = ctx.params[0], b = ctx.params[1], c = ctx.params[2];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) { s0 = s0 + q.c[j].x; s1 = s1 + q.c[j].y; }
    const double S = wave_sum(s0, s1);
    double l0 = 0.0, l1 = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int i0 = 128 * j + 2 * ctx.lane;
        const double x = q.c[j].x, y = q.c[j].y;
        const double x2 = x * x, y2 = y * y;
        const double gx = -(a * (x2 * x)) - b * x - c * S, gy = -(a * (y2 * y)) - b * y - c * S;
        grad.c[j].x = (i0 < ctx.D) ? gx : 0.0;
        grad.c[j].y = (i0 + 1 < ctx.D) ? gy : 0.0;
        l0 = l0 + (0.25 * a * (x2 * x2) + 0.5 * b * x2);
        l1 = l1 + (0.25 * a * (y2 * y2) + 0.5 * b * y2);
    }
    return -wave_sum(l0, l1) - 0.5 * c * (S * S);
}

__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double w = dexp(-a[0]);
    const double u = (o.y[0] - z) * w;
    v = 0.5 * (u * u) + a[0];
    r = u * w;
    s[0] = u * u - 1.0;
}
struct UserGlmObs {
    static constexpr int K = 1, A = 1, H = 0;
    static constexpr bool kResponses = false, kPriors = false, kLocal = false, kFactors = false, kSlopes = false, kCorr = false, kStruct = false, kGmrf = false, kBlock = false, kMulti = false;
    IDHMC_DEV static void terms(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
    {
        glm_observation(z, o, a, r, v, s);
    }
};

#define IDHMC_REHEARSE(N, MODEL, NUTS_MODEL)                                          \
    template __global__ void k_eval<N, MODEL>(DevState, int);                         \
    template __global__ void k_leapfrog<N, MODEL>(DevState, double, int, int);        \
    template __global__ void k_stepsize_search<N, MODEL>(DevState);                   \
    template __global__ void k_nuts<N, NUTS_MODEL, true>(DevState, uint32_t, uint32_t); \
    template __global__ void k_local_optimum<N, MODEL>(DevState, double, int);
#define IDHMC_COMMA ,
IDHMC_REHEARSE(8, JitModel<8>, JitModel<8>)
IDHMC_REHEARSE(2, GlmWave<2 IDHMC_COMMA UserGlmObs>, GlmCoop<2 IDHMC_COMMA UserGlmObs>)

}  // namespace idhmc
