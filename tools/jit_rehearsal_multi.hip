// jit_rehearsal_multi.hip -- tools/jit_rehearsal.hip for DESIGN section 27: the kernels hipRTC builds for a GLM with a factor term that
// has several weighted levels per observation (kFactors = true, kSlopes = true, kMulti = true), compiled ahead of time so that they
// cross-compile for gfx950 without a device and tools/kres.py shows their resource figures next to those of their kSlopes twins in
// tools/jit_rehearsal_slopes.hip (the same policies, kernels and sizes; MULTI = 0 instantiates the twins in this unit as well, so
// that one run of kres.py prints both; PoisObs<groups, priors, local, gmrf, multi>, GaussObs<multi>):
//     tools/kres.py tools/jit_rehearsal_multi.hip k_ -Iinplacedhmc.jl_amd/csrc
// Poisson (A = 0) without a group and with one, with the priors' table, local scales and a GMRF term (the P-spline), and the Gaussian
// with a sampled scale (A = 1, H = 1): the matrix-core form at NCH = 1 and NCH = 2, the per-wave form at NCH = 4 and NCH = 8.  Not part
// of the library.
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"
namespace idhmc {

// (integer flags and short names: tools/kres.py prints 70 characters of a kernel's name, and the last flag tells the twins apart)
template <int GROUPS, int PRIORS, int LOCAL, int GMRF, int MULTI>
struct PoisObs {
    static constexpr int K = 1, A = 0, H = GROUPS;
    static constexpr bool kResponses = false, kPriors = PRIORS != 0, kLocal = LOCAL != 0, kFactors = true, kSlopes = true, kCorr = false, kStruct = false,
                          kGmrf = GMRF != 0, kBlock = false, kMulti = MULTI != 0;
    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v)
    {
        const double e = dexp(z);
        v = e - o.y[0] * z;
        r = o.y[0] - e;
    }
};
template <int MULTI>
struct GaussObs {
    static constexpr int K = 1, A = 1, H = 1;
    static constexpr bool kResponses = false, kPriors = false, kLocal = false, kFactors = true, kSlopes = true, kCorr = false, kStruct = false,
                          kGmrf = false, kBlock = false, kMulti = MULTI != 0;
    IDHMC_DEV static void terms(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
    {
        const double w = dexp(-a[0]);
        const double u = (o.y[0] - z) * w;
        v = 0.5 * (u * u) + a[0];
        r = u * w;
        s[0] = u * u - 1.0;
    }
};

#define IDHMC_COMMA ,
#define IDHMC_REHEARSE_NUTS(N, MODEL)                                                  \
    template __global__ void k_nuts<N, MODEL, true>(DevState, uint32_t, uint32_t);    \
    template __global__ void k_nuts<N, MODEL, false>(DevState, uint32_t, uint32_t);
#define IDHMC_REHEARSE_OBS(OBS)                                  \
    IDHMC_REHEARSE_NUTS(1, GlmCoop<1 IDHMC_COMMA OBS>)           \
    IDHMC_REHEARSE_NUTS(2, GlmCoop<2 IDHMC_COMMA OBS>)           \
    IDHMC_REHEARSE_NUTS(4, GlmWave<4 IDHMC_COMMA OBS>)           \
    template __global__ void k_nuts<8, GlmWave<8 IDHMC_COMMA OBS>, true>(DevState, uint32_t, uint32_t);    \
    template __global__ void k_leapfrog<2, GlmWave<2 IDHMC_COMMA OBS>>(DevState, double, int, int);        \
    template __global__ void k_eval<1, GlmWave<1 IDHMC_COMMA OBS>>(DevState, int);
#define IDHMC_REHEARSE_PAIR(NAME, ...)              \
    using NAME##Multi = __VA_ARGS__ 1 > ;           \
    using NAME##Slopes = __VA_ARGS__ 0 > ;          \
    IDHMC_REHEARSE_OBS(NAME##Multi)                 \
    IDHMC_REHEARSE_OBS(NAME##Slopes)
IDHMC_REHEARSE_PAIR(Poisson, PoisObs < 0, 0, 0, 0,)
IDHMC_REHEARSE_PAIR(PoissonGroup, PoisObs < 1, 0, 0, 0,)
IDHMC_REHEARSE_PAIR(PoissonGroupPriorsLocal, PoisObs < 2, 1, 1, 0,)
IDHMC_REHEARSE_PAIR(PoissonGroupGmrf, PoisObs < 1, 1, 0, 1,)
IDHMC_REHEARSE_PAIR(Gauss, GaussObs <)

}  // namespace idhmc
