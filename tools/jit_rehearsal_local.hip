// jit_rehearsal_local.hip -- tools/jit_rehearsal.hip for DESIGN section 19: the kernels hipRTC builds for a GLM with per-coefficient
// local scales (kLocal = true), compiled ahead of time so that tools/kres.py shows their resource figures:
//     tools/kres.py tools/jit_rehearsal_local.hip k_ -Iinplacedhmc.jl_amd/csrc
// Poisson (A = 0) without a group and with one, with and without the priors' table, and the hierarchical Gaussian with a sampled
// scale (A = 1, H = 4): the matrix-core form at NCH = 1 and NCH = 2, the per-wave form at NCH = 4 and NCH = 8.  Not part of the library.
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"
namespace idhmc {

template <int GROUPS, bool PRIORS>
struct PoissonLocalObs {
    static constexpr int K = 1, A = 0, H = GROUPS;
    static constexpr bool kResponses = false, kPriors = PRIORS, kLocal = true, kFactors = false, kSlopes = false, kCorr = false, kStruct = false, kGmrf = false, kBlock = false, kMulti = false;
    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v)
    {
        const double e = dexp(z);
        v = e - o.y[0] * z;
        r = o.y[0] - e;
    }
};
struct HierGaussLocalObs {
    static constexpr int K = 1, A = 1, H = 4;
    static constexpr bool kResponses = false, kPriors = true, kLocal = true, kFactors = false, kSlopes = false, kCorr = false, kStruct = false, kGmrf = false, kBlock = false, kMulti = false;
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
    template __global__ void k_leapfrog<2, GlmWave<2 IDHMC_COMMA OBS>>(DevState, double, int, int);
using PoissonLocal = PoissonLocalObs<0, false>;
using PoissonLocalGroupPriors = PoissonLocalObs<1, true>;
IDHMC_REHEARSE_OBS(PoissonLocal)
IDHMC_REHEARSE_OBS(PoissonLocalGroupPriors)
IDHMC_REHEARSE_OBS(HierGaussLocalObs)

}  // namespace idhmc
