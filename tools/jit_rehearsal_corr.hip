// jit_rehearsal_corr.hip -- tools/jit_rehearsal.hip for DESIGN section 22: the kernels hipRTC builds for a GLM with correlated pairs of
// factor terms (kFactors = true, kSlopes = true, kCorr = true), compiled ahead of time so that they cross-compile for gfx950 without a
// device and tools/kres.py shows their resource figures next to those of tools/jit_rehearsal_slopes.hip:
//     tools/kres.py tools/jit_rehearsal_corr.hip k_ -Iinplacedhmc.jl_amd/csrc
// The same policies as there -- Poisson (A = 0) without a group and with one, with the priors' table (the LKJ row) and local scales, and
// the Gaussian with a sampled scale (A = 1, H = 1): the matrix-core form at NCH = 1 and NCH = 2, the per-wave form at NCH = 4 and
// NCH = 8.  Not part of the library.
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"
namespace idhmc {

template <int GROUPS, bool PRIORS, bool LOCAL>
struct PoissonCorrObs {
    static constexpr int K = 1, A = 0, H = GROUPS;
    static constexpr bool kResponses = false, kPriors = PRIORS, kLocal = LOCAL, kFactors = true, kSlopes = true, kCorr = true, kStruct = false, kGmrf = false, kBlock = false, kMulti = false;
    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v)
    {
        const double e = dexp(z);
        v = e - o.y[0] * z;
        r = o.y[0] - e;
    }
};
struct GaussCorrObs {
    static constexpr int K = 1, A = 1, H = 1;
    static constexpr bool kResponses = false, kPriors = true, kLocal = false, kFactors = true, kSlopes = true, kCorr = true, kStruct = false, kGmrf = false, kBlock = false, kMulti = false;
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
using PoissonCorr = PoissonCorrObs<0, false, false>;
using PoissonCorrGroupLkj = PoissonCorrObs<2, true, false>;
using PoissonCorrGroupLkjLocal = PoissonCorrObs<2, true, true>;
IDHMC_REHEARSE_OBS(PoissonCorr)
IDHMC_REHEARSE_OBS(PoissonCorrGroupLkj)
IDHMC_REHEARSE_OBS(PoissonCorrGroupLkjLocal)
IDHMC_REHEARSE_OBS(GaussCorrObs)

}  // namespace idhmc
