// jit_rehearsal_priors.hip -- tools/jit_rehearsal.hip for DESIGN section 18: the NUTS kernels hipRTC builds for a GLM, compiled ahead of
// time once with Gaussian priors (kPriors = false: the parent's kernels) and once with the priors' table in the last loop (kPriors =
// true), so that tools/kres.py shows both sets of resource figures side by side:
//     tools/kres.py tools/jit_rehearsal_priors.hip k_nuts -Iinplacedhmc.jl_amd/csrc
// Poisson (A = 0, H = 0) and the hierarchical Gaussian with a sampled scale (A = 1, H = 4), per-chain and shared metric: the
// matrix-core form at NCH = 1 and NCH = 2, the per-wave form at NCH = 4.  Not part of the library.
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"
namespace idhmc {

template <bool PRIORS>
struct PoissonObs {
    static constexpr int K = 1, A = 0, H = 0;
    static constexpr bool kResponses = false, kPriors = PRIORS, kLocal = false, kFactors = false, kSlopes = false, kCorr = false, kStruct = false, kGmrf = false, kBlock = false, kMulti = false;
    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v)
    {
        const double e = dexp(z);
        v = e - o.y[0] * z;
        r = o.y[0] - e;
    }
};
template <bool PRIORS>
struct HierGaussObs {
    static constexpr int K = 1, A = 1, H = 4;
    static constexpr bool kResponses = false, kPriors = PRIORS, kLocal = false, kFactors = false, kSlopes = false, kCorr = false, kStruct = false, kGmrf = false, kBlock = false, kMulti = false;
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
    template __global__ void k_leapfrog<2, GlmWave<2 IDHMC_COMMA OBS>>(DevState, double, int, int);
IDHMC_REHEARSE_OBS(PoissonObs<false>)
IDHMC_REHEARSE_OBS(PoissonObs<true>)
IDHMC_REHEARSE_OBS(HierGaussObs<false>)
IDHMC_REHEARSE_OBS(HierGaussObs<true>)

}  // namespace idhmc
