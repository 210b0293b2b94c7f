// jit_rehearsal_gmrf.hip -- tools/jit_rehearsal.hip for DESIGN section 25: the kernels hipRTC builds for a GLM with a Gaussian Markov
// random field prior on a factor term's levels (kFactors = true, kPriors = true, kGmrf = true), compiled ahead of time so that they
// cross-compile for gfx950 without a device and tools/kres.py shows their resource figures next to those of tools/jit_rehearsal_struct.hip:
//     tools/kres.py tools/jit_rehearsal_gmrf.hip k_ -Iinplacedhmc.jl_amd/csrc
// Poisson (A = 0) without a group and with groups, values on the term, and with a pair and a structured term next to the GMRF term
// (kCorr && kStruct && kGmrf), and the Gaussian with a sampled scale (A = 1, H = 1): the matrix-core form at NCH = 1 and NCH = 2, the
// per-wave form at NCH = 4 and NCH = 8.  Not part of the library.
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"
namespace idhmc {

template <int GROUPS, bool LOCAL, bool SLOPES, bool CORR, bool STRUCT>
struct PoissonGmrfObs {
    static constexpr int K = 1, A = 0, H = GROUPS;
    static constexpr bool kResponses = false, kPriors = true, kLocal = LOCAL, kFactors = true, kSlopes = SLOPES, kCorr = CORR, kStruct = STRUCT,
                          kGmrf = true, kBlock = false, kMulti = false;
    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v)
    {
        const double e = dexp(z);
        v = e - o.y[0] * z;
        r = o.y[0] - e;
    }
};
struct GaussGmrfObs {
    static constexpr int K = 1, A = 1, H = 1;
    static constexpr bool kResponses = false, kPriors = true, kLocal = false, kFactors = true, kSlopes = true, kCorr = false, kStruct = false,
                          kGmrf = true, kBlock = false, kMulti = false;
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
using PoissonIcar = PoissonGmrfObs<0, false, false, false, false>;
using PoissonIcarGroup = PoissonGmrfObs<2, false, true, false, false>;
using PoissonGmrfCorrStruct = PoissonGmrfObs<4, true, true, true, true>;
IDHMC_REHEARSE_OBS(PoissonIcar)
IDHMC_REHEARSE_OBS(PoissonIcarGroup)
IDHMC_REHEARSE_OBS(PoissonGmrfCorrStruct)
IDHMC_REHEARSE_OBS(GaussGmrfObs)

}  // namespace idhmc
