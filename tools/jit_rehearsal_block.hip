// jit_rehearsal_block.hip -- tools/jit_rehearsal.hip for DESIGN section 26: the kernels hipRTC builds for a GLM with a correlation block
// of three or four factor terms (kFactors = true, kSlopes = true, kBlock = true), compiled ahead of time so that they cross-compile for
// gfx950 without a device and tools/kres.py shows their resource figures next to those of tools/jit_rehearsal_corr.hip:
//     tools/kres.py tools/jit_rehearsal_block.hip k_ -Iinplacedhmc.jl_amd/csrc
// K is a run-time member of the model (DevState::lr_bk), so one instantiation serves K = 2, 3 and 4.  The policies of
// jit_rehearsal_corr.hip with the block in the pairs' place -- Poisson (A = 0) without a group and with groups, with the priors' table
// (the LKJ row), local scales and a structured term next to the block, and the Gaussian with a sampled scale (A = 1, H = 1): the
// matrix-core form at NCH = 1 and NCH = 2, the per-wave form at NCH = 4 and NCH = 8.  Not part of the library.
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"
namespace idhmc {

template <int GROUPS, bool PRIORS, bool LOCAL, bool STRUCT>
struct PoissonBlockObs {
    static constexpr int K = 1, A = 0, H = GROUPS;
    static constexpr bool kResponses = false, kPriors = PRIORS, kLocal = LOCAL, kFactors = true, kSlopes = true, kCorr = false, kStruct = STRUCT,
                          kGmrf = false, kBlock = true, kMulti = false;
    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v)
    {
        const double e = dexp(z);
        v = e - o.y[0] * z;
        r = o.y[0] - e;
    }
};
struct GaussBlockObs {
    static constexpr int K = 1, A = 1, H = 1;
    static constexpr bool kResponses = false, kPriors = true, kLocal = false, kFactors = true, kSlopes = true, kCorr = false, kStruct = false,
                          kGmrf = false, kBlock = true, kMulti = false;
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
using PoissonBlock = PoissonBlockObs<0, false, false, false>;
using PoissonBlockGroupLkj = PoissonBlockObs<3, true, false, false>;
using PoissonBlockGroupLkjLocal = PoissonBlockObs<3, true, true, false>;
using PoissonBlockGroupLkjStruct = PoissonBlockObs<4, true, false, true>;
IDHMC_REHEARSE_OBS(PoissonBlock)
IDHMC_REHEARSE_OBS(PoissonBlockGroupLkj)
IDHMC_REHEARSE_OBS(PoissonBlockGroupLkjLocal)
IDHMC_REHEARSE_OBS(PoissonBlockGroupLkjStruct)
IDHMC_REHEARSE_OBS(GaussBlockObs)

}  // namespace idhmc
