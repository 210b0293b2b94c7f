// idhmc_logistic.hip -- Bayesian logistic regression (IDHMC_MODEL_LOGISTIC_REGRESSION, idhmc_glm.hpp with Obs = LogisticObs):
// ahead-of-time instantiation of the general-density kernels (idhmc_general.hpp, idhmc_optimum.hpp) with the per-wave form, and
// of the NUTS transition with the matrix-core form where it applies (L <= 256) and the per-wave form beyond.  A user's GLM
// (IDHMC_MODEL_GLM) instantiates the same templates through hipRTC (idhmc_jit.hip) and takes its shape decisions from here.  The padded length is a power
// of two (L = 128, 256, 512, 1024), as for the dense density.
#include <type_traits>
#include "idhmc_general.hpp"
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"

namespace idhmc {

// one 16-column tile of G per wavefront covers L <= 256
bool glm_coop(int nch) { return nch <= 2; }

// dynamic LDS of a GLM's NUTS kernel: the launch_nuts_t sizing of the form glm_coop picks (the tiles do not depend on the observation)
template <int NCH>
static size_t glm_nuts_lds_t(bool shared)
{
    using M = typename std::conditional<(NCH <= 2), GlmCoop<NCH, LogisticObs>, GlmWave<NCH, LogisticObs>>::type;
    const int waves = nuts_waves(NCH, M::kSeparable, M::kCooperative, shared);
    return sizeof(double) * nuts_lds_doubles(128 * NCH, false, shared, M::kSeparable, coop_lds_doubles<M>(), waves);
}
size_t glm_nuts_lds_bytes(int nch, bool shared)
{
    switch (nch) {
    case 1: return glm_nuts_lds_t<1>(shared);
    case 2: return glm_nuts_lds_t<2>(shared);
    case 4: return glm_nuts_lds_t<4>(shared);
    case 8: return glm_nuts_lds_t<8>(shared);
    default: return 0;
    }
}

hipError_t launch_eval_logistic(const DevState &s, int random_q, hipStream_t st)
{
    IDHMC_DISPATCH_NCH_POW2(s.nch, hipLaunchKernelGGL((k_eval_general<NCH, LogisticRegression<NCH>>), dim3(general_grid(s.C)),
                                                      dim3(kGeneralWaves * 64), 0, st, s, random_q));
    return hipGetLastError();
}
hipError_t launch_leapfrog_logistic(const DevState &s, double eps, int own, int n_steps, hipStream_t st)
{
    IDHMC_DISPATCH_NCH_POW2(s.nch, hipLaunchKernelGGL((k_leapfrog_general<NCH, LogisticRegression<NCH>>), dim3(general_grid(s.C)),
                                                      dim3(kGeneralWaves * 64), 0, st, s, eps, own, n_steps));
    return hipGetLastError();
}
hipError_t launch_stepsize_search_logistic(const DevState &s, hipStream_t st)
{
    IDHMC_DISPATCH_NCH_POW2(s.nch, hipLaunchKernelGGL((k_stepsize_general<NCH, LogisticRegression<NCH>>), dim3(general_grid(s.C)),
                                                      dim3(kGeneralWaves * 64), 0, st, s));
    return hipGetLastError();
}
hipError_t launch_local_optimum_logistic(const DevState &s, double penalty, int iterations, hipStream_t st)
{
    IDHMC_DISPATCH_NCH_POW2(s.nch, hipLaunchKernelGGL((k_local_optimum_general<NCH, LogisticRegression<NCH>>), dim3(optimum_grid(s)),
                                                      dim3(kOptimumWaves * 64), 0, st, s, penalty, iterations));
    return hipGetLastError();
}
hipError_t launch_nuts_logistic(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st)
{
    const bool shared = s.minv_stride == 0;
    IDHMC_DISPATCH_NCH_POW2(s.nch, {
        if constexpr (NCH <= 2) {
            return shared ? launch_nuts_t<NCH, LogisticRegressionCoop<NCH>, true>(s, iter, flags, grid, st)
                          : launch_nuts_t<NCH, LogisticRegressionCoop<NCH>, false>(s, iter, flags, grid, st);
        } else {
            return shared ? launch_nuts_t<NCH, LogisticRegression<NCH>, true>(s, iter, flags, grid, st)
                          : launch_nuts_t<NCH, LogisticRegression<NCH>, false>(s, iter, flags, grid, st);
        }
    });
    return hipErrorInvalidValue;
}

}  // namespace idhmc
