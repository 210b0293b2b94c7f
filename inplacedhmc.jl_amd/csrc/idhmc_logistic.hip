// idhmc_logistic.hip -- Bayesian logistic regression (IDHMC_MODEL_LOGISTIC_REGRESSION, idhmc_glm.hpp with Obs = LogisticObs):
// ahead-of-time instantiation of the streaming kernels (idhmc_stream.hpp, idhmc_optimum.hpp) with the per-wave form, and
// of the NUTS transition with the matrix-core form where it applies (L <= 256) and the per-wave form beyond.  A user's GLM
// (IDHMC_MODEL_GLM) instantiates the same templates through hipRTC (idhmc_jit.hip) and takes its shape decisions from here.  The padded length is a power
// of two (L = 128, 256, 512, 1024), as for the dense density.
#include <type_traits>
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"
#include "idhmc_glm.hpp"

namespace idhmc {

// One 16-column tile of G per wavefront covers L <= 256.  Each auxiliary coordinate adds a [16][129] plane (16.5 KB) to the
// workgroup's tiles, and the whole NUTS kernel has a CU's 160 KiB: the combinations that fit are DESIGN section 12's table (a
// per-chain metric keeps M^-1 of 16 chains in LDS, a shared one is read from L2).  Every other shape runs one chain per wavefront.
bool glm_coop(int nch, int aux, bool shared)
{
    if (nch == 1) return aux <= 4;
    if (nch == 2) return aux <= 1 || (aux == 2 && shared);
    return false;
}

// the tiles depend on the observation through its A alone
template <int AUX>
struct GlmShapeObs { static constexpr int K = 1, A = AUX, H = 0; static constexpr bool kResponses = false, kPriors = false, kLocal = false, kFactors = false, kSlopes = false, kCorr = false, kStruct = false, kGmrf = false, kBlock = false, kMulti = false; };
// dynamic LDS of a GLM's NUTS kernel: the launch_nuts_t sizing of the form glm_coop picks
template <int NCH, int AUX>
static size_t glm_nuts_lds_t(bool shared)
{
    const bool coop = glm_coop(NCH, AUX, shared);
    const int tiles = coop ? GlmCoop<NCH, GlmShapeObs<AUX>>::kLdsDoubles : 0;
    return sizeof(double) * nuts_lds(NCH, false, false, tiles, shared, nuts_waves(NCH, false, coop, shared)).total;
}
template <int NCH>
static size_t glm_nuts_lds_a(bool shared, int aux)
{
    switch (aux) {
    case 0: return glm_nuts_lds_t<NCH, 0>(shared);
    case 1: return glm_nuts_lds_t<NCH, 1>(shared);
    case 2: return glm_nuts_lds_t<NCH, 2>(shared);
    case 3: return glm_nuts_lds_t<NCH, 3>(shared);
    case 4: return glm_nuts_lds_t<NCH, 4>(shared);
    default: return 0;
    }
}
size_t glm_nuts_lds_bytes(int nch, bool shared, int aux)
{
    switch (nch) {
    case 1: return glm_nuts_lds_a<1>(shared, aux);
    case 2: return glm_nuts_lds_a<2>(shared, aux);
    case 4: return glm_nuts_lds_a<4>(shared, aux);
    case 8: return glm_nuts_lds_a<8>(shared, aux);
    default: return 0;
    }
}

static hipError_t launch_nuts_logistic(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st)
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
static hipError_t launch_leapfrog_logistic(const DevState &s, double eps, int own, int n_steps, int, int, hipStream_t st)
{
    return launch_leapfrog_t<LogisticRegression>(s, eps, own, n_steps, st);
}
const Backend &logistic_backend()
{
    static const Backend row = {launch_eval_t<LogisticRegression>, launch_leapfrog_logistic,
                                launch_stepsize_search_t<LogisticRegression>, launch_local_optimum_t<LogisticRegression>,
                                launch_nuts_logistic};
    return row;
}

}  // namespace idhmc
