// idhmc_nuts_sep.inc -- the separable densities' NUTS kernels for NCH in [IDHMC_NUTS_LO, IDHMC_NUTS_HI], included
// by idhmc_nuts_sep{1,2,3,4}.hip (four translation units so that the sixteen padded lengths compile in parallel).
#include "idhmc_nuts_kernel.hpp"

namespace idhmc {

template <int NCH>
static hipError_t launch_nuts_sep_nch(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st)
{
    const bool shared = s.minv_stride == 0;
    if (s.model == IDHMC_MODEL_ISO_GAUSSIAN)
        return shared ? launch_nuts_t<NCH, IsoGaussian<NCH>, true>(s, iter, flags, grid, st)
                      : launch_nuts_t<NCH, IsoGaussian<NCH>, false>(s, iter, flags, grid, st);
    return shared ? launch_nuts_t<NCH, DiagGaussianLds<NCH>, true>(s, iter, flags, grid, st)
                  : launch_nuts_t<NCH, DiagGaussianLds<NCH>, false>(s, iter, flags, grid, st);
}

#define IDHMC_NUTS_SEP_NAME2(lo) launch_nuts_sep_from##lo
#define IDHMC_NUTS_SEP_NAME(lo) IDHMC_NUTS_SEP_NAME2(lo)
hipError_t IDHMC_NUTS_SEP_NAME(IDHMC_NUTS_LO)(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st)
{
    switch (s.nch) {
    case IDHMC_NUTS_LO: return launch_nuts_sep_nch<IDHMC_NUTS_LO>(s, iter, flags, grid, st);
    case IDHMC_NUTS_LO + 1: return launch_nuts_sep_nch<IDHMC_NUTS_LO + 1>(s, iter, flags, grid, st);
    case IDHMC_NUTS_LO + 2: return launch_nuts_sep_nch<IDHMC_NUTS_LO + 2>(s, iter, flags, grid, st);
    case IDHMC_NUTS_LO + 3: return launch_nuts_sep_nch<IDHMC_NUTS_LO + 3>(s, iter, flags, grid, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace idhmc
