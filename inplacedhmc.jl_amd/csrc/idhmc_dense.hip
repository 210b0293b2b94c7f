// idhmc_dense.hip -- dense multivariate-normal density (BASELINE.json configs[3]): ahead-of-time
// instantiation of the streaming kernels (idhmc_stream.hpp, idhmc_optimum.hpp) with DenseMvn (per-wave GEMV streaming the
// symmetric precision matrix from L2, idhmc_device.hpp).  The single-step leapfrog goes to the fp64 matrix-core
// kernel (idhmc_dense_mfma.hip) when the shape allows; the NUTS transition is k_nuts<.., DenseMvn, ..> (idhmc_nuts.hip).
#include "idhmc_optimum.hpp"

namespace idhmc {

// mfma: the matrix-core kernel where it covers the shape (L <= 512); 0 (or beyond): the per-wave GEMV kernel
static hipError_t launch_leapfrog_dense(const DevState &s, double eps, int own, int n_steps, int, int mfma, hipStream_t st)
{
    if (mfma) {
        const hipError_t r = launch_leapfrog_dense_mfma(s, eps, own, n_steps, st);
        if (r != hipErrorNotSupported) return r;
    }
    return launch_leapfrog_t<DenseMvn>(s, eps, own, n_steps, st);
}
const Backend &dense_backend()
{
    static const Backend row = {launch_eval_t<DenseMvn>, launch_leapfrog_dense, launch_stepsize_search_t<DenseMvn>,
                                launch_local_optimum_t<DenseMvn>, launch_nuts_dense};
    return row;
}

}  // namespace idhmc
