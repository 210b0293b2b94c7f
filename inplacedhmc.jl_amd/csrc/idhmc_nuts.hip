// idhmc_nuts.hip -- the NUTS transition: its shape decisions, its launcher, and the ahead-of-time instantiation of the dense
// density's kernels (idhmc_nuts_kernel.hpp); the separable densities' initial-stepsize search and optimum stage are instantiated
// here as well, beside the kernels of their size (idhmc_stream.hpp, idhmc_optimum.hpp).
#include "idhmc_nuts_kernel.hpp"
#include "idhmc_optimum.hpp"

namespace idhmc {

// the tree arena also serves as the L-BFGS history of the FindLocalOptimum stage (2 * kLbfgsR vectors)
int arena_vectors(int max_depth, bool separable, int L)
{
    const int n = arena_map(max_depth, separable, L).count();
    return n > 2 * kLbfgsR ? n : 2 * kLbfgsR;
}
// the dense MVN runs the workgroup-cooperative matrix-core gradient (DenseMvnCoop) when one 16-column tile per
// wavefront covers the matrix (L <= 256), the per-wave GEMV (DenseMvn) above that
static bool dense_coop(int nch) { return nch <= 2; }
int nuts_waves_per_block(int nch, int model, int shared_metric, int glm_aux)
{
    return nuts_waves(nch, model_is_separable(model),
                      (model == IDHMC_MODEL_DENSE_MVN && dense_coop(nch)) || ((model == IDHMC_MODEL_LOGISTIC_REGRESSION || model == IDHMC_MODEL_GLM) && glm_coop(nch, glm_aux, shared_metric != 0)),
                      shared_metric != 0);
}
// dynamic LDS of a custom density's kernel (the general form; a GLM's: glm_nuts_lds_bytes)
size_t nuts_lds_bytes(int nch, bool shared_metric)
{
    return sizeof(double) * nuts_lds(nch, false, false, 0, shared_metric, nuts_waves(nch, false, false, shared_metric)).total;
}

hipError_t launch_nuts(const DevState &s0, uint32_t iter, uint32_t flags, hipStream_t st, uint32_t n_iter, double *fz_q, idhmc_tree_stats *fz_st)
{
    if (s0.max_depth < 1 || s0.max_depth > kMaxDepth - 1) return hipErrorInvalidValue;
    if (n_iter < 1 || (uint64_t)s0.C * n_iter >= (1ull << 31)) return hipErrorInvalidValue;
    if (n_iter > 1 && (!s0.iters_done || (flags & IDHMC_T_USE_DIRECTIONS))) return hipErrorInvalidValue;
    DevState s = s0;
    s.n_iter = n_iter;
    s.fz_q = fz_q;
    s.fz_st = fz_st;
    hipError_t e = hipMemsetAsync(s.queue, 0, sizeof(uint32_t) * 16, st);       // 8 range queues, 8 XCD ids (idhmc_nuts_kernel.hpp)
    if (e != hipSuccess) return e;
    if (n_iter > 1) {
        e = hipMemsetAsync(s.iters_done, 0, sizeof(uint32_t) * (size_t)s.C, st);
        if (e != hipSuccess) return e;
    }
    const int W = nuts_waves_per_block(s.nch, s.model, s.minv_stride == 0, s.lr_a);
    int64_t need = (s.C + W - 1) / W;
    const int64_t have = s.nslots / W;
    const int grid = (int)(need < have ? need : have);
    const Backend *b = backend(s.model);
    return b ? b->nuts(s, iter, flags, grid, st) : hipErrorNotSupported;
}
hipError_t launch_nuts_dense(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st)
{
    const bool shared = s.minv_stride == 0;
    IDHMC_DISPATCH_NCH_POW2(s.nch, {
        if constexpr (NCH <= 2)
            return shared ? launch_nuts_t<NCH, DenseMvnCoop<NCH>, true>(s, iter, flags, grid, st)
                          : launch_nuts_t<NCH, DenseMvnCoop<NCH>, false>(s, iter, flags, grid, st);
        else
            return shared ? launch_nuts_t<NCH, DenseMvn<NCH>, true>(s, iter, flags, grid, st)
                          : launch_nuts_t<NCH, DenseMvn<NCH>, false>(s, iter, flags, grid, st);
    });
    return hipErrorInvalidValue;
}
// separable densities: one translation unit per four padded lengths (idhmc_nuts_sep.inc)
hipError_t launch_nuts_separable(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st)
{
    if (s.nch <= 4) return launch_nuts_sep_from1(s, iter, flags, grid, st);
    if (s.nch <= 8) return launch_nuts_sep_from5(s, iter, flags, grid, st);
    if (s.nch <= 12) return launch_nuts_sep_from9(s, iter, flags, grid, st);
    return launch_nuts_sep_from13(s, iter, flags, grid, st);
}

// the rest of the separable row (idhmc_kernels.hip)
hipError_t launch_stepsize_search_separable(const DevState &s, hipStream_t st)
{
    return IDHMC_SEPARABLE(launch_stepsize_search_t, s, st);
}
hipError_t launch_local_optimum_separable(const DevState &s, double penalty, int iterations, hipStream_t st)
{
    return IDHMC_SEPARABLE(launch_local_optimum_t, s, penalty, iterations, st);
}

}  // namespace idhmc
