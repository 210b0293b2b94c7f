// idhmc_nuts.hip -- ahead-of-time instantiation and launch of the NUTS transition kernel and the separable
// initial-stepsize search (templates in idhmc_nuts_kernel.hpp) for the built-in densities.
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
    return nuts_waves(nch, model == IDHMC_MODEL_ISO_GAUSSIAN || model == IDHMC_MODEL_DIAG_GAUSSIAN,
                      (model == IDHMC_MODEL_DENSE_MVN && dense_coop(nch)) || ((model == IDHMC_MODEL_LOGISTIC_REGRESSION || model == IDHMC_MODEL_GLM) && glm_coop(nch, glm_aux, shared_metric != 0)),
                      shared_metric != 0);
}
// dynamic LDS of a custom density's kernel (the general form; a GLM's: glm_nuts_lds_bytes)
size_t nuts_lds_bytes(int nch, bool shared_metric)
{
    return sizeof(double) * nuts_lds(nch, false, false, 0, shared_metric, nuts_waves(nch, false, false, shared_metric)).total;
}

hipError_t launch_nuts_sep_from1(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_nuts_sep_from5(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_nuts_sep_from9(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_nuts_sep_from13(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_stepsize_search_dense(const DevState &s, hipStream_t st);
hipError_t launch_nuts_jit(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st);
hipError_t launch_stepsize_search_jit(const DevState &s, hipStream_t st);

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
    const bool shared = s.minv_stride == 0;
    if (s.model == IDHMC_MODEL_CUSTOM || s.model == IDHMC_MODEL_GLM) return launch_nuts_jit(s, iter, flags, grid, st);
    if (s.model == IDHMC_MODEL_LOGISTIC_REGRESSION) return launch_nuts_logistic(s, iter, flags, grid, st);
    if (s.model == IDHMC_MODEL_DENSE_MVN) {
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
    if (s.nch <= 4) return launch_nuts_sep_from1(s, iter, flags, grid, st);
    if (s.nch <= 8) return launch_nuts_sep_from5(s, iter, flags, grid, st);
    if (s.nch <= 12) return launch_nuts_sep_from9(s, iter, flags, grid, st);
    return launch_nuts_sep_from13(s, iter, flags, grid, st);
}

hipError_t launch_local_optimum_dense(const DevState &s, double penalty, int iterations, hipStream_t st);
hipError_t launch_local_optimum_jit(const DevState &s, double penalty, int iterations, int grid, hipStream_t st);

// FindLocalOptimum (src/warmup.jl:137-187), idhmc_optimum.hpp
hipError_t launch_local_optimum(const DevState &s, double penalty, int iterations, hipStream_t st)
{
    if (s.model == IDHMC_MODEL_DENSE_MVN) return launch_local_optimum_dense(s, penalty, iterations, st);
    if (s.model == IDHMC_MODEL_CUSTOM || s.model == IDHMC_MODEL_GLM) return launch_local_optimum_jit(s, penalty, iterations, optimum_grid(s), st);
    if (s.model == IDHMC_MODEL_LOGISTIC_REGRESSION) return launch_local_optimum_logistic(s, penalty, iterations, st);
    IDHMC_DISPATCH_NCH(s.nch, {
        if (s.model == IDHMC_MODEL_ISO_GAUSSIAN)
            hipLaunchKernelGGL((k_local_optimum<NCH, IsoGaussian<NCH>>), dim3(optimum_grid(s)), dim3(kOptimumWaves * 64),
                               0, st, s, penalty, iterations);
        else
            hipLaunchKernelGGL((k_local_optimum<NCH, DiagGaussian<NCH>>), dim3(optimum_grid(s)), dim3(kOptimumWaves * 64),
                               0, st, s, penalty, iterations);
    });
    return hipGetLastError();
}

hipError_t launch_stepsize_search(const DevState &s, hipStream_t st)
{
    if (s.model == IDHMC_MODEL_DENSE_MVN) return launch_stepsize_search_dense(s, st);
    if (s.model == IDHMC_MODEL_CUSTOM || s.model == IDHMC_MODEL_GLM) return launch_stepsize_search_jit(s, st);
    if (s.model == IDHMC_MODEL_LOGISTIC_REGRESSION) return launch_stepsize_search_logistic(s, st);
    int64_t b = (s.C + 3) / 4;
    if (b > 4096) b = 4096;
    const int grid = (int)b;
    IDHMC_DISPATCH_NCH(s.nch, {
        if (s.model == IDHMC_MODEL_ISO_GAUSSIAN)
            hipLaunchKernelGGL((k_stepsize_search<NCH, IsoGaussian<NCH>>), dim3(grid), dim3(256), 0, st, s);
        else
            hipLaunchKernelGGL((k_stepsize_search<NCH, DiagGaussian<NCH>>), dim3(grid), dim3(256), 0, st, s);
    });
    return hipGetLastError();
}

}  // namespace idhmc
