// idhmc_jit.hip -- user-supplied densities (IDHMC_MODEL_CUSTOM): the user's HIP source is compiled with hipRTC
// against the engine's own kernel templates (idhmc_stream.hpp, idhmc_optimum.hpp, idhmc_nuts_kernel.hpp), so a custom density
// runs through exactly the code paths of the built-in general density (dense MVN): evaluation, fused
// leapfrog, initial-stepsize search and the NUTS transition.  This is the device form of the reference's
// downward boundary, logdensity_and_gradient!(grad, model, q, sptr) (src/kinetic_energy.jl:73).
// A user's GLM (IDHMC_MODEL_GLM) is compiled the same way: its glm_observation becomes the observation policy of the
// logistic regression's templates (idhmc_glm.hpp), the matrix-core form in the NUTS kernel where glm_coop says so; with auxiliary
// coordinates (IDHMC_MODEL_GLM_AUX) their number A is a compile-time constant of the policy, like K, and so is the number H of
// coefficient groups (idhmc_create_glm), and so is whether the chains sample several responses (idhmc_create_glm_responses with M > 1:
// kResponses), and so is whether some coordinate's prior is not Gaussian (idhmc_create_glm_priors: kPriors, DESIGN
// section 18), and so is whether some column has a local scale (idhmc_create_glm_local: kLocal), and so is whether
// the model has factor terms (idhmc_create_glm_factors with F > 0: kFactors), and so is whether some term carries a
// value per observation (idhmc_create_glm_slopes with a flag set: kSlopes), and so is whether two terms are paired with
// a sampled correlation (idhmc_create_glm_corr with P > 0: kCorr), and so is whether a term's levels form an AR(1) or
// random-walk sequence (idhmc_create_glm_struct with S > 0: kStruct), and so is whether a term's levels carry a sparse
// precision (idhmc_create_glm_gmrf with G > 0: kGmrf), and so is whether three or four terms form a correlation block
// (idhmc_create_glm_block with K > 0: kBlock; never together with kCorr), and so is whether a term has several
// weighted levels per observation (idhmc_create_glm_multi with a width > 1 or an absent entry: kMulti).
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "idhmc_internal.hpp"

namespace idhmc {

struct JitModule {
    hipModule_t mod = nullptr;
    hipFunction_t f_eval = nullptr, f_leapfrog = nullptr, f_stepsize = nullptr, f_nuts = nullptr, f_optimum = nullptr;
    size_t nuts_lds = 0;
};

static std::string library_dir()
{
    if (const char *e = getenv("IDHMC_SRC_DIR")) return e;
    Dl_info info;
    if (dladdr(reinterpret_cast<const void *>(&library_dir), &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        const size_t k = p.find_last_of('/');
        return k == std::string::npos ? "." : p.substr(0, k);
    }
    return ".";
}

static void put_log(char *log, size_t cap, const std::string &s)
{
    if (!log || !cap) return;
    const size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
    memcpy(log, s.data(), n);
    log[n] = 0;
}

int jit_build(const DevState &s, const char *source, JitModule **out, char *log, size_t log_cap, int glm_k, int glm_a, int glm_h)
{
    *out = nullptr;
    const std::string dir = library_dir();
    const bool shared = s.minv_stride == 0;
    const bool glm = s.model == IDHMC_MODEL_GLM;
    std::string src;
    if (!glm) {
        src = "#define IDHMC_JIT_USER_DENSITY 1\n#include \"idhmc_nuts_kernel.hpp\"\n#include \"idhmc_optimum.hpp\"\n"
              "namespace idhmc {\n#line 1 \"user_density.hip\"\n";
        src += source;
        src += "\n}\n";
    } else {
        // the user's glm_observation as the observation policy of idhmc_glm.hpp, K data columns
        src = "#include \"idhmc_nuts_kernel.hpp\"\n#include \"idhmc_optimum.hpp\"\n#include \"idhmc_glm.hpp\"\n"
              "namespace idhmc {\n#line 1 \"user_glm.hip\"\n";
        src += source;
        src += "\n#line 1 \"idhmc_glm_policy\"\nstruct UserGlmObs {\n    static constexpr int K = " + std::to_string(glm_k) +
               ", A = " + std::to_string(glm_a) + ", H = " + std::to_string(glm_h) + ";\n"
               "    static constexpr bool kResponses = " + (s.lr_m > 1 ? "true" : "false") + ", kPriors = " + (s.lr_pkind ? "true" : "false") +
               ", kLocal = " + (s.lr_lpart ? "true" : "false") + ", kFactors = " + (s.lr_f > 0 ? "true" : "false") +
               ", kSlopes = " + (s.lr_fval ? "true" : "false") + ", kCorr = " + (s.lr_cp > 0 ? "true" : "false") +
               ", kStruct = " + (s.lr_s > 0 ? "true" : "false") + ", kGmrf = " + (s.lr_g > 0 ? "true" : "false") +
               ", kBlock = " + (s.lr_bk > 0 ? "true" : "false") + ", kMulti = " + (s.lr_mp > 0 ? "true" : "false") + ";\n";
        // with auxiliary coordinates the observation also takes a (A of them) and returns the scores s
        src += glm_a > 0 ? "    IDHMC_DEV static void terms(double z, const GlmObs &o, const double *a, double &r, double &v, double *s) "
                           "{ glm_observation(z, o, a, r, v, s); }\n};\n}\n"
                         : "    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v) { glm_observation(z, o, r, v); }\n};\n}\n";
    }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), glm ? "idhmc_user_glm.hip" : "idhmc_custom_density.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        put_log(log, log_cap, "hiprtcCreateProgram failed");
        return 1;
    }
    const std::string n = std::to_string(s.nch);
    const std::string model = glm ? "idhmc::GlmWave<" + n + ", idhmc::UserGlmObs>" : "idhmc::JitModel<" + n + ">";
    const std::string nuts_model = glm && glm_coop(s.nch, glm_a, shared) ? "idhmc::GlmCoop<" + n + ", idhmc::UserGlmObs>" : model;
    constexpr int kKernels = 5;
    const std::string names[kKernels] = {"idhmc::k_eval<" + n + ", " + model + ">",
                                  "idhmc::k_leapfrog<" + n + ", " + model + ">",
                                  "idhmc::k_stepsize_search<" + n + ", " + model + ">",
                                  "idhmc::k_nuts<" + n + ", " + nuts_model + ", " + (shared ? "true" : "false") + ">",
                                  "idhmc::k_local_optimum<" + n + ", " + model + ">"};
    for (const std::string &nm : names) hiprtcAddNameExpression(prog, nm.c_str());

    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::string arch = "gfx950";
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.gcnArchName[0]) {
        arch = prop.gcnArchName;
        const size_t colon = arch.find(':');
        if (colon != std::string::npos) arch = arch.substr(0, colon);
    }
    const std::string o_arch = "--offload-arch=" + arch;
    const std::string o_inc1 = "-I" + dir + "/csrc";
    const std::string o_inc2 = "-I" + dir + "/../include";
    std::vector<const char *> opts = {o_arch.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", o_inc1.c_str(), o_inc2.c_str()};
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string clog(ls, 0);
    if (ls) hiprtcGetProgramLog(prog, &clog[0]);
    if (rc != HIPRTC_SUCCESS) {
        put_log(log, log_cap, std::string("hipRTC: ") + hiprtcGetErrorString(rc) + "\n" + clog);
        hiprtcDestroyProgram(&prog);
        return 2;
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    std::vector<char> code(cs);
    hiprtcGetCode(prog, code.data());
    JitModule *m = new JitModule();
    if (hipModuleLoadData(&m->mod, code.data()) != hipSuccess) {
        put_log(log, log_cap, "hipModuleLoadData failed for the compiled density");
        hiprtcDestroyProgram(&prog);
        delete m;
        return 3;
    }
    hipFunction_t *fs[kKernels] = {&m->f_eval, &m->f_leapfrog, &m->f_stepsize, &m->f_nuts, &m->f_optimum};
    for (int i = 0; i < kKernels; ++i) {
        const char *lowered = nullptr;
        if (hiprtcGetLoweredName(prog, names[i].c_str(), &lowered) != HIPRTC_SUCCESS ||
            hipModuleGetFunction(fs[i], m->mod, lowered) != hipSuccess) {
            put_log(log, log_cap, "kernel " + names[i] + " not found in the compiled module");
            hiprtcDestroyProgram(&prog);
            (void)hipModuleUnload(m->mod);
            delete m;
            return 4;
        }
    }
    hiprtcDestroyProgram(&prog);
    // a GLM's NUTS kernel may be the cooperative form: its tiles are sized by the density (kLdsDoubles), not by the general rule
    m->nuts_lds = glm ? glm_nuts_lds_bytes(s.nch, shared, glm_a) : nuts_lds_bytes(s.nch, shared);
    // glm_coop's table keeps the cooperative form inside a CU's LDS; a kernel whose static part outgrew it is refused here, not at its launch
    int static_lds = 0;
    if (glm && hipFuncGetAttribute(&static_lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, m->f_nuts) == hipSuccess &&
        m->nuts_lds + (size_t)static_lds > (size_t)kLdsBytes) {
        put_log(log, log_cap, "the NUTS kernel needs " + std::to_string(m->nuts_lds + (size_t)static_lds) + " bytes of LDS, a CU has 163840");
        (void)hipModuleUnload(m->mod);
        delete m;
        return 5;
    }
    if (m->nuts_lds > 48 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(m->f_nuts), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)m->nuts_lds) != hipSuccess) {
            (void)hipGetLastError();   // some runtimes accept large dynamic LDS for module kernels without the attribute
        }
    }
    *out = m;
    return 0;
}

void jit_destroy(JitModule *m)
{
    if (!m) return;
    if (m->mod) (void)hipModuleUnload(m->mod);
    delete m;
}

template <class Args>
static hipError_t launch_packed(hipFunction_t f, int grid, int block, size_t lds, hipStream_t st, Args &a)
{
    size_t sz = sizeof(Args);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(f, (unsigned)grid, 1, 1, (unsigned)block, 1, 1, (unsigned)lds, st, nullptr, extra);
}

static hipError_t launch_eval_jit(const DevState &s, int random_q, hipStream_t st)
{
    const JitModule *m = static_cast<const JitModule *>(s.jit);
    if (!m) return hipErrorInvalidValue;
    struct { DevState s; int r; } a{s, random_q};
    return launch_packed(m->f_eval, stream_grid(s.C, kGeneralBlocks), kStreamWaves * 64, 0, st, a);
}
static hipError_t launch_leapfrog_jit(const DevState &s, double eps, int own, int n_steps, int, int, hipStream_t st)
{
    const JitModule *m = static_cast<const JitModule *>(s.jit);
    if (!m) return hipErrorInvalidValue;
    struct { DevState s; double eps; int own; int n; } a{s, eps, own, n_steps};
    return launch_packed(m->f_leapfrog, stream_grid(s.C, kGeneralBlocks), kStreamWaves * 64, 0, st, a);
}
static hipError_t launch_stepsize_search_jit(const DevState &s, hipStream_t st)
{
    const JitModule *m = static_cast<const JitModule *>(s.jit);
    if (!m) return hipErrorInvalidValue;
    struct { DevState s; } a{s};
    return launch_packed(m->f_stepsize, stream_grid(s.C, kGeneralBlocks), kStreamWaves * 64, 0, st, a);
}
static hipError_t launch_local_optimum_jit(const DevState &s, double penalty, int iterations, hipStream_t st)
{
    const JitModule *m = static_cast<const JitModule *>(s.jit);
    if (!m) return hipErrorInvalidValue;
    struct { DevState s; double penalty; int iterations; } a{s, penalty, iterations};
    return launch_packed(m->f_optimum, optimum_grid(s), kStreamWaves * 64, 0, st, a);
}
static hipError_t launch_nuts_jit(const DevState &s, uint32_t iter, uint32_t flags, int grid, hipStream_t st)
{
    const JitModule *m = static_cast<const JitModule *>(s.jit);
    if (!m) return hipErrorInvalidValue;
    struct { DevState s; uint32_t iter; uint32_t flags; } a{s, iter, flags};
    return launch_packed(m->f_nuts, grid, nuts_waves_per_block(s.nch, s.model, s.minv_stride == 0, s.lr_a) * 64, m->nuts_lds, st, a);
}
const Backend &jit_backend()
{
    static const Backend row = {launch_eval_jit, launch_leapfrog_jit, launch_stepsize_search_jit, launch_local_optimum_jit,
                                launch_nuts_jit};
    return row;
}

}  // namespace idhmc
