"""User-defined GLM likelihoods (IDHMC_MODEL_GLM): NUTS leapfrog steps/s of a GLM source on the matrix-core
gradient against the same arithmetic as an IDHMC_MODEL_CUSTOM source (one chain per wavefront), and of the logistic likelihood
as a GLM source against the built-in LogisticRegression; plus idhmc_create's wall time per form (a GLM's is mostly the hipRTC
compile).  Fixed eps, several transitions per launch, a shared metric, seeded synthetic data; each pair runs the same
trajectories (checked: same bits), so their step counts agree.  Prints one JSON document.  GPU box only.

The `gaussian` pair (IDHMC_MODEL_GLM_AUX): a linear regression with a sampled log sigma as an auxiliary-parameter
GLM against the same arithmetic as a custom source; its shapes name the columns of X (the chains have one coordinate more).
--aux-cost adds, per shape and chain count, the cost of the auxiliary coordinates: a fixed-sigma Gaussian as a plain GLM (A = 0),
GAUSSIAN_IDENTITY_LOGSIGMA (A = 1) and a four-parameter Gaussian (A = 4) on the same design, each with the form its NUTS kernel
runs (idhmc_glm_form).

    python tools/bench_glm.py [--shapes 100x1000,25x1000] [--chains 16384,65536] [--pairs poisson,logistic,gaussian] [--transitions 5]
                              [--aux-cost] [--metric shared|per_chain]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import inplacedhmc_jl_amd as pkg  # noqa: E402
from bench_logistic import CUSTOM_SRC, PEAK_FP64_MFMA, custom_params, padded  # noqa: E402
from bench_logistic import problem as logistic_problem  # noqa: E402

# the Poisson log-link likelihood as a custom source: bench_logistic's per-wave logistic density with its terms swapped
_LR_TERMS = CUSTOM_SRC[CUSTOM_SRC.index("__device__ void lr_terms"):CUSTOM_SRC.index("template <int NCH>")]
CUSTOM_POISSON_SRC = CUSTOM_SRC.replace(_LR_TERMS, r"""__device__ void lr_terms(double z, double y, double &r, double &v)
{
    const double e = dexp(z);
    v = e - y * z;
    r = y - e;
}
""")


# the Gaussian likelihood with a sampled log sigma (the chain's last coordinate) as a custom source: GAUSSIAN_IDENTITY_LOGSIGMA's
# arithmetic in section 12's order -- z over the D - 1 columns of X, the score summed per residue like v, its tree into the owner lane
CUSTOM_GAUSSIAN_SRC = CUSTOM_SRC.replace(_LR_TERMS, r"""__device__ void lr_terms(double z, double y, double a, double &r, double &v, double &s)
{
    const double w = dexp(-a);
    const double u = (y - z) * w;
    v = 0.5 * (u * u) + a;
    r = u * w;
    s = u * u - 1.0;
}
""").replace("double a0 = 0.0, a1 = 0.0;", "double a0 = 0.0, a1 = 0.0, s0 = 0.0, s1 = 0.0;"
).replace("for (int c = 0; c < D; ++c) {", "for (int c = 0; c < D - 1; ++c) {"
).replace("double rx, vx, ry, vy;", "double rx, vx, ry, vy, ux, uy;\n        const double la = buf[D - 1];"
).replace("lr_terms(zx, yv.x, rx, vx);", "lr_terms(zx, yv.x, la, rx, vx, ux);"
).replace("lr_terms(zy, yv.y, ry, vy);", "lr_terms(zy, yv.y, la, ry, vy, uy);"
).replace("a1 = a1 + vy;", "a1 = a1 + vy;\n        s0 = s0 + (i0 >= n ? 0.0 : ux);\n        s1 = s1 + (i0 + 1 >= n ? 0.0 : uy);"
).replace("    double t0 = 0.0, t1 = 0.0;", r"""    {
        const double S = wave_sum(s0, s1);
        const int c = D - 1;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const bool here = (c >> 7) == j && lane == ((c & 127) >> 1);
            G.c[j].x = here && !(c & 1) ? S : G.c[j].x;
            G.c[j].y = here && (c & 1) ? S : G.c[j].y;
        }
    }
    double t0 = 0.0, t1 = 0.0;""")
assert CUSTOM_GAUSSIAN_SRC.count("la,") == 2 and "s1 = s1 +" in CUSTOM_GAUSSIAN_SRC and "wave_sum(s0, s1)" in CUSTOM_GAUSSIAN_SRC

# a fixed-sigma Gaussian as a plain GLM (constant log sigma), and one with four auxiliary parameters (mean and log scale move with y1)
GAUSSIAN_FIXED_SRC = r"""
__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)
{
    const double w = dexp(-o.c[0]);
    const double u = (o.y[0] - z) * w;
    v = 0.5 * (u * u) + o.c[0];
    r = u * w;
}
"""
GAUSSIAN_A4_SRC = r"""
__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    const double ls = a[0] + a[3] * o.y[1];
    const double w = dexp(-ls);
    const double u = (o.y[0] - z - a[1] * o.y[1] - a[2]) * w;
    v = 0.5 * (u * u) + ls;
    r = u * w;
    s[0] = u * u - 1.0;
    s[1] = r * o.y[1];
    s[2] = r;
    s[3] = s[0] * o.y[1];
}
"""


def gaussian_problem(n, D, seed):
    """y = X beta + sigma eps; the Laplace approximation at the MAP in (beta, log sigma), prior N(0, I)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    y = X @ (rng.standard_normal(D) * 0.5) + 0.7 * rng.standard_normal(n)
    q = np.zeros(D + 1)                               # Newton from the least-squares fit (from 0 its full steps in log sigma overshoot)
    q[:D] = np.linalg.lstsq(X, y, rcond=None)[0]
    q[D] = 0.5 * np.log(np.mean((y - X @ q[:D]) ** 2))
    for _ in range(40):
        w2, e = np.exp(-2.0 * q[D]), y - X @ q[:D]
        g = np.concatenate([w2 * X.T @ e, [w2 * e @ e - n]]) - q
        H = np.zeros((D + 1, D + 1))
        H[:D, :D] = w2 * X.T @ X
        H[:D, D] = H[D, :D] = 2.0 * w2 * X.T @ e
        H[D, D] = 2.0 * w2 * e @ e
        H += np.eye(D + 1)
        q = q + np.linalg.solve(H, g)
    return X, y, q, np.linalg.inv(H)


def poisson_problem(n, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    beta = rng.standard_normal(D) * 0.5
    y = rng.poisson(np.exp(X @ beta)).astype(np.float64)
    q = np.zeros(D)                                   # Laplace approximation at the MAP (prior N(0, I))
    for _ in range(40):
        m = np.exp(X @ q)
        H = (X.T * m) @ X + np.eye(D)
        q = q + np.linalg.solve(H, X.T @ (y - m) - q)
    return X, y, q, np.linalg.inv(H)


def model(form, X, y, q_map=None):
    D = X.shape[1]
    if form == "glm_gaussian":
        return pkg.GLM(X, y, pkg.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1)
    if form == "custom_gaussian":                     # the chain's D + 1 coordinates: a zero column of X in the place of log sigma
        return pkg.CustomDensity(D + 1, CUSTOM_GAUSSIAN_SRC, custom_params(np.c_[X, np.zeros(len(X))], y))
    if form == "glm_gaussian_fixed":
        return pkg.GLM(X, y, GAUSSIAN_FIXED_SRC, constants=[q_map[D]])
    if form == "glm_gaussian_a4":
        return pkg.GLM(X, np.c_[y, np.random.default_rng(5).uniform(-1.0, 1.0, len(y))], GAUSSIAN_A4_SRC, aux=4)
    if form == "glm_poisson":
        return pkg.GLM(X, y, pkg.glm.POISSON_LOG)
    if form == "custom_poisson":
        return pkg.CustomDensity(D, CUSTOM_POISSON_SRC, custom_params(X, y))
    if form == "glm_logistic":
        return pkg.GLM(X, y, pkg.glm.BERNOULLI_LOGIT)
    return pkg.LogisticRegression(X, y)


def run(form, X, y, q_map, cov, C, T, seed=1, metric=None):
    t0 = time.perf_counter()
    eng = pkg.Engine(model(form, X, y, q_map), C, pkg.default_options(metric_mode=pkg.METRIC_SHARED if metric is None else metric, max_depth=10),
                     seed=seed)
    create_s = time.perf_counter() - t0
    Dx = X.shape[1]
    if form == "glm_gaussian_fixed":                  # the coefficients alone
        q_map, cov = q_map[:Dx], cov[:Dx, :Dx]
    elif form == "glm_gaussian_a4":                   # three more coordinates, near 0 and narrow
        q_map = np.r_[q_map, np.zeros(3)]
        big = np.eye(Dx + 4) * 1e-4
        big[:Dx + 1, :Dx + 1] = cov
        cov = big
    D = q_map.size
    rng = np.random.default_rng(seed)
    eng.set_q(q_map + rng.standard_normal((C, D)) @ np.linalg.cholesky(cov).T)
    eps = 0.5 * np.sqrt(np.linalg.eigvalsh(cov)[0])
    eng.set_eps(eps)
    head = (eng.lq[:64].copy(), eng.grad[:64].copy())
    eng.nuts_transitions(1, 2)                        # warm-up (and the module's first launch)
    eng.synchronize()
    s0 = eng.total_steps()
    ms = eng.time_transitions_fused(T, 100)
    steps = eng.total_steps() - s0
    st = eng.tree_stats()
    out = dict(create_s=create_s, ms_per_transition=ms / T, leapfrog_steps_per_s=steps / ms * 1e3, steps=int(steps), eps=float(eps),
               mean_depth=float(st["depth"].mean()), acceptance=float(st["acceptance_rate"].mean()))
    if hasattr(eng, "glm_form"):
        out["glm_form"] = eng.glm_form()
    tail = eng.q[:64].copy()
    eng.close()
    return out, head, tail


PAIRS = {"poisson": ("glm_poisson", "custom_poisson", poisson_problem),
         "logistic": ("glm_logistic", "builtin_logistic", logistic_problem),
         "gaussian": ("glm_gaussian", "custom_gaussian", gaussian_problem)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100x1000,25x1000", help="DxN,...")
    ap.add_argument("--chains", default="16384,65536")
    ap.add_argument("--pairs", default="poisson,logistic")
    ap.add_argument("--transitions", type=int, default=5)
    ap.add_argument("--aux-cost", action="store_true", help="the fixed-sigma, A = 1 and A = 4 Gaussians per shape (DESIGN section 12)")
    ap.add_argument("--metric", default="shared", choices=["shared", "per_chain"])
    a = ap.parse_args()
    metric = pkg.METRIC_SHARED if a.metric == "shared" else pkg.METRIC_PER_CHAIN
    res = dict(device_peak_fp64_mfma_flops=PEAK_FP64_MFMA, transitions_per_launch=a.transitions, results=[])
    for shape in a.shapes.split(","):
        D, n = (int(v) for v in shape.split("x"))
        L, npad = padded(D), (n + 127) // 128 * 128
        flops = 4 * npad * L
        if a.aux_cost:
            X, y, q_map, cov = gaussian_problem(n, D, seed=D * 7919 + n)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair="aux_cost", D=D, n=n, chains=C, metric=a.metric)
                for f in ("glm_gaussian_fixed", "glm_gaussian", "glm_gaussian_a4"):
                    row[f] = run(f, X, y, q_map, cov, C, a.transitions, metric=metric)[0]
                    print("# D=%d n=%d C=%d %s (form %d): %.3e leapfrog steps/s, depth %.2f" %
                          (D, n, C, f, row[f]["glm_form"], row[f]["leapfrog_steps_per_s"], row[f]["mean_depth"]), file=sys.stderr, flush=True)
                res["results"].append(row)
        for pair in [p for p in a.pairs.split(",") if p]:
            fa, fb, prob = PAIRS[pair]
            X, y, q_map, cov = prob(n, D, seed=D * 7919 + n)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair=pair, D=D, n=n, L=L, n_pad=npad, chains=C, fp64_ops_per_gradient=flops)
                seen = {}
                for f in (fa, fb):
                    r, head, tail = run(f, X, y, q_map, cov, C, a.transitions, metric=metric)
                    r["fp64_tflops"] = r["leapfrog_steps_per_s"] * flops / 1e12
                    row[f] = r
                    seen[f] = head + (tail,)
                    print("# D=%d n=%d C=%d %s: %.3e leapfrog steps/s, %.2f ms/transition, depth %.2f, create %.2f s" %
                          (D, n, C, f, r["leapfrog_steps_per_s"], r["ms_per_transition"], r["mean_depth"], r["create_s"]),
                          file=sys.stderr, flush=True)
                row["same_bits"] = bool(all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(seen[fa], seen[fb])))
                row["speedup_%s_over_%s" % (fa, fb)] = row[fa]["leapfrog_steps_per_s"] / row[fb]["leapfrog_steps_per_s"]
                res["results"].append(row)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
