"""User-defined GLM likelihoods (IDHMC_MODEL_GLM): NUTS leapfrog steps/s of a GLM source on the matrix-core
gradient against the same arithmetic as an IDHMC_MODEL_CUSTOM source (one chain per wavefront), and of the logistic likelihood
as a GLM source against the built-in LogisticRegression; plus idhmc_create's wall time per form (a GLM's is mostly the hipRTC
compile).  Fixed eps, several transitions per launch, a shared metric, seeded synthetic data; each pair runs the same
trajectories (checked: same bits), so their step counts agree.  Prints one JSON document.  GPU box only.

    python tools/bench_glm.py [--shapes 100x1000,25x1000] [--chains 16384,65536] [--pairs poisson,logistic] [--transitions 5]
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


def model(form, X, y):
    D = X.shape[1]
    if form == "glm_poisson":
        return pkg.GLM(X, y, pkg.glm.POISSON_LOG)
    if form == "custom_poisson":
        return pkg.CustomDensity(D, CUSTOM_POISSON_SRC, custom_params(X, y))
    if form == "glm_logistic":
        return pkg.GLM(X, y, pkg.glm.BERNOULLI_LOGIT)
    return pkg.LogisticRegression(X, y)


def run(form, X, y, q_map, cov, C, T, seed=1):
    D = X.shape[1]
    t0 = time.perf_counter()
    eng = pkg.Engine(model(form, X, y), C, pkg.default_options(metric_mode=pkg.METRIC_SHARED, max_depth=10), seed=seed)
    create_s = time.perf_counter() - t0
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
    tail = eng.q[:64].copy()
    eng.close()
    return out, head, tail


PAIRS = {"poisson": ("glm_poisson", "custom_poisson", poisson_problem),
         "logistic": ("glm_logistic", "builtin_logistic", logistic_problem)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100x1000,25x1000", help="DxN,...")
    ap.add_argument("--chains", default="16384,65536")
    ap.add_argument("--pairs", default="poisson,logistic")
    ap.add_argument("--transitions", type=int, default=5)
    a = ap.parse_args()
    res = dict(device_peak_fp64_mfma_flops=PEAK_FP64_MFMA, transitions_per_launch=a.transitions, results=[])
    for shape in a.shapes.split(","):
        D, n = (int(v) for v in shape.split("x"))
        L, npad = padded(D), (n + 127) // 128 * 128
        flops = 4 * npad * L
        for pair in a.pairs.split(","):
            fa, fb, prob = PAIRS[pair]
            X, y, q_map, cov = prob(n, D, seed=D * 7919 + n)
            for C in (int(c) for c in a.chains.split(",")):
                row = dict(pair=pair, D=D, n=n, L=L, n_pad=npad, chains=C, fp64_ops_per_gradient=flops)
                seen = {}
                for f in (fa, fb):
                    r, head, tail = run(f, X, y, q_map, cov, C, a.transitions)
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
