"""What a posterior summary costs next to hauling the draws to the host.  Per shape, milliseconds per transition of
  a      idhmc_mcmc storing the draws in a host array (the path tools/bench_draws.py measures)
  b      idhmc_mcmc storing nothing
  c128   idhmc_mcmc with a summary open, bins = 128, a range set, no host arrays
  c0     the same with bins = 0 (no histogram)
and bytes_per_transition = C D 8, what the reduction reads of one transition.  A build without summaries (an older checkout run for
comparison) prints a and b alone.  One JSON line per shape.  GPU box.

    python tools/bench_summary.py [--shapes 4096x1024,65536x1024,glm] [--only c128,c0]

Shapes CxD are tools/bench_draws.py's diagonal Gaussian; `glm` is tools/bench_glm.py's Poisson regression at its default shape
(D = 100, n = 1000) with 16 384 chains in responses of R = 16."""
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


def gaussian(C, D):
    sig = np.logspace(-1, 1, D)
    mu = np.sin(np.arange(D, dtype=float))
    eng = pkg.Engine(pkg.DiagGaussian(mu, sigma=sig), C, pkg.default_options(metric_mode=pkg.METRIC_SHARED), seed=1)
    eng.set_minv(sig ** 2)
    rng = np.random.default_rng(1)
    q = np.empty((C, D))
    for c0 in range(0, C, 4096):                      # (in slices: the normals of 65 536 x 1024 at once are 0.5 GB of temporaries)
        q[c0:c0 + 4096] = mu + sig * rng.standard_normal((min(4096, C - c0), D))
    eng.set_q(q)
    eng.set_eps(0.25)
    return eng, None


def glm(C=16384, R=16, D=100, n=1000):
    from bench_glm import poisson_problem, responses_model
    X, y, q_map, cov = poisson_problem(n, D, 0)
    eng = pkg.Engine(responses_model(X, y, q_map, C // R, C), C, pkg.default_options(metric_mode=pkg.METRIC_SHARED), seed=1)
    eng.set_q(q_map + np.random.default_rng(1).standard_normal((C, D)) @ np.linalg.cholesky(cov).T)
    eng.set_eps(0.5 * np.sqrt(np.linalg.eigvalsh(cov)[0]))
    return eng, None               # the default groups: the R chains of a response


def timed(eng, N, it, **kw):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.mcmc(N, it, **kw)
    eng.synchronize()
    return (time.perf_counter() - t0) / N * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x1024,65536x1024,glm")
    ap.add_argument("--only", default="", help="of a, b, c128, c0: those rows alone, comma-separated (for a kernel trace)")
    ap.add_argument("--transitions", type=int, default=0, help="per timed call (default: 60, 40 where a draw exceeds 128 MiB, 30 for the GLM)")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        if shape == "glm":
            eng, cpg = glm()
            N = a.transitions or 30
        else:
            C, D = (int(v) for v in shape.split("x"))
            eng, cpg = gaussian(C, D)
            N = a.transitions or (40 if C * D * 8 > (128 << 20) else 60)
        row = dict(shape=shape, chains=eng.C, D=eng.D, transitions=N, bytes_per_transition=eng.C * eng.D * 8,
                   summaries=hasattr(eng, "summary_begin"), fused=list(eng.fused_launch_info()))
        it = 0
        want = lambda k: not a.only or k in a.only.split(",")     # noqa: E731
        Na = min(N, 8) if eng.C * eng.D * 8 > (128 << 20) else N   # the host array of row a: at most 4 GiB
        row["a_transitions"] = Na

        def measure(n, **kw):
            """the call once untimed (the staging buffers grow to the call's block size), then timed"""
            nonlocal it
            eng.mcmc(n, it, **kw)
            ms = timed(eng, n, it + n, **kw)
            it += 2 * n
            return ms
        if want("a"):
            row["a_ms"] = measure(Na, store_draws=True, store_stats=False)
        if want("b"):
            row["b_ms"] = measure(N, store_draws=False, store_stats=False)
        if row["summaries"]:
            for key, bins in (("c128", 128), ("c0", 0)):
                if not want(key):
                    continue
                eng.summary_begin(cpg, bins)
                if bins:
                    eng.mcmc(2, it, store_draws=False, store_stats=False)
                    it += 2
                    eng.summary_set_range()
                row[key + "_ms"] = measure(N, store_draws=False, store_stats=False)
                s = eng.summary()
                row[key + "_checksum"] = float(s.mean.sum())
                row["groups"], row["chains_per_group"] = len(s.n), s.chains_per_group
                if bins:
                    row["binned_per_group"] = int(s.binned[0])
                eng.summary_end()
        eng.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
