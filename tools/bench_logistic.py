"""Bayesian logistic regression: NUTS leapfrog steps/s of the built-in density (IDHMC_MODEL_LOGISTIC_REGRESSION: the matrix-core
gradient at L <= 256) against the same density written as an IDHMC_MODEL_CUSTOM source (one chain per wavefront: what a user can
do without the built-in), on seeded synthetic data.  Fixed eps, several transitions per launch (the drivers' fused form), timed
with HIP events after a warm-up; the two forms run the same trajectories (checked: same bits), so their step counts agree.
Prints one JSON document.  GPU box only.

    python tools/bench_logistic.py [--shapes 100x1000,25x1000] [--chains 16384,65536] [--forms builtin,custom] [--transitions 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import inplacedhmc_jl_amd as pkg  # noqa: E402

PEAK_FP64_MFMA = 78.6e12      # MI355X fp64 matrix peak, FLOP/s

# the density as a user would write it today: per wavefront, the arithmetic of the built-in's per-wave form (idhmc_logistic.hpp).
# params = [n, n_pad | X' (L x n_pad) | X (n_pad x L) | y (n_pad) | mu (L) | tau (L)], zero-padded
CUSTOM_SRC = r"""
__device__ void lr_terms(double z, double y, double &r, double &v)
{
    const double s = y != 0.0 ? -z : z;
    const double e = dexp(-__builtin_fabs(s));
    v = (s > 0.0 ? s : 0.0) + dlog1p(e);
    const double sg = (s >= 0.0 ? 1.0 : e) / (1.0 + e);
    r = y != 0.0 ? sg : -sg;
}
template <int NCH>
__device__ double logdensity_and_gradient(const Vec<NCH> &q, Vec<NCH> &g, const UserCtx &ctx)
{
    constexpr int L = 128 * NCH;
    const int n = (int)ctx.params[0], npad = (int)ctx.params[1], D = ctx.D, lane = ctx.lane;
    const double *xt = ctx.params + 2, *x = xt + (size_t)L * npad, *y = x + (size_t)npad * L, *mu = y + npad, *tau = mu + L;
    double *buf = ctx.lds;
    Vec<NCH> G = vfill<NCH>(0.0);
    double a0 = 0.0, a1 = 0.0;
    double2 *b2 = reinterpret_cast<double2 *>(buf) + lane;
    for (int b = 0; b < npad / 128; ++b) {
#pragma unroll
        for (int j = 0; j < NCH; ++j) b2[j * 64] = q.c[j];
        const double2 *xtp = reinterpret_cast<const double2 *>(xt + 128 * b) + lane;
        double zx = 0.0, zy = 0.0;
#pragma unroll 4
        for (int c = 0; c < D; ++c) {
            const double qc = buf[c];
            const double2 xv = xtp[(size_t)c * (npad / 2)];
            zx = dfma(xv.x, qc, zx);
            zy = dfma(xv.y, qc, zy);
        }
        const double2 yv = reinterpret_cast<const double2 *>(y)[b * 64 + lane];
        const int i0 = 128 * b + 2 * lane;
        double rx, vx, ry, vy;
        lr_terms(zx, yv.x, rx, vx);
        lr_terms(zy, yv.y, ry, vy);
        if (i0 >= n) { rx = 0.0; vx = 0.0; }
        if (i0 + 1 >= n) { ry = 0.0; vy = 0.0; }
        a0 = a0 + vx;
        a1 = a1 + vy;
        b2[0] = make_double2(rx, ry);
        const int m = n - 128 * b < 128 ? n - 128 * b : 128;
        const double2 *xr = reinterpret_cast<const double2 *>(x + (size_t)128 * b * L) + lane;
#pragma unroll 2
        for (int ii = 0; ii < m; ++ii) {
            const double ri = buf[ii];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const double2 xv = xr[(size_t)ii * (L / 2) + j * 64];
                G.c[j].x = dfma(xv.x, ri, G.c[j].x);
                G.c[j].y = dfma(xv.y, ri, G.c[j].y);
            }
        }
    }
    double t0 = 0.0, t1 = 0.0;
    const double2 *m2 = reinterpret_cast<const double2 *>(mu) + lane, *t2 = reinterpret_cast<const double2 *>(tau) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const double2 m = m2[j * 64], t = t2[j * 64];
        const double dx = q.c[j].x - m.x, dy = q.c[j].y - m.y;
        t0 = dfma(t.x * dx, dx, t0);
        t1 = dfma(t.y * dy, dy, t1);
        g.c[j] = make_double2(dfma(-t.x, dx, G.c[j].x), dfma(-t.y, dy, G.c[j].y));
    }
    return -0.5 * wave_sum(dfma(2.0, a0, t0), dfma(2.0, a1, t1));
}
"""


def padded(D):
    L = 128
    while L < D:
        L *= 2
    return L


def custom_params(X, y):
    n, D = X.shape
    L, npad = padded(D), (n + 127) // 128 * 128
    Xp = np.zeros((npad, L))
    Xp[:n, :D] = X
    yp = np.zeros(npad)
    yp[:n] = y
    mu, tau = np.zeros(L), np.zeros(L)
    tau[:D] = 1.0
    return np.concatenate([[float(n), float(npad)], Xp.T.ravel(), Xp.ravel(), yp, mu, tau])


def problem(n, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)) / np.sqrt(D)
    X[:, 0] = 1.0
    beta = rng.standard_normal(D)
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    # Laplace approximation at the MAP (prior N(0, I)): starting points and a step size that suit the posterior
    q = np.zeros(D)
    for _ in range(30):
        s = 1.0 / (1.0 + np.exp(-(X @ q)))
        H = (X.T * (s * (1 - s))) @ X + np.eye(D)
        q = q + np.linalg.solve(H, X.T @ (y - s) - q)
    cov = np.linalg.inv(H)
    return X, y, q, cov


def run(form, X, y, q_map, cov, C, T, seed=1):
    n, D = X.shape
    model = pkg.LogisticRegression(X, y) if form == "builtin" else pkg.CustomDensity(D, CUSTOM_SRC, custom_params(X, y))
    eng = pkg.Engine(model, C, pkg.default_options(metric_mode=pkg.METRIC_SHARED, max_depth=10), seed=seed)
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
    out = dict(ms_per_transition=ms / T, leapfrog_steps_per_s=steps / ms * 1e3, steps=int(steps), eps=float(eps),
               mean_depth=float(st["depth"].mean()), acceptance=float(st["acceptance_rate"].mean()))
    tail = eng.q[:64].copy()
    eng.close()
    return out, head, tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100x1000,25x1000", help="DxN,...")
    ap.add_argument("--chains", default="16384,65536")
    ap.add_argument("--forms", default="builtin,custom")
    ap.add_argument("--transitions", type=int, default=5)
    a = ap.parse_args()
    forms = a.forms.split(",")
    res = dict(device_peak_fp64_mfma_flops=PEAK_FP64_MFMA, transitions_per_launch=a.transitions, results=[])
    for shape in a.shapes.split(","):
        D, n = (int(v) for v in shape.split("x"))
        X, y, q_map, cov = problem(n, D, seed=D * 7919 + n)
        L, npad = padded(D), (n + 127) // 128 * 128
        flops = 4 * npad * L
        for C in (int(c) for c in a.chains.split(",")):
            row = dict(D=D, n=n, L=L, n_pad=npad, chains=C, fp64_ops_per_gradient=flops)
            seen = {}
            for f in forms:
                r, head, tail = run(f, X, y, q_map, cov, C, a.transitions)
                r["fp64_tflops"] = r["leapfrog_steps_per_s"] * flops / 1e12
                r["share_of_fp64_mfma_peak"] = r["leapfrog_steps_per_s"] * flops / PEAK_FP64_MFMA
                row[f] = r
                seen[f] = (head, tail)
                print("# D=%d n=%d C=%d %s: %.3e leapfrog steps/s, %.2f ms/transition, depth %.2f" %
                      (D, n, C, f, r["leapfrog_steps_per_s"], r["ms_per_transition"], r["mean_depth"]), file=sys.stderr, flush=True)
            if "builtin" in seen and "custom" in seen:
                same = all(np.array_equal(u.view(np.uint64), v.view(np.uint64))
                           for u, v in zip(seen["builtin"][0] + (seen["builtin"][1],), seen["custom"][0] + (seen["custom"][1],)))
                row["same_bits"] = bool(same)
                row["speedup_builtin_over_custom"] = row["builtin"]["leapfrog_steps_per_s"] / row["custom"]["leapfrog_steps_per_s"]
            res["results"].append(row)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
