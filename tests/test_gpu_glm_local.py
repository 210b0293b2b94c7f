"""Per-coefficient local scales (GLM(..., local=, slab_scale=), idhmc_create_glm_local) on the device.  Models with a
sampled local scale per flagged column, with and without a slab, are bit-identical to the CPU oracle running the C restatement of
section 19 (tests/test_glm_local_cpu.py, through oracle.OracleModel.custom) and within 1e-12 of numpy, in both device forms: one chain
per wavefront (evaluation, leapfrog; NUTS at L = 512) and the matrix-core gradient of the NUTS kernel.  No tolerance on the device
side.  Then: several responses, the model without a flagged column, idhmc_glm_form's table, a warm-up, exact stationarity on a model
whose posterior is its prior, and the device summaries of [beta | a | sigma | exp lambda].  Every context compiles its source with
hipRTC, so engines are shared across assertions."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import special, stats

import stationarity as S
import test_glm_hier_cpu as HIER
from test_glm_hier_cpu import SHAPE, consts
from test_glm_local_cpu import c_source_local, local_priors, make, numpy_density_local, oracle_params_local, start_local
from test_glm_priors_cpu import LOG_HALF_STUDENT_T, NORMAL
from test_gpu_summary import assert_histogram, assert_summary
from test_summary_cpu import range_twin, summary_twin, theta_twin

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def none(Dx):
    return np.full(Dx, -1, np.int32)


def flagged(Dx, rule):
    return np.array([1 if rule(c) else 0 for c in range(Dx)], np.int32)


# name: (family, Dx, grp, local, slab, D, padded length, matrix cores)
SHAPES = {
    "odd offset": ("GAUSSIAN_IDENTITY_LOGSIGMA", 40, HIER.blocks(40, 2, 10), flagged(40, lambda c: c % 3 != 0), 2.5, 69, 128, 1),
    "D = 128": ("POISSON_LOG", 63, HIER.interleaved(63, 2), flagged(63, lambda c: True), None, 128, 128, 1),
    "same lane": ("POISSON_LOG", 124, HIER.interleaved(124, 4), flagged(124, lambda c: c < 100), 1.0, 228, 256, 1),
    "straddle": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, HIER.interleaved(100, 1), flagged(100, lambda c: c % 5 < 3), None, 162, 256, 1),
    "L = 512": ("GAUSSIAN_IDENTITY_LOGSIGMA", 200, HIER.interleaved(200, 4), flagged(200, lambda c: True), 3.0, 405, 512, 0),
    "one": ("POISSON_LOG", 5, none(5), flagged(5, lambda c: c == 3), 2.0, 6, 128, 1),
}


def dims(family, grp, local):
    return SHAPE[family][2], int(grp.max()) + 1, int(local.sum())


def setup(idhmc, oracle, tmp_path, family, X, Y, grp, local, slab, kind, nu, mu, tau, C, seed, opt=None, oopt=None, **kw):
    A, H, J = dims(family, grp, local)
    D = X.shape[1] + A + H + J
    eng = idhmc.Engine(make(idhmc, family, X, Y, grp, local, slab, kind, nu, mu, tau, **kw), C, opt, seed=seed)
    om = oracle.OracleModel.custom(D, c_source_local(family), oracle_params_local(X, Y, A, grp, local, slab, kind, nu, consts(family), mu, tau),
                                   str(tmp_path))
    chains = [oracle.OracleChain(om, oopt, seed=seed, chain_id=c) for c in range(C)]
    return eng, om, chains


def check_density(eng, chains, family, X, Y, grp, local, slab, kind, nu, mu, tau, D, ends):
    q, g, lq = eng.q, eng.grad, eng.lq
    assert same_bits(lq, [c.lq for c in chains]) and same_bits(g, np.stack([c.grad[:D] for c in chains]))
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_local(family, X, Y, q[c], grp, local, slab, kind, nu, mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


def test_the_shapes_are_what_they_are_there_for():
    lane = lambda c: ((c & 127) >> 1, c >> 7, c & 1)
    for name, (family, Dx, grp, local, slab, D, L, form) in SHAPES.items():
        A, H, J = dims(family, grp, local)
        assert Dx + A + H + J == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))), name
    family, Dx, grp, local, *_ = SHAPES["odd offset"]
    cols = np.flatnonzero(local)
    assert {(int(grp[c] >= 0), int(local[c])) for c in range(Dx)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(lane(c)[0] != lane(43 + k)[0] for k, c in enumerate(cols)) and any(lane(c)[2] != lane(43 + k)[2] for k, c in enumerate(cols))
    assert lane(127) == (63, 0, 1)                       # "D = 128": the last lambda is the last lane's second component
    assert all(lane(c)[0::2] == lane(128 + c)[0::2] and lane(128 + c)[1] == 1 for c in range(100))      # "same lane"
    lam0 = 100 + 1 + 1
    assert lam0 < 128 <= lam0 + 59                       # "straddle"


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1, 130])
def test_density_leapfrog_and_nuts(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: single
    launches, then two in one launch) in the form the shape runs: bit-identical to the oracle, within 1e-12 of numpy"""
    family, Dx, grp, local, slab, D, L, form = SHAPES[shape]
    A, H, J = dims(family, grp, local)
    C_ = 18
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    X, Y = HIER.problem_hier(family, n, Dx, grp, False, seed=n + Dx)
    eng, om, chains = setup(idhmc, oracle, tmp_path, family, X, Y, grp, local, slab, kind, nu, mu, tau, C_, 3, idhmc.default_options(max_depth=4),
                            oracle.default_options(max_depth=4))
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D
    got_local, got_slab = eng.glm_local()
    assert got_local.dtype == np.int32 and np.array_equal(got_local, local) and got_slab == (slab or 0.0)
    assert np.array_equal(eng.glm_priors()[0], kind)
    q = start_local(family, C_, Dx, H, J)
    eng.set_q(q)
    for c, ch in enumerate(chains):
        ch.set_q(q[c])
    ends = (0, C_ - 1)
    args = (family, X, Y, grp, local, slab, kind, nu, mu, tau, D, ends)
    check_density(eng, chains, *args)
    eng.refresh_momentum(1)
    eng.leapfrog(0.01, 1)
    for ch in chains:
        ch.rand_p(1)
        ch.leapfrog(0.01)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains])) and same_bits(eng.p, np.stack([c.p[:D] for c in chains]))
    check_density(eng, chains, *args)
    eps = 0.02
    eng.set_eps(eps)
    for it in (1, 2):
        eng.nuts_transition(it)
        st = eng.tree_stats()
        ost = [ch.sample_tree(eps, it) for ch in chains]
        for f in ("depth", "steps", "term_left", "term_right"):
            np.testing.assert_array_equal(st[f], [getattr(s, f) for s in ost], err_msg="%s @%d" % (f, it))
        assert same_bits(st["pi"], [s.pi for s in ost]) and same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        check_density(eng, chains, *args)
    eng.nuts_transitions(3, 2)
    for it in (3, 4):
        for ch in chains:
            ch.sample_tree(eps, it)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    check_density(eng, chains, *args)
    assert eng.poll_abort() == 0
    eng.close()


def test_responses_are_single_response_oracle_chains(idhmc, oracle, tmp_path):
    """M = 6 responses of R = 3 chains on the "odd offset" shape: every chain is bit-identical to the single-response oracle chain on its Y
    (the same global chain id)"""
    family, Dx, grp, local, slab, D, L, form = SHAPES["odd offset"]
    A, H, J = dims(family, grp, local)
    M, R, n = 6, 3, 37
    X, Y0 = HIER.problem_hier(family, n, Dx, grp, False, seed=5)
    rng = np.random.default_rng(6)
    Y = Y0[None, :, None] + 0.4 * rng.standard_normal((M, n, 1))
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(make(idhmc, family, X, Y, grp, local, slab, kind, nu, mu, tau, chains_per_response=R), M * R, opt, seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form and eng.glm_local()[1] == slab
    q = start_local(family, M * R, Dx, H, J)
    eng.set_q(q)
    eps = 0.02
    eng.set_eps(eps)
    eng.nuts_transition(1)
    q1 = eng.q
    eng.nuts_transitions(2, 2)
    q3, lq3, g3 = eng.q, eng.lq, eng.grad
    assert eng.poll_abort() == 0
    eng.close()
    for m in range(M):
        om = oracle.OracleModel.custom(D, c_source_local(family),
                                       oracle_params_local(X, Y[m], A, grp, local, slab, kind, nu, consts(family), mu, tau), str(tmp_path))
        for c in range(R * m, R * m + R):
            ch = oracle.OracleChain(om, oopt, seed=13, chain_id=c)
            ch.set_q(q[c])
            ch.sample_tree(eps, 1)
            assert same_bits(q1[c], ch.q[:D]), c
            ch.sample_tree(eps, 2)
            ch.sample_tree(eps, 3)
            assert same_bits(q3[c], ch.q[:D]) and same_bits(lq3[c], ch.lq) and same_bits(g3[c], ch.grad[:D]), c


def test_no_flagged_column_is_the_model_without_the_keyword(idhmc):
    """local = zeros through the new keyword gives the bits of the model without it after a short warm-up plus 10 draws, packed (no groups)
    and through the descriptor (groups); glm_local() returns zeros"""
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    n, Dx, C_ = 50, 25, 6
    for family, grp in (("POISSON_LOG", None), ("GAUSSIAN_IDENTITY_LOGSIGMA", HIER.blocks(25, 2, 8))):
        A, H = SHAPE[family][2], 0 if grp is None else 2
        D = Dx + A + H
        X, Y = HIER.problem_hier(family, n, Dx, none(Dx) if grp is None else grp, grp is not None, seed=9)
        mu, tau = np.full(D, 0.1), np.full(D, 0.7)
        out = []
        for kw in ({}, {"local": np.zeros(Dx)}):
            eng = idhmc.Engine(idhmc.GLM(X, Y, getattr(idhmc.glm, family), None, mu, tau, aux=A, groups=grp, **kw), C_,
                               idhmc.default_options(**short), seed=77)
            loc, slab = eng.glm_local()
            assert loc.shape == (Dx,) and not loc.any() and slab == 0.0
            draws, stats_ = eng.mcmc_with_warmup(10)
            out.append((draws, stats_, eng.eps, eng.minv, eng.glm_form(), eng.device_bytes()))
            assert eng.poll_abort() == 0
            eng.close()
        a, b = out
        assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and a[4:] == b[4:]


def _form_source(A):
    """a Gaussian with known scale (A = 0), or with log sigma = a[0] whose further auxiliary coordinates see only their prior"""
    if A == 0:
        return "__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)\n{\n    r = o.y[0] - z;\n    v = 0.5 * (r * r);\n}\n"
    return ("__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)\n{\n"
            "    const double w = dexp(-a[0]);\n    const double u = (o.y[0] - z) * w;\n    v = 0.5 * (u * u) + a[0];\n    r = u * w;\n"
            "    s[0] = u * u - 1.0;\n" + "".join("    s[%d] = 0.0;\n" % j for j in range(1, A)) + "}\n")


# (columns with local scales: Dx = J, the same L without them: Dx, L, A, shared metric)
FORM_ROWS = [(15, 30, 128, 4, False), (100, 200, 256, 1, False), (100, 200, 256, 2, True), (100, 200, 256, 2, False), (150, 300, 512, 0, False)]


@pytest.mark.parametrize("Dl,Dx,L,A,shared", FORM_ROWS, ids=["L%d-A%d-%s" % (r[2], r[3], "shared" if r[4] else "perchain") for r in FORM_ROWS])
def test_local_scales_move_no_row_of_the_table(idhmc, Dl, Dx, L, A, shared):
    """idhmc_glm_form of a model with Dl columns, all with a local scale and a slab (L counts the lambdas), is that of the model with
    Dx = 2 Dl columns and none, at the rows where an LDS byte more would move it, and the kernel launches (no LDS is added)"""
    rng = np.random.default_rng(0)
    opt = idhmc.default_options(max_depth=3, metric_mode=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    forms = []
    for cols, kw in ((Dx, {}), (Dl, {"local": True, "slab_scale": 2.0})):
        X, Y = rng.standard_normal((40, cols)) * 0.3, rng.standard_normal(40)
        eng = idhmc.Engine(idhmc.GLM(X, Y, _form_source(A), aux=A, **kw), 20, opt, seed=2)
        assert eng.padded_dim() == L and eng.D == Dx + A
        forms.append(eng.glm_form())
        eng.set_q(rng.uniform(-0.1, 0.1, (20, Dx + A)))
        eng.set_eps(0.01)
        eng.nuts_transition(1)
        assert np.isfinite(eng.lq).all() and (eng.tree_stats()["steps"] >= 1).all() and eng.poll_abort() == 0
        eng.close()
    assert forms[0] == forms[1] == (1 if L == 128 or (L == 256 and (A <= 1 or shared)) else 0)


def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path):
    """per-chain adaptation on 8 chains, the stage lengths of the other GLM warm-up tests"""
    family, Dx, n, C_, N = "GAUSSIAN_IDENTITY_LOGSIGMA", 25, 200, 8, 8
    grp, local, slab = HIER.blocks(Dx, 2, 8), flagged(Dx, lambda c: c % 3 != 0), 2.0
    A, H, J = dims(family, grp, local)
    D = Dx + A + H + J
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    X, Y = HIER.problem_hier(family, n, Dx, grp, True, seed=9)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    eng = idhmc.Engine(make(idhmc, family, X, Y, grp, local, slab, kind, nu, mu, tau), C_, idhmc.default_options(**short), seed=77)
    draws, stats_ = eng.mcmc_with_warmup(N)
    om = oracle.OracleModel.custom(D, c_source_local(family), oracle_params_local(X, Y, A, grp, local, slab, kind, nu, consts(family), mu, tau),
                                   str(tmp_path))
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, C_, oracle.default_options(**short), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps)
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats_.T, ost[:, :N])
    assert eng.poll_abort() == 0
    eng.close()


# ---- exact stationarity: X = 0, so the posterior is the prior and its coordinates are independent -------------------------------------
@pytest.mark.parametrize("Dx,form,eps", [(30, 1, 0.25), (150, 0, 0.12)], ids=["L128-matrix-cores", "L512-per-wave"])
def test_nuts_leaves_the_prior_exact(idhmc, Dx, form, eps):
    """4096 chains start at exact draws from the prior -- u ~ N, half-t(4) group scales, half-Cauchy local scales on every column, a slab --
    and make 8 transitions at a fixed stepsize: u = F(q) per coordinate stays uniform (tests/stationarity.py, its FWER); the lambdas
    judged against the Gaussian of the same location are rejected"""
    C_, H, J = 4096, 2, Dx
    D = Dx + H + J
    grp = HIER.interleaved(Dx, H)
    rng = np.random.default_rng(17)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[Dx:], nu[Dx:Dx + H], nu[Dx + H:] = LOG_HALF_STUDENT_T, 4.0, 1.0
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx:] = 1.0
    X, Y = np.zeros((1, Dx)), np.array([2.0])
    eng = idhmc.Engine(idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, None, mu, tau, groups=grp, prior_kind=kind, prior_nu=nu, local=True, slab_scale=2.0),
                       C_, idhmc.default_options(max_depth=8), seed=5)
    assert eng.glm_form() == form
    q0 = np.empty((C_, D))
    q0[:, :Dx] = mu[:Dx] + rng.standard_normal((C_, Dx)) / np.sqrt(tau[:Dx])
    for c in range(Dx, D):
        q0[:, c] = mu[c] + np.log(np.abs(rng.standard_t(nu[c], C_)))

    def prior_u(q):
        u = np.empty_like(q)
        u[:, :Dx] = special.ndtr((q[:, :Dx] - mu[:Dx]) * np.sqrt(tau[:Dx]))
        for c in range(Dx, D):
            u[:, c] = 2.0 * stats.t.cdf(np.exp(q[:, c] - mu[c]), nu[c]) - 1.0
        return u
    eng.set_q(q0)
    assert np.isfinite(eng.lq).all()
    eng.set_eps(eps)
    eng.nuts_transitions(1, 8)
    q1, ts = eng.q, eng.tree_stats()
    assert eng.poll_abort() == 0
    eng.close()
    fam = S.Family()
    S.add_uniform(fam, prior_u(q1), "after 8 transitions")
    moved = S.moved_fraction(q0, q1)
    print("Dx = %d: %s; moved %.3f; terminations %s" % (Dx, fam.report(), moved, S.terminations(ts)))
    S.assert_stationary(fam, "local scales")
    assert moved > 0.9, moved
    ctl = S.Family()
    S.add_uniform(ctl, special.ndtr(q1[:, Dx + H:] - mu[Dx + H:]), "against the Gaussian prior")
    S.assert_rejects(ctl, "local scales")


# ---- the summaries --------------------------------------------------------------------------------------------------------------------
def slab_twin(s, inv2):
    """st = 1 / sqrt(fma(1 / s, 1 / s, inv2)) with every operation rounded once (the fma through exact rationals)"""
    if s == 0.0:
        return 0.0
    if np.isinf(s):
        return float(1.0 / np.sqrt(np.float64(inv2)))
    i = 1.0 / s
    nn = np.inf if abs(i) > 1e160 else float(Fraction(i) * Fraction(i) + Fraction(inv2))      # (1e160^2 is far past the largest double)
    return float(np.float64(1.0) / np.sqrt(np.float64(nn)))


def theta_local_twin(draws, Dx, A, H, grp, local, slab, dexp):
    """[..., D] sampled coordinates -> [beta | a raw | sigma | exp lambda] by section 19's expressions, dexp the oracle's"""
    draws = np.asarray(draws, dtype=np.float64)
    head = theta_twin(draws[..., :Dx + A + H], Dx, A, H, grp, dexp)
    vexp = np.vectorize(dexp, otypes=[np.float64])
    e, f = vexp(draws[..., Dx + A:Dx + A + H]), vexp(draws[..., Dx + A + H:])
    inv2 = 1.0 / (slab * slab) if slab else 0.0
    for k, c in enumerate(np.flatnonzero(local)):
        s = e[..., grp[c]] * f[..., k] if grp[c] >= 0 else f[..., k]
        st = np.vectorize(lambda x: slab_twin(x, inv2), otypes=[np.float64])(s) if slab else s
        head[..., c] = draws[..., c] * st
    return np.concatenate([head, f], axis=-1)


def test_summaries_of_the_reported_vector(idhmc, oracle):
    """the "odd offset" shape with its slab: summary_add_draws of host draws, and one mcmc_summary, against the host twins"""
    family, Dx, grp, local, slab, D, L, form = SHAPES["odd offset"]
    A, H, J = dims(family, grp, local)
    C_, N, G, bins = 16, 6, 8, 16
    X, Y = HIER.problem_hier(family, 37, Dx, grp, False, seed=5)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    eng = idhmc.Engine(make(idhmc, family, X, Y, grp, local, slab, kind, nu, mu, tau), C_, idhmc.default_options(max_depth=4), seed=21)
    dexp = oracle.lib().orc_exp_export
    draws = np.stack([start_local(family, C_, Dx, H, J, seed=k, scale=0.5) for k in range(N)])
    draws[0, 0, Dx + A + H] = 300.0                       # s far above the slab: st is the slab's, exp(lambda) is huge
    draws[1, 1, Dx + A + H + 1] = -400.0                  # s far below it (1 / s^2 overflows: st = 0)
    theta = theta_local_twin(draws, Dx, A, H, grp, local, slab, dexp)
    assert theta.shape == draws.shape and abs(theta[0, 0, np.flatnonzero(local)[0]]) <= slab * abs(draws[0, 0, np.flatnonzero(local)[0]]) * (1 + 1e-15)
    eng.summary_begin(chains_per_group=G, bins=bins)
    assert eng.summary_dims() == (C_ // G, G, D, bins)
    eng.summary_add_draws(draws[:2])
    eng.summary_set_range(span=3.0)
    eng.summary_add_draws(draws[2:])
    got = eng.summary()
    assert_summary(got, summary_twin(theta, G), "host draws")
    s = summary_twin(theta[:2], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 3.0, bins)
    assert_histogram(got, theta[2:], G, lo, hi, "host draws")
    eng.summary_end()
    # sampled: the same transitions stored, then reduced on the device
    q0 = start_local(family, C_, Dx, H, J)
    eng.set_eps(0.02)
    eng.set_q(q0)
    stored, _ = eng.mcmc(N, 3, store_draws=True, store_stats=False)
    eng.set_q(q0)
    got = eng.mcmc_summary(N, 3, pilot=2, chains_per_group=G, bins=bins)
    th = theta_local_twin(stored, Dx, A, H, grp, local, slab, dexp)
    assert np.all(got.n == N * G) and np.all(got.binned == (N - 2) * G)
    assert_summary(got, summary_twin(th, G), "mcmc_summary")
    s = summary_twin(th[:2], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 6.0, bins)
    assert_histogram(got, th[2:], G, lo, hi, "mcmc_summary")
    m = eng.model
    assert np.allclose(th[..., :Dx], idhmc.glm.coefficients(m, stored), rtol=1e-12, atol=1e-300)
    assert np.allclose(th[..., Dx + A + H:], idhmc.glm.local_scales(m, stored), rtol=1e-12)
    assert eng.poll_abort() == 0
    eng.close()
