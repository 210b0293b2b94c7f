"""Priors beyond the Gaussian (GLM(..., prior_kind=, prior_nu=), idhmc_create_glm_priors) on the device.  Models with
Student-t, half-normal, half-t and exponential priors are bit-identical to the CPU oracle running the C restatement of section 18's
table (tests/test_glm_priors_cpu.py, through oracle.OracleModel.custom) and within 1e-12 of numpy, in both device forms: one chain
per wavefront (evaluation, leapfrog; NUTS at L = 512) and the matrix-core gradient of the NUTS kernel.  No tolerance on the device
side.  Then: the priors move no row of idhmc_glm_form's table, several responses, the all-NORMAL model, a warm-up, and exact
stationarity on models whose posterior is their prior.  Every context compiles its source with hipRTC, so engines are shared across
assertions."""
import numpy as np
import pytest
from scipy import special, stats

import stationarity as S
import test_glm_hier_cpu as HIER
from test_glm_hier_cpu import SHAPE, consts
from test_glm_priors_cpu import (LOG_EXPONENTIAL, LOG_HALF_NORMAL, LOG_HALF_STUDENT_T, NORMAL, STUDENT_T, c_source_priors, make, mixed_priors,
                                 numpy_density_priors, oracle_params_priors)

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def straddling(Dx):
    """group 0: columns 100..160 (across column 128, the chunk boundary); group 1: the columns behind"""
    g = np.full(Dx, -1, np.int32)
    g[100:161] = 0
    g[161:] = 1
    return g


def shape_priors(name, Dx, A, H):
    """(kind, nu, mu, tau) of a shape of SHAPES"""
    D = Dx + A + H
    kind, nu, mu, tau = mixed_priors(Dx, A, H)
    if name == "L = 128":
        # coefficients alternate NORMAL and STUDENT_T (mixed_priors): the two coordinates of a lane differ
        kind[Dx:], nu[Dx:] = [LOG_HALF_STUDENT_T, LOG_EXPONENTIAL], [4.0, 0.0]
    elif name == "D = 128":
        kind[:], nu[:] = NORMAL, 0.0
        kind[3], nu[3] = STUDENT_T, 3.0
        kind[127] = LOG_HALF_NORMAL                     # the last lane, second component
    elif name == "L = 256":
        kind[:], nu[:] = NORMAL, 0.0
        kind[120:136], nu[120:136] = STUDENT_T, [1.0, 3.0] * 8      # across the chunk boundary
        kind[Dx:] = LOG_HALF_NORMAL
    else:
        assert set(kind) == {0, 1, 2, 3, 4}
    tau[kind >= LOG_HALF_NORMAL] = 1.0
    takes = (kind == STUDENT_T) | (kind == LOG_HALF_STUDENT_T)
    assert (nu[takes] > 0).all() and not nu[~takes].any() and kind.size == D
    return kind, nu, mu, tau


# name: (family, Dx, grp, padded length, matrix cores)
SHAPES = {
    "L = 128": ("GAUSSIAN_IDENTITY_LOGSIGMA", 25, HIER.blocks(25, 1, 10), 128, 1),
    "D = 128": ("POISSON_LOG", 127, HIER.interleaved(127, 1), 128, 1),
    "L = 256": ("POISSON_LOG", 200, straddling(200), 256, 1),
    "L = 512": ("GAUSSIAN_IDENTITY_LOGSIGMA", 300, HIER.interleaved(300, 4), 512, 0),
}


def setup(idhmc, oracle, tmp_path, family, X, Y, grp, kind, nu, mu, tau, C, seed, opt=None, oopt=None, **kw):
    A, H = SHAPE[family][2], int(grp.max()) + 1
    D = X.shape[1] + A + H
    eng = idhmc.Engine(make(idhmc, family, X, Y, grp, kind, nu, mu, tau, **kw), C, opt, seed=seed)
    om = oracle.OracleModel.custom(D, c_source_priors(family), oracle_params_priors(X, Y, A, grp, kind, nu, consts(family), mu, tau), str(tmp_path))
    chains = [oracle.OracleChain(om, oopt, seed=seed, chain_id=c) for c in range(C)]
    return eng, om, chains


def check_density(eng, chains, family, X, Y, grp, kind, nu, mu, tau, D, ends):
    q, g, lq = eng.q, eng.grad, eng.lq
    assert same_bits(lq, [c.lq for c in chains]) and same_bits(g, np.stack([c.grad[:D] for c in chains]))
    for c in ends:
        l_ref, g_ref, lscale, gscale = numpy_density_priors(family, X, Y, q[c], grp, kind, nu, mu, tau)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1, 130])
def test_density_leapfrog_and_nuts(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: single
    launches, then two in one launch) in the form the shape runs: bit-identical to the oracle, within 1e-12 of numpy"""
    family, Dx, grp, L, form = SHAPES[shape]
    A, H = SHAPE[family][2], int(grp.max()) + 1
    C_, D = 18, Dx + A + H
    kind, nu, mu, tau = shape_priors(shape, Dx, A, H)
    X, Y = HIER.problem_hier(family, n, Dx, grp, shape == "L = 128", seed=n + Dx)
    eng, om, chains = setup(idhmc, oracle, tmp_path, family, X, Y, grp, kind, nu, mu, tau, C_, 3, idhmc.default_options(max_depth=4),
                            oracle.default_options(max_depth=4))
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D
    got_kind, got_nu = eng.glm_priors()
    assert got_kind.dtype == np.int32 and np.array_equal(got_kind, kind) and same_bits(got_nu, nu)
    q = HIER.start_hier(family, C_, Dx, H)
    eng.set_q(q)
    for c, ch in enumerate(chains):
        ch.set_q(q[c])
    ends = (0, C_ - 1)
    check_density(eng, chains, family, X, Y, grp, kind, nu, mu, tau, D, ends)
    eng.refresh_momentum(1)
    eng.leapfrog(0.01, 1)
    for ch in chains:
        ch.rand_p(1)
        ch.leapfrog(0.01)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains])) and same_bits(eng.p, np.stack([c.p[:D] for c in chains]))
    check_density(eng, chains, family, X, Y, grp, kind, nu, mu, tau, D, ends)
    eps = 0.02
    eng.set_eps(eps)
    for it in (1, 2):
        eng.nuts_transition(it)
        st = eng.tree_stats()
        ost = [ch.sample_tree(eps, it) for ch in chains]
        for f in ("depth", "steps", "term_left", "term_right"):
            np.testing.assert_array_equal(st[f], [getattr(s, f) for s in ost], err_msg="%s @%d" % (f, it))
        assert same_bits(st["pi"], [s.pi for s in ost]) and same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
        check_density(eng, chains, family, X, Y, grp, kind, nu, mu, tau, D, ends)
    eng.nuts_transitions(3, 2)
    for it in (3, 4):
        for ch in chains:
            ch.sample_tree(eps, it)
    assert same_bits(eng.q, np.stack([c.q[:D] for c in chains]))
    check_density(eng, chains, family, X, Y, grp, kind, nu, mu, tau, D, ends)
    assert eng.poll_abort() == 0
    eng.close()


def _form_source(A):
    """a Gaussian with known scale (A = 0), or with log sigma = a[0] whose further auxiliary coordinates see only their prior"""
    if A == 0:
        return "__device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)\n{\n    r = o.y[0] - z;\n    v = 0.5 * (r * r);\n}\n"
    return ("__device__ void glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)\n{\n"
            "    const double w = dexp(-a[0]);\n    const double u = (o.y[0] - z) * w;\n    v = 0.5 * (u * u) + a[0];\n    r = u * w;\n"
            "    s[0] = u * u - 1.0;\n" + "".join("    s[%d] = 0.0;\n" % j for j in range(1, A)) + "}\n")


# (Dx, L, A, shared metric)
FORM_ROWS = [(30, 128, 4, False), (200, 256, 1, False), (200, 256, 2, True), (200, 256, 2, False), (300, 512, 0, False)]


@pytest.mark.parametrize("Dx,L,A,shared", FORM_ROWS, ids=["L%d-A%d-%s" % (r[1], r[2], "shared" if r[3] else "perchain") for r in FORM_ROWS])
def test_priors_move_no_row_of_the_table(idhmc, Dx, L, A, shared):
    """idhmc_glm_form with Student-t coefficients and half-t / exponential auxiliary coordinates is that of the same model with
    Gaussian priors, at the rows where an LDS byte more would move it, and the kernel launches (the priors add no LDS)"""
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((40, Dx)) * 0.3, rng.standard_normal(40)
    D = Dx + A
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[0:Dx:2], nu[0:Dx:2] = STUDENT_T, 3.0
    for j in range(A):
        kind[Dx + j], nu[Dx + j] = ((LOG_HALF_STUDENT_T, 4.0), (LOG_EXPONENTIAL, 0.0), (LOG_HALF_NORMAL, 0.0))[j % 3]
    opt = idhmc.default_options(max_depth=3, metric_mode=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    forms = []
    for kw in ({}, {"prior_kind": kind, "prior_nu": nu}):
        eng = idhmc.Engine(idhmc.GLM(X, Y, _form_source(A), aux=A, **kw), 20, opt, seed=2)
        assert eng.padded_dim() == L
        forms.append(eng.glm_form())
        eng.set_q(rng.uniform(-0.1, 0.1, (20, D)))
        eng.set_eps(0.01)
        eng.nuts_transition(1)
        assert np.isfinite(eng.lq).all() and (eng.tree_stats()["steps"] >= 1).all()
        eng.close()
    assert forms[0] == forms[1] == (1 if L == 128 or (L == 256 and (A <= 1 or shared)) else 0)


def test_responses_are_single_response_engines(idhmc):
    """M = 3 responses of R = 4 chains with non-Gaussian priors: each chain's draws are bit-identical to those of the single-response
    engine on its Y (the same global chain ids)"""
    M, R, n, Dx, N = 3, 4, 37, 25, 4
    family, grp = "POISSON_LOG", HIER.interleaved(25, 1)
    X, _ = HIER.problem_hier(family, n, Dx, grp, False, seed=5)
    rng = np.random.default_rng(6)
    Y = rng.poisson(np.exp(0.3 * rng.standard_normal((M, n, 1)))).astype(float)
    kind, nu, mu, tau = mixed_priors(Dx, 0, 1)
    kind[Dx], nu[Dx] = LOG_HALF_STUDENT_T, 1.0
    opt = idhmc.default_options(max_depth=4)
    q = HIER.start_hier(family, M * R, Dx, 1)

    def run(eng, rows):
        eng.set_q(q[rows])
        eng.set_eps(0.03)
        eng.nuts_transitions(1, 2)
        draws, stats_ = eng.mcmc(N, 3)
        out = (draws, stats_, eng.lq, eng.grad)
        eng.close()
        return out
    full = idhmc.Engine(make(idhmc, family, X, Y, grp, kind, nu, mu, tau, chains_per_response=R), M * R, opt, seed=13)
    assert full.glm_responses() == (M, R) and full.glm_form() == 1 and np.array_equal(full.glm_priors()[0], kind)
    fd, fs, flq, fg = run(full, slice(None))
    for m in range(M):
        rows = slice(R * m, R * m + R)
        one = idhmc.Engine(make(idhmc, family, X, Y[m], grp, kind, nu, mu, tau), R, opt, seed=13, first_chain=R * m)
        assert one.glm_responses() == (1, 0)
        d, s, lq, g = run(one, rows)
        assert same_bits(fd[:, rows], d) and np.array_equal(fs[:, rows], s) and same_bits(flq[rows], lq) and same_bits(fg[rows], g)


def test_all_normal_kinds_are_the_model_without_them(idhmc):
    """all-0 kinds through the new keywords -- packed (no groups) and through the descriptor (groups) -- give the bits of the model
    without the keywords after a short warm-up plus 10 draws; glm_priors() returns what was given"""
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    n, Dx, C_ = 50, 25, 6
    for family, grp in (("POISSON_LOG", None), ("GAUSSIAN_IDENTITY_LOGSIGMA", HIER.blocks(25, 2, 8))):
        A, H = SHAPE[family][2], 0 if grp is None else 2
        D = Dx + A + H
        g = np.full(Dx, -1) if grp is None else grp
        X, Y = HIER.problem_hier(family, n, Dx, g, grp is not None, seed=9)
        mu, tau = np.full(D, 0.1), np.full(D, 0.7)
        out = []
        for kw in ({}, {"prior_kind": np.zeros(D, np.int32), "prior_nu": np.zeros(D)}):
            eng = idhmc.Engine(idhmc.GLM(X, Y, getattr(idhmc.glm, family), None, mu, tau, aux=A, groups=grp, **kw), C_,
                               idhmc.default_options(**short), seed=77)
            k, v = eng.glm_priors()
            assert k.shape == (D,) and not k.any() and v.shape == (D,) and not v.any()
            draws, stats_ = eng.mcmc_with_warmup(10)
            out.append((draws, stats_, eng.eps, eng.minv, eng.glm_form(), eng.device_bytes()))
            eng.close()
        a, b = out
        assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and a[4:] == b[4:]


def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path):
    """per-chain adaptation on 8 chains, the stage lengths of the other GLM warm-up tests"""
    family, Dx, n, C_, N = "GAUSSIAN_IDENTITY_LOGSIGMA", 25, 200, 8, 8
    grp = HIER.blocks(Dx, 2, 8)
    A, H = 1, 2
    D = Dx + A + H
    short = dict(init_steps=12, middle_steps=8, doubling_stages=2, terminating_steps=8, max_depth=6)
    X, Y = HIER.problem_hier(family, n, Dx, grp, True, seed=9)
    kind, nu, mu, tau = mixed_priors(Dx, A, H)
    eng = idhmc.Engine(make(idhmc, family, X, Y, grp, kind, nu, mu, tau), C_, idhmc.default_options(**short), seed=77)
    draws, stats_ = eng.mcmc_with_warmup(N)
    om = oracle.OracleModel.custom(D, c_source_priors(family), oracle_params_priors(X, Y, A, grp, kind, nu, consts(family), mu, tau), str(tmp_path))
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, C_, oracle.default_options(**short), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps)
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats_.T, ost[:, :N])
    eng.close()


# ---- exact stationarity: X = 0, so the posterior is the prior and its coordinates are independent -------------------------------------
def prior_draws(rng, C, kind, nu, mu, tau):
    """exact host draws of every coordinate from its prior"""
    D = kind.size
    q = np.empty((C, D))
    for c in range(D):
        k = kind[c]
        if k == NORMAL:
            q[:, c] = mu[c] + rng.standard_normal(C) / np.sqrt(tau[c])
        elif k == STUDENT_T:
            q[:, c] = mu[c] + rng.standard_t(nu[c], C) / np.sqrt(tau[c])
        elif k == LOG_HALF_NORMAL:
            q[:, c] = mu[c] + np.log(np.abs(rng.standard_normal(C)))
        elif k == LOG_HALF_STUDENT_T:
            q[:, c] = mu[c] + np.log(np.abs(rng.standard_t(nu[c], C)))
        else:
            q[:, c] = mu[c] + np.log(rng.standard_exponential(C))
    return q


def prior_u(q, kind, nu, mu, tau):
    """u = F(q) per coordinate: the cdf of q under its prior (of sigma = exp(q) for the log kinds: the same number)"""
    u = np.empty_like(q)
    for c in range(kind.size):
        k, d = kind[c], q[:, c] - mu[c]
        if k == NORMAL:
            u[:, c] = special.ndtr(d * np.sqrt(tau[c]))
        elif k == STUDENT_T:
            u[:, c] = stats.t.cdf(d * np.sqrt(tau[c]), nu[c])
        elif k == LOG_HALF_NORMAL:
            u[:, c] = special.erf(np.exp(d) / np.sqrt(2.0))
        elif k == LOG_HALF_STUDENT_T:
            u[:, c] = 2.0 * stats.t.cdf(np.exp(d), nu[c]) - 1.0
        else:
            u[:, c] = -np.expm1(-np.exp(d))
    return u


@pytest.mark.parametrize("Dx,form,eps", [(30, 1, 0.25), (300, 0, 0.12)], ids=["L128-matrix-cores", "Dx300-per-wave"])
@pytest.mark.parametrize("scales", ["half-normal-and-half-t", "exponential"])
def test_nuts_leaves_the_prior_exact(idhmc, scales, Dx, form, eps):
    """4096 chains start at exact draws from the prior, 8 transitions at a fixed stepsize: u = F(q) per coordinate stays uniform
    (tests/stationarity.py, its FWER); the same draws judged against the Gaussian of the same mu and tau -- today's prior -- are rejected"""
    C_, H = 4096, 2
    D = Dx + H
    grp = HIER.interleaved(Dx, H)
    rng = np.random.default_rng(17)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[0:Dx:2], nu[0:Dx:2] = STUDENT_T, 3.0
    if scales == "exponential":
        kind[Dx:] = LOG_EXPONENTIAL
    else:
        kind[Dx:], nu[Dx:] = [LOG_HALF_NORMAL, LOG_HALF_STUDENT_T], [0.0, 4.0]
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[Dx:] = 1.0
    X, Y = np.zeros((1, Dx)), np.array([2.0])
    eng = idhmc.Engine(idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, None, mu, tau, groups=grp, prior_kind=kind, prior_nu=nu), C_,
                       idhmc.default_options(max_depth=8), seed=5)
    assert eng.glm_form() == form
    q0 = prior_draws(rng, C_, kind, nu, mu, tau)
    eng.set_q(q0)
    assert np.isfinite(eng.lq).all()
    eng.set_eps(eps)
    eng.nuts_transitions(1, 8)
    q1, ts = eng.q, eng.tree_stats()
    eng.close()
    fam = S.Family()
    S.add_uniform(fam, prior_u(q1, kind, nu, mu, tau), "after 8 transitions")
    moved = S.moved_fraction(q0, q1)
    print("%s, Dx = %d: %s; moved %.3f; terminations %s" % (scales, Dx, fam.report(), moved, S.terminations(ts)))
    S.assert_stationary(fam, scales)
    assert moved > 0.9, moved
    # the control: the non-Gaussian coordinates under the Gaussian of equal location and scale
    other = np.flatnonzero(kind != NORMAL)
    ctl = S.Family()
    S.add_uniform(ctl, special.ndtr((q1[:, other] - mu[other]) * np.sqrt(tau[other])), "against the Gaussian prior")
    S.assert_rejects(ctl, scales)
