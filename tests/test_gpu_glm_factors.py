"""Factor terms by level index (GLM(..., factors=), idhmc_create_glm_factors) on the device.  A model with factors
is bit-identical to the same model with its factors written out as indicator columns (glm.expand_factors), in two ways: an engine on
the expanded matrix, which runs the kernels that know nothing of factors, and oracle chains on the C restatement of section 19
(tests/test_glm_local_cpu.py) fed the expanded matrix.  No tolerance anywhere but against numpy at the one shape whose expansion does
not fit.  Both device forms: one chain per wavefront (evaluation, leapfrog; NUTS at L = 512) and the matrix-core gradient of the NUTS
kernel.  Then: several responses, an empty list of factors, a warm-up, the device summaries, and the limit on the observations.  Every
context compiles its source with hipRTC, so engines are shared across assertions."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_local_cpu import c_source_local, local_priors, oracle_params_local, start_local

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# name: (family, Dd, levels, groups on the levels, local scales on every third level and their slab, D, padded length, matrix cores)
SHAPES = {
    "straddle tile": ("POISSON_LOG", 20, (30,), True, None, 20 + 30 + 1, 128, 1),
    "tile aligned": ("POISSON_LOG", 32, (7, 50), True, None, 32 + 57 + 2, 128, 1),
    "chunk straddle": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, (120,), True, 2.0, 100 + 120 + 1 + 1 + 40, 512, 0),
    "intercept only": ("POISSON_LOG", 1, (5,), False, None, 6, 128, 1),
    "per wave": ("GAUSSIAN_IDENTITY_LOGSIGMA", 20, (400,), True, None, 20 + 400 + 1 + 1, 512, 0),
    "empty and full": ("POISSON_LOG", 5, (4, 3), True, None, 5 + 7 + 2, 128, 1),
}


def problem(shape, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,), local (Dx,), slab): data from the family's own model, levels drawn independently per factor
    (crossed); "empty and full": no observation has level 2 of factor 0, every observation has level 0 of factor 1"""
    family, Dd, levels, grouped, slab, D, L, form = SHAPES[shape]
    rng = np.random.default_rng(n + Dd if seed is None else seed)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    z = X @ (0.5 * rng.standard_normal(Dd) / np.sqrt(Dd))
    factors = []
    for f, N in enumerate(levels):
        idx = rng.integers(0, N, n)
        if shape == "empty and full":
            idx = rng.choice([0, 1, 3], n) if f == 0 else np.zeros(n, np.int64)
        z = z + (0.4 * rng.standard_normal(N))[idx]
        factors.append((idx, N))
    Y = rng.poisson(np.exp(z)).astype(float) if family == "POISSON_LOG" else z + 0.5 * rng.standard_normal(n)
    Dx = Dd + sum(levels)
    grp = np.full(Dx, -1, np.int32)
    if grouped:
        off = Dd
        for f, N in enumerate(levels):
            grp[off:off + N] = f
            off += N
    local = np.zeros(Dx, np.int32)
    if slab:
        local[Dd::3] = 1
    return X, Y, factors, grp, local, slab


def dims(shape):
    family, Dd, levels, grouped, slab, D, L, form = SHAPES[shape]
    Dx = Dd + sum(levels)
    return SHAPE[family][2], len(levels) if grouped else 0, len(range(Dd, Dx, 3)) if slab else 0


def models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, **kw):
    """the model with factors and its expansion"""
    family = SHAPES[shape][0]
    common = dict(constants=consts(family), prior_mu=mu, prior_tau=tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu,
                  local=local, slab_scale=slab, **kw)
    return (idhmc.GLM(X, Y, source(idhmc, family), factors=factors, **common),
            idhmc.GLM(idhmc.glm.expand_factors(X, factors), Y, source(idhmc, family), **common))


def oracle_model(oracle, tmp_path, shape, Xe, Y, grp, local, slab, kind, nu, mu, tau):
    family, D = SHAPES[shape][0], SHAPES[shape][5]
    return oracle.OracleModel.custom(D, c_source_local(family),
                                     oracle_params_local(Xe, Y, SHAPE[family][2], grp, local, slab, kind, nu, consts(family), mu, tau), str(tmp_path))


def test_the_shapes_are_what_they_are_there_for(idhmc):
    for name, (family, Dd, levels, grouped, slab, D, L, form) in SHAPES.items():
        A, H, J = dims(name)
        assert Dd + sum(levels) + A + H + J == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))), name
    assert 16 < 20 < 32 and 32 * ((20 + 31) // 32) == 32          # "straddle tile": tile 16..31 holds dense and level columns
    assert 32 % 16 == 0 and 32 + 7 < 48                           # "tile aligned": the first level tile starts at Dd, both factors in it
    assert 100 < 128 < 100 + 120                                  # "chunk straddle": levels on both sides of column 128
    X, Y, factors, grp, local, slab = problem("chunk straddle", 130)
    assert local[:100].sum() == 0 and local.sum() == 40 and local[100] == 1 and local[127] == 1 and local[130] == 1
    assert 128 * ((20 + 127) // 128) == 128 < 512                 # "per wave": Lx < L
    X, Y, factors, grp, local, slab = problem("empty and full", 130)
    assert 2 not in factors[0][0] and not factors[1][0].any() and factors[1][1] == 3
    E = idhmc.glm.expand_factors(X, factors)
    assert E.shape == (130, 12) and not E[:, 5 + 2].any() and E[:, 9].all() and not E[:, 10:].any()


def state(eng):
    return eng.q, eng.p, eng.lq, eng.grad


def assert_same_state(engF, engE, chains, D, what):
    for a, b in zip(state(engF), state(engE)):
        assert same_bits(a, b), what
    if chains is not None:
        q, p, lq, g = state(engF)
        assert same_bits(q, np.stack([c.q[:D] for c in chains])) and same_bits(lq, [c.lq for c in chains]), what
        assert same_bits(g, np.stack([c.grad[:D] for c in chains])), what


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1, 128, 130])
def test_density_leapfrog_and_nuts(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the shape runs: the bits of the engine on the expanded matrix and of the oracle chains
    on it"""
    family, Dd, levels, grouped, slab, D, L, form = SHAPES[shape]
    A, H, J = dims(shape)
    Dx, C_ = Dd + sum(levels), 18
    X, Y, factors, grp, local, slab = problem(shape, n)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    mF, mE = models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    assert (mF.D, mE.D, mF.Dx, mE.Dx, mF.Dd, mE.Dd) == (D, D, Dx, Dx, Dd, Dx)
    opt = idhmc.default_options(max_depth=4)
    engF, engE = idhmc.Engine(mF, C_, opt, seed=3), idhmc.Engine(mE, C_, opt, seed=3)
    om = oracle_model(oracle, tmp_path, shape, idhmc.glm.expand_factors(X, factors), Y, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert engF.glm_form() == engE.glm_form() == form and engF.padded_dim() == engE.padded_dim() == L and engF.D == D
    lev, idx = engF.glm_factors()
    assert lev.dtype == idx.dtype == np.int32 and list(lev) == list(levels) and np.array_equal(idx, [f[0] for f in factors])
    assert engE.glm_factors() == (None, None)
    assert engF.device_bytes() < engE.device_bytes() or L == 128
    q = start_local(family, C_, Dx, H, J)
    engF.set_q(q)
    engE.set_q(q)
    for c, ch in enumerate(chains):
        ch.set_q(q[c])
    assert np.isfinite(engF.lq).all()
    assert_same_state(engF, engE, chains, D, "evaluation")
    for eng in (engF, engE):
        eng.refresh_momentum(1)
        eng.leapfrog(0.01, 1)
    for ch in chains:
        ch.rand_p(1)
        ch.leapfrog(0.01)
    assert same_bits(engF.p, np.stack([c.p[:D] for c in chains]))
    assert_same_state(engF, engE, chains, D, "leapfrog")
    eps = 0.02
    engF.set_eps(eps)
    engE.set_eps(eps)
    for it in (1, 2):
        engF.nuts_transition(it)
        engE.nuts_transition(it)
        st, ste = engF.tree_stats(), engE.tree_stats()
        ost = [ch.sample_tree(eps, it) for ch in chains]
        assert np.array_equal(st, ste), it
        for f in ("depth", "steps", "term_left", "term_right"):
            np.testing.assert_array_equal(st[f], [getattr(s, f) for s in ost], err_msg="%s @%d" % (f, it))
        assert same_bits(st["pi"], [s.pi for s in ost])
        assert_same_state(engF, engE, chains, D, "transition %d" % it)
    engF.nuts_transitions(3, 2)
    engE.nuts_transitions(3, 2)
    for it in (3, 4):
        for ch in chains:
            ch.sample_tree(eps, it)
    assert_same_state(engF, engE, chains, D, "two transitions in one launch")
    assert engF.poll_abort() == 0 and engE.poll_abort() == 0
    engF.close()
    engE.close()


def test_responses_are_single_response_chains(idhmc, oracle, tmp_path):
    """M = 4 responses of R = 3 chains on "straddle tile": every chain is bit-identical to the single-response oracle chain on its Y and
    the expanded matrix (the same global chain id)"""
    shape = "straddle tile"
    family, Dd, levels, grouped, slab, D, L, form = SHAPES[shape]
    A, H, J = dims(shape)
    Dx, M, R, n = Dd + sum(levels), 4, 3, 130
    X, Y0, factors, grp, local, slab = problem(shape, n)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [rng.poisson(np.maximum(Y0, 0.5)).astype(float) for _ in range(M - 1)])[:, :, None]
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    mF, mE = models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, chains_per_response=R)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(mF, M * R, opt, seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form and list(eng.glm_factors()[0]) == list(levels)
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
        om = oracle_model(oracle, tmp_path, shape, idhmc.glm.expand_factors(X, factors), Y[m], grp, local, slab, kind, nu, mu, tau)
        for c in range(R * m, R * m + R):
            ch = oracle.OracleChain(om, oopt, seed=13, chain_id=c)
            ch.set_q(q[c])
            ch.sample_tree(eps, 1)
            assert same_bits(q1[c], ch.q[:D]), c
            ch.sample_tree(eps, 2)
            ch.sample_tree(eps, 3)
            assert same_bits(q3[c], ch.q[:D]) and same_bits(lq3[c], ch.lq) and same_bits(g3[c], ch.grad[:D]), c


SHORT = dict(init_steps=10, middle_steps=10, doubling_stages=1, terminating_steps=20, max_depth=6)      # 40 transitions


def test_no_factor_is_the_model_without_the_keyword(idhmc):
    """factors=[] gives the bits of the model without the keyword after a short warm-up plus 10 draws, packed (no groups) and through the
    descriptor (groups); glm_factors() returns (None, None)"""
    rng = np.random.default_rng(9)
    n, Dx, C_ = 50, 25, 6
    X = 0.3 * rng.standard_normal((n, Dx))
    Y = rng.poisson(np.exp(X @ rng.standard_normal(Dx) * 0.3)).astype(float)
    for grp in (None, np.where(np.arange(Dx) < 8, 0, -1)):
        out = []
        for kw in ({}, {"factors": []}):
            eng = idhmc.Engine(idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, None, 0.1, 0.7, groups=grp, **kw), C_, idhmc.default_options(**SHORT), seed=77)
            assert eng.glm_factors() == (None, None)
            draws, stats_ = eng.mcmc_with_warmup(10)
            out.append((draws, stats_, eng.eps, eng.minv, eng.glm_form(), eng.device_bytes()))
            assert eng.poll_abort() == 0
            eng.close()
        a, b = out
        assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and a[4:] == b[4:]


def test_warmup_matches_the_expanded_engine(idhmc):
    """a 40-transition warm-up with per-chain adaptation on "tile aligned", then 8 draws: the same stepsizes, metric, draws and records"""
    shape = "tile aligned"
    family, Dd, levels, grouped, slab, D, L, form = SHAPES[shape]
    A, H, J = dims(shape)
    Dx, C_, N = Dd + sum(levels), 8, 8
    X, Y, factors, grp, local, slab = problem(shape, 130)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    out = []
    for m in models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau):
        eng = idhmc.Engine(m, C_, idhmc.default_options(**SHORT), seed=77)
        draws, stats_ = eng.mcmc_with_warmup(N)
        out.append((draws, stats_, eng.eps, eng.minv, eng.lq, eng.grad))
        assert eng.poll_abort() == 0 and eng.glm_form() == form
        eng.close()
    a, b = out
    assert np.isfinite(a[0]).all() and len(np.unique(a[2])) > 1
    assert same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert same_bits(a[4], b[4]) and same_bits(a[5], b[5])


def test_summary_matches_the_expanded_engine(idhmc):
    """mcmc_summary on "straddle tile": every field of the device summary of [beta | sigma] equals the expanded engine's"""
    shape = "straddle tile"
    family, Dd, levels, grouped, slab, D, L, form = SHAPES[shape]
    A, H, J = dims(shape)
    Dx, C_, N, G, bins = Dd + sum(levels), 16, 6, 8, 16
    X, Y, factors, grp, local, slab = problem(shape, 130)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    q0 = start_local(family, C_, Dx, H, J)
    out = []
    for m in models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau):
        eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4), seed=21)
        eng.set_eps(0.02)
        eng.set_q(q0)
        out.append(eng.mcmc_summary(N, 3, pilot=2, chains_per_group=G, bins=bins))
        assert eng.poll_abort() == 0
        eng.close()
    a, b = (dataclasses.asdict(s) for s in out)
    assert np.all(a["n"] == N * G) and np.all(a["binned"] == (N - 2) * G) and a["mean"].shape == (C_ // G, D)
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], np.ndarray) and a[k].dtype == np.float64:
            assert same_bits(a[k], b[k]), k
        else:
            assert np.array_equal(a[k], b[k]), k


def test_the_limit_counts_the_stored_columns(idhmc):
    """Dd = 3 and one factor of 900 levels at n = 140 000: n_pad * L > 2^27, n_pad * Lx <= 2^27.  The context is created, evaluates, and
    matches numpy within 1e-12 of the magnitude of the terms summed on chains 0 and last; the expanded model is refused"""
    n, Dd, N, C_ = 140000, 3, 900, 2
    Dx = Dd + N
    rng = np.random.default_rng(1)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    idx = rng.integers(0, N, n)
    idx[:N] = np.arange(N)
    z = X @ np.array([0.3, -0.2, 0.1]) + (0.4 * rng.standard_normal(N))[idx]
    Y = rng.poisson(np.exp(z)).astype(float)
    mu, tau = np.full(Dx, 0.05), np.full(Dx, 1.5)
    m = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, None, mu, tau, factors=[(idx, N)])
    opt = idhmc.default_options(metric_mode=idhmc.METRIC_SHARED)
    eng = idhmc.Engine(m, C_, opt, seed=1)
    assert eng.padded_dim() == 1024 and eng.glm_form() == 0 and ((n + 127) // 128 * 128) * 1024 > 1 << 27
    assert eng.device_bytes() < 8 * 140032 * 1024                     # less than X alone would take 1024 columns wide
    q = rng.uniform(-0.3, 0.3, (C_, Dx))
    eng.set_q(q)
    lq, g = eng.lq, eng.grad
    eng.close()
    for c in (0, C_ - 1):
        zc = X @ q[c, :Dd] + q[c, Dd + idx]
        e = np.exp(zc)
        d = q[c] - mu
        l_ref = np.sum(Y * zc - e) - 0.5 * np.sum(tau * d * d)
        lscale = np.sum(np.abs(Y * zc)) + np.sum(e) + 0.5 * np.sum(tau * d * d)
        r = Y - e
        G = np.concatenate([X.T @ r, np.bincount(idx, r, N)])
        gscale = np.concatenate([np.abs(X).T @ np.abs(r), np.bincount(idx, np.abs(r), N)]) + np.abs(tau * d)
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale, (c, lq[c], l_ref)
        assert np.all(np.abs(g[c] - (G - tau * d)) <= 1e-12 * gscale + 1e-300), c
    # the expansion of this shape: refused at the C boundary before anything of X is read (never-touched zero pages stand in for it)
    d = m.glm_desc()
    wide = np.zeros((n, Dx))
    d.X = wide.ctypes.data_as(C.POINTER(C.c_double))
    h = C.c_void_p()
    lib = idhmc.load_library()
    rc = lib.idhmc_create_glm_factors(C.byref(h), 0, C_, 0, C.byref(d), None, None, None, 1, 0, C.byref(opt), 1)
    assert rc == idhmc.ERR_BAD_ARG and b"exceed n_pad * L <= 2^27" in lib.idhmc_last_error()
