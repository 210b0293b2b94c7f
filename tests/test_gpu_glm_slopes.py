"""Factor terms that carry a value per observation (glm.term(index, values=), idhmc_create_glm_slopes) on the device.
A model with valued terms is bit-identical to the same model on the expanded matrix (glm.expand_factors, whose column holds the value
where the level is and 0.0 elsewhere), in two ways: an engine on the expanded matrix, which runs the kernels that know nothing of
factors, and oracle chains on the C restatement of section 19 (tests/test_glm_local_cpu.py) fed the expanded matrix.  No tolerance
anywhere.  Both device forms: one chain per wavefront (evaluation, leapfrog; NUTS at L = 512) and the matrix-core gradient of the NUTS
kernel.  Then: values of 1.0 against the plain term, several responses, a warm-up, the device summaries, and a model without values
through the new entry point.  Every context compiles its source with hipRTC, so engines are shared across assertions."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_local_cpu import c_source_local, local_priors, oracle_params_local, start_local
from test_gpu_glm_factors import SHORT, assert_same_state, same_bits

pytestmark = pytest.mark.gpu


# name: (family, Dd, (levels, valued) per term, groups on the levels, local scales on every third level and their slab, D, padded length,
# matrix cores)
SHAPES = {
    "one tile": ("POISSON_LOG", 20, ((15, False), (15, True)), True, None, 20 + 30 + 2, 128, 1),
    "tile aligned": ("POISSON_LOG", 32, ((7, False), (50, True)), True, None, 32 + 57 + 2, 128, 1),
    "chunk straddle": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, ((120, True),), True, 2.0, 100 + 120 + 1 + 1 + 40, 512, 0),
    "intercept only": ("POISSON_LOG", 1, ((5, True),), False, None, 6, 128, 1),
    "zeros and signs": ("POISSON_LOG", 5, ((4, True), (3, True)), True, None, 5 + 7 + 2, 128, 1),
}


def problem(idhmc, shape, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,), local (Dx,), slab): data from the family's own model.  Values are 0.5 N(0, 1).  "one tile": both
    terms on one index, (1 + x | s); the other shapes draw their indices independently (crossed).  "zeros and signs": no observation has
    level 2 of term 0; every observation of term 1 is at level 0 or 1 and every value at its level 1 is 0.0; the values of term 0 hold an
    exact 0.0, a -0.0 and negatives"""
    family, Dd, terms, grouped, slab, D, L, form = SHAPES[shape]
    rng = np.random.default_rng(n + Dd if seed is None else seed)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    z = X @ (0.5 * rng.standard_normal(Dd) / np.sqrt(Dd))
    factors, shared = [], None
    for f, (N, valued) in enumerate(terms):
        idx = rng.integers(0, N, n)
        if shape == "one tile":
            shared = idx = idx if shared is None else shared
        if shape == "zeros and signs":
            idx = rng.choice([0, 1, 3], n) if f == 0 else rng.integers(0, 2, n)
        w = 0.5 * rng.standard_normal(n)
        if shape == "zeros and signs":
            if f == 0:
                w[0::5] = 0.0
                w[1::5] = -0.0
                w[2::5] = -np.abs(w[2::5])
            else:
                w[idx == 1] = 0.0
        z = z + (w if valued else 1.0) * (0.4 * rng.standard_normal(N))[idx]
        factors.append(idhmc.glm.term(idx, values=w, levels=N) if valued else (idx, N))
    Y = rng.poisson(np.exp(z)).astype(float) if family == "POISSON_LOG" else z + 0.5 * rng.standard_normal(n)
    Dx = Dd + sum(N for N, v in terms)
    grp = np.full(Dx, -1, np.int32)
    if grouped:
        off = Dd
        for f, (N, v) in enumerate(terms):
            grp[off:off + N] = f
            off += N
    local = np.zeros(Dx, np.int32)
    if slab:
        local[Dd::3] = 1
    return X, Y, factors, grp, local, slab


def dims(shape):
    family, Dd, terms, grouped, slab, D, L, form = SHAPES[shape]
    Dx = Dd + sum(N for N, v in terms)
    return Dx, SHAPE[family][2], len(terms) if grouped else 0, len(range(Dd, Dx, 3)) if slab else 0


def models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, **kw):
    """the model with factor terms and its expansion"""
    family = SHAPES[shape][0]
    common = dict(constants=consts(family), prior_mu=mu, prior_tau=tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu,
                  local=local, slab_scale=slab, **kw)
    return (idhmc.GLM(X, Y, source(idhmc, family), factors=factors, **common),
            idhmc.GLM(idhmc.glm.expand_factors(X, factors), Y, source(idhmc, family), **common))


def oracle_model(oracle, tmp_path, shape, Xe, Y, grp, local, slab, kind, nu, mu, tau):
    family, D = SHAPES[shape][0], SHAPES[shape][5]
    return oracle.OracleModel.custom(D, c_source_local(family),
                                     oracle_params_local(Xe, Y, SHAPE[family][2], grp, local, slab, kind, nu, consts(family), mu, tau), str(tmp_path))


def coefficients(shape, q, grp, local, slab):
    """b (C, Dx) of q = [u | a | omega | lambda] in numpy: u times the group's scale, and for a flagged column the regularised local scale"""
    Dx, A, H, J = dims(shape)
    u, om, lam = q[:, :Dx], q[:, Dx + A:Dx + A + H], q[:, Dx + A + H:]
    ls = np.where(grp >= 0, om[:, np.maximum(grp, 0)], 0.0) if H else np.zeros_like(u)
    b = u * np.exp(ls)
    cols = np.flatnonzero(local)
    if J:
        s = np.exp(ls[:, cols] + lam)
        b[:, cols] = u[:, cols] * s / np.sqrt(1.0 + s * s / (slab * slab))
    return b


def test_the_shapes_are_what_they_are_there_for(idhmc):
    for name, (family, Dd, terms, grouped, slab, D, L, form) in SHAPES.items():
        Dx, A, H, J = dims(name)
        assert Dx + A + H + J == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))), name
    # "one tile": the 16-column tile 16..31 holds dense columns (16..19) and plain levels (20..31); with 15 levels the plain term ends at
    # column 34, so it is the tile 32..47 that holds plain levels (32..34) and valued levels (35..47): every mixture is in some tile
    assert 16 < 20 < 32 < 20 + 15 < 48 and 20 + 30 > 48 and 32 * ((20 + 31) // 32) == 32
    X, Y, factors, grp, local, slab = problem(idhmc, "one tile", 130)
    assert factors[0][0] is factors[1].index and factors[1].values is not None            # (1 + x | s): one index, two terms
    # "tile aligned": the first level tile starts at Dd; the plain term and the head of the valued one share it
    assert 32 % 16 == 0 and 32 + 7 < 48 < 32 + 57
    X, Y, factors, grp, local, slab = problem(idhmc, "tile aligned", 130)
    assert not np.array_equal(factors[0][0] % 7, factors[1].index % 7)
    # "chunk straddle": valued levels on both sides of column 128, local scales on both sides
    assert 100 < 128 < 100 + 120 and 128 * ((100 + 127) // 128) == 128 < 512
    X, Y, factors, grp, local, slab = problem(idhmc, "chunk straddle", 130)
    assert local[:100].sum() == 0 and local.sum() == 40 and local[100] == 1 and local[127] == 1 and local[130] == 1
    # "zeros and signs"
    X, Y, factors, grp, local, slab = problem(idhmc, "zeros and signs", 130)
    t0, t1 = factors
    assert 2 not in t0.index and set(t1.index) == {0, 1} and t1.levels == 3
    assert (t0.values == 0.0).any() and np.signbit(t0.values[t0.values == 0.0]).any() and not np.signbit(t0.values[t0.values == 0.0]).all()
    assert (t0.values < 0).any() and (t0.values > 0).any()
    assert not t1.values[t1.index == 1].any() and (t1.index == 1).any() and t1.values[t1.index == 0].all()
    E = idhmc.glm.expand_factors(X, factors)
    assert E.shape == (130, 12) and not E[:, 5 + 2].any() and not E[:, 9 + 1:].any() and E[:, 9].any()
    # no product of a value with a coefficient or with a residual can underflow at the starts: whatever is not exactly zero is far above
    # 1e-300, so no chain reaches -0 (the one new edge)
    for name, (family, Dd, terms, grouped, slab, D, L, form) in SHAPES.items():
        Dx, A, H, J = dims(name)
        for n in (1, 128, 130):
            X, Y, factors, grp, local, slab = problem(idhmc, name, n)
            q = start_local(family, 18, Dx, H, J)
            b = coefficients(name, q, grp, local, slab)
            z = b @ idhmc.glm.expand_factors(X, factors).T
            r = Y - np.exp(z) if family == "POISSON_LOG" else (Y - z) * np.exp(-2.0 * q[:, Dx:Dx + 1])
            off = Dd
            for (N, valued), t in zip(terms, factors):
                if valued:
                    w = np.asarray(t.values)
                    assert np.all(np.abs(w[w != 0.0]) > 1e-8), name
                    for prod in (w * b[:, off + t.index], w * r):
                        assert np.all(np.abs(prod[prod != 0.0]) > 1e-100), (name, n)
                off += N


def state(eng):
    return eng.q, eng.p, eng.lq, eng.grad


def run_engines(engs, chains, D, q, what=""):
    """evaluation, one leapfrog, two single NUTS transitions and two in one launch (fixed eps) on every engine of engs and on the oracle
    chains (or None): after every stage all engines hold the bits of the first, and of the chains"""
    first = engs[0]

    def check(stage):
        for e in engs[1:]:
            for a, b in zip(state(first), state(e)):
                assert same_bits(a, b), (what, stage)
        if chains is not None:
            assert_same_state(first, first, chains, D, (what, stage))

    for e in engs:
        e.set_q(q)
    if chains is not None:
        for c, ch in enumerate(chains):
            ch.set_q(q[c])
    assert np.isfinite(first.lq).all()
    check("evaluation")
    for e in engs:
        e.refresh_momentum(1)
        e.leapfrog(0.01, 1)
    if chains is not None:
        for ch in chains:
            ch.rand_p(1)
            ch.leapfrog(0.01)
        assert same_bits(first.p, np.stack([c.p[:D] for c in chains]))
    check("leapfrog")
    eps = 0.02
    for e in engs:
        e.set_eps(eps)
    for it in (1, 2):
        for e in engs:
            e.nuts_transition(it)
        st = first.tree_stats()
        for e in engs[1:]:
            assert np.array_equal(st, e.tree_stats()), (what, it)
        if chains is not None:
            ost = [ch.sample_tree(eps, it) for ch in chains]
            for f in ("depth", "steps", "term_left", "term_right"):
                np.testing.assert_array_equal(st[f], [getattr(s, f) for s in ost], err_msg="%s @%d" % (f, it))
            assert same_bits(st["pi"], [s.pi for s in ost])
        check("transition %d" % it)
    for e in engs:
        e.nuts_transitions(3, 2)
    if chains is not None:
        for it in (3, 4):
            for ch in chains:
                ch.sample_tree(eps, it)
    check("two transitions in one launch")
    for e in engs:
        assert e.poll_abort() == 0


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1, 128, 130])
def test_density_leapfrog_and_nuts(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the shape runs: the bits of the engine on the expanded matrix and of the oracle chains
    on it"""
    family, Dd, terms, grouped, slab, D, L, form = SHAPES[shape]
    Dx, A, H, J = dims(shape)
    C_ = 18
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    mF, mE = models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    assert (mF.D, mE.D, mF.Dx, mE.Dx, mF.Dd, mE.Dd) == (D, D, Dx, Dx, Dd, Dx)
    assert list(mF.factor_has) == [int(v) for N, v in terms] and mE.factor_has is None
    opt = idhmc.default_options(max_depth=4)
    engF, engE = idhmc.Engine(mF, C_, opt, seed=3), idhmc.Engine(mE, C_, opt, seed=3)
    om = oracle_model(oracle, tmp_path, shape, idhmc.glm.expand_factors(X, factors), Y, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert engF.glm_form() == engE.glm_form() == form and engF.padded_dim() == engE.padded_dim() == L and engF.D == D
    lev, idx = engF.glm_factors()
    assert lev.dtype == idx.dtype == np.int32 and list(lev) == [N for N, v in terms]
    assert np.array_equal(idx, [f.index if v else f[0] for f, (N, v) in zip(factors, terms)])
    has, val = engF.glm_factor_values()
    assert has.dtype == np.int32 and val.dtype == np.float64 and list(has) == [int(v) for N, v in terms] and val.shape == (len(terms), n)
    for f, (N, v) in enumerate(terms):
        assert same_bits(val[f], factors[f].values if v else np.zeros(n)), f       # bits: the -0.0 of "zeros and signs" comes back as -0.0
    assert engE.glm_factors() == (None, None) and engE.glm_factor_values() == (None, None)
    run_engines([engF, engE], chains, D, start_local(family, C_, Dx, H, J), shape)
    engF.close()
    engE.close()


def test_values_of_one_are_the_plain_term(idhmc):
    """term(idx, values=ones) against the plain term (idx, N) on "one tile" at n = 130, both terms: kSlopes kernels against section 20's,
    evaluation and leapfrog in the per-wave form and NUTS on the matrix cores"""
    shape = "one tile"
    family, Dd, terms, grouped, slab, D, L, form = SHAPES[shape]
    Dx, A, H, J = dims(shape)
    C_, n = 18, 130
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    idx = factors[0][0]
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    opt = idhmc.default_options(max_depth=4)
    engs = []
    for fac in ([(idx, 15), (idx, 15)], [(idx, 15), idhmc.glm.term(idx, values=np.ones(n), levels=15)],
                [idhmc.glm.term(idx, values=np.ones(n)), idhmc.glm.term(idx, values=np.ones(n), levels=15)]):
        m = models(idhmc, shape, X, Y, fac, grp, local, slab, kind, nu, mu, tau)[0]
        engs.append(idhmc.Engine(m, C_, opt, seed=3))
    assert engs[0].glm_factor_values() == (None, None) and list(engs[1].glm_factor_values()[0]) == [0, 1]
    assert list(engs[2].glm_factor_values()[0]) == [1, 1] and all(e.glm_form() == form for e in engs)
    assert engs[0].device_bytes() < engs[1].device_bytes() == engs[2].device_bytes()      # the values are counted
    run_engines(engs, None, D, start_local(family, C_, Dx, H, J), shape)
    for e in engs:
        e.close()


def test_responses_are_single_response_chains(idhmc, oracle, tmp_path):
    """M = 4 responses of R = 3 chains on "one tile": every chain is bit-identical to the single-response oracle chain on its Y and
    the expanded matrix (the same global chain id)"""
    shape = "one tile"
    family, Dd, terms, grouped, slab, D, L, form = SHAPES[shape]
    Dx, A, H, J = dims(shape)
    M, R, n = 4, 3, 130
    X, Y0, factors, grp, local, slab = problem(idhmc, shape, n)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [rng.poisson(np.maximum(Y0, 0.5)).astype(float) for _ in range(M - 1)])[:, :, None]
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    mF, mE = models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, chains_per_response=R)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(mF, M * R, opt, seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form and list(eng.glm_factor_values()[0]) == [0, 1]
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


def test_warmup_matches_the_expanded_engine(idhmc):
    """a 40-transition warm-up with per-chain adaptation on "tile aligned", then 8 draws: the same stepsizes, metric, draws and records"""
    shape = "tile aligned"
    family, Dd, terms, grouped, slab, D, L, form = SHAPES[shape]
    Dx, A, H, J = dims(shape)
    C_, N = 8, 8
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 130)
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
    """mcmc_summary on "one tile": every field of the device summary of [beta | sigma] equals the expanded engine's"""
    shape = "one tile"
    family, Dd, terms, grouped, slab, D, L, form = SHAPES[shape]
    Dx, A, H, J = dims(shape)
    C_, N, G, bins = 16, 6, 8, 16
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 130)
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


def test_plain_models_through_the_new_entry_point(idhmc):
    """factors=[(idx, N)] through idhmc_create_glm_slopes with values = NULL, and with every flag 0, against the same model through
    idhmc_create_glm_factors: the same form, footprint and bits"""
    from inplacedhmc_jl_amd import _lib
    shape = "tile aligned"
    family, Dd, terms, grouped, slab, D, L, form = SHAPES[shape]
    Dx, A, H, J = dims(shape)
    C_, n = 18, 130
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    plain = [(factors[0][0], 7), (factors[1].index, 50)]
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    m = models(idhmc, shape, X, Y, plain, grp, local, slab, kind, nu, mu, tau)[0]
    assert m.factor_has is None
    opt = idhmc.default_options(max_depth=4)
    lib = idhmc.load_library()
    zeros = np.zeros(2, np.int32)
    engs = [idhmc.Engine(m, C_, opt, seed=3)]
    for fv in (None, _lib.GlmFactorValues(values=None, has=zeros.ctypes.data_as(C.POINTER(C.c_int32)))):
        desc = m.glm_desc()
        pr = _lib.GlmPriors(kind=m.prior_kind.ctypes.data_as(C.POINTER(C.c_int32)), nu=m.prior_nu.ctypes.data_as(C.POINTER(C.c_double)))
        fc = _lib.GlmFactors(F=m.F, levels=m.levels.ctypes.data_as(C.POINTER(C.c_int32)), index=m.factor_index.ctypes.data_as(C.POINTER(C.c_int32)))
        h = C.c_void_p()
        _lib.check(lib.idhmc_create_glm_slopes(C.byref(h), 0, C_, 0, C.byref(desc), C.byref(pr), None, C.byref(fc),
                                               None if fv is None else C.byref(fv), 1, 0, C.byref(opt), 3))
        eng = idhmc.Engine._adopt(m, h, C_, opt)     # an Engine around that context
        engs.append(eng)
    for e in engs:
        assert e.glm_form() == form and e.glm_factor_values() == (None, None) and list(e.glm_factors()[0]) == [7, 50]
    assert engs[0].device_bytes() == engs[1].device_bytes() == engs[2].device_bytes()
    run_engines(engs, None, D, start_local(family, C_, Dx, H, J), shape)
    for e in engs:
        e.close()
