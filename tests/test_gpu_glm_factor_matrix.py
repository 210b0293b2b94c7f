"""Factor and slope terms (DESIGN sections 20 and 21) on the device, on the table of tests/test_glm_factor_matrix_cpu.py: the stored
widths Lx = 256, 384 and Lx = L, four blocks of observations (n = 385), four terms, and on the matrix cores auxiliary coordinates (one
at L = 256, four with K = 2), local scales with and without a slab, H = 4 and a model with no prior table at all.  The contract is the
one of tests/test_gpu_glm_factors.py and tests/test_gpu_glm_slopes.py, bit-identity with the same model on glm.expand_factors: an engine
on the expanded matrix, which runs the kernels that know nothing of factors, and oracle chains on section 19's C restatement fed the
expanded matrix.  No tolerance anywhere but in test_device_density_against_numpy, which compares the device with numpy directly, through
no expansion and no twin.  Then three workgroups, a shared metric, several responses in the per-wave form, a warm-up with per-response
stepsize and metric, and the device summaries.  Every context compiles its source with hipRTC, so engines are shared across
assertions."""
import dataclasses

import numpy as np
import pytest

from test_glm_factor_matrix_cpu import NS, SHAPES, dims, index_and_values, indicator_matrix, models, oracle_model, priors, problem
from test_glm_local_cpu import numpy_density_local, start_local
from test_gpu_glm_factors import SHORT, same_bits
from test_gpu_glm_slopes import run_engines

pytestmark = pytest.mark.gpu


def engines(idhmc, shape, n, C_, opt, seed=3, **kw):
    """(the factor engine, the engine on the expansion, what problem() and priors() returned)"""
    data = problem(idhmc, shape, n)
    pri = priors(shape)
    mF, mE = models(idhmc, shape, *data, *pri, **kw)
    return idhmc.Engine(mF, C_, opt, seed=seed), idhmc.Engine(mE, C_, opt, seed=seed), data, pri


def oracle_chains(oracle, tmp_path, shape, data, pri, C_, seed=3, **opt):
    X, Y, factors, grp, local, slab = data
    om = oracle_model(oracle, tmp_path, shape, indicator_matrix(shape, X, factors), Y, grp, local, slab, *pri)
    return [oracle.OracleChain(om, oracle.default_options(**opt), seed=seed, chain_id=c) for c in range(C_)]


def check_what_the_engines_hold(engF, engE, shape, data, n):
    family, Dd, terms, grouped, loc, pk, D, L, Lx, form = SHAPES[shape]
    X, Y, factors, grp, local, slab = data
    assert engF.glm_form() == engE.glm_form() == form and engF.padded_dim() == engE.padded_dim() == L and engF.D == engE.D == D
    lev, idx = engF.glm_factors()
    assert lev.dtype == idx.dtype == np.int32 and list(lev) == [N for N, v in terms]
    assert np.array_equal(idx, [i for i, w in index_and_values(factors)])
    has, val = engF.glm_factor_values()
    if any(v for N, v in terms):
        assert has.dtype == np.int32 and val.dtype == np.float64 and list(has) == [int(v) for N, v in terms] and val.shape == (len(terms), n)
        for f, (i, w) in enumerate(index_and_values(factors)):
            assert same_bits(val[f], np.zeros(n) if w is None else w), f       # bits: a -0.0 comes back as -0.0
    else:
        assert (has, val) == (None, None)
    assert engE.glm_factors() == (None, None) and engE.glm_factor_values() == (None, None)
    assert engF.device_bytes() < engE.device_bytes() or Lx == L


CASES = [(s, n) for s in SHAPES for n in NS] + [("four terms coop", 1)]


@pytest.mark.parametrize("shape,n", CASES)
def test_density_leapfrog_and_nuts(idhmc, oracle, tmp_path, shape, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the shape runs: the bits of the engine on the expanded matrix and of the oracle chains
    on it.  "aux 4, K 2" goes through the C restatement and numpy like every other row (tests/test_glm_factor_matrix_cpu.py)"""
    family, D = SHAPES[shape][0], SHAPES[shape][6]
    Dx, A, H, J = dims(shape)
    C_ = 18
    engF, engE, data, pri = engines(idhmc, shape, n, C_, idhmc.default_options(max_depth=4))
    check_what_the_engines_hold(engF, engE, shape, data, n)
    chains = oracle_chains(oracle, tmp_path, shape, data, pri, C_, max_depth=4)
    run_engines([engF, engE], chains, D, start_local(family, C_, Dx, H, J), (shape, n))
    engF.close()
    engE.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_density_against_numpy(idhmc, shape):
    """lq and grad of the factor engine after set_q at n = 385 against numpy on the matrix built in the test from the definition, within
    1e-12 of the magnitude of the terms summed (the bound of the restatement's twin, tests/test_glm_local_cpu.py): the device against
    something that passes through no expansion and no twin"""
    family, D, form = SHAPES[shape][0], SHAPES[shape][6], SHAPES[shape][9]
    Dx, A, H, J = dims(shape)
    C_, n = 18, 385
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    kind, nu, mu, tau = priors(shape)
    eng = idhmc.Engine(models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)[0], C_, idhmc.default_options(max_depth=4), seed=3)
    q = start_local(family, C_, Dx, H, J)
    eng.set_q(q)
    lq, g = eng.lq, eng.grad
    assert eng.poll_abort() == 0 and eng.glm_form() == form
    eng.close()
    E = indicator_matrix(shape, X, factors)
    for c in range(C_):
        l_ref, g_ref, lscale, gscale = numpy_density_local(family, E, Y, q[c], grp, local, slab, kind, nu, mu, tau)
        print(shape, c, abs(lq[c] - l_ref) / lscale, np.max(np.abs(g[c] - g_ref) / (gscale + 1e-300)))
        assert abs(lq[c] - l_ref) <= 1e-12 * lscale, (c, lq[c], l_ref)
        assert np.all(np.abs(g[c] - g_ref) <= 1e-12 * gscale + 1e-300), (c, np.max(np.abs(g[c] - g_ref) / (gscale + 1e-300)))


def test_three_workgroups(idhmc):
    """"aux at 256" with 33 chains at n = 385: two full 16-chain tiles and one that holds a single chain, against the expanded engine"""
    shape, C_, n = "aux at 256", 33, 385
    family, D = SHAPES[shape][0], SHAPES[shape][6]
    Dx, A, H, J = dims(shape)
    engF, engE, data, pri = engines(idhmc, shape, n, C_, idhmc.default_options(max_depth=4))
    check_what_the_engines_hold(engF, engE, shape, data, n)
    run_engines([engF, engE], None, D, start_local(family, C_, Dx, H, J), shape)
    engF.close()
    engE.close()


@pytest.mark.parametrize("shape", ["bare", "wide coop"])
def test_shared_metric(idhmc, oracle, tmp_path, shape):
    """metric_mode = METRIC_SHARED at n = 385: the factor engine against the expanded engine under the same option, and against the oracle
    chains (the unit metric is the same metric shared or per chain, tests/test_gpu_dense.py)"""
    family, D = SHAPES[shape][0], SHAPES[shape][6]
    Dx, A, H, J = dims(shape)
    C_, n = 18, 385
    engF, engE, data, pri = engines(idhmc, shape, n, C_, idhmc.default_options(max_depth=4, metric_mode=idhmc.METRIC_SHARED))
    check_what_the_engines_hold(engF, engE, shape, data, n)
    assert same_bits(engF.minv, np.ones_like(engF.minv))
    chains = oracle_chains(oracle, tmp_path, shape, data, pri, C_, max_depth=4)
    run_engines([engF, engE], chains, D, start_local(family, C_, Dx, H, J), shape)
    engF.close()
    engE.close()


def test_responses_per_wave(idhmc, oracle, tmp_path):
    """M = 3 responses of R = 2 chains on "Lx 256 of 512" at n = 130 (GlmWave::bind_chain with the level planes): every chain is
    bit-identical to the single-response oracle chain on its Y and the expanded matrix (the same global chain id)"""
    shape = "Lx 256 of 512"
    family, D, form = SHAPES[shape][0], SHAPES[shape][6], SHAPES[shape][9]
    Dx, A, H, J = dims(shape)
    M, R, n = 3, 2, 130
    X, Y0, factors, grp, local, slab = problem(idhmc, shape, n)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [Y0 + 0.3 * rng.standard_normal(n) for _ in range(M - 1)])[:, :, None]
    pri = priors(shape)
    mF = models(idhmc, shape, X, Y, factors, grp, local, slab, *pri, chains_per_response=R)[0]
    eng = idhmc.Engine(mF, M * R, idhmc.default_options(max_depth=4), seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form == 0 and list(eng.glm_factor_values()[0]) == [1, 0]
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
    E = indicator_matrix(shape, X, factors)
    for m in range(M):
        om = oracle_model(oracle, tmp_path, shape, E, Y[m], grp, local, slab, *pri)
        for c in range(R * m, R * m + R):
            ch = oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=13, chain_id=c)
            ch.set_q(q[c])
            ch.sample_tree(eps, 1)
            assert same_bits(q1[c], ch.q[:D]), c
            ch.sample_tree(eps, 2)
            ch.sample_tree(eps, 3)
            assert same_bits(q3[c], ch.q[:D]) and same_bits(lq3[c], ch.lq) and same_bits(g3[c], ch.grad[:D]), c


def test_warmup_with_pooling(idhmc):
    """"wide coop" at n = 385 with M = 2 responses of R = 4 chains, stepsize and metric pooled per response: a
    40-transition warm-up, then 8 draws: the stepsizes, metric, draws, records, lq and grad of the expanded engine"""
    shape = "wide coop"
    form = SHAPES[shape][9]
    M, R, n, N = 2, 4, 385, 8
    X, Y0, factors, grp, local, slab = problem(idhmc, shape, n)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0, rng.poisson(np.maximum(Y0, 0.5)).astype(float)])[:, :, None]
    opt = idhmc.default_options(eps_mode=idhmc.EPS_PER_RESPONSE, metric_mode=idhmc.METRIC_PER_RESPONSE, **SHORT)
    out = []
    for m in models(idhmc, shape, X, Y, factors, grp, local, slab, *priors(shape), chains_per_response=R):
        eng = idhmc.Engine(m, M * R, opt, seed=77)
        draws, stats_ = eng.mcmc_with_warmup(N)
        out.append((draws, stats_, eng.eps, eng.minv, eng.lq, eng.grad))
        assert eng.poll_abort() == 0 and eng.glm_form() == form and eng.glm_responses() == (M, R)
        eng.close()
    a, b = out
    assert np.isfinite(a[0]).all()
    eps, minv = a[2].reshape(M, R), a[3].reshape(M, R, -1)
    assert np.all(eps == eps[:, :1]) and eps[0, 0] != eps[1, 0] and np.all(minv == minv[:, :1]) and not np.array_equal(minv[0, 0], minv[1, 0])
    assert same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert same_bits(a[4], b[4]) and same_bits(a[5], b[5])


def test_summary_on_a_wide_model(idhmc):
    """mcmc_summary on "four terms wave" at n = 130: every field of the device summary equals the expanded engine's"""
    shape = "four terms wave"
    family, D = SHAPES[shape][0], SHAPES[shape][6]
    Dx, A, H, J = dims(shape)
    C_, N, G, bins = 16, 6, 8, 16
    q0 = start_local(family, C_, Dx, H, J)
    engs = engines(idhmc, shape, 130, C_, idhmc.default_options(max_depth=4), seed=21)[:2]
    out = []
    for eng in engs:
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
