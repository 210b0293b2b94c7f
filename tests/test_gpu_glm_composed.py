"""Correlated pairs, structured terms and GMRF terms (DESIGN sections 22, 23 and 25) on the device, on the table of
tests/test_glm_composed_cpu.py: the shapes and flag combinations that tests/test_gpu_glm_corr.py, tests/test_gpu_glm_struct.py and
tests/test_gpu_glm_gmrf.py never execute -- L = 1024 (NCH = 8) with each feature, the scan's h = 512 stage, two sampled phi with the larger
term in slot 1, GMRF members in chunks j >= 4, more than 128 AR(1) levels and four blocks of observations on the matrix cores,
kStruct && kLocal && !kCorr, kGmrf && kLocal, kCorr && kStruct && kGmrf with A = 1 and local scales on the matrix cores, two pairs
across column 128 with D = L, the per-wave NUTS kernel at NCH = 2, and the summary kernels' pair mix, local scales with the slab, second
slot, A > 0 offsets, stages h >= 64 and a wavefront that is not live.  Every assertion against the oracle is bit identity; the C twin is
section 25's restatement, which tests/test_glm_composed_cpu.py holds within 1e-12 of numpy on these rows.  Every context compiles its
source with hipRTC, so engines are shared across assertions."""
import numpy as np
import pytest

from test_glm_composed_cpu import (C_, SHAPES, assert_host_helpers, check_numpy, dims, gmrf_columns, model, options, oracle_model, problem,
                                   shape_priors, stages, start, struct_columns, theta_of_shape)
from test_glm_factor_matrix_cpu import coop
from test_glm_priors_cpu import NORMAL
from test_gpu_glm_factors import SHORT, same_bits
from test_gpu_glm_slopes import run_engines
from test_gpu_summary import assert_histogram, assert_summary
from test_summary_cpu import range_twin, summary_twin

pytestmark = pytest.mark.gpu


def setup(idhmc, shape, n=None):
    X, Y, factors, grp, local, slab = problem(idhmc, shape, SHAPES[shape][11] if n is None else n)
    return (X, Y, factors, grp, local, slab) + shape_priors(shape)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_density_leapfrog_search_and_nuts(idhmc, oracle, tmp_path, shape):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the row runs, then the stepsize search: bit-identical to 37 oracle chains on the C
    twin, within 1e-12 of numpy on chains 0 and 36.  The per-chain metric, but at L = 1024, where a GLM takes the shared one only"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    Dx, A, H, J, P, Sz = dims(shape)
    args = setup(idhmc, shape)
    m = model(idhmc, shape, *args)
    assert (m.D, m.Dx, m.J, m.P, m.S, m.Sz, m.G) == (D, Dx, J, P, len(structs), Sz, len(gmrfs))
    eng = idhmc.Engine(m, C_, options(idhmc, shape, max_depth=4), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, *args)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.padded_dim() == L and eng.D == D
    got = eng.glm_pairs()
    assert ([(int(a), int(b), float(e)) for a, b, e in zip(*got)] if P else got) == (list(pairs) if P else (None, None, None))
    got = eng.glm_structs()
    assert ([(int(a), int(b), float(e)) for a, b, e in zip(*got)] if structs else got) == (list(structs) if structs else (None, None, None))
    got = eng.glm_gmrfs()
    if gmrfs:
        assert [(int(a), float(b)) for a, b in zip(got[0], got[1])] == [(t, k) for t, qn, k in gmrfs]
        assert list(got[2]) == [np.count_nonzero(Q) for o, N, Q, k in gmrf_columns(idhmc, shape)]
    else:
        assert got == (None, None, None)
    loc_, slab_ = eng.glm_local()
    assert (slab_ == 2.0 and np.array_equal(loc_, args[4])) if J else (slab_ == 0.0 and not loc_.any())
    assert np.array_equal(eng.glm_priors()[0], args[6]) and np.array_equal(eng.glm_priors()[1], args[7])
    cn = (idhmc, eng, shape) + args + ((0, C_ - 1),)
    q = start(shape, C_)
    eng.set_q(q)
    check_numpy(*cn)
    run_engines([eng], chains, D, q, shape)
    check_numpy(*cn)
    eng.refresh_momentum(0)
    eng.find_initial_stepsize()
    ref = []
    for ch in chains:
        ch.rand_p(0)
        rc, e = ch.find_initial_stepsize()
        assert rc == 0
        ref.append(e)
    assert same_bits(eng.eps, ref) and eng.poll_abort() == 0
    eng.close()


@pytest.mark.parametrize("shape", ["everything 1024", "composed coop", "A4 per wave 256"])
def test_shared_metric(idhmc, oracle, tmp_path, shape):
    """the same stages on a shared unit metric (METRIC_SHARED: the other instantiation of the NUTS kernel).  A = 4 at L = 256 is the
    per-wave form under both metrics (the matrix cores take A <= 1 there, A = 2 with the shared metric); at L = 1024 the shared metric
    is the only one, so "everything 1024" repeats the instantiation of the test above from its own context"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    args = setup(idhmc, shape)
    eng = idhmc.Engine(model(idhmc, shape, *args), C_, idhmc.default_options(max_depth=4, metric_mode=idhmc.METRIC_SHARED), seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, shape, *args)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form == coop(L, dims(shape)[1], shared=True) and eng.padded_dim() == L
    if shape == "A4 per wave 256":
        assert form == 0 == coop(L, 4) and L == 256
    run_engines([eng], chains, D, start(shape, C_), shape)
    assert eng.poll_abort() == 0
    eng.close()


@pytest.mark.parametrize("shape", ["two ar1 coop", "two ar1 two gmrf 1024"])
def test_zeta_zero_anchor(idhmc, oracle, tmp_path, shape):
    """The anchor of slot 1 to kernels that predate it: both zetas +0, eta = 0 and a normal entry on each.  lq and grad[:, :D - 2] are the
    bits of an engine on the same model without `structured` at the same leading coordinates: after evaluation (the per-wave form), and
    after a NUTS transition at eps = 1e-300, which moves nothing and leaves a state evaluated by the form the row runs in the NUTS
    kernel.  grad at both zetas is the twin's, and not zero"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    Dx, A, H, J, P, Sz = dims(shape)
    assert (P, Sz, len(structs)) == (0, 2, 2)
    X, Y, factors, grp, local, slab = problem(idhmc, shape, 37)
    kind, nu, mu, tau = shape_priors(shape, seta=[0.0, 0.0])
    kind[-2:], nu[-2:], mu[-2:], tau[-2:] = NORMAL, 0.0, 0.0, 1.5
    g = idhmc.glm
    opt = options(idhmc, shape, max_depth=4)
    engS = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, structured=[g.ar1(0, 0.0), g.ar1(1, 0.0)]), C_, opt, seed=3)
    engP = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind[:-2], nu[:-2], mu[:-2], tau[:-2], structured=None), C_, opt, seed=3)
    assert engS.glm_form() == engP.glm_form() == form and engS.D == engP.D + 2 == D and engP.glm_structs() == (None, None, None)
    assert [float(e) for e in engS.glm_structs()[2]] == [0.0, 0.0]
    om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, seta=[0.0, 0.0])
    q = start(shape, C_)
    q[:, -2:] = 0.0
    assert np.all(np.abs(q[:, :Dx]) > 1e-100) and not np.signbit(q[:, -2:]).any()
    engS.set_q(q)
    engP.set_q(q[:, :-2])

    def same_leading(stage):
        gS, gP = engS.grad, engP.grad
        assert same_bits(engS.lq, engP.lq) and same_bits(gS[:, :-2], gP), stage
        qS = engS.q
        assert same_bits(qS[:, :-2], q[:, :-2]) and same_bits(engP.q, q[:, :-2]), stage
        for c in range(C_):
            l_t, g_t = om.logdensity_and_gradient(qS[c])
            assert same_bits(g_t[:D], gS[c]) and same_bits(l_t, engS.lq[c]) and g_t[D - 1] != 0.0 and g_t[D - 2] != 0.0, (stage, c)
    same_leading("evaluation")
    for e in (engS, engP):
        e.set_eps(1e-300)
        e.nuts_transition(1)
        assert (e.tree_stats()["steps"] >= 1).all() and e.poll_abort() == 0
    assert np.all(np.abs(engS.q[:, -2:]) < 1e-290)
    same_leading("a transition that moves nothing")
    engS.close()
    engP.close()


def test_short_warmup_matches_oracle(idhmc, oracle, tmp_path):
    """a 40-transition warm-up with per-chain adaptation on "composed coop", then 8 draws: stepsizes, draws and records are the twin's"""
    shape = "composed coop"
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    chains, N = 8, 8
    args = setup(idhmc, shape)
    eng = idhmc.Engine(model(idhmc, shape, *args), chains, idhmc.default_options(**SHORT), seed=77)
    draws, stats_ = eng.mcmc_with_warmup(N)
    om = oracle_model(idhmc, oracle, tmp_path, shape, *args)
    rc, och, ost, oeps = oracle.threaded_mcmc(om, N, chains, oracle.default_options(**SHORT), seed=77)
    assert rc == 0 and same_bits(eng.eps, oeps) and len(np.unique(oeps)) > 1
    for k in range(N):
        assert same_bits(draws[k], och[:, k, :D])
    assert np.array_equal(stats_.T, ost[:, :N])
    assert eng.poll_abort() == 0 and eng.glm_form() == form
    eng.close()


# ---- the summaries --------------------------------------------------------------------------------------------------------------------
def planted(shape, chains, N):
    """N host draws of `chains` chains with zeta = 800, -40 and +0 (rho or phi = 1 exactly, nearly -1, +0) planted in every zeta"""
    Dx, A, H, J, P, Sz = dims(shape)
    draws = np.stack([start(shape, chains, seed=k) for k in range(N)])
    for z in range(1, P + Sz + 1):
        draws[0, 0, -z], draws[1, 1, -z], draws[min(2, N - 1), 2, -z] = 800.0, -40.0, 0.0
    return draws


def host_draws_against_the_twin(eng, draws, theta, G, bins, cut):
    """summary_add_draws one draw per call: draws[:cut], the range from their moments, draws[cut:]; moments, sign counts, extremes and the
    histogram against the host twins of theta"""
    chains, D = draws.shape[1:]
    eng.summary_begin(chains_per_group=G, bins=bins)
    assert eng.summary_dims() == (chains // G, G, D, bins)
    for k in range(cut):
        eng.summary_add_draws(draws[k:k + 1])
    eng.summary_set_range(span=3.0)
    for k in range(cut, draws.shape[0]):
        eng.summary_add_draws(draws[k:k + 1])
    got = eng.summary()
    assert_summary(got, summary_twin(theta, G), "host draws")
    s = summary_twin(theta[:cut], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 3.0, bins)
    assert_histogram(got, theta[cut:], G, lo, hi, "host draws")
    eng.summary_end()


def sampled_against_the_twin(idhmc, eng, shape, grp, local, slab, dexp, chains, N, G, bins):
    """the same transitions stored, then reduced on the device by mcmc_summary: against the twins of the stored draws, and the stored
    draws' theta against the host helpers"""
    q0 = start(shape, chains)
    eng.set_eps(0.02)
    eng.set_q(q0)
    stored, _ = eng.mcmc(N, 3, store_draws=True, store_stats=False)
    eng.set_q(q0)
    got = eng.mcmc_summary(N, 3, pilot=2, chains_per_group=G, bins=bins)
    th = theta_of_shape(stored, shape, grp, local, slab, dexp)
    assert np.all(got.n == N * G) and np.all(got.binned == (N - 2) * G)
    assert_summary(got, summary_twin(th, G), "mcmc_summary")
    s = summary_twin(th[:2], G)
    lo, hi, _ = range_twin(s["mean"], s["var"], 6.0, bins)
    assert_histogram(got, th[2:], G, lo, hi, "mcmc_summary")
    assert_host_helpers(idhmc, eng.model, shape, stored, th)


@pytest.mark.parametrize("shape", ["composed coop", "two ar1 coop", "two pairs local D=L"])
def test_summaries_of_the_reported_vector(idhmc, oracle, shape):
    """summary_add_draws of host draws, and one mcmc_summary, against theta_composed_twin.  15 chains in groups of 5, one draw per call:
    every call stages 15 rows, so the last workgroup of k_summary_struct_theta (two wavefronts, a row each) has a wavefront that is not
    live.  "composed coop": the pair's mix, the local scales with the slab on its second term, the offsets behind A = 1, six stages.
    "two ar1 coop": both slots with their own phi, eight stages, h up to 128 (a lane's c += 64 loop makes four trips).  "two pairs local
    D=L": k_summary_corr_theta's lp >= 0 branch next to pairs, the first term behind the second"""
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    chains, N, G, bins = 15, 6, 5, 16
    X, Y, factors, grp, local, slab, kind, nu, mu, tau = setup(idhmc, shape, 37)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau), chains, idhmc.default_options(max_depth=4), seed=21)
    dexp = oracle.lib().orc_exp_export
    draws = planted(shape, chains, N)
    assert draws[0:1].shape[0] * chains == 15 and 15 % 2 == 1                # the rows one call stages
    if structs:
        assert max(stages(N_) for o, N_, kd in struct_columns(shape)) == {"composed coop": 6, "two ar1 coop": 8}[shape]
    theta = theta_of_shape(draws, shape, grp, local, slab, dexp)
    Z = dims(shape)[4] + dims(shape)[5]
    assert Z == 2 and np.all(theta[0, 0, -Z:] == 1.0) and np.all((-1.0 <= theta[1, 1, -Z:]) & (theta[1, 1, -Z:] < -0.999)) and np.all(theta[2, 2, -Z:] == 0.0)
    host_draws_against_the_twin(eng, draws, theta, G, bins, 2)
    sampled_against_the_twin(idhmc, eng, shape, grp, local, slab, dexp, chains, N, G, bins)
    assert eng.poll_abort() == 0
    eng.close()


def test_summaries_at_1024(idhmc, oracle):
    """"two ar1 two gmrf 1024": two calls of one draw of 8 chains through k_summary_struct_theta with ten stages, h up to 512, the larger
    term in slot 1 and both phi sampled"""
    shape = "two ar1 two gmrf 1024"
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    chains, N, G, bins = 8, 2, 4, 16
    X, Y, factors, grp, local, slab, kind, nu, mu, tau = setup(idhmc, shape, 37)
    eng = idhmc.Engine(model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau), chains, options(idhmc, shape, max_depth=4), seed=21)
    draws = planted(shape, chains, N)
    theta = theta_of_shape(draws, shape, grp, local, slab, oracle.lib().orc_exp_export)
    assert [stages(N_) for o, N_, kd in struct_columns(shape)] == [8, 10] and theta[0, 0, -1] == theta[0, 0, -2] == 1.0
    host_draws_against_the_twin(eng, draws, theta, G, bins, 1)
    assert_host_helpers(idhmc, eng.model, shape, draws, theta)
    assert eng.poll_abort() == 0
    eng.close()


def test_responses_are_single_response_oracle_chains(idhmc, oracle, tmp_path):
    """M = 3 responses of R = 5 chains on "gmrf local 128": at a fixed eps every chain of responses 0 and 2 is bit-identical to the
    single-response oracle chain on its Y (the same global chain id)"""
    shape = "gmrf local 128"
    family, Dd, terms, groups, pairs, structs, gmrfs, loc, D, L, form, n = SHAPES[shape]
    M, R = 3, 5
    X, Y0, factors, grp, local, slab, kind, nu, mu, tau = setup(idhmc, shape)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [rng.poisson(np.maximum(Y0, 0.5)).astype(float) for _ in range(M - 1)])[:, :, None]
    full = model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, chains_per_response=R)
    opt, oopt = idhmc.default_options(max_depth=4), oracle.default_options(max_depth=4)
    eng = idhmc.Engine(full, M * R, opt, seed=13)
    assert eng.glm_responses() == (M, R) and eng.glm_form() == form and list(eng.glm_gmrfs()[1]) == [1.0] and eng.glm_local()[1] == 2.0
    q = start(shape, M * R)
    eng.set_q(q)
    eps = 0.02
    eng.set_eps(eps)
    eng.nuts_transition(1)
    q1 = eng.q
    eng.nuts_transitions(2, 2)
    q3, lq3, g3 = eng.q, eng.lq, eng.grad
    assert eng.poll_abort() == 0
    eng.close()
    for m in (0, 2):
        om = oracle_model(idhmc, oracle, tmp_path, shape, X, Y[m], factors, grp, local, slab, kind, nu, mu, tau)
        for c in range(R * m, R * m + R):
            ch = oracle.OracleChain(om, oopt, seed=13, chain_id=c)
            ch.set_q(q[c])
            ch.sample_tree(eps, 1)
            assert same_bits(q1[c], ch.q[:D]), c
            ch.sample_tree(eps, 2)
            ch.sample_tree(eps, 3)
            assert same_bits(q3[c], ch.q[:D]) and same_bits(lq3[c], ch.lq) and same_bits(g3[c], ch.grad[:D]), c
