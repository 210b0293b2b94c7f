"""Every option reaches every kernel that reads it: the option sets of tests/test_options_cpu.py on the device, against the CPU oracle
under the same options -- which that module holds against the numpy restatement, and shows to differ from the oracle under the default
options.  The stepsize search (k_stepsize_search: the separable Gaussians' instantiations and those of every other model) with
non-default a_min, a_max, eps0 and C and with both of its failures; dual averaging with non-default delta, gamma, kappa and t0 in the
NUTS kernel's epilogue (per-chain stepsizes, one launch per transition and fused) and in k_da_adapt_global; stepsize_search = 0,
eps_init and adapt_metric = 0 in mcmc_with_warmup.  min_delta is tests/test_gpu_deep_trees.py's.  Every comparison is of bits."""
import numpy as np
import pytest

from test_deep_trees_cpu import CASES, oracle_chains, oracle_models, problem
from test_options_cpu import (DA_N, DA_OPTIONS, DRIVER_N, DRIVER_OPTIONS, DRIVER_SEED, FAILURE_SETS, SEARCH_C, SEARCH_MODELS, SEARCH_SEED,
                              SEARCH_SETS, da_stage, diag_gaussian, iso32_chains, search_minv, search_model, search_oracle, search_start)

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the stepsize search ------------------------------------------------------------------------------------------------------------------
def search_engine(idhmc, name, **options):
    """16 chains at the starts, metrics and momenta of test_options_cpu.search_chains"""
    eng = idhmc.Engine(search_model(name)[1](idhmc), SEARCH_C, idhmc.default_options(**options), seed=SEARCH_SEED)
    eng.set_minv(search_minv(name))
    eng.set_q(search_start(name))
    eng.refresh_momentum(0)
    return eng


@pytest.mark.parametrize("sname", list(SEARCH_SETS))
@pytest.mark.parametrize("name", list(SEARCH_MODELS))
def test_search_options(idhmc, name, sname):
    rc, eps = search_oracle(name, **SEARCH_SETS[sname])
    assert not rc.any()
    eng = search_engine(idhmc, name, **SEARCH_SETS[sname])
    eng.find_initial_stepsize()
    got = eng.eps
    assert same_bits(got, eps), (got, eps)
    eng.close()


@pytest.mark.parametrize("fname", list(FAILURE_SETS))
@pytest.mark.parametrize("name", ["iso8", "custom128"])
def test_the_two_failures_of_the_search(idhmc, name, fname):
    """IDHMC_ERR_STEPSIZE_SEARCH from the crossing loop and from the bisection, in both kernels: raised once, with the text of the
    iteration limit; the chains whose search succeeded hold the oracle's eps; the context then goes on from the state its chains
    hold, bit for bit like a fresh one loaded with it (the shape of test_gpu_status.test_recovery_after_a_reported_error_is_exact)"""
    opts, code = FAILURE_SETS[fname]
    rc, eps = search_oracle(name, **opts)
    assert set(rc.tolist()) == {0, code}
    eng = search_engine(idhmc, name, max_depth=5, **opts)
    with pytest.raises(idhmc.IdhmcError) as e:
        eng.find_initial_stepsize()
    assert e.value.code == idhmc.ERR_STEPSIZE_SEARCH == 4 and "maximum number of iterations" in str(e.value)
    got = eng.eps
    assert same_bits(got[rc == 0], eps[rc == 0]), (got, eps, rc)
    q, minv = eng.q, eng.minv
    assert same_bits(q, search_start(name))
    eng.set_eps(np.where(rc == 0, got, 0.01))                    # (a failed chain's eps is no result: give it one)
    fresh = idhmc.Engine(search_model(name)[1](idhmc), SEARCH_C, idhmc.default_options(max_depth=5, **opts), seed=SEARCH_SEED)
    fresh.set_minv(minv)
    fresh.set_q(q)
    fresh.set_eps(eng.eps)
    d0, r0 = eng.mcmc(3, 100)                                    # succeeds: the error was reported once
    d1, r1 = fresh.mcmc(3, 100)
    assert same_bits(d0, d1) and np.array_equal(r0, r1) and eng.total_steps() == fresh.total_steps()
    eng.close()
    fresh.close()


def test_a_failed_search_stops_the_whole_schedule(idhmc, oracle):
    """mcmc_with_warmup from the random start: three doublings from eps0 = 1e-3 reach no chain's band"""
    opts = dict(FAILURE_SETS["crossing"][0], init_steps=4, middle_steps=4, doubling_stages=1, terminating_steps=4, max_depth=5)
    rc = oracle.threaded_mcmc(oracle.OracleModel.iso(8), 3, 4, oracle.default_options(**opts), seed=SEARCH_SEED)[0]
    assert rc == -1
    eng = idhmc.Engine(idhmc.IsoGaussian(8), 4, idhmc.default_options(**opts), seed=SEARCH_SEED)
    with pytest.raises(idhmc.IdhmcError) as e:
        eng.mcmc_with_warmup(3)
    assert e.value.code == idhmc.ERR_STEPSIZE_SEARCH and "maximum number of iterations" in str(e.value)
    eng.close()


# ---- dual averaging -----------------------------------------------------------------------------------------------------------------------
def da_case(idhmc, name, C_):
    """(engine model, oracle chains at their start, start [C][D], eps0, seed)"""
    if name == "iso32":
        chains = iso32_chains(C_, max_depth=7, **DA_OPTIONS)
        return idhmc.IsoGaussian(32), chains, np.stack([ch.q[:32].copy() for ch in chains]), 0.05, 9
    chains, q0 = oracle_chains(name, 7, -1000.0, nchains=C_)
    return problem(name)["engine"](idhmc), chains, q0, 0.02, CASES[name]["seed"]


@pytest.mark.parametrize("fuse", ["0", "1"])
@pytest.mark.parametrize("adapt_metric", [0, 1])
@pytest.mark.parametrize("name", ["iso32", "logistic_mc128", "custom128"])
def test_dual_averaging_options(idhmc, monkeypatch, name, adapt_metric, fuse):
    """tuning_stage(N = 20) under DA_OPTIONS: every draw and record (each tree is built at the eps the previous acceptance rates gave),
    the final eps and, with adapt_metric, M^-1 -- against the oracle's orc_da_adapt under the same options"""
    C_ = 18 if name == "logistic_mc128" else 6
    model, chains, q0, eps0, seed = da_case(idhmc, name, C_)
    ref = da_stage(chains, eps0, DA_N, **DA_OPTIONS)
    monkeypatch.setenv("IDHMC_FUSE", fuse)
    eng = idhmc.Engine(model, C_, idhmc.default_options(max_depth=7, **DA_OPTIONS), seed=seed)
    monkeypatch.delenv("IDHMC_FUSE")
    assert eng.fused_launch_info() == (True, fuse == "1")
    eng.set_q(q0)
    eng.set_eps(eps0)
    draws, stats = eng.tuning_stage(DA_N, adapt_metric, 0, store_draws=True, store_stats=True)
    assert same_bits(draws, ref["q"]) and np.array_equal(stats, ref["rec"])
    assert same_bits(eng.eps, ref["final"])
    assert same_bits(eng.minv, ref["minv"] if adapt_metric else np.ones_like(ref["minv"]))
    eng.close()


def test_dual_averaging_options_with_a_global_stepsize(idhmc, oracle):
    """EPS_GLOBAL on the iso Gaussian: k_da_adapt_global, fed the pooled mean of the acceptance rates (the exchange's fixed-point
    record), against orc_da_adapt fed xchg_mean of the same rates"""
    C_, eps0 = 16, 0.05
    chains = iso32_chains(C_, max_depth=7, **DA_OPTIONS)
    q0 = np.stack([ch.q[:32].copy() for ch in chains])
    used, final = oracle.global_eps_stage(chains, DA_N, 0, eps0, oracle.default_options(max_depth=7, **DA_OPTIONS))
    control = oracle.global_eps_stage(iso32_chains(C_, max_depth=7), DA_N, 0, eps0, oracle.default_options(max_depth=7))[1]
    assert final != control
    eng = idhmc.Engine(idhmc.IsoGaussian(32), C_, idhmc.default_options(max_depth=7, eps_mode=idhmc.EPS_GLOBAL, **DA_OPTIONS), seed=9)
    eng.set_q(q0)
    eng.set_eps(eps0)
    eng.tuning_stage(DA_N, False, 0)
    assert same_bits(eng.eps, np.full(C_, final)) and same_bits(eng.q, np.stack([ch.q[:32] for ch in chains]))
    eng.close()


# ---- the driver's own options ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diag100", "logistic_mc128"])
def test_the_drivers_own_options(idhmc, oracle, name):
    """mcmc_with_warmup with stepsize_search = 0, eps_init = 0.07 and adapt_metric = 0 against oracle.threaded_mcmc under the same"""
    C_ = 5
    if name == "diag100":
        mu, sig = diag_gaussian(100)
        model, om, D = idhmc.DiagGaussian(mu, sigma=sig), oracle.OracleModel.diag(mu, 1.0 / sig ** 2), 100
    else:
        model, om, D = problem(name)["engine"](idhmc), oracle_models(name)[0], problem(name)["D"]
    eng = idhmc.Engine(model, C_, idhmc.default_options(**DRIVER_OPTIONS), seed=DRIVER_SEED)
    draws, stats = eng.mcmc_with_warmup(DRIVER_N)
    rc, och, ost, oeps = oracle.threaded_mcmc(om, DRIVER_N, C_, oracle.default_options(**DRIVER_OPTIONS), seed=DRIVER_SEED)
    assert rc == 0 and same_bits(eng.eps, oeps)
    for n in range(DRIVER_N):
        assert same_bits(draws[n], och[:, n, :D]), n
    assert np.array_equal(stats.T, ost[:, :DRIVER_N])
    assert same_bits(eng.minv, np.ones((C_, D)))
    eng.close()
