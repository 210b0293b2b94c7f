"""The control path: a driver that returns IDHMC_OK must have run what it was asked to run.  A device-side error that is still pending
when a driver starts -- the abort word and a chain's status left set by a refused launch of several transitions, or by a caller's own
transition whose dual averaging drove eps below 1e-10 -- must be reported by that driver (and cleared), on every launch path: a launch of
several transitions hands out no transition at all while the abort word is set, so a driver that only synchronises returns success with
draws that were never written.  After the report the context continues exactly from the state its chains hold.

Errors are armed in two ways only, both diagonal / isotropic models (no abort is ever raised in a fused launch of a dense model):
  xcd       - IDHMC_TEST_XCC_MISMATCH=1 at creation lets transition flag bit 30 make the workgroups of one chain range report different
              XCD ids; the kernel refuses the launch (IDHMC_ERR_HIP), as tests/test_gpu_fused.py does.
  underflow - dual averaging with da_gamma = 1e-9 from q = 1e6 drives eps below 1e-10 (IDHMC_ERR_EPS_UNDERFLOW), as
              tests/test_gpu_edges.py does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

XCD_D, XCD_C = 40, 600          # 38 workgroups: every chain range has workgroups b and b + 8
UF_D, UF_C = 8, 2


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def xcd_engine(idhmc, monkeypatch, opt=None, opt_in=True):
    if opt_in:
        monkeypatch.setenv("IDHMC_TEST_XCC_MISMATCH", "1")
    else:
        monkeypatch.delenv("IDHMC_TEST_XCC_MISMATCH", raising=False)
    rng = np.random.default_rng(4)
    model = idhmc.DiagGaussian(rng.standard_normal(XCD_D), np.exp(rng.standard_normal(XCD_D)))
    eng = idhmc.Engine(model, XCD_C, opt if opt is not None else idhmc.default_options(max_depth=7), seed=9)
    eng.random_position()
    eng.set_eps(0.3)
    return eng


def arm_xcd(idhmc, eng):
    eng.nuts_transitions(1, 3, 1 << 30)
    assert eng.poll_abort(0) == idhmc.ERR_HIP
    return idhmc.ERR_HIP


def underflow_engine(idhmc):
    eng = idhmc.Engine(idhmc.IsoGaussian(UF_D), UF_C, idhmc.default_options(max_depth=2, da_gamma=1e-9), seed=1)
    eng.set_q(np.full((UF_C, UF_D), 1e6))
    eng.set_eps(1.0)
    return eng


def arm_underflow(idhmc, eng):
    eng.da_init()
    for it in range(1, 60):
        eng.nuts_transition(it, idhmc.T_ADAPT_EPS)
        if eng.poll_abort(0) != 0:
            break
    assert eng.poll_abort(0) == idhmc.ERR_EPS_UNDERFLOW
    return idhmc.ERR_EPS_UNDERFLOW


def armed(idhmc, monkeypatch, kind, fuse):
    """an engine with a pending device error of `kind`; fuse=False: IDHMC_FUSE=0 (one launch per transition in the drivers)"""
    if fuse:
        monkeypatch.delenv("IDHMC_FUSE", raising=False)
    else:
        monkeypatch.setenv("IDHMC_FUSE", "0")
    if kind == "xcd":
        eng = xcd_engine(idhmc, monkeypatch)
        code = arm_xcd(idhmc, eng)
    else:
        eng = underflow_engine(idhmc)
        code = arm_underflow(idhmc, eng)
    assert eng.fused_launch_info() == (True, fuse)
    return eng, code


# idhmc_mcmc's launch paths: (N, store_draws, store_stats, drivers fuse)
MCMC_PATHS = {
    "fused_one_launch": (3, False, False, True),            # one idhmc_nuts_transitions launch
    "blocks_draws_stats": (70, True, True, True),           # run_blocks, K = 64: a ragged last block
    "blocks_draws": (70, True, False, True),
    "blocks_stats": (70, False, True, True),
    "per_transition": (3, True, True, False),               # IDHMC_FUSE=0
    "single_transition": (1, True, True, True),
}


@pytest.mark.parametrize("path", list(MCMC_PATHS))
@pytest.mark.parametrize("kind", ["xcd", "underflow"])
def test_mcmc_reports_a_pending_error_on_every_path(idhmc, monkeypatch, kind, path):
    N, store_draws, store_stats, fuse = MCMC_PATHS[path]
    eng, code = armed(idhmc, monkeypatch, kind, fuse)
    with pytest.raises(idhmc.IdhmcError) as e:
        eng.mcmc(N, 100, store_draws=store_draws, store_stats=store_stats)
    assert e.value.code == code and "mcmc" in str(e.value)
    assert eng.poll_abort(0) == 0                    # reported once, then cleared
    steps = eng.total_steps()
    draws, stats = eng.mcmc(N, 100, store_draws=store_draws, store_stats=store_stats)
    # the same call now runs every transition of every chain: each one takes at least one leapfrog step
    assert eng.total_steps() - steps >= N * eng.C
    if store_stats:
        assert (stats["steps"] >= 1).all()
    if store_draws:
        assert same_bits(draws[-1], eng.q)
    assert eng.poll_abort(0) == 0
    eng.close()


@pytest.mark.parametrize("kind", ["xcd", "underflow"])
def test_recovery_after_a_reported_error_is_exact(idhmc, monkeypatch, kind):
    """After the report the context goes on from whatever its chains hold: a fresh context loaded with the same q, eps and M^-1
    (same model, options, seed, first chain) gives the same draws, records and leapfrog count bit for bit.  Catches state a refused
    launch leaves dirty (range queues, XCD ids, per-chain transition counts, a stale gradient).  xcd: reported by the fused
    path; underflow: by the per-transition path (IDHMC_FUSE=0)."""
    fuse = kind == "xcd"
    eng, code = armed(idhmc, monkeypatch, kind, fuse)
    with pytest.raises(idhmc.IdhmcError) as e:
        eng.mcmc(3, 100, store_draws=False, store_stats=False)
    assert e.value.code == code
    q, eps, minv = eng.q, eng.eps, eng.minv
    fresh = xcd_engine(idhmc, monkeypatch) if kind == "xcd" else underflow_engine(idhmc)
    assert fresh.fused_launch_info() == (True, fuse)
    fresh.set_q(q)
    fresh.set_eps(eps)
    fresh.set_minv(minv)
    assert same_bits(fresh.q, q) and same_bits(fresh.eps, eps) and same_bits(fresh.minv, minv)
    N = 5
    s0, s1 = eng.total_steps(), fresh.total_steps()
    d0, r0 = eng.mcmc(N, 200)
    d1, r1 = fresh.mcmc(N, 200)
    assert same_bits(d0, d1)
    assert np.array_equal(r0, r1)
    assert eng.total_steps() - s0 == fresh.total_steps() - s1 >= N * eng.C
    assert same_bits(eng.q, fresh.q)
    eng.close()
    fresh.close()


DRIVERS = ["tuning_stage_blocks", "tuning_stage_per_transition", "tuning_stage_global_eps", "find_initial_stepsize_per_chain",
           "mcmc_with_warmup"]


@pytest.mark.parametrize("driver", DRIVERS)
def test_every_driver_reports_a_pending_error(idhmc, monkeypatch, driver):
    """the other drivers: a pending refusal is reported (IDHMC_ERR_HIP) and cleared, and the same call then succeeds"""
    short = dict(max_depth=5, init_steps=3, middle_steps=4, doubling_stages=1, terminating_steps=3)
    if driver == "tuning_stage_per_transition":
        monkeypatch.setenv("IDHMC_FUSE", "0")
    else:
        monkeypatch.delenv("IDHMC_FUSE", raising=False)
    if driver == "tuning_stage_global_eps":
        opt = idhmc.default_options(max_depth=7, eps_mode=idhmc.EPS_GLOBAL)
    elif driver == "mcmc_with_warmup":
        opt = idhmc.default_options(**short)
    else:
        opt = idhmc.default_options(max_depth=7)
    eng = xcd_engine(idhmc, monkeypatch, opt)
    arm_xcd(idhmc, eng)
    call = {
        "tuning_stage_blocks": lambda: eng.tuning_stage(4, False, 10, store_stats=True),
        "tuning_stage_per_transition": lambda: eng.tuning_stage(4, False, 10, store_stats=False),
        "tuning_stage_global_eps": lambda: eng.tuning_stage(4, False, 10, store_stats=False),
        "find_initial_stepsize_per_chain": lambda: (eng.refresh_momentum(0), eng.find_initial_stepsize()),
        "mcmc_with_warmup": lambda: eng.mcmc_with_warmup(3),
    }[driver]
    with pytest.raises(idhmc.IdhmcError) as e:
        call()
    assert e.value.code == idhmc.ERR_HIP
    assert eng.poll_abort(0) == 0
    call()
    assert eng.poll_abort(0) == 0
    eng.close()


def test_transition_flags_outside_the_documented_set_are_refused(idhmc, monkeypatch):
    """only the IDHMC_T_* bits pass idhmc_nuts_transition(s); bit 30 (the XCD test) only on a context created with
    IDHMC_TEST_XCC_MISMATCH=1.  A refused call changes nothing: no abort, same q, no leapfrog step"""
    documented = (idhmc.T_ADAPT_EPS | idhmc.T_ACCUM_METRIC | idhmc.T_ACCUM_MOMENTS | idhmc.T_KEEP_P | idhmc.T_USE_DIRECTIONS
                  | idhmc.T_ACCUM_DIAG)
    assert documented == 63
    eng = xcd_engine(idhmc, monkeypatch, opt_in=False)
    eng.nuts_transitions(1, 3)
    q0, steps0 = eng.q, eng.total_steps()
    bad = [1 << 30, 1 << 6, 1 << 7, 1 << 16, 1 << 29, 1 << 31, 0xFFFFFFFF & ~documented, (1 << 30) | idhmc.T_ACCUM_DIAG]
    for flags in bad:
        for call in (lambda: eng.nuts_transition(4, flags), lambda: eng.nuts_transitions(4, 3, flags)):
            with pytest.raises(idhmc.IdhmcError) as e:
                call()
            assert e.value.code == idhmc.ERR_BAD_ARG
    assert eng.poll_abort(0) == 0
    assert same_bits(eng.q, q0) and eng.total_steps() == steps0
    eng.close()
    # with the opt-in bit 30 passes (tests/test_gpu_fused.py uses it); nothing else outside the set does
    eng = xcd_engine(idhmc, monkeypatch, opt_in=True)
    eng.nuts_transition(1, 1 << 30)                  # (one transition per launch: no hand-over, nothing to check)
    assert eng.poll_abort(0) == 0
    with pytest.raises(idhmc.IdhmcError) as e:
        eng.nuts_transitions(2, 3, (1 << 30) | (1 << 29))
    assert e.value.code == idhmc.ERR_BAD_ARG
    eng.close()
