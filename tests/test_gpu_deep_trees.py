"""Deep trees and a non-default min_delta on every form of k_nuts: the runs of tests/test_deep_trees_cpu.py on the device.  That module
runs each of them through the CPU oracle and asserts what the oracle's records reach -- every tree depth from 3 to max_depth (10, 12,
and 13 to 15 in the two runs at the largest depth idhmc_create accepts), trees that stop at max_depth, doublings of 64 and more leaves
stopped by a turning sub-tree, divergences inside long doublings under a tight min_delta, and depths 6 and more apart among the 16
chains of one workgroup.  Here the engine starts where the oracle's chains start, at the same per-chain stepsizes, and every record,
draw, log density and gradient must be the oracle's: integers equal, doubles bit for bit.  No tolerance appears in this module."""
import numpy as np
import pytest

from test_deep_trees_cpu import CASES, DEFAULT_MIN_DELTA, RUNS, T_FUSED, T_SINGLE, oracle_run, problem, run_id, stepsizes

pytestmark = pytest.mark.gpu

DEVICE_RUNS = [run + (False,) for run in RUNS] + [run + (True,) for run in RUNS if CASES[run[0]]["shared"]]


def device_run_id(run):
    return run_id(run[:3]) + ("/shared" if run[3] else "")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: %r against %r" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                               want[tuple(bad[0])])


def assert_records_equal(got, want, what):
    for f in ("depth", "steps", "term_left", "term_right"):
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s %s: chains %s have %s against %s (depths of the oracle's trees: %s)" % (
            what, f, bad.tolist(), got[f][bad].tolist(), want[f][bad].tolist(), want["depth"].tolist())
    assert_same_bits(got["pi"], want["pi"], what + " pi")
    assert_same_bits(got["acceptance_rate"], want["acceptance_rate"], what + " acceptance_rate")


def create(idhmc, name, max_depth, min_delta, shared):
    """the engine of a run at the start and stepsizes of the oracle's chains, in the form the case is there for"""
    prob, case, ref = problem(name), CASES[name], oracle_run(name, max_depth, min_delta)
    opt = dict(max_depth=max_depth, min_delta=min_delta)
    if shared:
        opt["metric_mode"] = idhmc.METRIC_SHARED
    eng = idhmc.Engine(prob["engine"](idhmc), case["C"], idhmc.default_options(**opt), seed=case["seed"])
    assert eng.padded_dim() == prob["padded"] and eng.glm_form() == prob["form"], (eng.padded_dim(), eng.glm_form())
    if prob["start"] is None:
        eng.random_position()
    else:
        eng.set_q(ref["start"])
    assert_same_bits(eng.q, ref["start"], "start")
    eng.set_eps(stepsizes(name))
    return eng, ref


@pytest.mark.parametrize("run", DEVICE_RUNS, ids=device_run_id)
def test_deep_trees_are_the_oracles(idhmc, run):
    """T_SINGLE launches of one transition, every record and state compared after each; then one launch of T_FUSED transitions (the
    hand-over between workgroups with trees of a few and of a thousand leaves in one queue) against the oracle's next T_FUSED"""
    name, max_depth, min_delta, shared = run
    eng, ref = create(idhmc, name, max_depth, min_delta, shared)
    for t in range(T_SINGLE):
        eng.nuts_transition(t + 1)
        what = "%s, transition %d:" % (device_run_id(run), t + 1)
        assert_records_equal(eng.tree_stats(), ref["rec"][t], what)
        assert_same_bits(eng.q, ref["q"][t], what + " q")
        assert_same_bits(eng.lq, ref["lq"][t], what + " lq")
    assert_same_bits(eng.grad, ref["grad"][T_SINGLE - 1], "grad after %d transitions" % T_SINGLE)
    assert eng.total_steps() == int(ref["rec"]["steps"][:T_SINGLE].sum(dtype=np.int64))
    eng.nuts_transitions(T_SINGLE + 1, T_FUSED)
    what = "%s, after one launch of %d transitions:" % (device_run_id(run), T_FUSED)
    assert_records_equal(eng.tree_stats(), ref["rec"][-1], what)
    assert_same_bits(eng.q, ref["q"][-1], what + " q")
    assert_same_bits(eng.lq, ref["lq"][-1], what + " lq")
    assert_same_bits(eng.grad, ref["grad"][-1], what + " grad")
    assert eng.total_steps() == int(ref["rec"]["steps"].sum(dtype=np.int64))
    assert eng.poll_abort() == 0
    eng.close()


@pytest.mark.parametrize("fuse", ["0", "1"])
@pytest.mark.parametrize("name", ["logistic_mc128", "dense_coop128"])
@pytest.mark.parametrize("min_delta", ["default", "tight"])
def test_deep_trees_through_the_sampling_driver(idhmc, monkeypatch, name, fuse, min_delta):
    """mcmc(N = 4) with one launch per transition (IDHMC_FUSE=0) and with the fused driver: the draws and records that reach the host"""
    delta = DEFAULT_MIN_DELTA if min_delta == "default" else CASES[name]["tight"]
    monkeypatch.setenv("IDHMC_FUSE", fuse)
    eng, ref = create(idhmc, name, 10, delta, False)
    monkeypatch.delenv("IDHMC_FUSE")
    assert eng.fused_launch_info() == (True, fuse == "1")
    draws, records = eng.mcmc(T_SINGLE, 0)
    for t in range(T_SINGLE):
        assert_records_equal(records[t], ref["rec"][t], "%s, IDHMC_FUSE=%s, draw %d:" % (name, fuse, t + 1))
        assert_same_bits(draws[t], ref["q"][t], "draw %d" % (t + 1))
    assert_same_bits(eng.q, ref["q"][T_SINGLE - 1], "q")
    assert_same_bits(eng.grad, ref["grad"][T_SINGLE - 1], "grad")
    assert eng.total_steps() == int(ref["rec"]["steps"][:T_SINGLE].sum(dtype=np.int64))
    eng.close()
