"""The GLM observation sources, the prior rows, a pair's factors with the LKJ row and the slab at their edges on the device, input by
input ("GLM terms at their edges").  The sources first; the other tables go through the same two legs on the
single-response models tests/test_glm_terms_edges_cpu.py describes next to each of them.

Every table of tests/test_glm_terms_edges_cpu.py goes through the shipped kernels as a many-response GLM with one observation and one
column (n = 1, X = [[1.0]]: z = q0 exactly): data row m is response m, table row j is chain m R + j, so a chain's lq and grad are one
call of the source plus the 2^-1000 prior.  The device's bits are compared with the C twins (held to mpmath there) with no tolerance
and no row left out, in two legs per context:

  the per-wave form       set_q(table), then lq and grad against the oracle chains at the same rows; eng.q read back equals the table;
  the NUTS kernel's form  (the matrix cores at L = 128: glm_form() == 1 is asserted) one nuts_transition at eps = 2^-1000, a stepsize
                          set_eps accepts and at which a leaf cannot leave a start above 1e-285 in size, against the oracle chains
                          after sample_tree at the same stepsize: q, lq, grad, depth, steps; and on every row that came back with q
                          unchanged against the first leg's own lq and grad, form against form at the same input.

Rows past the docstring's ends start at lq = -inf: they take the first leg (and q, lq of the second, as
test_gpu_glm_aux.test_an_overflowing_chain_is_a_rejected_start has it) and the rest of their workgroup keeps its bits.  One context,
so one hipRTC build, per test."""
import time

import numpy as np
import pytest

import test_glm_terms_edges_cpu as E
import test_math_edges_cpu as T

pytestmark = pytest.mark.gpu


def first_difference(fam, what, got, want, rows=None, nan_equal=True):
    """None, or where whole rows of got and want first differ in raw bits"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    got, want = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    same = T.same_bits(got, want, nan_equal)
    if rows is not None:
        same = same | ~rows[:, None]
    if same.all():
        return None
    g, k = np.argwhere(~same)[0]
    return "%s %s: %d of %d values differ, first at chain %d (%s) component %d: device %r (%#018x), twin %r (%#018x)" % (
        fam.name, what, (~same).sum(), same.size, g, fam.describe(g), k, got[g, k], T.u64(got[g, k:k + 1])[0],
        want[g, k], T.u64(want[g, k:k + 1])[0])


class Case:
    """what first_difference names a chain by"""

    def __init__(self, name, describe):
        self.name, self.describe = name, describe


def both_legs(idhmc, case, model, chains, table, D, promised, form=1, share=0.9, padded=128):
    """the two legs of the module docstring for one context: `chains` are the oracle's, set to `table` already"""
    C_ = table.shape[0]
    oq, olq, og = (a.copy() for a in E.chain_state(chains, D))
    ost = [ch.sample_tree(E.EPS, 1) for ch in chains]
    oq2, olq2, og2 = E.chain_state(chains, D)
    t0 = time.perf_counter()
    eng = idhmc.Engine(model, C_, idhmc.default_options(max_depth=E.MAX_DEPTH), seed=E.SEED)
    t1 = time.perf_counter()
    try:
        got_form, L = eng.glm_form(), eng.padded_dim()
        eng.set_q(table)
        q1, lq1, g1 = eng.q, eng.lq, eng.grad
        eng.set_eps(E.EPS)
        eng.nuts_transition(1)
        q2, lq2, g2, st = eng.q, eng.lq, eng.grad, eng.tree_stats()
        abort = eng.poll_abort()
    finally:
        eng.close()
    print("%s: %d chains, hipRTC build %.2f s, both legs %.3f s" % (case.name, C_, t1 - t0, time.perf_counter() - t1))
    assert got_form == form and L == padded and abort == 0
    finite = np.isfinite(olq)
    # the first leg: the per-wave form at the table itself
    for what, got, want, rows, nan_equal in (("q read back", q1, table, None, False), ("q of the twin", oq, table, None, False),
                                             ("lq (per-wave form)", lq1, olq, None, False), ("grad (per-wave form)", g1, og, None, True)):
        msg = first_difference(case, what, got, want, rows, nan_equal)
        assert msg is None, msg
    assert (lq1[~finite] == -np.inf).all() and finite[promised].mean() > 0.5
    # the second leg: the NUTS kernel's form against the oracle's transition
    # (a g that is NaN at a finite lq -- (nu + 1) tau d past the doubles -- is a NaN on both sides; its sign and payload are the machine's)
    for what, got, want, rows, nan_equal in (("q after the transition", q2, oq2, None, False), ("lq after the transition", lq2, olq2, None, False),
                                             ("grad after the transition", g2, og2, finite, True)):
        msg = first_difference(case, what, got, want, rows, nan_equal)
        assert msg is None, msg
    for f in ("depth", "steps"):
        np.testing.assert_array_equal(st[f][finite], np.array([getattr(s, f) for s in ost])[finite], err_msg=f)
    # form against form wherever the transition returned the start
    kept = T.same_bits(q2, table, nan_equal=False).all(1) & finite
    got_share = kept[promised & finite].mean()
    print("%s: form against form on %d of %d promised rows (%.3f)" % (case.name, kept[promised].sum(), (promised & finite).sum(), got_share))
    assert got_share >= share
    for what, got, want in (("lq, NUTS form against per-wave form", lq2, lq1), ("grad, NUTS form against per-wave form", g2, g1)):
        msg = first_difference(case, what, got, want, kept, nan_equal=True)
        assert msg is None, msg


@pytest.mark.parametrize("name", E.NAMES)
def test_device_has_the_twins_bits(idhmc, oracle, tmp_path, name):
    """every shipped source: its whole table, promised rows and rows past the ends, in both legs"""
    fam = E.FAMILIES[name]
    models = E.twin_models(oracle, fam, tmp_path)
    chains = E.twin_chains(oracle, fam, models)
    model = fam.model(idhmc)
    assert (model.M, model.R) == (fam.M, fam.R)
    promised = np.tile(np.arange(fam.R) < fam.rows.shape[0], fam.M)
    both_legs(idhmc, Case(name, lambda g: E.describe(fam, g // fam.R, g % fam.R)), model, chains, fam.positions(), 1 + fam.A, promised)


def single_chains(oracle, om, table):
    opt = oracle.default_options(max_depth=E.MAX_DEPTH)
    chains = [oracle.OracleChain(om, opt, seed=E.SEED, chain_id=g) for g in range(table.shape[0])]
    for ch, q in zip(chains, table):
        ch.set_q(q)
    return chains


def test_prior_rows_on_the_device(idhmc, oracle, tmp_path):
    """kinds 0 .. 4 with nu at the smallest and largest accepted values, 1 and 3 and tau = 1, 2^-1000, 2^60 as the coordinates of one
    model (tests/test_glm_terms_edges_cpu.py, 'the prior rows'): grad[c] is row c's g alone and lq the sum of the rows' T"""
    table, block_a = E.prior_table()
    om = E.prior_twin(oracle, E.PRIOR_PLAIN, E.PRIOR_LOG, tmp_path)
    chains = single_chains(oracle, om, table)
    case = Case("prior rows", lambda g: "row %d: q = %r" % (g, table[g].tolist()))
    both_legs(idhmc, case, E.prior_device_model(idhmc, E.PRIOR_PLAIN, E.PRIOR_LOG), chains, table, table.shape[1],
              block_a)


@pytest.mark.parametrize("N,eta", E.PAIR_CASES)
def test_pair_factors_and_lkj_row_on_the_device(idhmc, oracle, tmp_path, N, eta):
    """the zeta table through stages 1, 2 and 11 and PRIOR row 5 (tests/test_glm_terms_edges_cpu.py, 'a pair's factors and the LKJ
    row'): grad holds rho, c, the pair's zeta gradient and the LKJ row's g, each by itself"""
    table = E.pair_table(idhmc, N, eta)
    chains = single_chains(oracle, E.pair_twin(oracle, idhmc, N, eta, tmp_path), table)
    case = Case("pair N = %d, eta = %r" % (N, eta), lambda g: "zeta = %r" % table[g, -1])
    both_legs(idhmc, case, E.pair_device_model(idhmc, N, eta), chains, table, table.shape[1], np.ones(table.shape[0], bool))


@pytest.mark.parametrize("S", E.SLABS)
def test_slab_on_the_device(idhmc, oracle, tmp_path, S):
    """a flagged column inside a group and one outside, with a slab (tests/test_glm_terms_edges_cpu.py, 'local scales and the slab'):
    s from below the 1.5e-154 edge to +inf, omega and lambda at the ends of dexp, through stages 4 and 10"""
    table = E.slab_table()
    chains = single_chains(oracle, E.slab_twin(oracle, S, tmp_path), table)
    case = Case("slab S = %r" % S, lambda g: "omega, lambda = %r" % table[g, 3:].tolist())
    both_legs(idhmc, case, E.slab_device_model(idhmc, S), chains, table, table.shape[1], np.ones(table.shape[0], bool))


@pytest.mark.parametrize("N,walk", E.SCAN_CASES)
def test_scan_on_the_device(idhmc, oracle, tmp_path, N, walk):
    """an AR(1) term of N = 2, 3 (with a random walk of 3 levels next to it) and 130 levels over the zeta table, through stages 1, 3
    and 12 (tests/test_glm_terms_edges_cpu.py, 'the AR(1) and random-walk scan'): N = 130 crosses the 128-coordinate chunk"""
    table = E.scan_table(idhmc, N, walk)
    chains = single_chains(oracle, E.scan_twin(oracle, idhmc, N, walk, tmp_path), table)
    case = Case("scan N = %d%s" % (N, " + RW1" if walk else ""), lambda g: "zeta = %r" % table[g, -1])
    both_legs(idhmc, case, E.scan_device_model(idhmc, N, walk), chains, table, table.shape[1], np.ones(table.shape[0], bool),
              padded=128 if N < 127 else 256)


@pytest.mark.parametrize("which,x", E.SCALE_CASES)
def test_scales_without_a_slab_on_the_device(idhmc, oracle, tmp_path, which, x):
    """a group scale alone, a flagged column inside the group and one outside, no slab (tests/test_glm_terms_edges_cpu.py, 'group and
    local scales without a slab'): s from below dexp's range to the largest double, and the rows past it as rejected starts"""
    table, inside = E.scale_table(which)
    chains = single_chains(oracle, E.scale_twin(oracle, x, tmp_path), table)
    case = Case("scales without a slab, " + which, lambda g: "omega, lambda = %r" % table[g, 4:].tolist())
    both_legs(idhmc, case, E.scale_device_model(idhmc, x), chains, table, table.shape[1], inside)
