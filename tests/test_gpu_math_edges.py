"""The device's math layer and RNG at their edges, input by input ("Math layer and RNG address space").

The probe: one test-only CustomDensity source at D = 256 (two chunks per wave: the second one carries third arguments, the second
pattern of wave_sum2 and, in coordinate 255, the selector; at D = 128 a whole 128-vector for the reductions would leave the selector
no coordinate).  It maps its chain's coordinates through ONE function of idhmc_math.hpp, chosen by the selector (broadcast with
read_lane, so one hipRTC module serves every table), writes the results into grad and returns wave_sum of the first chunk.  Every
table of tests/test_math_edges_cpu.py goes in with one set_q and comes back with eng.grad / eng.lq; the device's bits are compared
with the C twin's (PROBE_TWIN_C, held to mpmath / IEEE there) with no tolerance and no input left out, and the fp64 primitives
directly with numpy's correctly rounded results and exact rational arithmetic.

The ahead-of-time kernels' RNG address space (seed bits above 32, chain ids and transition numbers next to 2^32) is compared with
oracle chains at the same address."""
import time

import numpy as np
import pytest

import test_math_edges_cpu as T

pytestmark = pytest.mark.gpu

PROBE_SRC = r"""
#define PROBE_EACH(EXPR_X, EXPR_Y)                                            \
    _Pragma("unroll") for (int j = 0; j < NCH; ++j) {                         \
        const double x = q.c[j].x, y = q.c[j].y;                              \
        grad.c[j].x = (EXPR_X);                                               \
        grad.c[j].y = (EXPR_Y);                                               \
    }
IDHMC_DEV double probe_bits2(uint32_t lo, uint32_t hi) { return u2d(((uint64_t)hi << 32) | lo); }

template <int NCH>
__device__ double logdensity_and_gradient(const Vec<NCH> &q, Vec<NCH> &grad, const UserCtx &ctx)
{
    constexpr int J1 = NCH - 1;                                  // the chunk of the selector (coordinate 128 * NCH - 1) and third arguments
    const int sel = (int)read_lane(q.c[J1].y, 63);
    const double x0 = q.c[0].x, y0 = q.c[0].y, x1 = q.c[J1].x, y1 = q.c[J1].y;
#pragma unroll
    for (int j = 0; j < NCH; ++j) grad.c[j] = make_double2(0.0, 0.0);
    switch (sel) {
    case 1: PROBE_EACH(dlog(x), dlog(y)) break;
    case 2: PROBE_EACH(dexp(x), dexp(y)) break;
    case 3: PROBE_EACH(dlog1p(x), dlog1p(y)) break;
    case 4:
#pragma unroll
        for (int j = 0; j < NCH; ++j) dsincos2pi(q.c[j].x, grad.c[j].x, grad.c[j].y);
        break;
    case 5: PROBE_EACH(dlogaddexp(x, y), dlogaddexp(y, x)) break;
    case 6:
#pragma unroll
        for (int j = 0; j < NCH; ++j) dlgamma_psi(q.c[j].x, grad.c[j].x, grad.c[j].y);
        break;
    case 7: PROBE_EACH(x / y, 1.0 / x) break;
    case 8: PROBE_EACH(__builtin_sqrt(x), __builtin_sqrt(y)) break;
    case 9: PROBE_EACH(__builtin_rint(x), __builtin_rint(y)) break;
    case 10: PROBE_EACH((double)(int)x, (double)(int)y) break;
    case 11: grad.c[0].x = dfma(x0, y0, x1); break;
    case 12:
        grad.c[0].x = dfma_c(x0, y0, 1.0);
        grad.c[0].y = dfma_c(x0, y0, -1.0);
        grad.c[J1].x = dfma_c(x0, y0, 0x1p-1074);
        grad.c[J1].y = dfma_c(x0, y0, 0x1.fffffffffffffp+1023);
        break;
    case 13: PROBE_EACH(u01((uint32_t)d2u(x), (uint32_t)(d2u(x) >> 32)), u01((uint32_t)d2u(y), (uint32_t)(d2u(y) >> 32))) break;
    case 14: PROBE_EACH(u01_open0((uint32_t)d2u(x), (uint32_t)(d2u(x) >> 32)), u01_open0((uint32_t)d2u(y), (uint32_t)(d2u(y) >> 32))) break;
    case 15: {
        const uint64_t c01 = d2u(x0), c23 = d2u(y0), k = d2u(x1);
        const u32x4 o = philox4x32_10((uint32_t)c01, (uint32_t)(c01 >> 32), (uint32_t)c23, (uint32_t)(c23 >> 32), (uint32_t)k, (uint32_t)(k >> 32));
        grad.c[0].x = probe_bits2(o.x, o.y);
        grad.c[0].y = probe_bits2(o.z, o.w);
        break;
    }
    case 16:                                                     // randn_pair from (u1, u2) on
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const double r = __builtin_sqrt(-2.0 * dlog(q.c[j].x));
            double s, c;
            dsincos2pi(q.c[j].y, s, c);
            grad.c[j].x = r * c;
            grad.c[j].y = r * s;
        }
        break;
    case 17: {                                                   // this lane's own copy of every reduction's result
        const double b1 = ctx.lane == 63 ? x1 : y1;              // the selector's place repeats its neighbour
        double sa, sb;
        wave_sum2(x0, y0, x1, b1, sa, sb);
        grad.c[0].x = wave_sum(x0, y0);
        grad.c[0].y = sa;
        grad.c[J1].x = sb;
        grad.c[J1].y = rows_sum(x0);
        break;
    }
    default: break;
    }
    return wave_sum(x0, y0);
}
"""
D = T.W


@pytest.fixture(scope="module")
def probe(idhmc, tmp_path_factory):
    """every table through the probe in one launch, and through the twin: (blocks, row ranges, q, device grad, device lq, twin grad,
    twin lq); the engine is closed before the first assertion"""
    blocks = T.all_blocks()
    q, where = T.pack(blocks)
    twin = T.build_twin(tmp_path_factory.mktemp("probe_twin"))
    tg, tlq = twin(q)
    t0 = time.perf_counter()
    eng = idhmc.Engine(idhmc.CustomDensity(D, PROBE_SRC, np.zeros(1)), q.shape[0], idhmc.default_options(max_depth=3), seed=1)
    t1 = time.perf_counter()
    try:
        assert eng.padded_dim() == D
        eng.set_q(q)
        g, lq, back = eng.grad, eng.lq, eng.q
    finally:
        eng.close()
    print("probe: %d chains, hipRTC build %.2f s, set_q + read-back %.3f s" % (q.shape[0], t1 - t0, time.perf_counter() - t1))
    assert T.same_bits(back, q, nan_equal=False).all()            # the tables reached the device bit for bit, NaN payloads included
    return blocks, where, q, g, lq, tg, tlq


def mismatch(block, got, want, nan_equal=True):
    same = T.same_bits(got, want, nan_equal)
    if same.all():
        return None
    r, c = np.argwhere(~same)[0]
    return "%s: %d of %d values differ, first at row %d coordinate %d (input %r / pair %r): device %r (%#018x), twin %r (%#018x)" % (
        block.name, (~same).sum(), same.size, r, c, block.rows()[r, c], block.rows()[r, c ^ 1], got[r, c], T.u64(got[r, c:c + 1])[0],
        want[r, c], T.u64(want[r, c:c + 1])[0])


ELEMENTARY = ["sweep/log", "log", "sweep/exp", "exp", "sweep/log1p", "log1p", "sincos", "logaddexp", "lgamma_psi", "randn"]
PRIMITIVE = ["div", "sqrt", "sweep/rint", "rint", "d2i2d", "fma", "fma_c"]
INTEGER = ["u01", "u01_open0", "philox"]


@pytest.mark.parametrize("name", ELEMENTARY + PRIMITIVE + INTEGER + ["reduce"])
def test_device_has_the_twins_bits(probe, name):
    """whole rows, padding and the selector's own place included: every value the probe wrote equals the twin's on raw bits (any NaN
    equals any NaN; the integer tables carry bit patterns and compare as integers)"""
    blocks, where, q, g, lq, tg, tlq = probe
    b = next(x for x in blocks if x.name == name)
    msg = mismatch(b, g[where[name]], tg[where[name]], nan_equal=name not in INTEGER)
    assert msg is None, msg
    assert T.same_bits(lq[where[name]], tlq[where[name]], nan_equal=False).all()


def test_exp_contract_on_the_device(probe):
    """0 below the lower threshold, +inf above the upper one, never a subnormal result"""
    blocks, where, q, g, lq, tg, tlq = probe
    for name in ("exp", "sweep/exp"):
        b = next(x for x in blocks if x.name == name)
        x, (got,) = b.cols[0], b.outputs(g[where[name]])
        assert T.same_bits(got[x < T.EXP_LO], 0.0).all() and (got[x > T.EXP_HI] == np.inf).all()
        assert (got[(x >= T.EXP_LO) & (x <= T.EXP_HI)] >= 2.0 ** -1022).all() and np.isfinite(got[x <= T.EXP_HI]).all()


def test_primitives_are_correctly_rounded_on_the_device(probe):
    """the premise of DESIGN section 4, directly: / sqrt rint, (int) and (double), fma and dfma_c on the device equal numpy's
    correctly rounded results and the once-rounded exact a b + c bit for bit"""
    blocks, where, q, g, lq, tg, tlq = probe
    out = {b.name: (b, b.outputs(g[where[b.name]])) for b in blocks if b.name in PRIMITIVE}
    b, (quo, inv) = out["div"]
    with np.errstate(all="ignore"):
        assert T.same_bits(quo, b.cols[0] / b.cols[1]).all() and T.same_bits(inv, 1.0 / b.cols[0]).all()
        b, (got,) = out["sqrt"]
        assert T.same_bits(got, np.sqrt(b.cols[0])).all()
    for name in ("rint", "sweep/rint"):
        b, (got,) = out[name]
        assert T.same_bits(got, np.rint(b.cols[0])).all()
    b, (got,) = out["d2i2d"]
    assert T.same_bits(got, np.trunc(b.cols[0]) + 0.0).all()
    b, (got, _, _, _) = out["fma"]
    want = np.array([T.fma_reference(*t) for t in zip(*(c.tolist() for c in b.cols))])
    assert T.same_bits(got, want, nan_equal=False).all()
    b, outs = out["fma_c"]
    for cst, got in zip(T.FMA_C_CONSTANTS, outs):
        want = np.array([T.fma_reference(x, y, cst) for x, y in zip(b.cols[0].tolist(), b.cols[1].tolist())])
        assert T.same_bits(got, want, nan_equal=False).all(), cst


def test_rng_helpers_on_the_device(probe):
    """integer equality against the numpy Philox (the Random123 known answers first) and the exact v / 2^53"""
    blocks, where, q, g, lq, tg, tlq = probe
    out = {b.name: b.outputs(g[where[b.name]]) for b in blocks if b.name in INTEGER}
    words = T.table_philox()
    ref = T.philox_reference(words)
    o01, o23 = T.u64(out["philox"][0]), T.u64(out["philox"][1])
    for k, (_, _, want) in enumerate(T.PHILOX_KAT):
        assert (int(o01[k]) & 0xffffffff, int(o01[k]) >> 32, int(o23[k]) & 0xffffffff, int(o23[k]) >> 32) == want
    assert np.array_equal(o01, ref[:, 0] | (ref[:, 1] << np.uint64(32))) and np.array_equal(o23, ref[:, 2] | (ref[:, 3] << np.uint64(32)))
    lo, hi = T.table_u01()
    v = ((hi << np.uint64(32)) | lo) >> np.uint64(11)
    assert T.same_bits(out["u01"][0], np.array([int(t) / 2.0 ** 53 for t in v]), nan_equal=False).all()
    assert T.same_bits(out["u01_open0"][0], np.array([(int(t) + 1) / 2.0 ** 53 for t in v]), nan_equal=False).all()


def test_every_lane_holds_the_reductions_bits(probe):
    """wave_sum, both sums of wave_sum2 (two different patterns) and the probe's own return value: all 64 lanes' copies are
    identical and equal the canonical tree (numpy restatement, exact on the cancellation vectors); rows_sum alone on 64 different
    values gives every row the same 16 sums"""
    blocks, where, q, g, lq, tg, tlq = probe
    b = next(x for x in blocks if x.name == "reduce")
    a, second = b.cols
    G = g[where["reduce"]]
    _, want = T.cancellation_vectors()
    for k in range(b.n):
        S, Tt = T.tree_sum(a[k]), T.tree_sum(np.concatenate([second[k], second[k][-1:]]))
        for lanes, ref in ((G[k, 0:128:2], S), (G[k, 1:128:2], S), (G[k, 128::2], Tt)):
            assert lanes.size == 64 and T.same_bits(lanes, lanes[0]).all() and T.same_bits(lanes[0], ref), (k, lanes[:4], ref)
        r = G[k, 129::2].reshape(4, 16)
        assert T.same_bits(r, r[0]).all(), k
    assert T.same_bits(G[12:24, 0], want).all()
    assert T.same_bits(lq[where["reduce"]][12:24], want, nan_equal=False).all()


# ---- the ahead-of-time kernels and the RNG address space ------------------------------------------------------------------------------
SEEDS = [2 ** 32 + 3, 0xfedcba9876543210, 2 ** 64 - 1]
ITERS = [0, 2 ** 31, 2 ** 32 - 1]
LAST = 2 ** 32 - 1                                       # first_chain + nchains may reach it (idhmc_create)


def models(idhmc, oracle, kind, Dm):
    if kind == "iso":
        return idhmc.IsoGaussian(Dm), oracle.OracleModel.iso(Dm)
    sig, mu = np.logspace(-0.5, 0.5, Dm), np.cos(np.arange(Dm, dtype=np.float64))
    return idhmc.DiagGaussian(mu, sigma=sig), oracle.OracleModel.diag(mu, 1.0 / sig ** 2)


def stack(chains, field, Dm):
    return np.stack([getattr(c, field)[:Dm] for c in chains])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind,Dm,C", [("iso", 32, 5), ("diag", 200, 9)])
def test_rng_address_space(idhmc, oracle, kind, Dm, C, seed):
    """seed bits above 32 (k1), the largest chain ids create accepts, transition numbers 0, 2^31 and 2^32 - 1: the initial position,
    the momentum of each of those transitions and four NUTS transitions (direction and exponential streams; max_depth 6) equal the
    oracle chains of the same seed and chain id bit for bit"""
    first = LAST - C
    gm, om = models(idhmc, oracle, kind, Dm)
    eng = idhmc.Engine(gm, C, idhmc.default_options(max_depth=6), seed=seed, first_chain=first)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=6), seed=seed, chain_id=first + c) for c in range(C)]
    try:
        eng.random_position()
        for ch in chains:
            ch.random_position()
        assert T.same_bits(eng.q, stack(chains, "q", Dm), nan_equal=False).all(), "initial position, seed %#x, chains from %d" % (seed, first)
        for it in ITERS:
            eng.refresh_momentum(it)
            for ch in chains:
                ch.rand_p(it)
            assert T.same_bits(eng.p, stack(chains, "p", Dm), nan_equal=False).all(), "momentum of transition %d, seed %#x" % (it, seed)
        eps = 0.3 if kind == "iso" else 0.1
        eng.set_eps(eps)
        for it in ITERS + [1]:
            eng.nuts_transition(it)
            st = eng.tree_stats()
            ost = [ch.sample_tree(eps, it) for ch in chains]
            for f in ("depth", "steps", "term_left", "term_right"):
                np.testing.assert_array_equal(st[f], [getattr(s, f) for s in ost], err_msg="%s @%d" % (f, it))
            assert T.same_bits(st["pi"], [s.pi for s in ost], nan_equal=False).all(), "pi @%d" % it
            assert T.same_bits(st["acceptance_rate"], [s.acceptance_rate for s in ost], nan_equal=False).all(), "acceptance rate @%d" % it
            assert T.same_bits(eng.q, stack(chains, "q", Dm), nan_equal=False).all(), "draw @%d" % it
    finally:
        eng.close()


def test_seed_bits_above_32_matter_and_the_chain_id_limit(idhmc):
    """two engines whose seeds differ only in bit 32, and only in bit 63, draw different positions and momenta; first_chain one past
    the limit is refused"""
    Dm, C = 32, 5
    draws = []
    for seed in (7, 7 + 2 ** 32, 7 + 2 ** 63):
        eng = idhmc.Engine(idhmc.IsoGaussian(Dm), C, seed=seed, first_chain=LAST - C)
        eng.random_position()
        eng.refresh_momentum(3)
        draws.append((eng.q, eng.p))
        eng.close()
    for i in range(3):
        for j in range(i + 1, 3):
            assert not T.same_bits(draws[i][0], draws[j][0]).any() and not T.same_bits(draws[i][1], draws[j][1]).any()
    with pytest.raises(idhmc.IdhmcError) as e:
        idhmc.Engine(idhmc.IsoGaussian(Dm), C, seed=7, first_chain=LAST - C + 1)
    assert "chain ids must fit 32 bits" in str(e.value)
