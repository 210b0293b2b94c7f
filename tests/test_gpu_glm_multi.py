"""Factor terms with several weighted levels per observation (glm.members, glm.bspline, idhmc_create_glm_multi) on
the device.  A model with a wide term is bit-identical to the same model on the expanded matrix (glm.expand_factors, whose column
off_f + k holds w where an entry names level k and 0.0 elsewhere), in two ways: an engine on the expanded matrix, which runs the kernels
that know nothing of factors, and oracle chains on the C restatement of section 25 (tests/test_glm_gmrf_cpu.py) fed the expanded matrix
-- the one yardstick where the term is structured or carries a GMRF prior, which exist for factor terms only.  No tolerance anywhere.
Both device forms in every case with L <= 256: evaluation and leapfrog run one chain per wavefront, the NUTS kernel on the matrix
cores; the case at L = 512 runs NUTS per wavefront too.  Every context compiles its source with hipRTC, so engines are shared across
assertions."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from test_glm_gmrf_cpu import c_source_gmrf, oracle_params_gmrf
from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_priors_cpu import LOG_HALF_STUDENT_T, NORMAL, STUDENT_T
from test_glm_struct_cpu import RW1, start_struct
from test_gpu_glm_factors import SHORT, same_bits
from test_gpu_glm_slopes import run_engines

pytestmark = pytest.mark.gpu

C_ = 32
# name: (family, Dd, (levels, width, how its rows are made) per term, local scales on every third level column and their slab, D, padded
# length, matrix cores).  Every term is a group of its own.  How the rows of a term are made:
#   "full"    level 1 holds EVERY observation, the even ones through plane 0 and the odd ones through plane 1 (behind level 0): in a block
#             of 128 its list has 128 entries, reached through two planes; further planes random; weights signed, with exact 0.0
#   "counts"  0, 1, .. M present entries per observation (all of them in every block of at least M + 1 observations), weights signed
#   "convex"  M present entries, adjacent levels, weights positive and summing to 1 (a spline basis, a multi-membership)
#   "valued"  a glm.term with values (width 1);   "plain"  an index array (width 1)
# and the last level of every wide term has no observation.
CASES = {
    "plane limit": ("POISSON_LOG", 20, ((30, 4, "full"), (40, 4, "counts")), None, 20 + 70 + 2, 128, 1),
    "four terms": ("POISSON_LOG", 100, ((20, 4, "full"), (10, 2, "counts"), (6, 1, "valued"), (5, 1, "plain")), None, 100 + 41 + 4, 256, 1),
    "per wave": ("POISSON_LOG", 130, ((150, 3, "convex"),), None, 130 + 150 + 1, 512, 0),
    "local": ("POISSON_LOG", 5, ((30, 4, "counts"),), 2.0, 5 + 30 + 1 + 10, 128, 1),
    "aux": ("GAUSSIAN_IDENTITY_LOGSIGMA", 3, ((12, 2, "convex"), (9, 3, "counts")), None, 3 + 21 + 1 + 2, 128, 1),
}


def rows_of(rng, n, N, M, how):
    """(index (n, M), weights (n, M)) of one wide term"""
    idx, w = np.full((n, M), -1), np.zeros((n, M))
    for i in range(n):
        if how == "convex":
            k0 = int(rng.integers(0, N - M))                      # levels k0 .. k0 + M - 1 <= N - 2
            idx[i] = k0 + np.arange(M)
            v = rng.uniform(0.1, 1.0, M)
            w[i] = v / v.sum()
            continue
        if how == "full":
            head = [1] if i % 2 == 0 else [0, 1]
            more = int(rng.integers(0, M - len(head) + 1))
            lv = head + sorted(rng.choice(np.arange(2, N - 1), more, replace=False).tolist())
        else:
            cnt = i % (M + 1) if i < 2 * (M + 1) else int(rng.integers(0, M + 1))
            lv = sorted(rng.choice(np.arange(0, N - 1), cnt, replace=False).tolist())
        idx[i, :len(lv)] = lv
        w[i, :len(lv)] = 0.5 * rng.standard_normal(len(lv))
        w[i, len(lv):] = 7.0                                       # (the weight of an absent entry is ignored)
    if how != "convex":
        w[(idx >= 0) & (rng.uniform(size=idx.shape) < 0.15)] = 0.0
    return idx, w


def problem(idhmc, case, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,), local (Dx,), slab): data from the family's own model"""
    family, Dd, terms, slab, D, L, form = CASES[case]
    rng = np.random.default_rng(n + Dd if seed is None else seed)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    z = X @ (0.5 * rng.standard_normal(Dd) / np.sqrt(Dd))
    factors = []
    for N, M, how in terms:
        if how in ("valued", "plain"):
            idx, w = rng.integers(0, N, n), 0.5 * rng.standard_normal(n)
            factors.append(idhmc.glm.term(idx, values=w, levels=N) if how == "valued" else (idx, N))
            z = z + (w if how == "valued" else 1.0) * (0.4 * rng.standard_normal(N))[idx]
            continue
        idx, w = rows_of(rng, n, N, M, how)
        factors.append(idhmc.glm.members(idx, w, N))
        z = z + (np.where(idx >= 0, w, 0.0) * (0.4 * rng.standard_normal(N))[np.maximum(idx, 0)]).sum(1)
    Y = rng.poisson(np.exp(z)).astype(float) if family == "POISSON_LOG" else z + 0.5 * rng.standard_normal(n)
    Dx = Dd + sum(t[0] for t in terms)
    grp, off = np.full(Dx, -1, np.int32), Dd
    for f, t in enumerate(terms):
        grp[off:off + t[0]] = f
        off += t[0]
    local = np.zeros(Dx, np.int32)
    if slab:
        local[Dd::3] = 1
    return X, Y, factors, grp, local, slab


def dims(case):
    """Dx, A, H, J"""
    family, Dd, terms, slab = CASES[case][:4]
    Dx = Dd + sum(t[0] for t in terms)
    return Dx, SHAPE[family][2], len(terms), len(range(Dd, Dx, 3)) if slab else 0


def case_priors(case, gmrf_cols=()):
    """normal and Student-t coefficients, log half-t on the scales and on every other lambda; the defaults on the columns of a GMRF term"""
    Dx, A, H, J = dims(case)
    D = CASES[case][4]
    rng = np.random.default_rng(D)
    kind, nu = np.zeros(D, np.int32), np.zeros(D)
    kind[1:Dx:2] = STUDENT_T
    kind[Dx + A:Dx + A + H] = LOG_HALF_STUDENT_T
    kind[Dx + A + H::2] = LOG_HALF_STUDENT_T
    mu, tau = rng.standard_normal(D) * 0.2, rng.uniform(0.5, 2.0, D)
    tau[kind == LOG_HALF_STUDENT_T] = 1.0
    for o, N in gmrf_cols:
        kind[o:o + N], mu[o:o + N], tau[o:o + N] = NORMAL, 0.0, 1.0
    nu[kind == STUDENT_T], nu[kind == LOG_HALF_STUDENT_T] = 4.0, 3.0
    return kind, nu, mu, tau


def models(idhmc, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau, expanded=True, **kw):
    """the model with its factor terms and (expanded) the same model on the expanded matrix"""
    family = CASES[case][0]
    common = dict(constants=consts(family), prior_mu=mu, prior_tau=tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu,
                  local=local if slab else None, slab_scale=slab)
    mF = idhmc.GLM(X, Y, source(idhmc, family), factors=factors, **common, **kw)
    return (mF, idhmc.GLM(idhmc.glm.expand_factors(X, factors), Y, source(idhmc, family), **common)) if expanded else mF


def oracle_model(idhmc, oracle, tmp_path, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau, structs=(), gmrfs=()):
    """the restatement of section 25 on the expanded matrix; structs: (off, N, kind), gmrfs: (off, N, Q, kappa)"""
    family, D = CASES[case][0], CASES[case][4]
    Xe = idhmc.glm.expand_factors(X, factors)
    return oracle.OracleModel.custom(D, c_source_gmrf(family),
                                     oracle_params_gmrf(Xe, Y, SHAPE[family][2], grp, local if slab else None, slab, kind, nu, [], [], list(structs),
                                                        [0.0] * len(structs), list(gmrfs), consts(family), mu, tau), str(tmp_path))


def start(case, chains, seed=0):
    Dx, A, H, J = dims(case)
    return start_struct(CASES[case][0], chains, Dx, H, J, 0, 0, seed)


def table_of(idhmc, factors, n):
    return idhmc.glm.factor_members(factors, n)


def test_the_cases_are_what_they_are_there_for(idhmc):
    for name, (family, Dd, terms, slab, D, L, form) in CASES.items():
        Dx, A, H, J = dims(name)
        assert Dx + A + H + J == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))), name
        assert form == int(L <= 256)
    assert [t[1] for t in CASES["plane limit"][2]] == [4, 4] and [t[1] for t in CASES["four terms"][2]] == [4, 2, 1, 1]
    assert [t[1] for t in CASES["per wave"][2]] == [3]
    # "four terms": the second term's columns 120 .. 129 straddle coordinate 127 / 128, its lists live in two chunks
    assert 100 + 20 < 127 < 128 < 100 + 20 + 10
    # "per wave": 130 dense columns are stored 256 wide
    assert 128 * ((130 + 127) // 128) == 256
    for name in CASES:
        for n in (1, 128, 130):
            X, Y, factors, grp, local, slab = problem(idhmc, name, n)
            width, idx, val = table_of(idhmc, factors, n)
            assert list(width) == [t[1] for t in CASES[name][2]] and int(width.sum()) <= 8
            p0 = 0
            for (N, M, how), fac in zip(CASES[name][2], factors):
                pl, pv = idx[p0:p0 + M], val[p0:p0 + M]
                p0 += M
                if how in ("valued", "plain"):
                    continue
                assert not (pl == N - 1).any()                                        # a level with no observation
                cnt = (pl >= 0).sum(0)
                if how == "full" and n >= 128:
                    assert ((pl[:, :128] == 1).sum(0) == 1).all()                      # level 1: all 128 observations of block 0 ..
                    assert (pl[0, 0:128:2] == 1).all() and (pl[1, 1:128:2] == 1).all()  # .. even ones by plane 0, odd ones by plane 1
                    assert ((pv == 0.0) & (pl >= 0)).any() and (pv < 0).any()
                if how == "counts" and n >= 128:
                    assert set(cnt[:128]) == set(range(M + 1))                         # 0, 1, .. M present entries in one block
                    assert ((pv == 0.0) & (pl >= 0)).any() and (pv < 0).any()
                if how == "convex":
                    assert (cnt == M).all() and np.all(np.abs(pv.sum(0) - 1.0) < 1e-15) and (pv > 0).all()
    # the term may be a level short of its columns (a list of length 0), never the other way round
    E = idhmc.glm.expand_factors(*problem(idhmc, "plane limit", 130)[0:3:2])
    assert E.shape == (130, 90) and not E[:, 20 + 29].any() and not E[:, 89].any() and (E[:128, 21] != 0).sum() > 90


@pytest.mark.parametrize("case", ["plane limit", "four terms", "per wave"])
@pytest.mark.parametrize("n", [1, 128, 130])
def test_density_leapfrog_and_nuts(idhmc, oracle, tmp_path, case, n):
    """lq and grad l after evaluation (the per-wave form), one leapfrog, and NUTS transitions (max_depth = 4, fixed eps: two single
    launches, then two in one launch) in the form the case runs: the bits of the engine on the expanded matrix and of the oracle chains
    on it.  Engine.glm_members() returns the table as it was given."""
    family, Dd, terms, slab, D, L, form = CASES[case]
    Dx, A, H, J = dims(case)
    X, Y, factors, grp, local, slab = problem(idhmc, case, n)
    kind, nu, mu, tau = case_priors(case)
    mF, mE = models(idhmc, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    assert (mF.D, mE.D, mF.Dx, mE.Dx, mF.Dd, mE.Dd) == (D, D, Dx, Dx, Dd, Dx) and mE.member_width is None
    opt = idhmc.default_options(max_depth=4)
    engF, engE = idhmc.Engine(mF, C_, opt, seed=3), idhmc.Engine(mE, C_, opt, seed=3)
    om = oracle_model(idhmc, oracle, tmp_path, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=3, chain_id=c) for c in range(C_)]
    assert engF.glm_form() == engE.glm_form() == form and engF.padded_dim() == engE.padded_dim() == L and engF.D == D
    width, idx, val = engF.glm_members()
    w0, i0, v0 = table_of(idhmc, factors, n)
    assert width.dtype == idx.dtype == np.int32 and np.array_equal(width, w0) and np.array_equal(idx, i0) and same_bits(val, v0)
    assert list(engF.glm_factors()[0]) == [t[0] for t in terms] and engF.glm_factor_values() == (None, None)
    assert engE.glm_members() == (None, None, None)
    # the planes are counted: 4 + 8 + 8 bytes per entry of the padded planes and a byte per list entry, the starts and the table
    npad, P, cols = (n + 127) // 128 * 128, int(w0.sum()), Dx - Dd
    planes = (4 + 8 + 8 + 1) * P * npad + 4 * ((npad // 128) * (cols + 1) + 8)
    stored = 2 * 8 * npad * (L - 128 * ((Dd + 127) // 128))       # X and X' of the expanded model are L wide, here Lx
    assert engF.device_bytes() - engE.device_bytes() == planes - stored
    run_engines([engF, engE], chains, D, start(case, C_), case)
    engF.close()
    engE.close()


@pytest.mark.parametrize("case", ["local", "aux"])
def test_local_scales_and_an_auxiliary_coordinate(idhmc, oracle, tmp_path, case):
    """"local": a group scale and local scales with a slab on the columns of a wide term; "aux": A = 1 (the Gaussian's log sigma) with a
    multi-membership term whose weights sum to 1 next to a signed one -- against the expanded engine and the oracle, n = 130"""
    family, Dd, terms, slab, D, L, form = CASES[case]
    Dx, A, H, J = dims(case)
    assert (A, J > 0) == ((0, True) if case == "local" else (1, False))
    X, Y, factors, grp, local, slab = problem(idhmc, case, 130)
    kind, nu, mu, tau = case_priors(case)
    mF, mE = models(idhmc, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    assert (mF.J, mF.A, mF.H) == (J, A, H)
    opt = idhmc.default_options(max_depth=4)
    engF, engE = idhmc.Engine(mF, C_, opt, seed=5), idhmc.Engine(mE, C_, opt, seed=5)
    om = oracle_model(idhmc, oracle, tmp_path, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=5, chain_id=c) for c in range(C_)]
    assert engF.glm_form() == engE.glm_form() == form
    run_engines([engF, engE], chains, D, start(case, C_), case)
    engF.close()
    engE.close()


def smooth_problem(idhmc, n, N=24, seed=0):
    """y ~ 1 + x + s(x), Poisson: (X (n, 2), Y, the cubic B-spline term of N basis functions)"""
    rng = np.random.default_rng(seed + n)
    x = np.r_[0.0, 1.0, rng.uniform(0.0, 1.0, n)][:n] if n > 1 else np.array([0.3])
    X = np.c_[np.ones(n), x - 0.5]
    Y = rng.poisson(np.exp(0.5 + np.sin(6.0 * x))).astype(float)
    return X, Y, idhmc.glm.bspline(x, N, lo=0.0, hi=1.0)


def test_a_p_spline_is_the_gmrf_prior_on_a_wide_term(idhmc, oracle, tmp_path):
    """GLM(X, Y, source, factors=[glm.bspline(x, 24)], **glm.smooth_effects(2, [24])): the scaled RW2 precision with sum_to_zero = 1 on
    the levels of a term of width 4, against oracle chains on the expanded matrix with the same precision as their table (a GMRF prior
    exists for factor terms only, so there is no expanded engine to hold it to)"""
    g = idhmc.glm
    n, N = 130, 24
    X, Y, term = smooth_problem(idhmc, n, N)
    kw = g.smooth_effects(2, [N], scale=g.half_student_t(3.0))
    m = idhmc.GLM(X, Y, source(idhmc, "POISSON_LOG"), consts("POISSON_LOG"), factors=[term], **kw)
    D = 2 + N + 1
    assert (m.D, m.G, m.H, list(m.member_width), m.gmrf_kappa[0]) == (D, 1, 1, [4], 1.0)
    Q = g.scale_precision(g.rw2_precision(N))
    assert np.array_equal(g.gmrf_precision(m, 0), Q)
    Xe = g.expand_factors(X, [term])
    om = oracle.OracleModel.custom(D, c_source_gmrf("POISSON_LOG"),
                                   oracle_params_gmrf(Xe, Y, 0, m.groups, None, None, m.prior_kind, m.prior_nu, [], [], [], [], [(2, N, Q, 1.0)],
                                                      consts("POISSON_LOG"), m.mu, m.tau), str(tmp_path))
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4), seed=9)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=9, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == 1 and eng.padded_dim() == 128 and list(eng.glm_members()[0]) == [4]
    run_engines([eng], chains, D, start_struct("POISSON_LOG", C_, 2 + N, 1, 0, 0, 0), "p-spline")
    eng.close()


def test_a_random_walk_over_the_levels_of_a_wide_term(idhmc, oracle, tmp_path):
    """structured=[glm.rw1(0)] on the first term of "plane limit" (width 4, a level that holds a whole block): the scan runs on the
    term's columns whatever the number of entries an observation has in them -- against oracle chains on the expanded matrix"""
    case = "plane limit"
    family, Dd, terms, slab, D, L, form = CASES[case]
    Dx, A, H, J = dims(case)
    X, Y, factors, grp, local, slab = problem(idhmc, case, 130)
    kind, nu, mu, tau = case_priors(case)
    m = models(idhmc, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau, expanded=False, structured=[idhmc.glm.rw1(0)])
    assert (m.S, m.Sz, m.D) == (1, 0, D)
    om = oracle_model(idhmc, oracle, tmp_path, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau, structs=[(Dd, terms[0][0], RW1)])
    eng = idhmc.Engine(m, C_, idhmc.default_options(max_depth=4), seed=11)
    chains = [oracle.OracleChain(om, oracle.default_options(max_depth=4), seed=11, chain_id=c) for c in range(C_)]
    assert eng.glm_form() == form and eng.glm_structs()[0] is not None
    run_engines([eng], chains, D, start(case, C_), "rw1")
    eng.close()


def test_three_responses_with_per_response_adaptation(idhmc):
    """M = 3 responses of R = 16 chains on "four terms" with EPS_PER_RESPONSE and METRIC_PER_RESPONSE: a searched stepsize and a tuning
    stage that adapts both, then draws -- the bits of the expanded engine in the same modes"""
    case = "four terms"
    family, Dd, terms, slab, D, L, form = CASES[case]
    M, R, n = 3, 16, 130
    X, Y0, factors, grp, local, slab = problem(idhmc, case, n)
    rng = np.random.default_rng(6)
    Y = np.stack([Y0] + [rng.poisson(np.maximum(Y0, 0.5)).astype(float) for _ in range(M - 1)])[:, :, None]
    kind, nu, mu, tau = case_priors(case)
    mF = models(idhmc, case, X, Y, factors, grp, local, slab, kind, nu, mu, tau, expanded=False, chains_per_response=R)
    mE = idhmc.GLM(idhmc.glm.expand_factors(X, factors), Y, source(idhmc, family), constants=consts(family), prior_mu=mu, prior_tau=tau,
                   groups=grp, prior_kind=kind, prior_nu=nu, chains_per_response=R)
    got = []
    for m in (mF, mE):
        opt = idhmc.default_options(eps_mode=idhmc.EPS_PER_RESPONSE, metric_mode=idhmc.METRIC_PER_RESPONSE, max_depth=5)
        eng = idhmc.Engine(m, M * R, opt, seed=17)
        assert eng.glm_responses() == (M, R) and eng.glm_form() == form
        eng.random_position()
        eng.set_q(0.1 * eng.q)
        eng.refresh_momentum(0)
        eng.find_initial_stepsize()
        draws, stats_ = eng.tuning_stage(12, True, 0, store_draws=True)
        got.append((draws, stats_, eng.eps, eng.minv, eng.q, eng.lq))
        assert eng.poll_abort() == 0
        eng.close()
    a, b = got
    assert np.isfinite(a[0]).all() and len(np.unique(a[2])) == M       # one stepsize per response
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in (2, 3, 4, 5):
        assert same_bits(a[k], b[k]), k


def test_warmup_and_summary_of_a_smooth_match_the_expanded_engine(idhmc):
    """y ~ 1 + x + s(x) with the cubic basis as a wide term and a sampled scale on its levels (the iid prior: the expanded engine has no
    factor term to put the penalty on; the P-spline is held to the oracle above): a 40-transition warm-up with per-chain adaptation
    and 8 draws, then mcmc_summary -- stepsizes, metric, draws, records and every field of the device summary"""
    g = idhmc.glm
    n, N, Cw, G, bins = 130, 24, 16, 8, 16
    X, Y, term = smooth_problem(idhmc, n, N)
    kw = g.random_intercepts(2, [N], scale=g.half_student_t(3.0))
    mods = (idhmc.GLM(X, Y, source(idhmc, "POISSON_LOG"), consts("POISSON_LOG"), factors=[term], **kw),
            idhmc.GLM(g.expand_factors(X, [term]), Y, source(idhmc, "POISSON_LOG"), consts("POISSON_LOG"), **kw))
    assert mods[0].D == mods[1].D == 2 + N + 1 and list(mods[0].member_width) == [4]
    out = []
    for m in mods:
        eng = idhmc.Engine(m, Cw, idhmc.default_options(**SHORT), seed=77)
        draws, stats_ = eng.mcmc_with_warmup(8)
        res = [draws, stats_, eng.eps, eng.minv, eng.lq, eng.grad]
        res.append(eng.mcmc_summary(6, 100, pilot=2, chains_per_group=G, bins=bins))
        assert eng.poll_abort() == 0 and eng.glm_form() == 1
        out.append(res)
        eng.close()
    a, b = out
    assert np.isfinite(a[0]).all() and len(np.unique(a[2])) > 1
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in (2, 3, 4, 5):
        assert same_bits(a[k], b[k]), k
    sa, sb = (dataclasses.asdict(s) for s in (a[6], b[6]))
    assert sorted(sa) == sorted(sb) and np.all(sa["n"] == 6 * G)
    for k in sa:
        if isinstance(sa[k], np.ndarray) and sa[k].dtype == np.float64:
            assert same_bits(sa[k], sb[k]), k
        else:
            assert np.array_equal(sa[k], sb[k]), k


@pytest.mark.parametrize("valued", [True, False])
def test_widths_of_one_through_the_new_entry_point(idhmc, valued):
    """idhmc_create_glm_multi with every width 1 -- with values, without -- against the context the library builds from the same planes
    as factors (glm.term values; plain index arrays): the same form, footprint, state and draws; and with members = NULL"""
    from inplacedhmc_jl_amd import _lib
    n, Cn = 130, 32
    rng = np.random.default_rng(4)
    X = 0.3 * rng.standard_normal((n, 4))
    X[:, 0] = 1.0
    Y = rng.poisson(2.0, n).astype(float)
    i0, i1 = rng.integers(0, 7, n), rng.integers(0, 50, n)
    w = 0.5 * rng.standard_normal((2, n))
    grp = np.r_[np.full(4, -1), np.zeros(7), np.ones(50)].astype(np.int32)
    D = 4 + 57 + 2
    opt = idhmc.default_options(max_depth=4)
    lib = idhmc.load_library()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    fac = [idhmc.glm.term(i0, values=w[0], levels=7), idhmc.glm.term(i1, values=w[1], levels=50)] if valued else [(i0, 7), (i1, 50)]
    m = idhmc.GLM(X, Y, source(idhmc, "POISSON_LOG"), consts("POISSON_LOG"), factors=fac, groups=grp)
    engs = [idhmc.Engine(m, Cn, opt, seed=3)]
    width = np.ones(2, np.int32)
    index = np.ascontiguousarray([i0, i1], dtype=np.int32)
    vals = np.ascontiguousarray(w)
    for members in (True, False):
        desc = m.glm_desc()
        fc = _lib.GlmFactors(F=2, levels=m.levels.ctypes.data_as(ip), index=None if members else index.ctypes.data_as(ip))
        mm = _lib.GlmMembers(width=width.ctypes.data_as(ip), index=index.ctypes.data_as(ip), values=vals.ctypes.data_as(dp) if valued else None)
        fv = _lib.GlmFactorValues(values=vals.ctypes.data_as(dp), has=width.ctypes.data_as(ip))
        h = C.c_void_p()
        _lib.check(lib.idhmc_create_glm_multi(C.byref(h), 0, Cn, 0, C.byref(desc), None, None, C.byref(fc),
                                              C.byref(fv) if valued and not members else None, None, None, None, None,
                                              C.byref(mm) if members else None, 1, 0, C.byref(opt), 3))
        eng = idhmc.Engine._adopt(m, h, Cn, opt)     # an Engine around that context
        engs.append(eng)
    for e in engs:
        assert e.glm_form() == 1 and list(e.glm_factors()[0]) == [7, 50] and np.array_equal(e.glm_factors()[1], index)
        assert (e.glm_factor_values()[0] is not None) == valued
        wd, ix, vl = e.glm_members()
        assert list(wd) == [1, 1] and np.array_equal(ix, index) and same_bits(vl, vals if valued else np.ones((2, n)))
    assert engs[0].device_bytes() == engs[1].device_bytes() == engs[2].device_bytes()
    run_engines(engs, None, D, start_struct("POISSON_LOG", Cn, 4 + 57, 2, 0, 0, 0), "widths of one")
    for e in engs:
        e.close()
