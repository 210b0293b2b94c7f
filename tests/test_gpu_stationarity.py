"""Exact stationarity of the GPU kernels (tests/stationarity.py): the parity suites prove that the kernels do what the oracle
does; these prove that what they do leaves the target exact.  Every chain starts at an exact draw (Engine.set_q), with a stepsize
drawn independently of the state (set_eps(array)) and a metric deliberately mismatched to the target (minv = var * U(0.3, 3)),
and must still be an exact draw after one nuts_transition, after several transitions in one nuts_transitions launch (the
hand-over of a chain inside a launch) and at every draw stored by mcmc (the driver with its staging blocks).  Each case's id
names the kernel it reaches (idhmc_nuts.hip, idhmc_nuts_sep.inc).  Also: the leapfrog identity E[exp(dH)] = 1, the momentum
refresh, and the negative controls of test_stationarity_cpu.py, which must be rejected here too."""
import numpy as np
import pytest
from scipy import stats

import stationarity as S
from test_stationarity_cpu import NOACC_EPS, NOACC_STEPS

pytestmark = pytest.mark.gpu


# ---- targets: (engine model, exact sampler, standard form, per-coordinate variance) ---------------------------------------

def target(idhmc, kind, D):
    if kind == "diag":
        mu, sigma = S.diag_target(D)
        return (idhmc.DiagGaussian(mu, sigma=sigma), lambda rng, n: S.diag_gaussian(rng, n, mu, sigma),
                ("z", lambda q: (q - mu) / sigma), sigma ** 2)
    if kind == "iso":
        return (idhmc.IsoGaussian(D), lambda rng, n: rng.standard_normal((n, D)), ("z", lambda q: q), np.ones(D))
    if kind == "dense":
        pr = S.dense_mvn(D)
        return (idhmc.DenseMVN(pr["mu"], pr["P"]), lambda rng, n: S.dense_draws(rng, n, pr), ("z", lambda q: S.dense_z(q, pr)),
                (pr["Q"] ** 2 * pr["lam"]).sum(axis=1))
    if kind == "logistic":
        loc, scale = np.sin(np.arange(D, dtype=np.float64)), np.logspace(-0.3, 0.3, D)
        return (idhmc.CustomDensity(D, S.LOGISTIC_HIP, np.concatenate([loc, scale])),
                lambda rng, n: S.logistic_draws(rng, n, loc, scale), ("u", lambda q: S.logistic_u(q, loc, scale)),
                (np.pi * scale) ** 2 / 3.0)
    if kind == "truncnorm":
        a = 2.0
        return (idhmc.CustomDensity(D, S.TRUNCNORM_HIP, [a]), lambda rng, n: S.truncnorm_draws(rng, n, D, a),
                ("u", lambda q: S.truncnorm_u(q, a)), np.full(D, stats.truncnorm(-a, a).var()))
    raise ValueError(kind)


def judge(fam, form, q, tag):
    (S.add_gaussian if form[0] == "z" else S.add_uniform)(fam, form[1](q), tag)


# id: kernel reached | kind, D, C, shared metric, eps range, max_depth, draws kept by mcmc, environment
CASES = [
    ("diag8-k_nuts-DiagGaussianLds<1>-perchain", "diag", 8, 1 << 18, False, (0.2, 0.6), 10, 3, {}),
    ("diag8-k_nuts-DiagGaussianLds<1>-shared", "diag", 8, 1 << 18, True, (0.2, 0.6), 10, 3, {}),
    ("iso129-k_nuts-IsoGaussian<2>-ragged", "iso", 129, 1 << 16, False, (0.3, 0.8), 10, 2, {}),
    ("diag1024-k_nuts<8>", "diag", 1024, 1 << 16, False, (0.15, 0.35), 10, 0, {}),
    ("diag1500-k_nuts<12>-beyond1024", "diag", 1500, 1 << 14, False, (0.15, 0.35), 10, 2, {}),
    ("dense40-k_nuts-DenseMvnCoop<1>-perchain", "dense", 40, 1 << 16, False, (0.1, 0.2), 10, 2, {}),
    ("dense256-k_nuts-DenseMvnCoop<2>-shared", "dense", 256, 1 << 15, True, (0.1, 0.2), 10, 2, {}),
    ("dense256-k_nuts-DenseMvnCoop<2>-perchain", "dense", 256, 1 << 15, False, (0.1, 0.2), 10, 2, {}),
    ("dense500-k_nuts-DenseMvn<4>-GEMV", "dense", 500, 1 << 13, False, (0.1, 0.2), 10, 2, {}),
    ("logistic40-k_nuts-hipRTC-dexp-dlog1p", "logistic", 40, 1 << 16, False, (0.3, 0.8), 10, 2, {}),
    ("truncnorm6-k_nuts-hipRTC-wall", "truncnorm", 6, 1 << 17, False, (0.1, 0.3), 10, 2, {}),
    ("diag8-max_depth2", "diag", 8, 1 << 16, False, (0.05, 0.1), 2, 2, {}),
]
SPOT = lambda C: (0, (1 << 16) - 1, 1 << 16, (1 << 17) + 1, C - 1)       # full-size parity checks stop at 65 536 chains


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_nuts_leaves_the_target_exact(idhmc, oracle, monkeypatch, tmp_path, case):
    name, kind, D, C, shared, (elo, ehi), max_depth, N, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, draw, form, var = target(idhmc, kind, D)
    rng = np.random.default_rng(11)
    q0 = draw(rng, C)
    minv = var * rng.uniform(0.3, 3.0, D if shared else (C, D))
    eps = rng.uniform(elo, ehi, C)
    opt = idhmc.default_options(max_depth=max_depth, metric_mode=idhmc.METRIC_SHARED if shared else idhmc.METRIC_PER_CHAIN)
    eng = idhmc.Engine(model, C, opt, seed=3)
    eng.set_minv(minv)
    eng.set_q(q0)
    eng.set_eps(eps)
    fam = S.Family()
    eng.nuts_transition(1)
    q1, ts = eng.q, eng.tree_stats()
    judge(fam, form, q1, "one transition")
    term = S.terminations(ts)
    moved = S.moved_fraction(q0, q1)
    if kind == "diag" and C > (1 << 17):
        om = oracle.OracleModel.diag(*(lambda m, s: (m, 1.0 / s ** 2))(*S.diag_target(D)))
        for c in SPOT(C):
            ch = oracle.OracleChain(om, oracle.default_options(max_depth=max_depth), seed=3, chain_id=c)
            ch.set_minv(minv if shared else minv[c])
            ch.set_q(q0[c])
            st = ch.sample_tree(eps[c], 1)
            assert (ts["depth"][c], ts["steps"][c]) == (st.depth, st.steps), c
            assert np.array_equal(q1[c].view(np.uint64), ch.q[:D].view(np.uint64)), "chain %d differs from the oracle" % c
    del q1
    eng.nuts_transitions(2, 3)                       # transitions 2, 3, 4 in one launch
    judge(fam, form, eng.q, "after nuts_transitions(2, 3)")
    if N:
        draws, dstats = eng.mcmc(N, 4)
        for n in range(N):
            judge(fam, form, draws[n], "mcmc draw %d" % n)
        del draws
    eng.close()
    print("%s: %s; moved %.3f; terminations %s; 5-sigma-equivalent bias %.4f sd" % (
        name, fam.report(), moved, term, S.detectable_bias(C, fam)))
    S.assert_stationary(fam, name)
    assert moved > 0.8, moved
    if max_depth > 3:
        assert term["mean_depth"] >= 2, term
    else:
        assert term["max_depth"] > 0.5, term
    if kind == "truncnorm":
        assert term["divergence"] >= 0.01, term


# ---- the leapfrog identity: from an exact (q, p), E[exp(dH)] = 1 for the volume-preserving leapfrog map ------------------

def leapfrog_start(idhmc, kind, D, C, seed, opt=None):
    model, draw, form, var = target(idhmc, kind, D)
    rng = np.random.default_rng(seed)
    minv = var * rng.uniform(0.3, 3.0, (C, D))
    eng = idhmc.Engine(model, C, opt if opt is not None else idhmc.default_options(), seed=seed)
    eng.set_minv(minv)
    q0 = draw(rng, C)
    eng.set_q(q0)
    eng.set_p(rng.standard_normal((C, D)) / np.sqrt(minv))
    return eng, rng, q0, minv


def judge_energy(eng, before, what):
    dh = eng.logdensity() - before
    fam = S.Family()
    S.add_mean_one(fam, np.exp(dh), what)
    S.add_nonpositive_mean(fam, dh, what)
    s2 = float(dh.var())
    print("%s: %s; Var dH %.3f" % (what, fam.report(), s2))
    S.assert_stationary(fam, what)
    assert 0.05 < s2 < 3.0, s2                       # the identity is not trivially met and its estimate is not heavy-tailed


@pytest.mark.parametrize("how", ["single-steps", "n-steps", "grad-recompute"])
@pytest.mark.parametrize("D,C,escale", [(8, 1 << 18, 0.7), (1024, 1 << 16, 0.2)])
def test_leapfrog_energy_identity(idhmc, D, C, escale, how):
    eng, rng, q0, minv = leapfrog_start(idhmc, "diag", D, C, 21)
    before = eng.logdensity()
    eps = escale * rng.uniform(0.8, 1.2, C)
    eng.set_eps(eps)
    if how == "grad-recompute":
        eng.set_leapfrog_grad_mode(idhmc.GRAD_RECOMPUTE)
    if how == "n-steps":
        eng.leapfrog(None, 4)
    else:
        for _ in range(4):
            eng.leapfrog(None, 1)
    assert S.moved_fraction(q0, eng.q) > 0.99
    judge_energy(eng, before, "leapfrog D=%d C=%d %s" % (D, C, how))
    eng.close()


@pytest.mark.parametrize("mfma", ["2", "0"])
@pytest.mark.parametrize("D,C", [(256, 1 << 14), (100, 16 * 256 * 4 + 16 * 7 + 1)])
def test_dense_leapfrog_energy_identity(idhmc, monkeypatch, D, C, mfma):
    """the dense single-step sweep on the matrix cores (IDHMC_DENSE_MFMA=2) and the per-wave GEMV (0); above 768 16-chain tiles
    the sweep is cut into lanes on several streams"""
    monkeypatch.setenv("IDHMC_DENSE_MFMA", mfma)
    eng, rng, q0, minv = leapfrog_start(idhmc, "dense", D, C, 22)
    before = eng.logdensity()
    eng.set_eps(0.12 * rng.uniform(0.8, 1.2, C))
    for _ in range(3):
        eng.leapfrog(None, 1)
    if mfma == "2" and C > 768 * 16:
        assert eng.lanes_info()[0] >= 2              # the matrix-core sweep ran in lanes
    assert S.moved_fraction(q0, eng.q) > 0.99
    judge_energy(eng, before, "dense leapfrog D=%d C=%d mfma=%s" % (D, C, mfma))
    eng.close()


# ---- the momentum refresh: p * sqrt(minv) iid N(0, 1) over coordinates, chains and iterations ---------------------------

@pytest.mark.parametrize("D,C", [(8, 1 << 20), (1024, 1 << 16)])
def test_momentum_refresh_is_iid_normal(idhmc, D, C):
    rng = np.random.default_rng(31)
    mu, sigma = S.diag_target(D)
    minv = sigma ** 2 * rng.uniform(0.3, 3.0, (C, D))
    eng = idhmc.Engine(idhmc.DiagGaussian(mu, sigma=sigma), C, seed=17)
    eng.set_minv(minv)
    fam = S.Family()
    eng.refresh_momentum(7)
    z7 = eng.p * np.sqrt(minv)
    eng.refresh_momentum(8)
    z8 = eng.p * np.sqrt(minv)
    eng.close()
    S.add_gaussian(fam, z7, "it 7")
    S.add_gaussian(fam, z8, "it 8")
    S.add_uncorrelated(fam, z7[:, 0::2] ** 2, z7[:, 1::2] ** 2, "Box-Muller partners' squares")
    S.add_uncorrelated(fam, z7, z8, "iterations 7 and 8")
    S.add_uncorrelated(fam, z7[:-1], z7[1:], "neighbouring chains")
    if C > (1 << 16):
        S.add_uncorrelated(fam, z7[:C - (1 << 16)], z7[1 << 16:], "chains 2^16 apart")
    print("refresh D=%d C=%d: %s" % (D, C, fam.report()))
    S.assert_stationary(fam, "momentum refresh")
    rows = np.unique(z7.view(np.dtype((np.void, 8 * D))))
    assert rows.size == C                            # no two chains share a momentum


# ---- negative controls: the statistics must see a wrong sampler on the device too ---------------------------------------

@pytest.mark.parametrize("momentum", ["right", "wrong"])
def test_kept_momentum_control(idhmc, momentum):
    """nuts_transition(T_KEEP_P) with a momentum drawn with variance 1/minv passes; with variance minv it is rejected"""
    D, C = 8, 1 << 16
    eng, rng, q0, minv = leapfrog_start(idhmc, "diag", D, C, 23, idhmc.default_options(metric_mode=idhmc.METRIC_PER_CHAIN))
    n = rng.standard_normal((C, D))
    eng.set_p(n / np.sqrt(minv) if momentum == "right" else n * np.sqrt(minv))
    eng.set_eps(rng.uniform(0.2, 0.6, C))
    eng.nuts_transition(1, idhmc.T_KEEP_P)
    mu, sigma = S.diag_target(D)
    fam = S.Family()
    S.add_gaussian(fam, (eng.q - mu) / sigma, "kept momentum")
    print("kept %s momentum: %s" % (momentum, fam.report()))
    if momentum == "right":
        assert S.moved_fraction(q0, eng.q) > 0.9
        S.assert_stationary(fam, "right momentum")
    else:
        S.assert_rejects(fam, "wrong momentum")
    eng.close()


def test_leapfrog_without_accept_step_control(idhmc):
    D, C = 8, 1 << 16
    eng, rng, q0, minv = leapfrog_start(idhmc, "diag", D, C, 24)
    mu, sigma = S.diag_target(D)
    eng.set_eps(NOACC_EPS * np.sqrt(np.min(sigma ** 2 / minv, axis=1)))
    eng.leapfrog(None, NOACC_STEPS)
    fam = S.Family()
    S.add_gaussian(fam, (eng.q - mu) / sigma, "leapfrog without accept")
    print("no accept step: %s" % fam.report())
    S.assert_rejects(fam, "leapfrog without accept step")
    eng.close()
