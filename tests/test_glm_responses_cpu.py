"""GLMs with several responses on one design matrix (GLM(..., chains_per_response=R), idhmc_create_glm_responses)
without a GPU: the constructor's validation, the helpers that sort chains and draws by response (glm.response_of_chain,
glm.by_response, diagnostics.rhat_by_response) on hand-made arrays, and the C boundary's argument checks, every one of which answers
before the device is looked for.  The device side is tests/test_gpu_glm_responses.py."""
import ctypes as C

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
import test_glm_cpu as FLAT


def responses(family, M, n, D, seed=3):
    """one design matrix and M responses from the family's own model, each drawn with its own seed: (X, Y (M, n, K))"""
    X = FLAT.problem(family, n, D, seed=seed)[0]
    Ys = []
    for m in range(M):
        rng = np.random.default_rng(1000 * seed + m)
        z = X @ (rng.standard_normal(D) / np.sqrt(D))
        if family == "POISSON_LOG":
            y = rng.poisson(np.exp(z)).astype(float)[:, None]
        elif family == "BINOMIAL_LOGIT":
            t = rng.integers(1, 20, n)
            y = np.stack([rng.binomial(t, 1.0 / (1.0 + np.exp(-z))).astype(float), t.astype(float)], 1)
        elif family == "BERNOULLI_LOGIT":
            y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-z))).astype(float)[:, None]
        else:
            raise KeyError(family)
        Ys.append(y)
    return X, np.stack(Ys)


# ---- the constructor ---------------------------------------------------------------------------------------------------------------
def test_constructor_keeps_the_parts(idhmc):
    X, Y = responses("BINOMIAL_LOGIT", 5, 9, 4)
    m = idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, prior_mu=0.5, prior_tau=2.0, chains_per_response=7)
    assert m.kind == idhmc.MODEL_GLM and m.D == 4 and (m.M, m.R, m.n, m.K, m.nc, m.Dx, m.A, m.H) == (5, 7, 9, 2, 0, 4, 0, 0)
    assert m.params is None and m.groups is None and m.Y.shape == (5, 9, 2) and m.Y.flags.c_contiguous
    d = m.glm_desc()
    assert (d.n, d.Dx, d.K, d.nc, d.A, d.H) == (9, 4, 2, 0, 0, 0) and not d.groups and not d.constants
    assert d.Y[(3 * 9 + 8) * 2 + 1] == Y[3, 8, 1] and d.X[5] == X[1, 1] and d.mu[3] == 0.5 and d.tau[0] == 2.0
    # with what is already there: auxiliary coordinates and groups
    Xa, ya = AUX.problem_aux("GAUSSIAN_IDENTITY_LOGSIGMA", 9, 6)
    Y3 = np.stack([ya, ya + 1.0, ya - 1.0])[:, :, None]
    m = idhmc.GLM(Xa, Y3, idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=[-1, 0, 1, 0, -1, 1], chains_per_response=np.int64(2))
    assert m.kind == idhmc.MODEL_GLM_AUX and m.D == 9 and (m.M, m.R, m.K, m.A, m.H) == (3, 2, 1, 1, 2) and isinstance(m.R, int)
    # one response is a model of its own kind too: M = 1 and the parts, not the packed params
    m = idhmc.GLM(X, Y[:1], idhmc.glm.BINOMIAL_LOGIT, chains_per_response=40)
    assert (m.M, m.R) == (1, 40) and m.params is None


def test_without_the_keyword_nothing_changes(idhmc):
    X, Y = FLAT.problem("BINOMIAL_LOGIT", 7, 3)
    c = [2.0, 0.5, -1.0]
    want = np.concatenate([[2.0, 3.0], c, X.ravel(), Y.ravel()])
    for kw in ({}, {"chains_per_response": None}):
        m = idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, c, 0.5, 2.0, **kw)
        assert m.kind == idhmc.MODEL_GLM and (m.M, m.R) == (1, None) and m.params.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        idhmc.GLM(X, Y[None], idhmc.glm.BINOMIAL_LOGIT)                    # a 3-D Y needs the keyword


def test_constructor_validates_responses(idhmc):
    X, Y = responses("BINOMIAL_LOGIT", 3, 20, 5)
    src = idhmc.glm.BINOMIAL_LOGIT
    with pytest.raises(ValueError, match="add the K axis"):
        idhmc.GLM(X, Y[:, :, 0], src, chains_per_response=4)               # (M, n): could be (n, K)
    with pytest.raises(ValueError, match="add the K axis"):
        idhmc.GLM(X, Y[0], src, chains_per_response=4)                     # (n, K): could be (M, n)
    for bad in (Y[0, :, 0], Y[None], Y[:, :-1], np.zeros((3, 20, 5)), np.zeros((3, 20, 0)), np.zeros((0, 20, 2)), Y.transpose(1, 0, 2)):
        with pytest.raises(ValueError, match=r"\(M, 20, K\)"):
            idhmc.GLM(X, bad, src, chains_per_response=4)
    for m_, i, k in ((0, 0, 0), (1, 7, 1), (2, 19, 0)):                    # a non-finite value in any plane
        bad = Y.copy()
        bad[m_, i, k] = np.nan
        with pytest.raises(ValueError, match="finite"):
            idhmc.GLM(X, bad, src, chains_per_response=4)
    for R in (0, -1, 2.0, 1.5, True, "3", [3], np.float64(2)):
        with pytest.raises(ValueError, match="positive integer"):
            idhmc.GLM(X, Y, src, chains_per_response=R)
    assert idhmc.GLM(X, Y, src, chains_per_response=1).R == 1


# ---- sorting chains and draws by response ----------------------------------------------------------------------------------------------
def test_response_of_chain(idhmc):
    X, Y = responses("POISSON_LOG", 3, 10, 4)
    m = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, chains_per_response=6)
    ids = idhmc.glm.response_of_chain(m, 18)
    assert ids.shape == (18,) and np.issubdtype(ids.dtype, np.integer) and np.array_equal(ids, np.repeat([0, 1, 2], 6))
    assert np.array_equal(idhmc.glm.response_of_chain(m, 9, first_chain=5), [0, 1, 1, 1, 1, 1, 1, 2, 2])
    assert np.array_equal(idhmc.glm.response_of_chain(m, 1, 17), [2])
    for n_, f in ((19, 0), (1, 18), (9, 10), (0, 0), (3, -1)):
        with pytest.raises(ValueError):
            idhmc.glm.response_of_chain(m, n_, f)
    with pytest.raises(ValueError, match="one response"):
        idhmc.glm.response_of_chain(idhmc.GLM(X, Y[0], idhmc.glm.POISSON_LOG), 4)


def test_by_response(idhmc):
    X, Y = responses("POISSON_LOG", 3, 10, 4)
    m = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, chains_per_response=6)
    draws = np.arange(5 * 18 * 4, dtype=float).reshape(5, 18, 4)           # (N, C, D)
    out = idhmc.glm.by_response(m, draws)
    assert out.shape == (3, 5, 6, 4)
    for r in range(3):
        assert np.array_equal(out[r], draws[:, 6 * r:6 * r + 6])
    q = draws[0]                                                           # (C, D)
    assert np.array_equal(idhmc.glm.by_response(m, q), q.reshape(3, 6, 4))
    # a shard of whole responses: responses 1 and 2
    part = idhmc.glm.by_response(m, draws[:, 6:], first_chain=6)
    assert part.shape == (2, 5, 6, 4) and np.array_equal(part[0], draws[:, 6:12]) and np.array_equal(part[1], draws[:, 12:])
    # a partial response is refused
    with pytest.raises(ValueError, match="whole responses"):
        idhmc.glm.by_response(m, draws[:, 5:14], first_chain=5)
    with pytest.raises(ValueError, match="whole responses"):
        idhmc.glm.by_response(m, draws[:, :9])
    with pytest.raises(ValueError, match="whole responses"):
        idhmc.glm.by_response(m, draws[:, 3:15], first_chain=3)
    with pytest.raises(ValueError):
        idhmc.glm.by_response(m, draws[:, :12], first_chain=12)            # past the model's chains
    with pytest.raises(ValueError):
        idhmc.glm.by_response(m, np.zeros(18))
    # coefficients and group_scales take the sorted array as it is
    Xa, ya = AUX.problem_aux("GAUSSIAN_IDENTITY_LOGSIGMA", 9, 6)
    grp = np.array([-1, 0, 1, 0, -1, 1])
    mg = idhmc.GLM(Xa, np.stack([ya, ya + 1.0])[:, :, None], idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=grp, chains_per_response=3)
    d = np.random.default_rng(0).standard_normal((4, 6, 9))
    s = idhmc.glm.by_response(mg, d)
    assert np.array_equal(idhmc.glm.coefficients(mg, s), idhmc.glm.by_response(mg, idhmc.glm.coefficients(mg, d)))
    assert idhmc.glm.group_scales(mg, s).shape == (2, 4, 3, 2)


def test_rhat_by_response(idhmc):
    X, Y = responses("POISSON_LOG", 4, 10, 3)
    m = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, chains_per_response=50)
    rng = np.random.default_rng(0)
    n, C_, D = 40, 200, 3
    x = rng.standard_normal((C_, n, D)) + np.repeat(np.arange(4.0), 50)[:, None, None] * 10.0     # each response around its own mean
    x[100:125] += 3.0                                                                               # response 2: half its chains elsewhere
    mean, var = x.mean(1), x.var(1, ddof=1)
    r = idhmc.rhat_by_response(m, mean, var, n)
    assert r.shape == (4, D)
    for k in range(4):
        assert np.array_equal(r[k], idhmc.rhat_from_moments(mean[50 * k:50 * k + 50], var[50 * k:50 * k + 50], n))
    assert np.all(np.abs(r[[0, 1, 3]] - 1.0) < 0.1) and np.all(r[2] > 1.3)
    assert np.all(idhmc.rhat_from_moments(mean, var, n) > 3.0)             # pooled over the responses it says nothing
    assert np.array_equal(idhmc.rhat_by_response(m, mean, var, np.full(C_, n)), r)
    assert np.array_equal(idhmc.rhat_by_response(m, mean[50:150], var[50:150], n, first_chain=50), r[1:3])
    with pytest.raises(ValueError, match="whole responses"):
        idhmc.rhat_by_response(m, mean[:75], var[:75], n)
    with pytest.raises(ValueError):
        idhmc.rhat_by_response(m, mean, var[:, :2], n)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def _create(idhmc, desc, M, R, nchains=4, first=0, opt=None):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create_glm_responses(C.byref(h), 0, nchains, first, C.byref(desc), M, R, None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def test_a_valid_call_passes_the_argument_checks(idhmc):
    X, Y = responses("BINOMIAL_LOGIT", 5, 50, 6)
    m = idhmc.GLM(X, Y, idhmc.glm.BINOMIAL_LOGIT, prior_mu=0.1, prior_tau=0.5, chains_per_response=7)     # kept alive: the descriptor points into it
    for kw in (dict(nchains=35), dict(nchains=9, first=5), dict(nchains=1, first=34),
               dict(nchains=35, opt=idhmc.default_options(metric_mode=idhmc.METRIC_SHARED))):
        rc, msg = _create(idhmc, m.glm_desc(), 5, 7, **kw)
        # a context where a device exists; otherwise the constructor stops at its device check, past every argument check
        assert rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg), (kw, rc, msg)
    # M = 1 allows the pooled statistics: they pool chains of one posterior
    for o in (idhmc.default_options(eps_mode=idhmc.EPS_GLOBAL), idhmc.default_options(metric_mode=idhmc.METRIC_POOLED)):
        rc, msg = _create(idhmc, m.glm_desc(), 1, 40, nchains=40, opt=o)
        assert rc in (0, idhmc.ERR_NO_DEVICE), (rc, msg)
    # the Engine takes the same road
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(idhmc.IdhmcError) as e:
            idhmc.Engine(m, 35)
        assert e.value.code == idhmc.ERR_NO_DEVICE
        with pytest.raises(idhmc.IdhmcError) as e:
            idhmc.Engine(m, 36)                                             # a chain without a response: refused before the device
        assert e.value.code == idhmc.ERR_BAD_ARG


def test_glm_responses_is_null_safe(idhmc):
    lib = idhmc.load_library()
    a, b = C.c_int64(7), C.c_int64(7)
    assert lib.idhmc_glm_responses(None, C.byref(a), C.byref(b)) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()


def test_bad_calls_are_refused_before_the_device(idhmc):
    grp = np.array([-1, 0, 0, 1, 1, -1], np.int32)
    X, Y1 = AUX.problem_aux("WEIBULL_LOG_LOGSHAPE", 50, 6)
    Y = np.stack([Y1, Y1, Y1])
    Y[1, :, 0] += 0.25
    m = idhmc.GLM(X, Y, idhmc.glm.WEIBULL_LOG_LOGSHAPE, constants=[1.0, 2.0], aux=1, groups=grp, chains_per_response=6)      # D = 6 + 1 + 2

    def refused(what, M=3, R=6, nchains=4, first=0, opt=None, model=m, **fields):
        d = model.glm_desc()
        keep = []
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data_as(C.POINTER(C.c_int32 if v.dtype == np.int32 else C.c_double))
            setattr(d, k, v)
        rc, msg = _create(idhmc, d, M, R, nchains, first, opt)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    lib = idhmc.load_library()
    h = C.c_void_p()
    assert lib.idhmc_create_glm_responses(C.byref(h), 0, 4, 0, None, 3, 6, None, 1) == idhmc.ERR_BAD_ARG
    assert b"null argument" in lib.idhmc_last_error()
    # the responses' own
    for M in (0, -1, -100):
        refused(b"M = %d" % M, M=M)
    for R in (0, -1, -7):
        refused(b"chains_per_response = %d" % R, R=R)
    refused(b"first_chain_id + nchains = 19", nchains=19)                  # M R = 18
    refused(b"first_chain_id + nchains = 19", nchains=1, first=18)
    refused(b"first_chain_id + nchains = 14", nchains=9, first=5, M=2)
    refused(b"first_chain_id + nchains = 5", nchains=5, R=1, M=3)
    # M K n_pad <= 2^27: K = 2, n_pad = 128 -> M <= 2^19 (refused before Y is read)
    refused(b"M = %d" % ((1 << 19) + 1), M=(1 << 19) + 1)
    refused(b"2^27", M=(1 << 19) + 1)
    refused(b"2^27", M=1 << 40)
    refused(b"2^27", M=1 << 62, R=1 << 62)
    for o, word in ((idhmc.default_options(eps_mode=idhmc.EPS_GLOBAL), b"GLOBAL"), (idhmc.default_options(metric_mode=idhmc.METRIC_POOLED), b"POOLED")):
        refused(b"M = 3 responses", opt=o)
        refused(word, opt=o)
        refused(b"different posteriors", opt=o)
        refused(b"different posteriors", opt=o, M=2, R=9)
    # a non-finite value in every plane of Y
    for m_, i, k in ((0, 3, 1), (1, 0, 0), (2, 49, 1)):
        bad = Y.copy()
        bad[m_, i, k] = np.inf
        refused((b"Y[%d, %d] is not finite" % (i, k)) if m_ == 0 else (b"Y[%d, %d, %d] is not finite" % (m_, i, k)), Y=bad)
    bad = Y.copy()
    bad[2, 10, 0] = np.nan
    assert _create(idhmc, m.glm_desc(), 2, 9)[0] in (0, idhmc.ERR_NO_DEVICE)          # (two planes are read: the third is not there)
    refused(b"Y[2, 10, 0] is not finite", Y=bad)
    # everything idhmc_create_glm refuses
    for H in (-1, 5):
        refused(b"H = ", H=H)
    refused(b"groups is NULL", groups=None)
    refused(b"groups must be NULL with H = 0", H=0)
    g = grp.copy()
    g[3] = 2
    refused(b"groups[3] = 2 is outside -1..1", groups=g)
    refused(b"group 1 has no column", groups=np.array([-1, 0, 0, 0, 0, -1], np.int32))
    refused(b"Dx = ", Dx=0)
    for K in (0, 5):
        refused(b"K = ", K=K)
    for nc in (-1, 17):
        refused(b"nc = ", nc=nc)
    for A in (-1, 5):
        refused(b"A = ", A=A)
    refused(b"n = 0", n=0)
    refused(b"X and Y are needed", X=None)
    refused(b"X and Y are needed", Y=None)
    refused(b"constants are needed", constants=None)
    refused(b"c[1] is not finite", constants=np.array([1.0, np.nan]))
    bad = X.copy()
    bad[2, 5] = np.inf
    refused(b"X[2, 5] is not finite", X=bad)
    refused(b"needs HIP source", source=None)
    tau = np.ones(9)
    tau[8] = 0.0
    refused(b"tau[8]", tau=tau)
    mu = np.zeros(9)
    mu[7] = np.nan
    refused(b"mu[7]", mu=mu)
    refused(b"nchains = 0", nchains=0)
    refused(b"chain ids", nchains=2, first=-1)
    big = idhmc.GLM(np.ones((2, 510)), np.zeros((2, 2, 1)), idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, groups=[0, 1] * 255, chains_per_response=2)
    refused(b"SHARED", model=big, M=2, R=2)
    refused(b"D <= 1024", model=big, M=2, R=2, Dx=1022)
    refused(b"2^27", n=(1 << 27) // 128 + 1)                               # refused before X is read
