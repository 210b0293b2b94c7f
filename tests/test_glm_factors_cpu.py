"""Factor terms by level index (GLM(..., factors=), idhmc_create_glm_factors) without a GPU: the constructor's
validation and packing, glm.expand_factors against a hand-written matrix, glm.factor_columns, glm.random_intercepts, and the C boundary's
argument checks, every one answered before the device is looked for.  The arithmetic is tested on the device against the expanded model
(tests/test_gpu_glm_factors.py)."""
import ctypes as C

import numpy as np
import pytest


def _data(n=7, Dd=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, Dd)), rng.poisson(2.0, n).astype(float)


SUBJECT = np.array([0, 2, 1, 2, 0, 0, 3])          # 4 levels
ITEM = np.array([1, 1, 0, 1, 0, 1, 0])             # 2 levels


# ---- the constructor ------------------------------------------------------------------------------------------------------------------
def test_constructor_keeps_the_factors(idhmc):
    g = idhmc.glm
    X, Y = _data()
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[SUBJECT, (ITEM, 3)])
    assert (m.Dd, m.F, m.Dx, m.D, m.n) == (2, 2, 2 + 4 + 3, 9, 7)
    assert m.levels.dtype == np.int32 and list(m.levels) == [4, 3]
    assert m.factor_index.dtype == np.int32 and m.factor_index.shape == (2, 7) and m.factor_index.flags.c_contiguous
    assert np.array_equal(m.factor_index, [SUBJECT, ITEM])
    assert m.params is None and m.X.shape == (7, 2)              # handed over in parts: X holds the dense columns only
    d = m.glm_desc()
    assert (d.n, d.Dx, d.K, d.A, d.H) == (7, 9, 1, 0, 0)
    assert g.factor_columns(m, 0) == slice(2, 6) and g.factor_columns(m, 1) == slice(6, 9)
    for f in (-1, 2, True, 0.0):
        with pytest.raises(ValueError, match="factors 0..1"):
            g.factor_columns(m, f)
    with pytest.raises(ValueError, match="no factor terms"):
        g.factor_columns(idhmc.GLM(X, Y, g.POISSON_LOG), 0)
    # groups, local scales and priors count the level columns
    kw = g.random_intercepts(2, [4, 3])
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[(SUBJECT, 4), (ITEM, 3)], local=[0] * 2 + [1, 0, 0, 1] + [0] * 3,
                  groups=kw["groups"], prior_mu=0.0, prior_tau=1.0)
    assert (m.H, m.J, m.D) == (2, 2, 9 + 2 + 2)
    with pytest.raises(ValueError, match=r"one entry per column of the model \(9\)"):
        idhmc.GLM(X, Y, g.POISSON_LOG, factors=[SUBJECT, (ITEM, 3)], groups=[-1, -1])
    with pytest.raises(ValueError, match="D <= 1024"):
        idhmc.GLM(X, Y, g.POISSON_LOG, factors=[(SUBJECT, 600), (ITEM, 423)])


def test_bad_factors_raise_python_side(idhmc):
    g = idhmc.glm
    X, Y = _data()
    bad = [
        (SUBJECT, "must be a list"),                                # a bare array, not a list of them
        ([SUBJECT[:6]], r"one index per observation, shape \(7,\)"),
        ([SUBJECT, ITEM[:3]], r"factors\[1\] must have one index per observation"),      # ragged
        ([np.stack([SUBJECT, SUBJECT])], "one index per observation"),
        ([SUBJECT - 1], r"factors\[0\]: a level index is 0 .. N-1, got -1"),
        ([SUBJECT, -ITEM], r"factors\[1\]: a level index is 0 .. N-1, got -1"),
        ([SUBJECT.astype(float)], "must be integers"),
        ([SUBJECT > 0], "must be integers"),
        ([(SUBJECT, 3)], r"index 3 is outside 0..2"),
        ([(SUBJECT, 0)], "positive integer"),
        ([(SUBJECT, 4.0)], "positive integer"),
        ([(SUBJECT, 4, 1)], "a pair"),
        ([SUBJECT] * 5, "at most 4 factors"),
    ]
    for factors, msg in bad:
        with pytest.raises(ValueError, match=msg):
            idhmc.GLM(X, Y, g.POISSON_LOG, factors=factors)
        if isinstance(factors, list):
            with pytest.raises(ValueError, match=msg):
                g.expand_factors(X, factors)


def test_no_factor_packs_to_the_same_bytes(idhmc):
    g = idhmc.glm
    X, Y = _data()
    plain = idhmc.GLM(X, Y, g.POISSON_LOG, None, 0.1, 0.7)
    for kw in ({"factors": None}, {"factors": []}, {"factors": ()}):
        m = idhmc.GLM(X, Y, g.POISSON_LOG, None, 0.1, 0.7, **kw)
        assert m.kind == plain.kind and m.D == plain.D and m.params.tobytes() == plain.params.tobytes()
        assert m.mu.tobytes() == plain.mu.tobytes() and m.tau.tobytes() == plain.tau.tobytes()
        assert (m.F, m.Dd, m.levels, m.factor_index) == (0, 2, None, None)
    assert (plain.F, plain.Dd) == (0, 2)


def test_expand_factors_is_the_indicator_matrix(idhmc):
    g = idhmc.glm
    X = np.arange(14.0).reshape(7, 2)
    E = g.expand_factors(X, [SUBJECT, (ITEM, 3)])
    want = np.array([
        # dense   subject 0..3   item 0..2
        [0, 1,    1, 0, 0, 0,    0, 1, 0],
        [2, 3,    0, 0, 1, 0,    0, 1, 0],
        [4, 5,    0, 1, 0, 0,    1, 0, 0],
        [6, 7,    0, 0, 1, 0,    0, 1, 0],
        [8, 9,    1, 0, 0, 0,    1, 0, 0],
        [10, 11,  1, 0, 0, 0,    0, 1, 0],
        [12, 13,  0, 0, 0, 1,    1, 0, 0]], float)
    assert E.dtype == np.float64 and np.array_equal(E, want)
    assert not np.signbit(E).any()                                # +0, never -0
    for kw in (None, []):
        E0 = g.expand_factors(X, kw)
        assert np.array_equal(E0, X) and E0 is not X
    m = idhmc.GLM(X, np.ones(7), g.POISSON_LOG, factors=[SUBJECT, (ITEM, 3)])
    assert E.shape[1] == m.Dx and np.array_equal(E[:, g.factor_columns(m, 1)], want[:, 6:])


def test_random_intercepts_keywords(idhmc):
    g = idhmc.glm
    kw = g.random_intercepts(3, [4, 2], A=1, scale=g.half_student_t(3.0, 0.5), coefficients=g.student_t(4.0), aux=g.exponential(2.0))
    assert sorted(kw) == ["groups", "prior_kind", "prior_mu", "prior_nu", "prior_tau"]
    assert kw["groups"].dtype == np.int32 and list(kw["groups"]) == [-1] * 3 + [0] * 4 + [1] * 2
    D = 3 + 6 + 1 + 2
    assert all(kw[k].shape == (D,) for k in ("prior_mu", "prior_tau", "prior_kind", "prior_nu"))
    assert list(kw["prior_kind"]) == [g.PRIOR_STUDENT_T] * 3 + [g.PRIOR_NORMAL] * 6 + [g.PRIOR_LOG_EXPONENTIAL] + [g.PRIOR_LOG_HALF_STUDENT_T] * 2
    assert list(kw["prior_nu"]) == [4.0] * 3 + [0.0] * 7 + [3.0] * 2
    assert np.array_equal(kw["prior_mu"][-2:], np.log([0.5, 0.5])) and np.all(kw["prior_tau"][3:] == 1.0)
    # they make the model they describe
    X, Y = _data(Dd=3)
    m = idhmc.GLM(X, Y, g.GAUSSIAN_IDENTITY_LOGSIGMA, aux=1, factors=[SUBJECT, ITEM], **kw)
    assert (m.Dx, m.A, m.H, m.D) == (9, 1, 2, D) and np.array_equal(m.groups[g.factor_columns(m, 1)], [1, 1])
    # defaults: N(0, 1) everywhere, one group per factor
    kw = g.random_intercepts(1, [5])
    assert list(kw["groups"]) == [-1] + [0] * 5 and not kw["prior_kind"].any() and np.all(kw["prior_tau"] == 1.0)
    with pytest.raises(ValueError, match="at most 4 factors"):
        g.random_intercepts(2, [3] * 5)                         # H > 4
    for Dd, lev in ((0, [3]), (2, []), (2, [3, 0])):
        with pytest.raises(ValueError):
            g.random_intercepts(Dd, lev)
    with pytest.raises(ValueError, match="Dd = 2"):
        g.random_intercepts(2, [3], coefficients=[g.normal()] * 3)


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _factors_struct(F, levels, index):
    from inplacedhmc_jl_amd import _lib
    lev = None if levels is None else np.ascontiguousarray(levels, dtype=np.int32)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    fc = _lib.GlmFactors(F=F)
    if lev is not None:
        fc.levels = lev.ctypes.data_as(C.POINTER(C.c_int32))
    if idx is not None:
        fc.index = idx.ctypes.data_as(C.POINTER(C.c_int32))
    return fc, (lev, idx)


def _create(idhmc, desc, factors, M=1, R=0, opt=None, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create_glm_factors(C.byref(h), 0, nchains, 0, C.byref(desc), None, None, None if factors is None else C.byref(factors),
                                      M, R, None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def _model(idhmc, **kw):
    X, Y = _data()
    return idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, factors=[SUBJECT, (ITEM, 3)], groups=[-1, -1, 0, 0, 0, 0, 1, 1, 1], **kw)


def test_good_factors_pass_every_check(idhmc):
    """a valid descriptor reaches the device (or its absence), with the factors, without them, and with F = 0"""
    ok = (0, idhmc.ERR_NO_DEVICE)
    m = _model(idhmc)
    fc, keep = _factors_struct(2, m.levels, m.factor_index)
    rc, msg = _create(idhmc, m.glm_desc(), fc)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    X, Y = _data()
    m0 = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, groups=[0, -1])
    for fc0 in (None, _factors_struct(0, None, None)[0], _factors_struct(0, [9], None)[0]):
        rc, msg = _create(idhmc, m0.glm_desc(), fc0)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)


def test_bad_factors_are_refused_before_the_device(idhmc):
    m = _model(idhmc)
    lib = idhmc.load_library()

    def refused(what, F=2, levels=(4, 3), index=m.factor_index, desc=None, **kw):
        fc, keep = _factors_struct(F, levels, index)
        rc, msg = _create(idhmc, m.glm_desc() if desc is None else desc, fc, **kw)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    h = C.c_void_p()
    fc, keep = _factors_struct(2, m.levels, m.factor_index)
    assert lib.idhmc_create_glm_factors(C.byref(h), 0, 4, 0, None, None, None, C.byref(fc), 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert b"null argument" in lib.idhmc_last_error()
    assert lib.idhmc_glm_factors_get(None, None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    for F in (-1, 5, 1 << 20):
        refused(b"F = %d factors must be an integer in 0..4" % F, F=F)
    refused(b"levels is NULL", levels=None)
    refused(b"index is NULL", index=None)
    for N in (0, -3):
        refused(b"levels[1] = %d: at least one level" % N, levels=(4, N))
    idx = m.factor_index.copy()
    idx[0, 3] = 4
    refused(b"index[0][3] = 4 is outside 0..3", index=idx)
    idx = m.factor_index.copy()
    idx[1, 6] = -1
    refused(b"index[1][6] = -1 is outside 0..2", index=idx)
    # Dd = Dx - sum of levels < 1
    refused(b"at least one dense column", levels=(6, 3))
    refused(b"at least one dense column", levels=(4, 30))
    # what the other functions refuse: groups over the Dx columns, responses, the options
    d = m.glm_desc()
    d.H = 3
    refused(b"group 2 has no column", desc=d)
    d = m.glm_desc()
    d.X = None
    refused(b"X and Y are needed", desc=d)
    refused(b"needs a context made by idhmc_create_glm_responses", opt=idhmc.default_options(eps_mode=idhmc.EPS_PER_RESPONSE))
    refused(b"chains_per_response = 0", M=2, R=0)
    # a non-finite dense entry is found at its place in the n x Dd matrix
    X, Y = _data()
    X[4, 1] = np.nan
    mb = _model(idhmc)
    mb.X = X
    refused(b"X[4, 1] is not finite", desc=mb.glm_desc())


def test_the_limit_counts_the_stored_columns(idhmc):
    """n_pad * Lx <= 2^27 for a model with factors, n_pad * L <= 2^27 for its expansion: Dd = 3 and 900 levels at n = 140 000 pass the
    first (Lx = 128) and fail the second (L = 1024); at n_pad * 128 > 2^27 the factor model is refused too.  Nothing is read before the
    refusal, so the matrices are never-touched zero pages"""
    g = idhmc.glm
    n = 140000
    m = idhmc.GLM(np.zeros((n, 3)), np.zeros(n), g.POISSON_LOG, factors=[(np.arange(n) % 900, 900)])
    fc, keep = _factors_struct(1, m.levels, m.factor_index)
    rc, msg = _create(idhmc, m.glm_desc(), fc, opt=idhmc.default_options(metric_mode=idhmc.METRIC_SHARED), nchains=2)
    assert rc in (0, idhmc.ERR_NO_DEVICE), (rc, msg)
    d = m.glm_desc()
    wide = np.zeros((n, 903))
    d.X = wide.ctypes.data_as(C.POINTER(C.c_double))
    rc, msg = _create(idhmc, d, None, opt=idhmc.default_options(metric_mode=idhmc.METRIC_SHARED), nchains=2)
    assert rc == idhmc.ERR_BAD_ARG and b"exceed n_pad * L <= 2^27 (at most 131072)" in msg, (rc, msg)
    n = (1 << 20) + 1
    m = idhmc.GLM(np.zeros((n, 3)), np.zeros(n), g.POISSON_LOG, factors=[(np.zeros(n, np.int32), 2)])
    fc, keep = _factors_struct(1, m.levels, m.factor_index)
    rc, msg = _create(idhmc, m.glm_desc(), fc)
    assert rc == idhmc.ERR_BAD_ARG and b"exceed n_pad * Lx <= 2^27 (at most 1048576)" in msg, (rc, msg)
