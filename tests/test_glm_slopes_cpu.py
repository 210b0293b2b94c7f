"""Factor terms that carry a value per observation (glm.term(index, values=), idhmc_create_glm_slopes) without a GPU:
glm.term and glm.factor_values with every refusal, the packing of the three spellings of a plain term, glm.expand_factors with values
against a hand-written matrix, and the C boundary's argument checks, every one answered before the device is looked for.  The arithmetic
is tested on the device against the expanded model (tests/test_gpu_glm_slopes.py)."""
import ctypes as C

import numpy as np
import pytest

from test_glm_factors_cpu import ITEM, SUBJECT, _data, _factors_struct

DOSE = np.array([0.5, -1.25, 0.0, 2.0, -0.0, 3.5, 1.0])        # an exact 0.0 at observation 2, -0.0 at 4


# ---- glm.term and glm.factor_values ---------------------------------------------------------------------------------------------------
def test_term_is_a_small_named_tuple(idhmc):
    g = idhmc.glm
    t = g.term(SUBJECT)
    assert isinstance(t, tuple) and t._fields == ("index", "values", "levels") and t.index is SUBJECT and t.values is None and t.levels is None
    t = g.term(SUBJECT, DOSE, 4)
    assert t.values is DOSE and t.levels == 4 and g.term(SUBJECT, levels=4, values=DOSE) == t


def test_factor_values(idhmc):
    g = idhmc.glm
    assert g.factor_values(None, 7) == (None, None) and g.factor_values([], 7) == (None, None)
    assert g.factor_values([SUBJECT, (ITEM, 3), g.term(SUBJECT), g.term(ITEM, levels=2)], 7) == (None, None)
    has, val = g.factor_values([SUBJECT, g.term(SUBJECT, values=DOSE), (ITEM, 3), g.term(ITEM, values=np.arange(7), levels=2)], 7)
    assert has.dtype == np.int32 and list(has) == [0, 1, 0, 1]
    assert val.dtype == np.float64 and val.shape == (4, 7) and val.flags.c_contiguous
    assert np.array_equal(val[1], DOSE) and np.signbit(val[1, 4]) and np.array_equal(val[3], np.arange(7.0)) and not val[0].any() and not val[2].any()
    lev, idx = g.factor_terms([SUBJECT, g.term(SUBJECT, values=DOSE), (ITEM, 3), g.term(ITEM, values=np.arange(7), levels=2)], 7)
    assert list(lev) == [4, 4, 3, 2] and np.array_equal(idx, [SUBJECT, SUBJECT, ITEM, ITEM])


def test_bad_values_raise_python_side(idhmc):
    g = idhmc.glm
    X, Y = _data()
    nan, inf = DOSE.copy(), DOSE.copy()
    nan[5], inf[1] = np.nan, -np.inf
    bad = [
        ([SUBJECT, g.term(ITEM, values=DOSE[:6])], r"factors\[1\]: values must have one value per observation, shape \(7,\), got \(6,\)"),   # ragged
        ([g.term(SUBJECT, values=np.stack([DOSE, DOSE]))], r"factors\[0\]: values must have one value per observation"),
        ([g.term(SUBJECT, values=1.0)], r"factors\[0\]: values must have one value per observation"),
        ([g.term(SUBJECT, values=DOSE > 0)], r"factors\[0\]: values must be real numbers, got dtype bool"),
        ([SUBJECT, ITEM, g.term(SUBJECT, values=DOSE + 0j)], r"factors\[2\]: values must be real numbers, got dtype complex128"),
        ([g.term(SUBJECT, values=np.array(["a"] * 7))], r"factors\[0\]: values must be real numbers"),
        ([g.term(SUBJECT, values=nan)], r"factors\[0\]: values\[5\] = nan is not finite"),
        ([SUBJECT, g.term(SUBJECT, values=inf)], r"factors\[1\]: values\[1\] = -inf is not finite"),
        # values on an entry that is not a term: a plain tuple is a pair (index, levels) and nothing else
        ([(SUBJECT, DOSE, 4)], r"factors\[0\] must be an index array, a pair \(index, levels\) or a glm.term"),
        ([(SUBJECT, DOSE)], r"factors\[0\]: the number of levels must be a positive integer"),
        # what holds for a pair holds for a term
        ([g.term(SUBJECT, DOSE, 3)], r"factors\[0\]: index 3 is outside 0..2"),
        ([g.term(SUBJECT, DOSE, 0)], "positive integer"),
        ([g.term(SUBJECT.astype(float), DOSE)], "must be integers"),
        ([g.term(SUBJECT, DOSE)] * 5, "at most 4 factors"),
    ]
    for factors, msg in bad:
        with pytest.raises(ValueError, match=msg):
            g.factor_values(factors, 7)
        with pytest.raises(ValueError, match=msg):
            idhmc.GLM(X, Y, g.POISSON_LOG, factors=factors)
        with pytest.raises(ValueError, match=msg):
            g.expand_factors(X, factors)


def test_the_three_spellings_of_a_plain_term_pack_alike(idhmc):
    g = idhmc.glm
    X, Y = _data()
    kw = g.random_intercepts(2, [4])
    ms = [idhmc.GLM(X, Y, g.POISSON_LOG, factors=f, **kw) for f in ([SUBJECT], [(SUBJECT, 4)], [g.term(SUBJECT, levels=4)], [g.term(SUBJECT)])]
    a = ms[0]
    assert a.factor_has is None and a.factor_values is None and (a.F, a.Dd, a.Dx, a.D) == (1, 2, 6, 7)
    for b in ms[1:]:
        assert (b.kind, b.D, b.Dd, b.F, b.Dx, b.H, b.params) == (a.kind, a.D, a.Dd, a.F, a.Dx, a.H, None)
        assert b.levels.tobytes() == a.levels.tobytes() and b.factor_index.tobytes() == a.factor_index.tobytes()
        assert b.mu.tobytes() == a.mu.tobytes() and b.tau.tobytes() == a.tau.tobytes() and b.X.tobytes() == a.X.tobytes()
        assert b.factor_has is None and b.factor_values is None
        da, db = a.glm_desc(), b.glm_desc()
        assert all(getattr(da, k) == getattr(db, k) for k in ("n", "Dx", "K", "A", "H"))
    # a model without factors has the members too
    m = idhmc.GLM(X, Y, g.POISSON_LOG)
    assert m.factor_has is None and m.factor_values is None
    # and the valued model keeps what it was given
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[SUBJECT, g.term(SUBJECT, values=DOSE)], **g.random_effects(2, [4, 4]))
    assert (m.F, m.Dd, m.Dx, m.H, m.D) == (2, 2, 10, 2, 12) and list(m.levels) == [4, 4] and list(m.factor_has) == [0, 1]
    assert np.array_equal(m.factor_values, [np.zeros(7), DOSE]) and m.X.shape == (7, 2)
    assert g.factor_columns(m, 0) == slice(2, 6) and g.factor_columns(m, 1) == slice(6, 10)
    assert g.random_effects is g.random_intercepts


def test_expand_factors_writes_the_values(idhmc):
    g = idhmc.glm
    X = np.arange(14.0).reshape(7, 2)
    E = g.expand_factors(X, [SUBJECT, g.term(SUBJECT, values=DOSE), g.term(ITEM, values=DOSE, levels=3)])     # SUBJECT is shared by two terms
    want = np.array([
        # dense   subject 0..3   dose | subject 0..3        dose | item 0..2
        [0, 1,    1, 0, 0, 0,    0.5, 0, 0, 0,              0, 0.5, 0],
        [2, 3,    0, 0, 1, 0,    0, 0, -1.25, 0,            0, -1.25, 0],
        [4, 5,    0, 1, 0, 0,    0, 0.0, 0, 0,              0.0, 0, 0],          # an exact 0.0 where the level is
        [6, 7,    0, 0, 1, 0,    0, 0, 2.0, 0,              0, 2.0, 0],
        [8, 9,    1, 0, 0, 0,    -0.0, 0, 0, 0,             -0.0, 0, 0],
        [10, 11,  1, 0, 0, 0,    3.5, 0, 0, 0,              0, 3.5, 0],
        [12, 13,  0, 0, 0, 1,    0, 0, 0, 1.0,              1.0, 0, 0]], float)
    assert E.dtype == np.float64 and E.shape == (7, 13) and np.array_equal(E, want)
    # the signs of the zeros: -0.0 only where the value is -0.0
    sign = np.zeros((7, 13), bool)
    sign[1, 8] = sign[1, 11] = True          # -1.25
    sign[4, 6] = sign[4, 10] = True          # -0.0
    assert np.array_equal(np.signbit(E), sign)
    # without values the output is what it was
    assert np.array_equal(g.expand_factors(X, [g.term(SUBJECT), g.term(ITEM, levels=3)]), g.expand_factors(X, [SUBJECT, (ITEM, 3)]))
    assert np.array_equal(g.expand_factors(X, [g.term(SUBJECT, values=np.ones(7))]), g.expand_factors(X, [SUBJECT]))


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _values_struct(values, has):
    from inplacedhmc_jl_amd import _lib
    val = None if values is None else np.ascontiguousarray(values, dtype=np.float64)
    hs = None if has is None else np.ascontiguousarray(has, dtype=np.int32)
    fv = _lib.GlmFactorValues()
    if val is not None:
        fv.values = val.ctypes.data_as(C.POINTER(C.c_double))
    if hs is not None:
        fv.has = hs.ctypes.data_as(C.POINTER(C.c_int32))
    return fv, (val, hs)


def _create(idhmc, desc, factors, values, M=1, R=0, opt=None, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    rc = lib.idhmc_create_glm_slopes(C.byref(h), 0, nchains, 0, C.byref(desc), None, None, None if factors is None else C.byref(factors),
                                     None if values is None else C.byref(values), M, R, None if opt is None else C.byref(opt), 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def _model(idhmc):
    X, Y = _data()
    return idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, factors=[SUBJECT, idhmc.glm.term(ITEM, values=DOSE, levels=3)], groups=[-1, -1, 0, 0, 0, 0, 1, 1, 1])


def test_good_values_pass_every_check(idhmc):
    """a valid descriptor reaches the device (or its absence): with values, with values = NULL, with every flag 0 and
    values->values NULL, and with an unflagged row that holds what a flagged row may not"""
    ok = (0, idhmc.ERR_NO_DEVICE)
    m = _model(idhmc)
    fc, keep = _factors_struct(2, m.levels, m.factor_index)
    junk = m.factor_values.copy()
    junk[0] = np.nan                                              # rows of unflagged terms are not read
    for values, has in ((junk, [0, 1]), (None, [0, 0])):
        fv, keep2 = _values_struct(values, has)
        rc, msg = _create(idhmc, m.glm_desc(), fc, fv)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    rc, msg = _create(idhmc, m.glm_desc(), fc, None)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    # no factors and no values: the context of idhmc_create_glm_local
    X, Y = _data()
    m0 = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, groups=[0, -1])
    rc, msg = _create(idhmc, m0.glm_desc(), None, None)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)


def test_bad_values_are_refused_before_the_device(idhmc):
    m = _model(idhmc)
    lib = idhmc.load_library()

    def refused(what, values=m.factor_values, has=(0, 1), F=2, levels=(4, 3), index=m.factor_index, factors=True, desc=None, **kw):
        fc, keep = _factors_struct(F, levels, index)
        fv, keep2 = _values_struct(values, has)
        rc, msg = _create(idhmc, m.glm_desc() if desc is None else desc, fc if factors else None, fv, **kw)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    h = C.c_void_p()
    fc, keep = _factors_struct(2, m.levels, m.factor_index)
    fv, keep2 = _values_struct(m.factor_values, m.factor_has)
    assert lib.idhmc_create_glm_slopes(C.byref(h), 0, 4, 0, None, None, None, C.byref(fc), C.byref(fv), 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert b"idhmc_create_glm_slopes: null argument" in lib.idhmc_last_error()
    assert lib.idhmc_create_glm_slopes(None, 0, 4, 0, C.byref(m.glm_desc()), None, None, C.byref(fc), C.byref(fv), 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert lib.idhmc_glm_factor_values_get(None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    # values without factor terms
    X, Y = _data()
    m0 = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, groups=[0, -1])
    refused(b"factor values need factor terms (factors is NULL)", factors=False, desc=m0.glm_desc())
    refused(b"factor values need factor terms (factors is given with F = 0)", F=0, desc=m0.glm_desc())
    refused(b"factor values need factor terms", has=(0, 0), factors=False, desc=m0.glm_desc())
    # the flags
    refused(b"has is NULL", has=None)
    for v in (2, -1, 1 << 20):
        refused(b"has[1] = %d must be 0 or 1" % v, has=(1, v))
    refused(b"has[0] = 7 must be 0 or 1", has=(7, 0))
    # the values
    refused(b"values is NULL", values=None)
    refused(b"values is NULL", values=None, has=(1, 0))
    for v in (np.nan, np.inf, -np.inf):
        val = m.factor_values.copy()
        val[1, 6] = v
        refused(b"values[1][6] is not finite", values=val)
    val = m.factor_values.copy()
    val[0, 0] = np.nan
    refused(b"values[0][0] is not finite", values=val, has=(1, 1))
    # everything idhmc_create_glm_factors refuses, first
    refused(b"F = 5 factors must be an integer in 0..4", F=5)
    refused(b"levels is NULL", levels=None)
    refused(b"index is NULL", index=None)
    refused(b"levels[1] = 0: at least one level", levels=(4, 0))
    idx = m.factor_index.copy()
    idx[1, 6] = 3
    refused(b"index[1][6] = 3 is outside 0..2", index=idx)
    refused(b"at least one dense column", levels=(6, 3))
    d = m.glm_desc()
    d.H = 3
    refused(b"group 2 has no column", desc=d)
    d = m.glm_desc()
    d.X = None
    refused(b"X and Y are needed", desc=d)
    refused(b"needs a context made by idhmc_create_glm_responses", opt=idhmc.default_options(eps_mode=idhmc.EPS_PER_RESPONSE))
    refused(b"chains_per_response = 0", M=2, R=0)


def test_the_limit_is_unchanged_by_values(idhmc):
    """n_pad * Lx <= 2^27 with values as without: Dd = 3 and 900 levels at n = 140 000 pass (Lx = 128), n = 2^20 + 1 is refused with the
    same message.  Nothing but the values is read before the refusal (zeros: finite)"""
    g = idhmc.glm
    n = 140000
    m = idhmc.GLM(np.zeros((n, 3)), np.zeros(n), g.POISSON_LOG, factors=[g.term(np.arange(n) % 900, values=np.zeros(n), levels=900)])
    fc, keep = _factors_struct(1, m.levels, m.factor_index)
    fv, keep2 = _values_struct(m.factor_values, m.factor_has)
    rc, msg = _create(idhmc, m.glm_desc(), fc, fv, opt=idhmc.default_options(metric_mode=idhmc.METRIC_SHARED), nchains=2)
    assert rc in (0, idhmc.ERR_NO_DEVICE), (rc, msg)
    n = (1 << 20) + 1
    m = idhmc.GLM(np.zeros((n, 3)), np.zeros(n), g.POISSON_LOG, factors=[g.term(np.zeros(n, np.int32), values=np.zeros(n), levels=2)])
    fc, keep = _factors_struct(1, m.levels, m.factor_index)
    fv, keep2 = _values_struct(m.factor_values, m.factor_has)
    rc, msg = _create(idhmc, m.glm_desc(), fc, fv)
    assert rc == idhmc.ERR_BAD_ARG and b"exceed n_pad * Lx <= 2^27 (at most 1048576)" in msg, (rc, msg)
