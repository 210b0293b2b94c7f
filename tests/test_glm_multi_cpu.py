"""Factor terms with several weighted levels per observation (glm.members, glm.bspline, idhmc_create_glm_multi)
without a device: the expanded matrix by hand, every refusal at the Python layer and at the C boundary (which comes before the device is
touched), the B-spline basis against an exact Cox-de Boor recursion, and smooth_effects against gmrf_effects."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from test_glm_factors_cpu import _data, _factors_struct
from test_glm_slopes_cpu import _values_struct

# five observations, a term of width 2 over 3 levels: two members, one member (an absent entry), a 0.0 weight, a negative weight
INDEX = np.array([[0, 2], [1, -1], [0, 1], [1, 2], [2, -1]])
WEIGHTS = np.array([[0.5, 0.5], [1.0, 99.0], [0.0, -2.0], [0.25, 0.75], [3.0, 7.0]])
ITEM = np.array([1, 0, 1, 1, 0])


def _xy(n=5):
    X, Y = _data(n)
    return X, Y


# ---- the expanded matrix ---------------------------------------------------------------------------------------------------------------
def test_expand_factors_on_a_wide_term_by_hand(idhmc):
    g = idhmc.glm
    X, _ = _xy()
    E = g.expand_factors(X, [g.members(INDEX, WEIGHTS, 3), ITEM])
    want = np.array([[0.5, 0.0, 0.5, 0.0, 1.0],
                     [0.0, 1.0, 0.0, 1.0, 0.0],              # the absent entry's 99.0 is ignored
                     [0.0, -2.0, 0.0, 0.0, 1.0],             # the 0.0 weight is an entry like any other: the column holds 0.0
                     [0.0, 0.25, 0.75, 0.0, 1.0],
                     [0.0, 0.0, 3.0, 1.0, 0.0]])
    assert E.shape == (5, 2 + 3 + 2)
    assert np.array_equal(E[:, :2], X) and np.array_equal(E[:, 2:], want)
    # without weights every present entry is 1.0, and a level nobody has is a column of zeros
    E1 = g.expand_factors(X, [g.members(INDEX, levels=4)])
    assert E1.shape == (5, 2 + 4) and np.array_equal(E1[:, 2:], np.array([[1, 0, 1, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 1, 1, 0], [0, 0, 1, 0.0]]))


def test_constructor_keeps_the_members(idhmc):
    g = idhmc.glm
    X, Y = _xy()
    dose = np.arange(5.0)
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[g.members(INDEX, WEIGHTS, 3), ITEM, g.term(ITEM, values=dose)])
    assert (m.Dd, m.F, m.Dx, m.D) == (2, 3, 2 + 3 + 2 + 2, 9) and list(m.levels) == [3, 2, 2]
    assert m.member_width.dtype == np.int32 and list(m.member_width) == [2, 1, 1]
    assert m.member_index.dtype == np.int32 and m.member_index.flags.c_contiguous and m.member_values.flags.c_contiguous
    assert np.array_equal(m.member_index, [INDEX[:, 0], INDEX[:, 1], ITEM, ITEM])
    assert np.array_equal(m.member_values, [WEIGHTS[:, 0], np.where(INDEX[:, 1] >= 0, WEIGHTS[:, 1], 0.0), np.ones(5), dose])
    assert m.factor_has is None and m.factor_values is None        # every term's values are in the table
    assert np.array_equal(m.factor_index[0], INDEX[:, 0])
    assert g.factor_columns(m, 0) == slice(2, 5) and g.factor_columns(m, 2) == slice(7, 9)
    # a model without such an entry has no table
    m0 = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[ITEM])
    assert m0.member_width is None and m0.member_index is None and m0.member_values is None
    assert g.factor_members([ITEM], 5) == (None, None, None)


def test_constructor_validates_the_members(idhmc):
    g = idhmc.glm
    X, Y = _xy()

    def bad(what, factors, **kw):
        with pytest.raises(ValueError, match=what):
            idhmc.GLM(X, Y, g.POISSON_LOG, factors=factors, **kw)

    def idx(i, m, v):
        a = INDEX.copy()
        a[i, m] = v
        return a

    bad(r"width 5", [g.members(np.zeros((5, 5), int))])
    bad(r"shape \(5, M\)", [g.members(np.zeros(5, int))])
    bad(r"shape \(5, M\)", [g.members(np.zeros((4, 2), int))])
    bad(r"sum to 9 planes: at most 8", [g.members(np.tile(np.arange(4), (5, 1))), g.members(np.tile(np.arange(4), (5, 1))), ITEM])
    bad(r"factors\[0\]: plane 1, observation 3: level 3 is outside -1..2", [g.members(idx(3, 1, 3), WEIGHTS, 3)])
    bad(r"factors\[0\]: plane 0, observation 2: level -2 is outside -1..2", [g.members(idx(2, 0, -2), WEIGHTS, 3)])
    bad(r"factors\[1\]: plane 0, observation 4: an absent entry \(-1\) in a term of width 1", [ITEM, g.members(np.array([[0], [1], [0], [1], [-1]]))])
    bad(r"factors\[0\]: plane 1, observation 2: a present entry behind an absent one", [g.members(idx(2, 0, -1), WEIGHTS, 3)])
    bad(r"factors\[0\]: plane 1, observation 0: level 0 after level 0", [g.members(idx(0, 1, 0), WEIGHTS, 3)])
    bad(r"factors\[0\]: plane 1, observation 3: level 0 after level 1", [g.members(idx(3, 1, 0), WEIGHTS, 3)])
    for v in (np.nan, np.inf):
        w = WEIGHTS.copy()
        w[3, 1] = v
        bad(r"factors\[0\]: plane 1, observation 3: the weight is not finite", [g.members(INDEX, w, 3)])
    w = WEIGHTS.copy()
    w[1, 1] = np.nan                                              # the weight of an absent entry is ignored
    idhmc.GLM(X, Y, g.POISSON_LOG, factors=[g.members(INDEX, w, 3)])
    bad(r"weights must have the shape of index", [g.members(INDEX, WEIGHTS[:, :1], 3)])
    bad(r"weights must be real numbers", [g.members(INDEX, WEIGHTS > 0, 3)])
    bad(r"must be integers", [g.members(INDEX.astype(float), WEIGHTS, 3)])
    bad(r"the number of levels must be a positive integer", [g.members(INDEX, WEIGHTS, 0)])
    # a wide term is in no pair and no block
    wide, wide2 = g.members(INDEX, WEIGHTS, 3), g.members(INDEX, None, 3)
    bad(r"correlated: pair names term 0, a glm.members term of width 2", [wide, (ITEM, 3)], correlated=[g.pair(0, 1)])
    bad(r"correlated: block names term 1, a glm.members term of width 2", [(ITEM, 3), wide2, (ITEM, 3)], correlated=[g.block((0, 1, 2))])
    # a term of width 1 given as members may be paired
    idhmc.GLM(X, Y, g.POISSON_LOG, factors=[g.members(ITEM[:, None], None, 3), (ITEM, 3), wide], correlated=[g.pair(0, 1)])


# ---- the C boundary --------------------------------------------------------------------------------------------------------------------
def _members_struct(width, index, values):
    from inplacedhmc_jl_amd import _lib
    keep = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((width, np.int32), (index, np.int32), (values, np.float64))]
    mm = _lib.GlmMembers()
    if keep[0] is not None:
        mm.width = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
    if keep[1] is not None:
        mm.index = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
    if keep[2] is not None:
        mm.values = keep[2].ctypes.data_as(C.POINTER(C.c_double))
    return mm, keep


def _create(idhmc, desc, factors, members, values=None, pairs=None, block=None, M=1, R=0, nchains=4):
    lib = idhmc.load_library()
    h = C.c_void_p()
    ref = lambda x: None if x is None else C.byref(x)
    rc = lib.idhmc_create_glm_multi(C.byref(h), 0, nchains, 0, C.byref(desc), None, None, ref(factors), ref(values), ref(pairs), None, None,
                                    ref(block), ref(members), M, R, None, 1)
    if rc == 0:
        lib.idhmc_destroy(h)
    return rc, lib.idhmc_last_error()


def _c_model(idhmc, **kw):
    g = idhmc.glm
    X, Y = _xy()
    return idhmc.GLM(X, Y, g.POISSON_LOG, factors=[g.members(INDEX, WEIGHTS, 3), (ITEM, 3), (ITEM, 3)], **kw)


def test_good_members_pass_every_check(idhmc):
    """a valid table reaches the device (or its absence): a wide one, one of width 1 only, one without values, and members = NULL"""
    ok = (0, idhmc.ERR_NO_DEVICE)
    m = _c_model(idhmc)
    fc, k1 = _factors_struct(3, m.levels, None)
    for values in (m.member_values, None):
        mm, k2 = _members_struct(m.member_width, m.member_index, values)
        rc, msg = _create(idhmc, m.glm_desc(), fc, mm)
        assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    mm, k2 = _members_struct([1, 1, 1], m.member_index[[0, 2, 3]].clip(0), None)
    rc, msg = _create(idhmc, m.glm_desc(), fc, mm)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)
    fc1, k3 = _factors_struct(3, m.levels, m.member_index[[0, 2, 3]].clip(0))
    rc, msg = _create(idhmc, m.glm_desc(), fc1, None)
    assert rc in ok and (rc == 0 or b"no HIP device" in msg), (rc, msg)


def test_bad_members_are_refused_before_the_device(idhmc):
    m = _c_model(idhmc)
    lib = idhmc.load_library()
    n = 5

    def refused(what, width=(2, 1, 1), index=None, mvalues="given", levels=(3, 3, 3), F=3, findex=None, factors=True, desc=None, **kw):
        index = m.member_index if index is None else index
        fc, k1 = _factors_struct(F, levels, findex)
        mm, k2 = _members_struct(width, index, m.member_values if isinstance(mvalues, str) else mvalues)
        rc, msg = _create(idhmc, m.glm_desc() if desc is None else desc, fc if factors else None, mm, **kw)
        assert rc == idhmc.ERR_BAD_ARG and what in msg, (what, rc, msg)

    def idx(p, i, v):
        a = m.member_index.copy()
        a[p, i] = v
        return a

    h = C.c_void_p()
    assert lib.idhmc_create_glm_multi(C.byref(h), 0, 4, 0, None, None, None, None, None, None, None, None, None, None, 1, 0, None, 1) == idhmc.ERR_BAD_ARG
    assert b"idhmc_create_glm_multi: null argument" in lib.idhmc_last_error()
    assert lib.idhmc_glm_members_get(None, None, None, None) == idhmc.ERR_BAD_ARG and b"null argument" in lib.idhmc_last_error()
    for w in (0, 5, -1):
        refused(b"width[0] = %d of term 0 must be in 1..4" % w, width=(w, 1, 1))
    wide = np.tile(np.arange(3, dtype=np.int32)[:, None], (3, n))          # three planes 0, 1, 2 per term
    refused(b"the widths sum to P = 9 planes: at most 8", width=(3, 3, 3), index=wide, mvalues=None)
    refused(b"members need width and index (width is NULL)", width=None)
    mm, k = _members_struct((2, 1, 1), None, None)
    fc, k1 = _factors_struct(3, (3, 3, 3), None)
    rc, msg = _create(idhmc, m.glm_desc(), fc, mm)
    assert rc == idhmc.ERR_BAD_ARG and b"members need width and index (index is NULL)" in msg
    # members without factors
    X, Y = _xy()
    m0 = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, groups=[0, -1])
    refused(b"members need factor terms: factors gives F and levels (factors is NULL)", factors=False, desc=m0.glm_desc())
    refused(b"members need factor terms: factors gives F and levels (factors is given with F = 0)", F=0, desc=m0.glm_desc())
    # both index sources, both value sources
    refused(b"members and factors->index are both given", findex=m.member_index[[0, 2, 3]].clip(0))
    fv, k3 = _values_struct(np.ones((3, n)), np.ones(3, np.int32))
    refused(b"members and factor values are both given", values=fv)
    # the entries, each naming term, plane and observation
    refused(b"term 0, plane 1, observation 3: level 3 is outside -1..2", index=idx(1, 3, 3))
    refused(b"term 0, plane 0, observation 2: level -2 is outside -1..2", index=idx(0, 2, -2))
    refused(b"term 2, plane 3, observation 4: level 3 is outside -1..2", index=idx(3, 4, 3))
    refused(b"term 1, plane 2, observation 4: an absent entry (-1) in a term of width 1", index=idx(2, 4, -1))
    refused(b"term 0, plane 1, observation 2: a present entry (level 1) behind an absent one", index=idx(0, 2, -1))
    refused(b"term 0, plane 1, observation 0: level 0 after level 0: the levels of an observation must be strictly ascending", index=idx(1, 0, 0))
    refused(b"term 0, plane 1, observation 3: level 0 after level 1", index=idx(1, 3, 0))
    for v in (np.nan, np.inf, -np.inf):
        val = m.member_values.copy()
        val[1, 3] = v
        refused(b"term 0, plane 1, observation 3: the value is not finite", mvalues=val)
    val = m.member_values.copy()
    val[1, 1] = np.nan                                             # (observation 1 has no second member: its value is not read)
    mm, k = _members_struct((2, 1, 1), m.member_index, val)
    rc, msg = _create(idhmc, m.glm_desc(), fc, mm)
    assert rc in (0, idhmc.ERR_NO_DEVICE), (rc, msg)
    # a wide term in a pair or a block
    from test_glm_block_cpu import _block_struct
    from test_glm_corr_cpu import _pairs_struct
    mp_ = _c_model(idhmc, correlated=[idhmc.glm.pair(1, 2)])
    pp, k4 = _pairs_struct(1, [0], [1], [2.0])
    refused(b"pair 0 names term 0, which has width 2", desc=mp_.glm_desc(), pairs=pp)
    pp, k4 = _pairs_struct(1, [1], [0], [2.0])
    refused(b"pair 0 names term 0, which has width 2", desc=mp_.glm_desc(), pairs=pp)
    mb = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, factors=[(ITEM, 3)] * 3, correlated=[idhmc.glm.block((0, 1, 2))])
    bk, k5 = _block_struct(3, (1, 2, 0), 2.0)
    refused(b"the block names term 0, which has width 2", desc=mb.glm_desc(), block=bk)
    # everything idhmc_create_glm_block refuses
    refused(b"F = 5 factors must be an integer in 0..4", F=5)
    refused(b"levels[1] = 0: at least one level", levels=(3, 0, 3))
    refused(b"chains_per_response = 0", M=2, R=0)


# ---- the B-spline basis ----------------------------------------------------------------------------------------------------------------
def _cox_de_boor(i, p, x, t, last):
    """B_{i,p}(x) on the knots t, exactly: the recursion as it is written down, half-open intervals, the last one closed"""
    if p == 0:
        if x == t[last]:                                           # x = hi belongs to the last interval of [lo, hi], and to no other
            return Fraction(int(i == last - 1))
        return Fraction(int(t[i] <= x < t[i + 1]))
    a = (x - t[i]) / (t[i + p] - t[i]) * _cox_de_boor(i, p - 1, x, t, last)
    b = (t[i + p + 1] - x) / (t[i + p + 1] - t[i + 1]) * _cox_de_boor(i + 1, p - 1, x, t, last)
    return a + b


@pytest.mark.parametrize("degree, n_basis, lo, hi", [(3, 24, None, None), (3, 4, -1.0, 2.5), (2, 7, 0.0, 1.0), (1, 5, None, None), (3, 9, 0.1, 0.7)])
def test_bspline_against_exact_cox_de_boor(idhmc, degree, n_basis, lo, hi):
    """every value within 32 * 2^-53 of the exact recursion on the same knots: values lie in [0, 1], and degree 3 is at most three
    levels of convex combinations with a few roundings each"""
    g = idhmc.glm
    rng = np.random.default_rng(degree * 100 + n_basis)
    a, b = (0.0, 1.0) if lo is None else (lo, hi)
    x = np.r_[a, b, rng.uniform(a, b, 60)]
    t = g.bspline_knots(n_basis, degree, a, b)
    x = np.r_[x, t[degree:n_basis + 1], np.nextafter(t[degree + 1:n_basis], -np.inf)]     # on the knots and just below them
    mem = g.bspline(x, n_basis, degree, lo, hi)                    # (lo, hi None: the data range, which is [a, b])
    assert isinstance(mem, g.Members) and mem.levels == n_basis
    assert mem.index.shape == mem.weights.shape == (x.size, degree + 1)
    assert (np.diff(mem.index, axis=1) == 1).all()                 # strictly ascending, adjacent
    assert mem.index.min() >= 0 and mem.index.max() <= n_basis - 1
    assert mem.index[0, 0] >= 0 and mem.index[1, -1] == n_basis - 1          # x = lo and x = hi land inside 0 .. N-1
    tol = 32 * 2.0 ** -53
    tf = [Fraction(float(v)) for v in t]
    for i in range(x.size):
        xf = Fraction(float(x[i]))
        exact = [_cox_de_boor(int(k), degree, xf, tf, n_basis) for k in mem.index[i]]
        # the functions outside the row are zero at x: the row holds the whole basis
        assert sum(exact) == 1
        for k in range(degree + 1):
            assert abs(Fraction(float(mem.weights[i, k])) - exact[k]) <= Fraction(tol), (i, k, float(x[i]), mem.weights[i, k], float(exact[k]))
        assert abs(sum(Fraction(float(w)) for w in mem.weights[i]) - 1) <= Fraction(tol)
    assert (mem.weights >= 0).all() and (mem.weights <= 1).all()
    # the term passes GLM()'s checks as it stands
    X, Y = _data(x.size)
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[mem])
    assert list(m.member_width) == [degree + 1] and list(m.levels) == [n_basis]


def test_bspline_refuses(idhmc):
    g = idhmc.glm
    x = np.linspace(0.0, 1.0, 9)
    for what, args in ((r"x\[8\] = 1.0 is outside \[lo, hi\]", (x, 6, 3, 0.0, 0.9)), (r"x\[0\] = 0.0 is outside", (x, 6, 3, 0.1, 1.0)),
                       (r"degree = 4 must be 1, 2 or 3", (x, 6, 4)), (r"degree = 0 must be", (x, 6, 0)),
                       (r"n_basis = 3 must be an integer in degree \+ 1 = 4", (x, 3)), (r"finite interval of positive length", (x, 6, 3, 1.0, 1.0)),
                       (r"finite numbers", (np.r_[x, np.nan], 6)), (r"positive length", (np.zeros(4), 6))):
        with pytest.raises(ValueError, match=what):
            g.bspline(*args)


# ---- smooth_effects ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_smooth_effects_is_gmrf_effects_on_the_term(idhmc, order):
    g = idhmc.glm
    prec = g.rw2_precision if order == 2 else g.rw1_precision
    kw = g.smooth_effects(2, [20, 8], order=order, sum_to_zero=0.5, levels=[3], scale=g.half_normal(2.0))
    want = g.gmrf_effects(2, [20, 8, 3], [g.gmrf(0, g.scale_precision(prec(20)), 0.5), g.gmrf(1, g.scale_precision(prec(8)), 0.5)],
                          scale=g.half_normal(2.0))
    assert sorted(kw) == sorted(want)
    for k in want:
        if k == "gmrf":
            assert len(kw[k]) == 2
            for a, b in zip(kw[k], want[k]):
                assert a.term == b.term and a.kappa == b.kappa
                assert all(np.array_equal(u, v) for u, v in zip(a[1:], b[1:]) if isinstance(u, np.ndarray))
        else:
            assert np.array_equal(kw[k], want[k]), k
    # and it makes y ~ 1 + s(x) + (1 | item)
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 1, 40)
    X, Y = np.ones((40, 2)), rng.poisson(2.0, 40).astype(float)
    m = idhmc.GLM(X, Y, g.POISSON_LOG, factors=[g.bspline(x, 20), g.bspline(x, 8, degree=2), rng.integers(0, 3, 40)], **kw)
    assert (m.G, m.H, m.F) == (2, 3, 3) and list(m.member_width) == [4, 3, 1] and m.D == 2 + 31 + 3
    with pytest.raises(ValueError, match="order = 3"):
        g.smooth_effects(2, [20], order=3)
    with pytest.raises(ValueError, match="one or two smooths"):
        g.smooth_effects(2, [5, 5, 5])
