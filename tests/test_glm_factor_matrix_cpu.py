"""Factor and slope terms (DESIGN sections 20 and 21) on the shapes and flags that tests/test_gpu_glm_factors.py and
tests/test_gpu_glm_slopes.py leave out: a stored width Lx of 256, 384 and L itself, four blocks of observations, four terms, and on the
matrix cores auxiliary coordinates, K = 2, local scales with and without a slab, H = 4, no priors at all.  This file holds the one table
of shapes that tests/test_gpu_glm_factor_matrix.py runs on the device, and pins without a GPU the reference the device is compared
with: the indicator-and-value matrix is built here from its definition, must have the bits of glm.expand_factors, and section 19's C
restatement (tests/test_glm_local_cpu.py) on it must agree with the numpy closed form, which shares no code with it, within 1e-12 of
the magnitude of the terms summed.  It also asserts section 21's precondition (no product of a value with a coefficient or a residual
anywhere near underflow at the starts the tests use) and that idhmc_create_glm_slopes accepts every shape."""
import ctypes as C

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
import test_glm_cpu as FLAT
from test_glm_hier_cpu import SHAPE, consts, source
from test_glm_local_cpu import c_source_local, local_priors, numpy_density_local, oracle_params_local, start_local
from test_gpu_glm_factors import same_bits

NS = (130, 385)          # two blocks (the second of two observations) and four (the last of one)

# name: (family, Dd, (levels, valued) per term, a group per term, local scales on every third level: None, "no slab" or the slab's scale,
# priors, D, padded length L, stored width Lx, matrix cores)
SHAPES = {
    "wide coop": ("POISSON_LOG", 140, ((20, False), (30, True)), True, None, "mixed", 192, 256, 256, 1),
    "aux at 256": ("GAUSSIAN_IDENTITY_LOGSIGMA", 100, ((60, True), (40, False)), True, 2.0, "mixed", 237, 256, 128, 1),
    "aux 4, K 2": ("TEST_A4", 20, ((15, True), (15, False)), True, 2.0, "mixed", 66, 128, 128, 1),
    "four terms coop": ("POISSON_LOG", 10, ((6, False), (5, True), (1, True), (9, False)), True, "no slab", "mixed", 42, 128, 128, 1),
    "bare": ("BERNOULLI_LOGIT", 33, ((40, True),), False, None, "normal", 73, 128, 128, 1),
    "Lx 256 of 512": ("GAUSSIAN_IDENTITY_LOGSIGMA", 200, ((120, True), (60, False)), True, 2.0, "mixed", 443, 512, 256, 0),
    "Lx 384 of 512": ("GAUSSIAN_IDENTITY_LOGSIGMA", 300, ((100, True),), True, None, "mixed", 402, 512, 384, 0),
    "Lx is L": ("GAUSSIAN_IDENTITY_LOGSIGMA", 400, ((50, False),), True, None, "mixed", 452, 512, 512, 0),
    "four terms wave": ("GAUSSIAN_IDENTITY_LOGSIGMA", 130, ((80, True), (70, False), (50, True), (30, False)), True, 1.5, "mixed", 442, 512, 256, 0),
}
# the chain counts whose start_local positions some test of the two files uses
STARTS = (6, 16, 18, 33)


def dims(shape):
    """Dx, A, H, J"""
    family, Dd, terms, grouped, loc = SHAPES[shape][:5]
    Dx = Dd + sum(N for N, v in terms)
    return Dx, SHAPE[family][2], len(terms) if grouped else 0, len(range(Dd, Dx, 3)) if loc else 0


def offsets(shape):
    """off_f: the column of level 0 of term f"""
    Dd, terms = SHAPES[shape][1:3]
    return [Dd + sum(N for N, v in terms[:f]) for f in range(len(terms))]


def problem(idhmc, shape, n, seed=None):
    """(X (n, Dd), Y, factors, grp (Dx,), local (Dx,), slab): data from the family's own model; values are 0.5 N(0, 1); the indices of the
    terms are drawn independently (crossed) but for "aux 4, K 2", whose terms share one index, (x + 1 | s).  "wide coop": no observation
    has level 3 of term 0.  "four terms coop": term 2 has one level, so every observation of a block is in its list, and its values hold
    an exact 0.0, a -0.0, negatives and positives"""
    family, Dd, terms, grouped, loc = SHAPES[shape][:5]
    rng = np.random.default_rng(n + Dd if seed is None else seed)
    X = 0.3 * rng.standard_normal((n, Dd))
    X[:, 0] = 1.0
    z = X @ (0.5 * rng.standard_normal(Dd) / np.sqrt(Dd))
    factors, shared = [], None
    for f, (N, valued) in enumerate(terms):
        idx = rng.integers(0, N, n)
        if shape == "aux 4, K 2":
            shared = idx = idx if shared is None else shared
        if shape == "wide coop" and f == 0:
            idx = rng.choice(np.delete(np.arange(N), 3), n)
        w = 0.5 * rng.standard_normal(n)
        if shape == "four terms coop" and N == 1:
            w[0::5] = 0.0
            w[1::5] = -0.0
            w[2::5] = -np.abs(w[2::5])
            w[3::5] = np.abs(w[3::5])
        z = z + (w if valued else 1.0) * (0.4 * rng.standard_normal(N))[idx]
        factors.append(idhmc.glm.term(idx, values=w, levels=N) if valued else (idx, N))
    if family == "POISSON_LOG":
        Y = rng.poisson(np.exp(z)).astype(float)
    elif family == "BERNOULLI_LOGIT":
        Y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-z))).astype(float)
    elif family == "GAUSSIAN_IDENTITY_LOGSIGMA":
        Y = z + 0.5 * rng.standard_normal(n)
    else:
        a = AUX.TRUE_A["TEST_A4"]
        y1 = rng.uniform(-1.0, 1.0, n)
        Y = np.stack([z + a[1] * y1 + a[2] + np.exp(a[0] + a[3] * y1) * rng.standard_normal(n), y1], 1)
    Dx = Dd + sum(N for N, v in terms)
    grp = np.full(Dx, -1, np.int32)
    if grouped:
        for f, (off, (N, v)) in enumerate(zip(offsets(shape), terms)):
            grp[off:off + N] = f
    local = np.zeros(Dx, np.int32)
    if loc:
        local[Dd::3] = 1
    return X, Y, factors, grp, local, None if loc in (None, "no slab") else loc


def index_and_values(factors):
    """(index, values or None) of every term"""
    return [(t.index, t.values) if hasattr(t, "values") else (t[0], None) for t in factors]


def indicator_matrix(shape, X, factors):
    """the expanded matrix from its definition: E[i, c] = X[i, c] for c < Dd, E[i, off_f + idx_f[i]] = w_f[i] (1.0 for a term without
    values), +0.0 everywhere else"""
    n, Dd = X.shape
    E = np.zeros((n, dims(shape)[0]))
    E[:, :Dd] = X
    for off, (idx, w) in zip(offsets(shape), index_and_values(factors)):
        E[np.arange(n), off + np.asarray(idx)] = 1.0 if w is None else np.asarray(w)
    return E


def priors(shape):
    """(kind, nu, mu, tau): local_priors, and for "normal" the same mu and tau with every kind NORMAL, so that no prior table is uploaded"""
    Dx, A, H, J = dims(shape)
    kind, nu, mu, tau = local_priors(Dx, A, H, J)
    if SHAPES[shape][5] == "normal":
        assert A == H == J == 0                              # (no log coordinate, whose tau a log kind would have pinned to 1)
        kind, nu = np.zeros_like(kind), np.zeros_like(nu)
    return kind, nu, mu, tau


def models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau, **kw):
    """the model with factor terms and its expansion"""
    family = SHAPES[shape][0]
    common = dict(constants=consts(family), prior_mu=mu, prior_tau=tau, aux=SHAPE[family][2], groups=grp, prior_kind=kind, prior_nu=nu,
                  local=local, slab_scale=slab, **kw)
    return (idhmc.GLM(X, Y, source(idhmc, family), factors=factors, **common),
            idhmc.GLM(idhmc.glm.expand_factors(X, factors), Y, source(idhmc, family), **common))


def oracle_model(oracle, work, shape, Xe, Y, grp, local, slab, kind, nu, mu, tau):
    family, D = SHAPES[shape][0], SHAPES[shape][6]
    return oracle.OracleModel.custom(D, c_source_local(family),
                                     oracle_params_local(Xe, Y, SHAPE[family][2], grp, local, slab, kind, nu, consts(family), mu, tau), str(work))


def coefficients(shape, q, grp, local, slab):
    """b (C, Dx) of q = [u | a | omega | lambda] in numpy: u times the group's scale, and for a flagged column times the local scale,
    regularised where there is a slab (tests/test_gpu_glm_slopes.py's, which knows its own table and no flagged column without a slab)"""
    Dx, A, H, J = dims(shape)
    u, om, lam = q[:, :Dx], q[:, Dx + A:Dx + A + H], q[:, Dx + A + H:]
    ls = np.where(grp >= 0, om[:, np.maximum(grp, 0)], 0.0) if H else np.zeros_like(u)
    b = u * np.exp(ls)
    cols = np.flatnonzero(local)
    if J:
        s = np.exp(ls[:, cols] + lam)
        b[:, cols] = u[:, cols] * (s / np.sqrt(1.0 + s * s / (slab * slab)) if slab else s)
    return b


def residuals(shape, z, Y, a):
    """r_i = d log p / dz of every observation at z (n,), in numpy"""
    family = SHAPES[shape][0]
    return FLAT.numpy_terms(family, z, Y)[1] if SHAPE[family][2] == 0 else AUX.numpy_terms_aux(family, z, Y, a)[1]


def coop(L, A, shared=False):
    """the form of the NUTS kernel: DESIGN section 12's table of what fits a CU's LDS"""
    return int(A <= 4 if L == 128 else (A <= 1 or (A == 2 and shared)) if L == 256 else False)


def test_the_shapes_are_what_they_are_there_for(idhmc):
    for name, (family, Dd, terms, grouped, loc, pri, D, L, Lx, form) in SHAPES.items():
        Dx, A, H, J = dims(name)
        assert Dx + A + H + J == D and L == 128 * (1 << int(np.ceil(np.log2(max(1, (D + 127) // 128))))), name
        assert Lx == 128 * ((Dd + 127) // 128) <= L and form == coop(L, A) and len(terms) <= 4, name
        X, Y, factors, grp, local, slab = problem(idhmc, name, 385)
        m = models(idhmc, name, X, Y, factors, grp, local, slab, *priors(name))[0]
        assert (m.D, m.Dx, m.Dd, m.F, m.A, m.H, m.J, m.K) == (D, Dx, Dd, len(terms), A, H, J, SHAPE[family][0]), name
        assert (m.factor_has is not None) == any(v for N, v in terms) and (m.slab_scale is None) == (loc in (None, "no slab")), name
    S = SHAPES
    # "wide coop": Lx = 256 on the matrix cores; the Z loop's bound 8 ceil(Dd / 32) = 40 is past the 32 of one chunk; the G tile 8
    # (columns 128..143, in the second chunk of the stored rows) holds dense columns 128..139 and levels 0..3 of term 0, of which level 3
    # has an empty list in every block
    assert S["wide coop"][8] == 256 > 128 and S["wide coop"][9] == 1 and 8 * ((140 + 31) >> 5) == 40 > 32 and 16 * 8 < 140 < 16 * 9
    X, Y, factors, grp, local, slab = problem(idhmc, "wide coop", 385)
    assert 3 not in factors[0][0] and set(factors[0][0]) == set(range(20)) - {3} and factors[1].values is not None
    assert not indicator_matrix("wide coop", X, factors)[:, 143].any()
    # "aux at 256": a score plane, local scales with a slab and two groups at L = 256; levels and flagged levels on both sides of column 128
    assert S["aux at 256"][7] == 256 and dims("aux at 256")[1:] == (1, 2, 34) and 100 < 128 < 100 + 60 < 200
    X, Y, factors, grp, local, slab = problem(idhmc, "aux at 256", 385)
    assert slab == 2.0 and local[:100].sum() == 0 and local[100] == local[127] == local[130] == local[199] == 1 and local.sum() == 34
    # "aux 4, K 2": four score planes and two columns of Y; both terms on one index
    assert SHAPE["TEST_A4"] == (2, 0, 4) and dims("aux 4, K 2")[1:] == (4, 2, 10)
    X, Y, factors, grp, local, slab = problem(idhmc, "aux 4, K 2", 385)
    assert factors[0].index is factors[1][0] and Y.shape == (385, 2)
    # "four terms coop": F = 4 = H, local scales without a slab, and the single level of term 2: all 128 observations of a full block in
    # one valued list, whose values hold an exact 0.0, a -0.0, negatives and positives
    assert len(S["four terms coop"][2]) == 4 == dims("four terms coop")[2] and S["four terms coop"][4] == "no slab"
    X, Y, factors, grp, local, slab = problem(idhmc, "four terms coop", 385)
    t = factors[2]
    assert slab is None and local.sum() == 7 and t.levels == 1 and not t.index.any() and np.bincount(t.index[:128], minlength=1)[0] == 128
    zero = t.values[:128] == 0.0
    assert zero.any() and np.signbit(t.values[:128][zero]).any() and not np.signbit(t.values[:128][zero]).all()
    assert (t.values[:128] < 0).any() and (t.values[:128] > 0).any()
    assert offsets("four terms coop") == [10, 16, 21, 22]
    # "bare": no group, no local scale, no auxiliary coordinate and every prior NORMAL: nothing but kFactors and kSlopes
    kind, nu, mu, tau = priors("bare")
    assert dims("bare")[1:] == (0, 0, 0) and not kind.any() and not nu.any() and len(np.unique(tau)) > 1
    for name in ("wide coop", "aux at 256", "aux 4, K 2", "four terms coop", "Lx 256 of 512", "Lx 384 of 512", "Lx is L", "four terms wave"):
        assert priors(name)[0].any(), name
    # the per-wave rows: Lx = 256 < L, Lx = 384 (no power of two), Lx = L, and four terms with four groups at Lx = 256
    assert S["Lx 256 of 512"][7:] == (512, 256, 0) and 200 < 256 < 200 + 120                    # valued levels on both sides of column 256
    assert S["Lx 384 of 512"][7:] == (512, 384, 0) and 384 & (384 - 1) != 0 and 300 < 384 < 400
    assert S["Lx is L"][7:] == (512, 512, 0)
    assert S["four terms wave"][7:] == (512, 256, 0) and len(S["four terms wave"][2]) == 4 == dims("four terms wave")[2]
    # four blocks, the last of one observation
    assert (385 + 127) // 128 == 4 and 385 - 3 * 128 == 1


def test_no_product_is_near_underflow(idhmc):
    """DESIGN section 21's one new edge cannot occur: at every start the two files use, whatever w b or w r is not exactly zero is far
    above 1e-300 in magnitude (in numpy, on the reference alone)"""
    for name, (family, Dd, terms, grouped, loc, pri, D, L, Lx, form) in SHAPES.items():
        Dx, A, H, J = dims(name)
        for n in (1,) + NS:
            X, Y, factors, grp, local, slab = problem(idhmc, name, n)
            E = indicator_matrix(name, X, factors)
            starts = [start_local(family, C_, Dx, H, J) for C_ in STARTS]
            starts += [start_local(family, 1, Dx, H, J, seed=k, scale=0.3 + 0.3 * k) for k in range(3)]
            for q in starts:
                b = coefficients(name, q, grp, local, slab)
                r = np.stack([residuals(name, E @ b[c], Y, q[c, Dx:Dx + A]) for c in range(q.shape[0])])
                for off, (idx, w) in zip(offsets(name), index_and_values(factors)):
                    if w is None:
                        continue
                    w = np.asarray(w)
                    assert np.all(np.abs(w[w != 0.0]) > 1e-8), name
                    for prod in (w * b[:, off + np.asarray(idx)], w * r):
                        assert np.all(np.abs(prod[prod != 0.0]) > 1e-100), (name, n)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """one directory per family for the compiled restatement"""
    dirs = {}

    def of(family):
        if family not in dirs:
            dirs[family] = str(tmp_path_factory.mktemp(family.lower()))
        return dirs[family]
    return of


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", NS)
def test_reference_on_the_expanded_matrix(idhmc, oracle, work, shape, n):
    """the matrix built from the definition has the bits of glm.expand_factors, and on it l and every gradient coordinate of the C
    restatement agree with numpy within 1e-12 of the magnitude of the terms summed, at three starts"""
    family, D = SHAPES[shape][0], SHAPES[shape][6]
    Dx, A, H, J = dims(shape)
    X, Y, factors, grp, local, slab = problem(idhmc, shape, n)
    E = indicator_matrix(shape, X, factors)
    assert E.shape == (n, Dx) and same_bits(E, idhmc.glm.expand_factors(X, factors))
    assert all(np.count_nonzero(E[:, off:off + N], axis=1).max() <= 1 for off, (N, v) in zip(offsets(shape), SHAPES[shape][2]))
    kind, nu, mu, tau = priors(shape)
    om = oracle_model(oracle, work(family), shape, E, Y, grp, local, slab, kind, nu, mu, tau)
    for k in range(3):
        q = start_local(family, 1, Dx, H, J, seed=k, scale=0.3 + 0.3 * k)[0]
        lq, g = om.logdensity_and_gradient(q)
        l_ref, g_ref, lscale, gscale = numpy_density_local(family, E, Y, q, grp, local, slab, kind, nu, mu, tau)
        assert np.isfinite(lq) and abs(lq - l_ref) <= 1e-12 * lscale, (lq, l_ref)
        assert np.all(np.abs(g[:D] - g_ref) <= 1e-12 * gscale + 1e-300), np.max(np.abs(g[:D] - g_ref) / gscale)


def test_every_shape_passes_the_argument_checks(idhmc):
    """idhmc_create_glm_slopes at n = 385 with 18 chains: accepted, or stopped at the device check, which is past every argument check"""
    from inplacedhmc_jl_amd import _lib
    lib = idhmc.load_library()
    opt = idhmc.default_options(max_depth=4)
    for name in SHAPES:
        X, Y, factors, grp, local, slab = problem(idhmc, name, 385)
        kind, nu, mu, tau = priors(name)
        m = models(idhmc, name, X, Y, factors, grp, local, slab, kind, nu, mu, tau)[0]              # kept alive: the descriptor points into it
        desc = m.glm_desc()
        pr = _lib.GlmPriors(kind=m.prior_kind.ctypes.data_as(C.POINTER(C.c_int32)), nu=m.prior_nu.ctypes.data_as(C.POINTER(C.c_double)))
        lc = None
        if m.J > 0:
            lc = _lib.GlmLocal(local=m.local.ctypes.data_as(C.POINTER(C.c_int32)), slab_scale=m.slab_scale or 0.0)
        fc = _lib.GlmFactors(F=m.F, levels=m.levels.ctypes.data_as(C.POINTER(C.c_int32)), index=m.factor_index.ctypes.data_as(C.POINTER(C.c_int32)))
        fv = None
        if m.factor_has is not None:
            fv = _lib.GlmFactorValues(values=m.factor_values.ctypes.data_as(C.POINTER(C.c_double)),
                                      has=m.factor_has.ctypes.data_as(C.POINTER(C.c_int32)))
        h = C.c_void_p()
        rc = lib.idhmc_create_glm_slopes(C.byref(h), 0, 18, 0, C.byref(desc), C.byref(pr), None if lc is None else C.byref(lc), C.byref(fc),
                                         None if fv is None else C.byref(fv), 1, 0, C.byref(opt), 3)
        msg = lib.idhmc_last_error()
        if rc == 0:
            lib.idhmc_destroy(h)
        assert rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg), (name, rc, msg)
