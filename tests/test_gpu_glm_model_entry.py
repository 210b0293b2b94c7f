"""The wiring of idhmc_create_glm_model on the six entries no other test compares with an Engine: the context a direct
call of idhmc_create_glm_responses, _priors, _local, _factors, _struct or _block makes of a model against Engine(model), which goes
through the model entry -- the same form, the same footprint, and after an evaluation, a leapfrog and four NUTS transitions the same bits
in positions, momenta, densities, gradients and tree statistics (the stepsize is the fixed one run_engines sets on both, so its
comparison only shows that both hold it).  (_slopes, _corr, _gmrf, _multi and idhmc_create_glm are
compared the same way in their own files.)  No kernel path is new here: n = 130 is a full block of 128 observations and a ragged one, 18
chains one 16-chain group of the matrix-core kernel and a partial one."""
import ctypes as C

import numpy as np
import pytest

import test_glm_hier_cpu as HIER
import test_glm_local_cpu as LOCAL
import test_glm_priors_cpu as PRIORS
import test_gpu_glm_block as BLOCK
import test_gpu_glm_factors as FACTORS
import test_gpu_glm_local as GLOCAL
import test_gpu_glm_priors as GPRIORS
import test_gpu_glm_struct as STRUCT
from test_glm_hier_cpu import SHAPE
from test_glm_responses_cpu import responses
from test_gpu_glm import prior
from test_gpu_glm_factors import same_bits
from test_gpu_glm_slopes import run_engines

pytestmark = pytest.mark.gpu

C_, N = 18, 130
PARTS = ("priors", "local", "factors", "values", "pairs", "structs")      # the arguments of idhmc_create_glm_struct behind the descriptor


def case_responses(idhmc):
    D = 25
    X, Y = responses("POISSON_LOG", 2, N, D, seed=N + D)
    mu, tau = prior(D)
    m = idhmc.GLM(X, Y, idhmc.glm.POISSON_LOG, None, mu, tau, chains_per_response=16)
    q = np.random.default_rng(D).uniform(-0.3, 0.3, (C_, D)) / np.sqrt(D)
    return m, q, 1, ()


def case_priors(idhmc):
    family, Dx, grp, L, form = GPRIORS.SHAPES["L = 128"]
    A, H = SHAPE[family][2], int(grp.max()) + 1
    kind, nu, mu, tau = GPRIORS.shape_priors("L = 128", Dx, A, H)
    X, Y = HIER.problem_hier(family, N, Dx, grp, True, seed=N + Dx)
    return PRIORS.make(idhmc, family, X, Y, grp, kind, nu, mu, tau), HIER.start_hier(family, C_, Dx, H), form, ("priors",)


def case_local(idhmc):
    family, Dx, grp, local, slab, D, L, form = GLOCAL.SHAPES["odd offset"]
    A, H, J = GLOCAL.dims(family, grp, local)
    kind, nu, mu, tau = LOCAL.local_priors(Dx, A, H, J)
    X, Y = HIER.problem_hier(family, N, Dx, grp, False, seed=N + Dx)
    return LOCAL.make(idhmc, family, X, Y, grp, local, slab, kind, nu, mu, tau), LOCAL.start_local(family, C_, Dx, H, J), form, ("priors", "local")


def case_factors(idhmc):
    shape = "tile aligned"
    family, Dd, levels, grouped, slab, D, L, form = FACTORS.SHAPES[shape]
    A, H, J = FACTORS.dims(shape)
    Dx = Dd + sum(levels)
    X, Y, factors, grp, local, slab = FACTORS.problem(shape, N)
    kind, nu, mu, tau = LOCAL.local_priors(Dx, A, H, J)
    m = FACTORS.models(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)[0]
    return m, LOCAL.start_local(family, C_, Dx, H, J), form, ("priors", "factors")


def case_struct(idhmc):
    shape = "two slots"
    form = STRUCT.SHAPES[shape][9]
    X, Y, factors, grp, local, slab = STRUCT.problem(idhmc, shape, N)
    kind, nu, mu, tau = STRUCT.shape_priors(shape)
    m = STRUCT.model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    return m, STRUCT.start(shape, C_), form, ("priors", "local", "factors", "values", "pairs", "structs")


def case_block(idhmc):
    shape = "one tile"
    form = BLOCK.SHAPES[shape][10]
    X, Y, factors, grp, local, slab = BLOCK.problem(idhmc, shape, N)
    kind, nu, mu, tau = BLOCK.shape_priors(shape)
    m = BLOCK.model(idhmc, shape, X, Y, factors, grp, local, slab, kind, nu, mu, tau)
    return m, BLOCK.start(shape, C_), form, ("priors", "factors", "values", "block")


CASES = {"responses": case_responses, "priors": case_priors, "local": case_local, "factors": case_factors, "struct": case_struct,
         "block": case_block}


def part_structs(m):
    """the part structs of model m from its arrays, by hand (Model.glm_model() is the other side of the comparison)"""
    from inplacedhmc_jl_amd import _lib
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    i, d = (lambda a: a.ctypes.data_as(ip)), (lambda a: a.ctypes.data_as(dp))
    s = {}
    if m.prior_kind is not None:
        s["priors"] = _lib.GlmPriors(kind=i(m.prior_kind), nu=d(m.prior_nu))
    if m.J:
        s["local"] = _lib.GlmLocal(local=i(m.local), slab_scale=m.slab_scale or 0.0)
    if m.F:
        s["factors"] = _lib.GlmFactors(F=m.F, levels=i(m.levels), index=i(m.factor_index))
    if m.factor_has is not None:
        s["values"] = _lib.GlmFactorValues(values=d(m.factor_values), has=i(m.factor_has))
    if m.P:
        s["pairs"] = _lib.GlmPairs(P=m.P, first=i(m.pair_first), second=i(m.pair_second), eta=d(m.pair_eta))
    if m.S:
        s["structs"] = _lib.GlmStructs(S=m.S, term=i(m.struct_term), kind=i(m.struct_kind), eta=d(m.struct_eta))
    if m.BK:
        s["block"] = _lib.GlmBlock(K=m.BK, term=i(m.block_term), eta=m.block_eta)
    return s


@pytest.mark.parametrize("entry", list(CASES))
def test_the_legacy_entry_and_the_engine_make_the_same_context(idhmc, entry):
    from inplacedhmc_jl_amd import _lib
    m, q, form, want = CASES[entry](idhmc)
    s = part_structs(m)
    assert tuple(p for p in PARTS + ("block",) if p in s) == want and m.G == 0 and m.member_width is None       # the model needs this entry, and no later one
    assert q.shape == (C_, m.D) and m.n == N
    opt = idhmc.default_options(max_depth=4)
    lib = idhmc.load_library()
    ref = lambda p: C.byref(s[p]) if p in s else None
    desc = m.glm_desc()
    M, R = (m.M, m.R) if m.R is not None else (1, 0)
    assert (M, R) == ((2, 16) if entry == "responses" else (1, 0))
    h = C.c_void_p()
    head = (C.byref(h), 0, C_, 0, C.byref(desc))
    if entry == "responses":
        rc = lib.idhmc_create_glm_responses(*head, M, R, C.byref(opt), 3)
    elif entry == "block":
        rc = lib.idhmc_create_glm_block(*head, *[ref(p) for p in PARTS], None, ref("block"), M, R, C.byref(opt), 3)
    else:
        k = {"priors": 1, "local": 2, "factors": 3, "struct": 6}[entry]
        rc = getattr(lib, "idhmc_create_glm_" + entry)(*head, *[ref(p) for p in PARTS[:k]], M, R, C.byref(opt), 3)
    _lib.check(rc)
    engs = [idhmc.Engine(m, C_, opt, seed=3), idhmc.Engine._adopt(m, h, C_, opt)]
    for e in engs:
        assert e.glm_form() == form and e.glm_responses() == (M, R)
    assert engs[0].device_bytes() == engs[1].device_bytes()
    for got, legacy in zip((engs[0].glm_priors(), engs[0].glm_local(), engs[0].glm_factors(), engs[0].glm_structs(), engs[0].glm_block()),
                           (engs[1].glm_priors(), engs[1].glm_local(), engs[1].glm_factors(), engs[1].glm_structs(), engs[1].glm_block())):
        for a, b in zip(got, legacy):
            assert (a is None and b is None) or np.array_equal(a, b)
    run_engines(engs, None, m.D, q, entry)
    assert same_bits(engs[0].eps, engs[1].eps)
    for e in engs:
        e.close()
