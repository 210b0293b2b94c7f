"""idhmc_create_glm_model against the eleven entries it replaces, without a device: every refusal of a GLM in parts
happens before the device is looked for, so the same parts through the narrowest legacy entry that takes them and through the model
entry must give the same return code and the same bytes of idhmc_last_error().  One row per validate_* function of idhmc_create.hip and
one per members / values conflict of create_glm; the null arguments, (M, chains_per_response) and Model.glm_model() separately."""
import ctypes as C

import numpy as np
import pytest

N, DD, LEVELS = 24, 2, (2, 2, 2)                   # Dx = 2 dense columns + 3 terms of 2 levels = 8
DX = DD + sum(LEVELS)
PARTS = ("priors", "local", "factors", "values", "pairs", "structs", "gmrfs", "block", "members")     # in the order the entries grew
ENTRY_OF_LAST_PART = dict(zip(PARTS, ("priors", "local", "factors", "slopes", "corr", "struct", "gmrf", "block", "multi")))
I32, I64, F64 = np.int32, np.int64, np.float64


def _base(idhmc, Dx=DX):
    """(descriptor fields, arrays): a Poisson regression on n = 24 observations.  X holds n x Dx numbers whatever parts the call has: a
    call without factor terms reads all of them, one with terms the first n x Dd as its dense columns, and none reads past the array"""
    rng = np.random.default_rng(5)
    X = np.ascontiguousarray(rng.standard_normal((N, max(Dx, 1))))
    Y = np.ascontiguousarray(rng.poisson(2.0, (N, 1)).astype(F64))
    return dict(n=N, Dx=Dx, K=1, nc=0, A=0, H=0, source=idhmc.glm.POISSON_LOG.encode()), dict(X=X, Y=Y)


INDEX = np.ascontiguousarray([np.arange(N) % 2, np.arange(N) // 2 % 2, np.arange(N) // 4 % 2], dtype=I32)
PLANES = np.ascontiguousarray([np.zeros(N), np.ones(N), INDEX[1], INDEX[2]], dtype=I32)      # term 0 of width 2: levels 0 and 1
Q2 = dict(start=[0, 1, 2], col=[0, 1], val=[1.0, 1.0])                                        # the 2 x 2 identity of a GMRF term


class Built:
    """ctypes structs of one call and the arrays they point into"""

    def __init__(self, idhmc, desc=None, M=1, R=0, **parts):
        from inplacedhmc_jl_amd import _lib
        self.keep = []
        fields, arrays = _base(idhmc, **({} if desc is None or "Dx" not in desc else {"Dx": desc["Dx"]}))
        fields.update({k: v for k, v in (desc or {}).items() if not isinstance(v, np.ndarray)})
        arrays.update({k: v for k, v in (desc or {}).items() if isinstance(v, np.ndarray)})
        self.desc = self.struct(_lib.GlmDesc, dict(fields, **arrays))
        types = dict(priors=_lib.GlmPriors, local=_lib.GlmLocal, factors=_lib.GlmFactors, values=_lib.GlmFactorValues, pairs=_lib.GlmPairs,
                     structs=_lib.GlmStructs, gmrfs=_lib.GlmGmrfs, block=_lib.GlmBlock, members=_lib.GlmMembers)
        self.parts = {k: self.struct(types[k], v) for k, v in parts.items()}
        self.M, self.R = M, R

    def struct(self, cls, values):
        s = cls()
        for name, ctype in cls._fields_:
            v = values.get(name)
            if v is None:
                continue
            if hasattr(ctype, "contents"):                         # a pointer field: an array of its element type, kept alive here
                a = np.ascontiguousarray(v, dtype=np.dtype(ctype._type_))
                self.keep.append(a)
                v = a.ctypes.data_as(ctype)
            setattr(s, name, v)
        return s

    def legacy_entry(self):
        """the narrowest of the eleven that takes these parts"""
        last = [p for p in PARTS if p in self.parts]
        if last:
            return "idhmc_create_glm_" + ENTRY_OF_LAST_PART[last[-1]]
        return "idhmc_create_glm" if (self.M, self.R) == (1, 0) else "idhmc_create_glm_responses"

    def legacy(self, lib, entry=None):
        entry = entry or self.legacy_entry()
        h = C.c_void_p()
        args = [C.byref(h), 0, 4, 0, C.byref(self.desc)]
        if entry not in ("idhmc_create_glm", "idhmc_create_glm_responses"):
            k = list(ENTRY_OF_LAST_PART.values()).index(entry[len("idhmc_create_glm_"):]) + 1
            assert not set(self.parts) - set(PARTS[:k]), "%s cannot express %s" % (entry, sorted(self.parts))
            args += [C.byref(self.parts[p]) if p in self.parts else None for p in PARTS[:k]]
        if entry != "idhmc_create_glm":
            args += [self.M, self.R]
        return self.finish(lib, getattr(lib, entry)(*args, None, 1), h)

    def model(self):
        from inplacedhmc_jl_amd import _lib
        return _lib.GlmModel(glm=C.pointer(self.desc), M=self.M, chains_per_response=self.R, **{k: C.pointer(v) for k, v in self.parts.items()})

    def new(self, lib):
        h = C.c_void_p()
        gm = self.model()
        return self.finish(lib, lib.idhmc_create_glm_model(C.byref(h), 0, 4, 0, C.byref(gm), None, 1), h)

    @staticmethod
    def finish(lib, rc, h):
        msg = lib.idhmc_last_error()
        if rc == 0:
            lib.idhmc_destroy(h)
        return rc, msg


FACTORS = dict(F=3, levels=LEVELS, index=INDEX)
MEMBERS = dict(width=(2, 1, 1), index=PLANES)
TABLE = dict(F=3, levels=LEVELS)                       # factors next to a table of members: F and levels only
KIND = np.zeros(DX + 2, I32)                           # (room for the zetas some rows add)

# what is wrong -> (the message's distinguishing part, the call).  The parts are well formed up to the one thing the row is about.
ROWS = {
    "create_glm: Dx": (b"GLM: Dx = 0: at least one coefficient is needed", dict(desc=dict(Dx=0))),
    "create_glm: A": (b"GLM: A = 5 must be an integer in 0..4", dict(desc=dict(A=5))),
    "create_glm: groups": (b"GLM: H = 1 groups need the group of every column (groups is NULL)", dict(desc=dict(H=1))),
    "validate_regression: responses": (b"GLM: chains_per_response = 0: at least one chain per response is needed", dict(M=2, R=0)),
    "validate_priors": (b"GLM: prior kind[3] = 7 is outside 0..4", dict(priors=dict(kind=np.r_[0, 0, 0, 7, KIND[4:DX]]))),
    "validate_local": (b"GLM: slab_scale = -1 must be finite and >= 0", dict(local=dict(slab_scale=-1.0))),
    "validate_factors": (b"GLM: index[1][5] = 2 is outside 0..1 (the levels of factor 1)",
                         dict(factors=dict(FACTORS, index=np.where((np.arange(3)[:, None] == 1) & (np.arange(N) == 5), 2, INDEX)))),
    "validate_factor_values": (b"GLM: a term is flagged in has and values is NULL", dict(factors=FACTORS, values=dict(has=(0, 1, 0)))),
    "validate_pairs": (b"GLM: pair 0: first = second = 1 (a pair is two distinct terms)",
                       dict(factors=FACTORS, pairs=dict(P=1, first=[1], second=[1], eta=[2.0]))),
    "validate_structs": (b"GLM: structure 0: kind = 3 must be IDHMC_STRUCT_AR1 (1) or IDHMC_STRUCT_RW1 (2)",
                         dict(factors=FACTORS, structs=dict(S=1, term=[0], kind=[3], eta=[0.0]))),
    "validate_structs behind a block": (b"GLM: structure 0: prior kind[9] = 2 is a prior on exp(q): coordinate 9 is zeta = atanh phi",
                                        dict(priors=dict(kind=np.r_[KIND[:DX + 1], 2]), factors=FACTORS,
                                             structs=dict(S=1, term=[2], kind=[1], eta=[0.0]), block=dict(K=2, term=[0, 1], eta=2.0))),
    "validate_gmrfs": (b"GLM: GMRF start[0] = 1 must be 0", dict(factors=FACTORS, gmrfs=dict(Q2, G=1, term=[0], kappa=[0.0], start=[1, 2, 3]))),
    "validate_block": (b"GLM: a block of K = 5 terms: K must be 0, 2, 3 or 4", dict(factors=FACTORS, block=dict(K=5, term=[0, 1, 2], eta=2.0))),
    "validate_block next to pairs": (b"GLM: a block next to P = 1 pairs (a model has pairs or a block, not both)",
                                     dict(factors=FACTORS, pairs=dict(P=1, first=[0], second=[1], eta=[2.0]), block=dict(K=2, term=[0, 1], eta=2.0))),
    "create_glm: the block's zetas past D = 1024": (b"D = Dx + A + H + J + K (K - 1) / 2 = 1025: a GLM is limited to D <= 1024 (a block of K = 2 terms)",
                                                   dict(desc=dict(Dx=1024), factors=FACTORS, block=dict(K=2, term=[0, 1], eta=2.0))),
    "create_glm: members without factors": (b"GLM: members need factor terms: factors gives F and levels (factors is NULL)", dict(members=MEMBERS)),
    "create_glm: members and values": (b"GLM: members and factor values are both given",
                                       dict(factors=TABLE, values=dict(has=(1, 1, 1), values=np.ones((3, N))), members=MEMBERS)),
    "create_glm: members and index": (b"GLM: members and factors->index are both given", dict(factors=FACTORS, members=MEMBERS)),
    "check_members": (b"term 0, plane 1, observation 0: level 0 after level 0", dict(factors=TABLE, members=dict(MEMBERS, index=PLANES * [[1], [0], [1], [1]]))),
    "create_glm: a wide term in a pair": (b"GLM: pair 0 names term 0, which has width 2",
                                          dict(factors=TABLE, pairs=dict(P=1, first=[1], second=[0], eta=[2.0]), members=MEMBERS)),
    "create_glm: a wide term in a block": (b"GLM: the block names term 0, which has width 2",
                                           dict(factors=TABLE, block=dict(K=2, term=[1, 0], eta=2.0), members=MEMBERS)),
    "behind a table of width 1": (b"GLM: structure 0: kind = 3 must be IDHMC_STRUCT_AR1 (1) or IDHMC_STRUCT_RW1 (2)",
                                  dict(factors=TABLE, structs=dict(S=1, term=[0], kind=[3], eta=[0.0]), members=dict(width=(1, 1, 1), index=INDEX))),
    "the order: local before pairs": (b"GLM: slab_scale = -1 must be finite and >= 0",
                                      dict(local=dict(slab_scale=-1.0), factors=FACTORS, pairs=dict(P=1, first=[1], second=[1], eta=[2.0]))),
    "the order: pairs before priors": (b"GLM: pair 0: first = second = 1",
                                       dict(priors=dict(kind=np.r_[7, KIND[1:DX + 1]]), factors=FACTORS, pairs=dict(P=1, first=[1], second=[1], eta=[2.0]))),
    "validate_regression: X": (b"GLM: X[0, 1] is not finite", dict(desc=dict(X=np.where(np.arange(N * DD) == 1, np.inf, 0.5).reshape(N, DD)), factors=FACTORS)),
}


@pytest.mark.parametrize("row", sorted(ROWS))
def test_the_same_refusal_through_the_legacy_entry_and_the_model_entry(idhmc, row):
    what, call = ROWS[row]
    lib = idhmc.load_library()
    b = Built(idhmc, **call)
    old, new = b.legacy(lib), b.new(lib)
    assert old[0] == idhmc.ERR_BAD_ARG and what in old[1], (b.legacy_entry(), old)        # the row is refused for what it is about
    assert new == old, (b.legacy_entry(), old, new)


def test_every_legacy_entry_is_in_the_table(idhmc):
    used = {Built(idhmc, **call).legacy_entry() for _, call in ROWS.values()}
    assert used == {"idhmc_create_glm", "idhmc_create_glm_responses"} | {"idhmc_create_glm_" + e for e in ENTRY_OF_LAST_PART.values()}


def test_null_arguments_of_the_model_entry(idhmc):
    from inplacedhmc_jl_amd import _lib
    lib = idhmc.load_library()
    b = Built(idhmc)
    h = C.c_void_p()
    gm, no_glm = b.model(), _lib.GlmModel(M=1)
    for out, model in ((None, C.byref(gm)), (C.byref(h), None), (C.byref(h), C.byref(no_glm))):
        assert lib.idhmc_create_glm_model(out, 0, 4, 0, model, None, 1) == idhmc.ERR_BAD_ARG
        assert lib.idhmc_last_error() == b"idhmc_create_glm_model: null argument"


def test_the_callers_struct_is_not_written_to(idhmc):
    """a table of width 1 is rewritten into plain factors and values, and (0, 0) into (1, 0): both in the library's copy"""
    lib = idhmc.load_library()
    b = Built(idhmc, M=0, R=0, **ROWS["behind a table of width 1"][1])
    gm, h = b.model(), C.c_void_p()
    before = bytes(gm)
    assert lib.idhmc_create_glm_model(C.byref(h), 0, 4, 0, C.byref(gm), None, 1) == idhmc.ERR_BAD_ARG
    assert ROWS["behind a table of width 1"][0] in lib.idhmc_last_error() and bytes(gm) == before and bool(gm.members) and not gm.values


def test_zero_responses_fields_are_one_response(idhmc):
    """(0, 0), what a zero-initialised struct holds, is (1, 0): the call gets as far as the data, which is refused after everything about
    the responses; (2, 0) and every legacy entry's (0, 0) are refused as they were; idhmc_create_glm_responses forces its context"""
    lib = idhmc.load_library()
    what, call = ROWS["validate_regression: X"]
    one = Built(idhmc, **call).new(lib)
    zero = Built(idhmc, M=0, R=0, **call)
    assert zero.new(lib) == one and one[0] == idhmc.ERR_BAD_ARG and what in one[1]
    rc, msg = zero.legacy(lib)
    assert rc == idhmc.ERR_BAD_ARG and b"GLM: M = 0: at least one response is needed" in msg
    rc, msg = Built(idhmc, M=2, R=0, **call).new(lib)
    assert rc == idhmc.ERR_BAD_ARG and b"GLM: chains_per_response = 0: at least one chain per response is needed" in msg
    plain = Built(idhmc, M=1, R=0)
    rc, msg = plain.legacy(lib, "idhmc_create_glm_responses")
    assert rc == idhmc.ERR_BAD_ARG and b"GLM: chains_per_response = 0: at least one chain per response is needed" in msg
    rc, msg = plain.new(lib)                               # the same fields through the model entry: the plain context, up to the device
    assert rc in (0, idhmc.ERR_NO_DEVICE) and (rc == 0 or b"no HIP device" in msg)


def _models(idhmc):
    """name -> (GLM keywords, the parts Model.glm_model() must hand over): one model per part"""
    g = idhmc.glm
    f3 = [(INDEX[0], 2), (INDEX[1], 2), (INDEX[2], 2)]
    grp = np.r_[np.full(DD, -1), 0, 0, 1, 1, 2, 2]
    return {
        "groups": (dict(groups=np.r_[0, np.full(DD - 1, -1)]), set()),
        "responses": (dict(chains_per_response=3), set()),
        "priors": (dict(prior_kind=np.r_[np.zeros(DD - 1, int), 1], prior_nu=np.r_[np.zeros(DD - 1), 4.0]), {"priors"}),
        "local": (dict(local=True), {"local"}),
        "factors": (dict(factors=f3), {"factors"}),
        "values": (dict(factors=[f3[0], g.term(INDEX[1], values=np.linspace(-1, 1, N), levels=2)]), {"factors", "values"}),
        "pairs": (dict(factors=f3, groups=grp, correlated=[g.pair(0, 1)]), {"factors", "pairs"}),
        "structs": (dict(factors=f3, groups=grp, structured=[g.ar1(2)]), {"factors", "structs"}),
        "gmrfs": (dict(factors=f3, groups=grp, gmrf=[g.gmrf(1, np.eye(2))]), {"factors", "gmrfs"}),
        "block": (dict(factors=f3, groups=grp, correlated=[g.block((0, 1, 2))]), {"factors", "block"}),
        "members": (dict(factors=[g.members(PLANES[:2].T, None, 2), f3[1]]), {"factors", "members"}),
    }


@pytest.mark.parametrize("name", ["groups", "responses", "priors", "local", "factors", "values", "pairs", "structs", "gmrfs", "block", "members"])
def test_glm_model_hands_over_exactly_the_parts_the_model_has(idhmc, name):
    kw, want = _models(idhmc)[name]
    fields, arrays = _base(idhmc, Dx=DD)
    Y = np.stack([arrays["Y"], arrays["Y"] + 1.0]) if name == "responses" else arrays["Y"]
    m = idhmc.GLM(arrays["X"], Y, idhmc.glm.POISSON_LOG, **kw)
    gm = m.glm_model()
    have = {p for p in PARTS if getattr(gm, p)}
    if m.prior_kind is not None:
        want = want | {"priors"}                           # (a pair's, a structure's or a block's zeta brings the prior arrays along)
    assert bool(gm.glm) and have == want and set(gm.parts) == want | {"glm"}
    assert (gm.M, gm.chains_per_response) == ((2, 3) if name == "responses" else (1, 0))
    assert gm.glm.contents.n == N and gm.glm.contents.Dx == m.Dx
    if "factors" in want:
        assert gm.factors.contents.F == m.F and bool(gm.factors.contents.index) == (name != "members")
    if name == "members":
        assert not gm.values and gm.members.contents.width[0] == 2
    if name == "priors":
        assert gm.priors.contents.kind[DD - 1] == 1 and gm.priors.contents.nu[DD - 1] == 4.0
