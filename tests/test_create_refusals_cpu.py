"""Every refusal of idhmc_create, idhmc_create_glm and idhmc_create_glm_responses, as ONE table: each row is a call, the code it returns
and the complete text of idhmc_last_error() as a literal.  Every check answers before the device is looked for, so the table runs
without a GPU; it was recorded from the library as it was before the host API was cut into units and holds unchanged since: a
refactoring of the validation that changes which defect is reported, or one word of a message, fails here.  The inputs are those of
the test_bad_descs_... / test_bad_calls_... functions of test_{glm, glm_aux, glm_hier, glm_responses, logistic}_cpu.py, the other
checks of the creation path, and the smallest shapes of every form (Dx = 1, n = 1, nc = 0 and 16, A = 4 at D = 5, nparams equal to
and one short of the header), where unpacking a packed description can go wrong.  Valid rows expect a context (a device exists) or
"no HIP device", which is past every argument check."""
import ctypes as C

import numpy as np
import pytest

import test_glm_aux_cpu as AUX
import test_glm_cpu as FLAT
import test_glm_hier_cpu as HIER
import test_logistic_cpu as LOGIT

BAD = "BAD"          # idhmc.ERR_BAD_ARG
OK = "OK"            # a context, or ERR_NO_DEVICE with "no HIP device"
P = C.POINTER(C.c_double)
N_BIG = (1 << 27) // 128 + 1      # n_pad L > 2^27 at L = 128


def _ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_int32) if a.dtype == np.int32 else P)


class World:
    """the arrays every row is cut from (kept alive for the whole test)"""

    def __init__(self, idhmc):
        from inplacedhmc_jl_amd import _lib
        self.idhmc, self._lib, self.keep = idhmc, _lib, []
        self.X, self.Y2 = FLAT.problem("POISSON_LOG_OFFSET", 50, 6)                      # K = 2
        self.Xa, self.Ya = AUX.problem_aux("WEIBULL_LOG_LOGSHAPE", 50, 6)               # K = 2, A = 1
        Xl, yl = LOGIT.problem(50, 6)
        self.logit = np.concatenate([Xl.ravel(), np.asarray(yl, float).ravel()])
        self.glm = np.concatenate([[2.0, 2.0, 1.0, 2.0], self.X.ravel(), self.Y2.ravel()])
        self.aux = np.concatenate([[2.0, 2.0, 1.0, 1.0, 2.0], self.Xa.ravel(), self.Ya.ravel()])
        self.grp = np.array([-1, 0, 0, 1, 1, -1], np.int32)
        self.Y3 = np.stack([self.Ya, self.Ya, self.Ya])
        self.Y3[1, :, 0] += 0.25

    def hold(self, a):
        self.keep.append(a)
        return a

    def opt(self, **kw):
        return self.hold(self.idhmc.default_options(**kw))

    # ---- idhmc_create ------------------------------------------------------------------------------------------------------------
    def packed(self, kind, D, params=None, edit=None, nparams=None, null_params=False, source=b"x", mu=None, tau=None, prec=None,
               opt=None, nchains=4, first=0, null_model=False):
        """idhmc_create with a model descriptor; `params` in an exactly sized array, `edit` = {index: value} applied to a copy"""
        d = self._lib.ModelDesc()
        d.kind, d.D, d.source = kind, D, source
        if params is not None:
            p = self.hold(np.array(params, float))
            for i, v in (edit or {}).items():
                p[i] = v
            d.params, d.nparams = _ptr(p), p.size
        if nparams is not None:
            d.nparams = nparams
        if null_params:
            d.params = None
        for name, a in (("mu", mu), ("tau", tau), ("prec", prec)):
            if a is not None:
                setattr(d, name, _ptr(self.hold(np.array(a, float))))
        lib = self.idhmc.load_library()
        h = C.c_void_p()
        rc = lib.idhmc_create(C.byref(h), 0, nchains, first, None if null_model else C.byref(d), None if opt is None else C.byref(opt), 1)
        return self.done(rc, h)

    # ---- idhmc_create_glm (M is None) and idhmc_create_glm_responses ---------------------------------------------------------------
    def parts(self, X=None, Y=None, n=None, Dx=None, K=2, nc=2, A=1, H=2, constants=(1.0, 2.0), groups="grp", mu=None, tau=None,
              source=b"x", M=None, R=6, nchains=4, first=0, opt=None, null_desc=False, null_X=False, null_Y=False):
        X = self.Xa if X is None else X
        Y = (self.Ya if M is None else self.Y3) if Y is None else Y
        X, Y = self.hold(np.ascontiguousarray(X, float)), self.hold(np.ascontiguousarray(Y, float))
        d = self._lib.GlmDesc()
        d.n, d.Dx, d.K, d.nc, d.A, d.H = X.shape[0] if n is None else n, X.shape[1] if Dx is None else Dx, K, nc, A, H
        d.X, d.Y, d.source = None if null_X else _ptr(X), None if null_Y else _ptr(Y), source
        if constants is not None:
            d.constants = _ptr(self.hold(np.array(constants, float)))
        groups = self.grp if isinstance(groups, str) else groups
        if groups is not None:
            d.groups = _ptr(self.hold(np.array(groups, np.int32)))
        for name, a in (("mu", mu), ("tau", tau)):
            if a is not None:
                setattr(d, name, _ptr(self.hold(np.array(a, float))))
        lib = self.idhmc.load_library()
        h = C.c_void_p()
        o = None if opt is None else C.byref(opt)
        dp = None if null_desc else C.byref(d)
        if M is None:
            rc = lib.idhmc_create_glm(C.byref(h), 0, nchains, first, dp, o, 1)
        else:
            rc = lib.idhmc_create_glm_responses(C.byref(h), 0, nchains, first, dp, M, R, o, 1)
        return self.done(rc, h)

    def done(self, rc, h):
        lib = self.idhmc.load_library()
        msg = lib.idhmc_last_error()
        if rc == 0:
            lib.idhmc_destroy(h)
        return rc, msg


def _rows():
    """(id, call(world) -> (rc, message), expected code, expected message)"""
    R = []

    def row(name, call, code, msg=None):
        R.append((name, call, code, msg))

    ISO, DIAG, DENSE, CUSTOM, LR, GLM, GAUX = 0, 1, 2, 3, 4, 5, 6
    # ---- every model of idhmc_create: chains, D, options, the kinds without data ----------------------------------------------------
    row("null-model", lambda w: w.packed(ISO, 4, null_model=True), BAD, b"idhmc_create: null argument")
    row("nchains-0", lambda w: w.packed(ISO, 4, nchains=0), BAD, b"nchains = 0 out of range")
    row("nchains-2^31", lambda w: w.packed(ISO, 4, nchains=1 << 31), BAD, b"nchains = 2147483648 out of range")
    row("first-negative", lambda w: w.packed(ISO, 4, nchains=2, first=-1), BAD, b"chain ids must fit 32 bits")
    row("first-past-32-bits", lambda w: w.packed(ISO, 4, nchains=2, first=(1 << 32) - 2), BAD, b"chain ids must fit 32 bits")
    row("D-0", lambda w: w.packed(ISO, 0), BAD, b"D = 0 unsupported (1..2048)")
    row("D-2049", lambda w: w.packed(ISO, 2049), BAD, b"D = 2049 unsupported (1..2048)")
    row("dense-D-1100", lambda w: w.packed(DENSE, 1100), BAD, b"D = 1100: the dense density is limited to D <= 1024")
    row("metric-mode-7", lambda w: w.packed(ISO, 4, opt=w.opt(metric_mode=7)), BAD, b"unknown metric_mode 7")
    row("kind-7", lambda w: w.packed(7, 4), BAD, b"unknown model kind 7")
    row("kind-negative", lambda w: w.packed(-1, 4, mu=np.zeros(4)), BAD, b"unknown model kind -1")
    row("custom-no-source", lambda w: w.packed(CUSTOM, 4, source=None), BAD, b"custom model needs HIP source")
    row("custom-empty-source", lambda w: w.packed(CUSTOM, 4, source=b""), BAD, b"custom model needs HIP source")
    row("custom-nparams-negative", lambda w: w.packed(CUSTOM, 4, nparams=-1), BAD, b"custom model: bad params")
    row("custom-params-null", lambda w: w.packed(CUSTOM, 4, nparams=3), BAD, b"custom model: bad params")
    row("custom-D-600", lambda w: w.packed(CUSTOM, 600), BAD, b"custom model with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)")
    row("diag-no-mu", lambda w: w.packed(DIAG, 4, tau=np.ones(4)), BAD, b"model needs mu")
    row("diag-no-tau", lambda w: w.packed(DIAG, 4, mu=np.zeros(4)), BAD, b"diagonal model needs tau")
    row("dense-no-prec", lambda w: w.packed(DENSE, 3, mu=np.zeros(3)), BAD, b"dense model needs prec")
    row("dense-asymmetric", lambda w: w.packed(DENSE, 3, mu=np.zeros(3), prec=np.eye(3) + np.eye(3, k=1) * np.array([[0.0], [0.5], [0.0]])), BAD, b"prec must be exactly symmetric (differs at [1,2]); pass (P+P')/2")
    row("dense-D-600", lambda w: w.packed(DENSE, 600, mu=np.zeros(600), prec=np.eye(600)), BAD, b"dense model with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)")
    row("max-depth-0", lambda w: w.packed(ISO, 4, opt=w.opt(max_depth=0)), BAD, b"max_depth = 0 unsupported (1..15)")
    row("max-depth-16", lambda w: w.packed(ISO, 4, opt=w.opt(max_depth=16)), BAD, b"max_depth = 16 unsupported (1..15)")
    row("min-delta-0", lambda w: w.packed(ISO, 4, opt=w.opt(min_delta=0.0)), BAD, b"min_delta must be negative")
    row("eps-init-0", lambda w: w.packed(ISO, 4, opt=w.opt(eps_init=0.0)), BAD, b"eps_init must be positive")
    row("iso-valid", lambda w: w.packed(ISO, 4), OK)
    # ---- logistic regression, [X | y] -------------------------------------------------------------------------------------------------
    row("lr-valid", lambda w: w.packed(LR, 6, w.logit, source=None), OK)
    row("lr-valid-prior", lambda w: w.packed(LR, 6, w.logit, source=None, mu=np.full(6, 1.0), tau=np.full(6, 0.25)), OK)
    row("lr-valid-n-1-D-1", lambda w: w.packed(LR, 1, [0.5, 1.0], source=None), OK)
    row("lr-nparams-not-multiple", lambda w: w.packed(LR, 6, w.logit[:-1], source=None), BAD, b"logistic regression: nparams = 349 must be a positive multiple of D + 1 = 7 ([X | y])")
    row("lr-nparams-0", lambda w: w.packed(LR, 6, w.logit, nparams=0, source=None), BAD, b"logistic regression: nparams = 0 must be a positive multiple of D + 1 = 7 ([X | y])")
    row("lr-params-null", lambda w: w.packed(LR, 6, w.logit, null_params=True, source=None), BAD, b"logistic regression: nparams = 350 must be a positive multiple of D + 1 = 7 ([X | y])")
    row("lr-y-half", lambda w: w.packed(LR, 6, w.logit, {300 + 3: 0.5}, source=None), BAD, b"logistic regression: y[3] = 0.5 is neither 0 nor 1")
    row("lr-y-nan", lambda w: w.packed(LR, 6, w.logit, {300 + 49: np.nan}, source=None), BAD, b"logistic regression: y[49] = nan is neither 0 nor 1")
    row("lr-X-inf", lambda w: w.packed(LR, 6, w.logit, {17: np.inf}, source=None), BAD, b"logistic regression: X[2, 5] is not finite")
    row("lr-tau-0", lambda w: w.packed(LR, 6, w.logit, source=None, tau=[1, 1, 1, 1, 0, 1]), BAD, b"logistic regression: prior precision tau[4] = 0 must be finite and > 0")
    row("lr-mu-nan", lambda w: w.packed(LR, 6, w.logit, source=None, mu=[0, np.nan, 0, 0, 0, 0]), BAD, b"logistic regression: prior mean mu[1] is not finite")
    row("lr-D-600", lambda w: w.packed(LR, 600, np.r_[np.ones(1200), 0.0, 1.0], source=None), BAD, b"logistic regression with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)")
    row("lr-D-600-shared", lambda w: w.packed(LR, 600, np.r_[np.ones(1200), 0.0, 1.0], source=None, opt=w.opt(metric_mode=w.idhmc.METRIC_SHARED)), OK)
    row("lr-D-1100", lambda w: w.packed(LR, 1100, np.zeros(1101), source=None), BAD, b"D = 1100: logistic regression is limited to D <= 1024")
    row("lr-n-too-large", lambda w: w.packed(LR, 6, w.logit, nparams=N_BIG * 7, source=None), BAD, b"logistic regression: n = 1048577 observations at D = 6 exceed n_pad * L <= 2^27 (at most 1048576)")
    # ---- packed GLM, [K, nc, c | X | Y] -----------------------------------------------------------------------------------------------
    src = lambda w: w.idhmc.glm.POISSON_LOG_OFFSET.encode()
    row("glm-valid", lambda w: w.packed(GLM, 6, w.glm, source=src(w)), OK)
    row("glm-valid-n-1-D-1-nc-0", lambda w: w.packed(GLM, 1, [1.0, 0.0, 0.5, 2.0], source=w.idhmc.glm.POISSON_LOG.encode()), OK)
    row("glm-valid-nc-16", lambda w: w.packed(GLM, 2, np.r_[1.0, 16.0, np.arange(1.0, 17.0), 0.5, -0.5, 0.25, 1.0, 0.0, 2.0],
                                              source=HIER.GAUSSIAN_KNOWN_SOURCE.encode()), OK)
    for k, msg in ((0.0, b"GLM: K = 0 must be an integer in 1..4"),
                   (5.0, b"GLM: K = 5 must be an integer in 1..4"),
                   (1.5, b"GLM: K = 1.5 must be an integer in 1..4"),
                   (-1.0, b"GLM: K = -1 must be an integer in 1..4"),
                   (np.nan, b"GLM: K = nan must be an integer in 1..4"),
                   (np.inf, b"GLM: K = inf must be an integer in 1..4")):
        row("glm-K-%g" % k, lambda w, k=k: w.packed(GLM, 6, w.glm, {0: k}), BAD, msg)
    for nc, msg in ((-1.0, b"GLM: nc = -1 must be an integer in 0..16"),
                    (17.0, b"GLM: nc = 17 must be an integer in 0..16"),
                    (0.5, b"GLM: nc = 0.5 must be an integer in 0..16"),
                    (np.nan, b"GLM: nc = nan must be an integer in 0..16")):
        row("glm-nc-%g" % nc, lambda w, nc=nc: w.packed(GLM, 6, w.glm, {1: nc}), BAD, msg)
    row("glm-K-and-nc-bad", lambda w: w.packed(GLM, 6, w.glm, {0: 9.0, 1: 99.0}), BAD, b"GLM: K = 9 must be an integer in 1..4")
    row("glm-rest-not-multiple", lambda w: w.packed(GLM, 6, w.glm[:-1]), BAD, b"GLM: nparams - 2 - nc = 399 must be a positive multiple of D + K = 8 ([X | Y])")
    row("glm-no-observations", lambda w: w.packed(GLM, 6, w.glm[:4]), BAD, b"GLM: nparams - 2 - nc = 0 must be a positive multiple of D + K = 8 ([X | Y])")
    row("glm-nparams-is-header", lambda w: w.packed(GLM, 6, [1.0, 0.0]), BAD, b"GLM: nparams - 2 - nc = 0 must be a positive multiple of D + K = 7 ([X | Y])")
    row("glm-nparams-is-header-nc-2", lambda w: w.packed(GLM, 6, [2.0, 2.0]), BAD, b"GLM: nparams - 2 - nc = -2 must be a positive multiple of D + K = 8 ([X | Y])")
    row("glm-nparams-one-short", lambda w: w.packed(GLM, 6, [1.0]), BAD, b"GLM: params must begin with K and nc ([K, nc, c | X | Y])")
    row("glm-nparams-0", lambda w: w.packed(GLM, 6, w.glm, nparams=0), BAD, b"GLM: params must begin with K and nc ([K, nc, c | X | Y])")
    row("glm-params-null", lambda w: w.packed(GLM, 6, w.glm, null_params=True), BAD, b"GLM: params must begin with K and nc ([K, nc, c | X | Y])")
    row("glm-c-nan", lambda w: w.packed(GLM, 6, w.glm, {3: np.nan}), BAD, b"GLM: constant c[1] is not finite")
    row("glm-X-inf", lambda w: w.packed(GLM, 6, w.glm, {4 + 17: np.inf}), BAD, b"GLM: X[2, 5] is not finite")
    row("glm-Y-inf", lambda w: w.packed(GLM, 6, w.glm, {4 + 300 + 7: -np.inf}), BAD, b"GLM: Y[3, 1] is not finite")
    row("glm-X-last-nan", lambda w: w.packed(GLM, 6, w.glm, {4 + 299: np.nan}), BAD, b"GLM: X[49, 5] is not finite")
    row("glm-Y-last-nan", lambda w: w.packed(GLM, 6, w.glm, {4 + 399: np.nan}), BAD, b"GLM: Y[49, 1] is not finite")
    row("glm-source-null", lambda w: w.packed(GLM, 6, w.glm, source=None), BAD, b"GLM needs HIP source (glm_observation)")
    row("glm-source-empty", lambda w: w.packed(GLM, 6, w.glm, source=b""), BAD, b"GLM needs HIP source (glm_observation)")
    row("glm-source-null-and-no-params", lambda w: w.packed(GLM, 6, source=None), BAD, b"GLM needs HIP source (glm_observation)")
    row("glm-tau-0", lambda w: w.packed(GLM, 6, w.glm, tau=[1, 1, 1, 1, 0, 1]), BAD, b"GLM: prior precision tau[4] = 0 must be finite and > 0")
    row("glm-tau-inf", lambda w: w.packed(GLM, 6, w.glm, tau=[np.inf, 1, 1, 1, 1, 1]), BAD, b"GLM: prior precision tau[0] = inf must be finite and > 0")
    row("glm-mu-nan", lambda w: w.packed(GLM, 6, w.glm, mu=[0, np.nan, 0, 0, 0, 0]), BAD, b"GLM: prior mean mu[1] is not finite")
    row("glm-D-600", lambda w: w.packed(GLM, 600, np.r_[1.0, 0.0, np.ones(1200), 0.0, 1.0]), BAD, b"GLM with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)")
    row("glm-D-600-shared", lambda w: w.packed(GLM, 600, np.r_[1.0, 0.0, np.ones(1200), 0.0, 1.0], source=w.idhmc.glm.POISSON_LOG.encode(),
                                               opt=w.opt(metric_mode=w.idhmc.METRIC_SHARED)), OK)
    row("glm-D-1100", lambda w: w.packed(GLM, 1100, np.r_[1.0, 0.0, np.zeros(1101)]), BAD, b"D = 1100: a GLM is limited to D <= 1024")
    row("glm-n-too-large", lambda w: w.packed(GLM, 6, w.glm, nparams=4 + N_BIG * 8), BAD, b"GLM: n = 1048577 observations at D = 6 exceed n_pad * L <= 2^27 (at most 1048576)")
    # ---- packed GLM with auxiliary coordinates, [K, nc, A, c | X | Y] -------------------------------------------------------------------
    srca = lambda w: w.idhmc.glm.WEIBULL_LOG_LOGSHAPE.encode()
    row("aux-valid", lambda w: w.packed(GAUX, 7, w.aux, source=srca(w)), OK)
    row("aux-valid-Dx-1", lambda w: w.packed(GAUX, 2, [1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0], source=w.idhmc.glm.GAUSSIAN_IDENTITY_LOGSIGMA.encode()), OK)
    row("aux-valid-A-4-D-5-n-1", lambda w: w.packed(GAUX, 5, [2.0, 0.0, 4.0, 0.5, 1.0, 2.0], source=AUX.TEST_A4_SOURCE.encode()), OK)
    for a, msg in ((0.0, b"GLM_AUX: A = 0 must be an integer in 1..4"),
                   (5.0, b"GLM_AUX: A = 5 must be an integer in 1..4"),
                   (1.5, b"GLM_AUX: A = 1.5 must be an integer in 1..4"),
                   (-1.0, b"GLM_AUX: A = -1 must be an integer in 1..4"),
                   (np.nan, b"GLM_AUX: A = nan must be an integer in 1..4"),
                   (np.inf, b"GLM_AUX: A = inf must be an integer in 1..4")):
        row("aux-A-%g" % a, lambda w, a=a: w.packed(GAUX, 7, w.aux, {2: a}), BAD, msg)
    row("aux-A-4-D-4", lambda w: w.packed(GAUX, 4, w.aux, {2: 4.0}), BAD, b"GLM_AUX: Dx = D - A = 0: at least one coefficient is needed")
    row("aux-A-4-D-3", lambda w: w.packed(GAUX, 3, w.aux, {2: 4.0}), BAD, b"GLM_AUX: Dx = D - A = -1: at least one coefficient is needed")
    for k, msg in ((0.0, b"GLM_AUX: K = 0 must be an integer in 1..4"),
                   (5.0, b"GLM_AUX: K = 5 must be an integer in 1..4"),
                   (1.5, b"GLM_AUX: K = 1.5 must be an integer in 1..4"),
                   (-1.0, b"GLM_AUX: K = -1 must be an integer in 1..4"),
                   (np.nan, b"GLM_AUX: K = nan must be an integer in 1..4"),
                   (np.inf, b"GLM_AUX: K = inf must be an integer in 1..4")):
        row("aux-K-%g" % k, lambda w, k=k: w.packed(GAUX, 7, w.aux, {0: k}), BAD, msg)
    for nc, msg in ((-1.0, b"GLM_AUX: nc = -1 must be an integer in 0..16"),
                    (17.0, b"GLM_AUX: nc = 17 must be an integer in 0..16"),
                    (0.5, b"GLM_AUX: nc = 0.5 must be an integer in 0..16"),
                    (np.nan, b"GLM_AUX: nc = nan must be an integer in 0..16")):
        row("aux-nc-%g" % nc, lambda w, nc=nc: w.packed(GAUX, 7, w.aux, {1: nc}), BAD, msg)
    row("aux-nc-and-A-bad", lambda w: w.packed(GAUX, 7, w.aux, {1: 20.0, 2: 0.0}), BAD, b"GLM_AUX: nc = 20 must be an integer in 0..16")
    row("aux-rest-not-multiple", lambda w: w.packed(GAUX, 7, w.aux[:-1]), BAD, b"GLM_AUX: nparams - 3 - nc = 399 must be a positive multiple of Dx + K = 8 ([X | Y])")
    row("aux-no-observations", lambda w: w.packed(GAUX, 7, w.aux[:5]), BAD, b"GLM_AUX: nparams - 3 - nc = 0 must be a positive multiple of Dx + K = 8 ([X | Y])")
    row("aux-D-8", lambda w: w.packed(GAUX, 8, w.aux), BAD, b"GLM_AUX: nparams - 3 - nc = 400 must be a positive multiple of Dx + K = 9 ([X | Y])")
    row("aux-nparams-is-header", lambda w: w.packed(GAUX, 7, [1.0, 0.0, 1.0]), BAD, b"GLM_AUX: nparams - 3 - nc = 0 must be a positive multiple of Dx + K = 7 ([X | Y])")
    row("aux-nparams-one-short", lambda w: w.packed(GAUX, 7, [1.0, 0.0]), BAD, b"GLM_AUX: params must begin with K, nc and A ([K, nc, A, c | X | Y])")
    row("aux-params-null", lambda w: w.packed(GAUX, 7, w.aux, null_params=True), BAD, b"GLM_AUX: params must begin with K, nc and A ([K, nc, A, c | X | Y])")
    row("aux-c-nan", lambda w: w.packed(GAUX, 7, w.aux, {4: np.nan}), BAD, b"GLM_AUX: constant c[1] is not finite")
    row("aux-X-inf", lambda w: w.packed(GAUX, 7, w.aux, {5 + 17: np.inf}), BAD, b"GLM_AUX: X[2, 5] is not finite")
    row("aux-Y-inf", lambda w: w.packed(GAUX, 7, w.aux, {5 + 300 + 7: -np.inf}), BAD, b"GLM_AUX: Y[3, 1] is not finite")
    row("aux-source-null", lambda w: w.packed(GAUX, 7, w.aux, source=None), BAD, b"GLM needs HIP source (glm_observation)")
    row("aux-source-empty", lambda w: w.packed(GAUX, 7, w.aux, source=b""), BAD, b"GLM needs HIP source (glm_observation)")
    row("aux-tau-0", lambda w: w.packed(GAUX, 7, w.aux, tau=[1, 1, 1, 1, 1, 1, 0]), BAD, b"GLM_AUX: prior precision tau[6] = 0 must be finite and > 0")
    row("aux-mu-nan", lambda w: w.packed(GAUX, 7, w.aux, mu=[0, 0, 0, 0, 0, 0, np.nan]), BAD, b"GLM_AUX: prior mean mu[6] is not finite")
    row("aux-D-513", lambda w: w.packed(GAUX, 513, np.r_[1.0, 0.0, 1.0, np.ones(1024), 0.0, 1.0]), BAD, b"GLM_AUX with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)")
    row("aux-D-1100", lambda w: w.packed(GAUX, 1100, np.r_[1.0, 0.0, 1.0, np.zeros(1100)]), BAD, b"D = 1100: a GLM is limited to D <= 1024")
    row("aux-n-too-large", lambda w: w.packed(GAUX, 7, w.aux, nparams=5 + N_BIG * 8), BAD, b"GLM_AUX: n = 1048577 observations at D = 7 exceed n_pad * L <= 2^27 (at most 1048576)")
    # ---- idhmc_create_glm: a GLM in parts, with groups ---------------------------------------------------------------------------------
    row("parts-valid", lambda w: w.parts(source=srca(w)), OK)
    row("parts-valid-plain", lambda w: w.parts(X=w.X[:30, :5], Y=w.Y2[:30, :1], K=1, nc=0, A=0, H=0, constants=None, groups=None,
                                               source=w.idhmc.glm.POISSON_LOG.encode()), OK)
    row("parts-valid-Dx-1-n-1", lambda w: w.parts(X=[[0.5]], Y=[[2.0]], K=1, nc=0, A=0, H=0, constants=None, groups=None,
                                                  source=w.idhmc.glm.POISSON_LOG.encode()), OK)
    row("parts-valid-A-4", lambda w: w.parts(X=[[0.5]], Y=[[1.0, 2.0]], K=2, nc=0, A=4, H=0, constants=None, groups=None, source=AUX.TEST_A4_SOURCE.encode()), OK)
    row("parts-null-desc", lambda w: w.parts(null_desc=True), BAD, b"idhmc_create_glm: null argument")
    for H, msg in ((-1, b"GLM: H = -1 must be an integer in 0..4"),
                   (5, b"GLM: H = 5 must be an integer in 0..4"),
                   (100, b"GLM: H = 100 must be an integer in 0..4")):
        row("parts-H-%d" % H, lambda w, H=H: w.parts(H=H), BAD, msg)
    row("parts-groups-null", lambda w: w.parts(groups=None), BAD, b"GLM: H = 2 groups need the group of every column (groups is NULL)")
    row("parts-groups-with-H-0", lambda w: w.parts(H=0), BAD, b"GLM: groups must be NULL with H = 0")
    for g, msg in ((-2, b"GLM: groups[3] = -2 is outside -1..1"),
                   (2, b"GLM: groups[3] = 2 is outside -1..1"),
                   (7, b"GLM: groups[3] = 7 is outside -1..1")):
        row("parts-groups-3-is-%d" % g, lambda w, g=g: w.parts(groups=[-1, 0, 0, g, 1, -1]), BAD, msg)
    row("parts-group-1-empty", lambda w: w.parts(groups=[-1, 0, 0, 0, 0, -1]), BAD, b"GLM: group 1 has no column")
    row("parts-group-0-empty", lambda w: w.parts(groups=[-1, 1, 1, 1, 1, -1]), BAD, b"GLM: group 0 has no column")
    row("parts-group-2-empty", lambda w: w.parts(H=3), BAD, b"GLM: group 2 has no column")
    for Dx, msg in ((0, b"GLM: Dx = 0: at least one coefficient is needed"),
                    (-3, b"GLM: Dx = -3: at least one coefficient is needed")):
        row("parts-Dx-%d" % Dx, lambda w, Dx=Dx: w.parts(Dx=Dx), BAD, msg)
    for K, msg in ((0, b"GLM_AUX: K = 0 must be an integer in 1..4"),
                   (5, b"GLM_AUX: K = 5 must be an integer in 1..4"),
                   (-1, b"GLM_AUX: K = -1 must be an integer in 1..4")):
        row("parts-K-%d" % K, lambda w, K=K: w.parts(K=K), BAD, msg)
    for nc, msg in ((-1, b"GLM_AUX: nc = -1 must be an integer in 0..16"),
                    (17, b"GLM_AUX: nc = 17 must be an integer in 0..16")):
        row("parts-nc-%d" % nc, lambda w, nc=nc: w.parts(nc=nc), BAD, msg)
    for A, msg in ((-1, b"GLM: A = -1 must be an integer in 0..4"),
                   (5, b"GLM: A = 5 must be an integer in 0..4")):
        row("parts-A-%d" % A, lambda w, A=A: w.parts(A=A), BAD, msg)
    row("parts-plain-K-0", lambda w: w.parts(K=0, A=0, H=0, groups=None), BAD, b"GLM: K = 0 must be an integer in 1..4")
    row("parts-n-0", lambda w: w.parts(n=0), BAD, b"GLM_AUX: n = 0: at least one observation is needed")
    row("parts-X-null", lambda w: w.parts(null_X=True), BAD, b"GLM_AUX: X and Y are needed")
    row("parts-Y-null", lambda w: w.parts(null_Y=True), BAD, b"GLM_AUX: X and Y are needed")
    row("parts-constants-null", lambda w: w.parts(constants=None), BAD, b"GLM_AUX: nc = 2 constants are needed")
    row("parts-c-nan", lambda w: w.parts(constants=[1.0, np.nan]), BAD, b"GLM_AUX: constant c[1] is not finite")
    row("parts-X-inf", lambda w: w.parts(X=_with(w.Xa, (2, 5), np.inf)), BAD, b"GLM_AUX: X[2, 5] is not finite")
    row("parts-Y-inf", lambda w: w.parts(Y=_with(w.Ya, (3, 1), -np.inf)), BAD, b"GLM_AUX: Y[3, 1] is not finite")
    row("parts-source-null", lambda w: w.parts(source=None), BAD, b"GLM needs HIP source (glm_observation)")
    row("parts-source-empty", lambda w: w.parts(source=b""), BAD, b"GLM needs HIP source (glm_observation)")
    row("parts-tau-0", lambda w: w.parts(tau=[1, 1, 1, 1, 1, 1, 1, 1, 0]), BAD, b"GLM_AUX: prior precision tau[8] = 0 must be finite and > 0")
    row("parts-mu-nan", lambda w: w.parts(mu=[0, 0, 0, 0, 0, 0, 0, np.nan, 0]), BAD, b"GLM_AUX: prior mean mu[7] is not finite")
    row("parts-D-513", lambda w: w.parts(X=np.ones((2, 510)), Y=np.zeros((2, 1)), K=1, nc=0, constants=None, groups=[0, 1] * 255), BAD, b"GLM_AUX with D > 512 needs metric_mode = SHARED (LDS budget of the NUTS kernel)")
    row("parts-D-1025", lambda w: w.parts(X=np.ones((2, 510)), Y=np.zeros((2, 1)), K=1, nc=0, constants=None, groups=[0, 1] * 255, Dx=1022), BAD, b"D = Dx + A + H = 1025: a GLM is limited to D <= 1024")
    row("parts-n-too-large", lambda w: w.parts(n=N_BIG), BAD, b"GLM_AUX: n = 1048577 observations at D = 9 exceed n_pad * L <= 2^27 (at most 1048576)")
    row("parts-nchains-0", lambda w: w.parts(nchains=0), BAD, b"nchains = 0 out of range")
    row("parts-K-bad-and-no-source", lambda w: w.parts(K=0, source=None), BAD, b"GLM needs HIP source (glm_observation)")
    # ---- idhmc_create_glm_responses -----------------------------------------------------------------------------------------------------
    row("resp-valid", lambda w: w.parts(M=3, source=srca(w)), OK)
    row("resp-valid-shard", lambda w: w.parts(M=3, nchains=9, first=5, source=srca(w)), OK)
    row("resp-valid-M-1-global", lambda w: w.parts(M=1, R=40, nchains=40, source=srca(w), opt=w.opt(eps_mode=w.idhmc.EPS_GLOBAL)), OK)
    row("resp-valid-two-planes", lambda w: w.parts(M=2, R=9, Y=_with(w.Y3, (2, 10, 0), np.nan), source=srca(w)), OK)
    row("resp-null-desc", lambda w: w.parts(M=3, null_desc=True), BAD, b"idhmc_create_glm_responses: null argument")
    for M, msg in ((0, b"GLM_AUX: M = 0: at least one response is needed"),
                   (-1, b"GLM_AUX: M = -1: at least one response is needed"),
                   (-100, b"GLM_AUX: M = -100: at least one response is needed")):
        row("resp-M-%d" % M, lambda w, M=M: w.parts(M=M), BAD, msg)
    for R_, msg in ((0, b"GLM_AUX: chains_per_response = 0: at least one chain per response is needed"),
                    (-1, b"GLM_AUX: chains_per_response = -1: at least one chain per response is needed"),
                    (-7, b"GLM_AUX: chains_per_response = -7: at least one chain per response is needed")):
        row("resp-R-%d" % R_, lambda w, R_=R_: w.parts(M=3, R=R_), BAD, msg)
    row("resp-19-chains", lambda w: w.parts(M=3, nchains=19), BAD, b"GLM_AUX: first_chain_id + nchains = 19 is past the M * chains_per_response = 3 * 6 chains of the model")
    row("resp-chain-18", lambda w: w.parts(M=3, nchains=1, first=18), BAD, b"GLM_AUX: first_chain_id + nchains = 19 is past the M * chains_per_response = 3 * 6 chains of the model")
    row("resp-M-2-chains-5-to-13", lambda w: w.parts(M=2, nchains=9, first=5), BAD, b"GLM_AUX: first_chain_id + nchains = 14 is past the M * chains_per_response = 2 * 6 chains of the model")
    row("resp-R-1-5-chains", lambda w: w.parts(M=3, R=1, nchains=5), BAD, b"GLM_AUX: first_chain_id + nchains = 5 is past the M * chains_per_response = 3 * 1 chains of the model")
    row("resp-M-2^19+1", lambda w: w.parts(M=(1 << 19) + 1), BAD, b"GLM_AUX: M = 524289 responses of K = 2 columns and n = 50 observations exceed M * K * n_pad <= 2^27")
    row("resp-M-2^40", lambda w: w.parts(M=1 << 40), BAD, b"GLM_AUX: M = 1099511627776 responses of K = 2 columns and n = 50 observations exceed M * K * n_pad <= 2^27")
    row("resp-M-R-2^62", lambda w: w.parts(M=1 << 62, R=1 << 62), BAD, b"GLM_AUX: M = 4611686018427387904 responses of K = 2 columns and n = 50 observations exceed M * K * n_pad <= 2^27")
    row("resp-global-eps", lambda w: w.parts(M=3, opt=w.opt(eps_mode=w.idhmc.EPS_GLOBAL)), BAD, b"GLM_AUX: M = 3 responses with eps_mode = GLOBAL: the global stepsize pools the acceptance of chains that sample different posteriors (use PER_CHAIN)")
    row("resp-pooled-metric", lambda w: w.parts(M=2, R=9, opt=w.opt(metric_mode=w.idhmc.METRIC_POOLED)), BAD, b"GLM_AUX: M = 2 responses with metric_mode = POOLED: the pooled metric pools the windows of chains that sample different posteriors (use PER_CHAIN or SHARED)")
    for (m_, i, k), msg in (((0, 3, 1), b"GLM_AUX: Y[3, 1] is not finite"),
                            ((1, 0, 0), b"GLM_AUX: Y[1, 0, 0] is not finite"),
                            ((2, 49, 1), b"GLM_AUX: Y[2, 49, 1] is not finite")):
        row("resp-Y-%d-%d-%d-inf" % (m_, i, k), lambda w, at=(m_, i, k): w.parts(M=3, Y=_with(w.Y3, at, np.inf)), BAD, msg)
    row("resp-H-5", lambda w: w.parts(M=3, H=5), BAD, b"GLM: H = 5 must be an integer in 0..4")
    row("resp-groups-null", lambda w: w.parts(M=3, groups=None), BAD, b"GLM: H = 2 groups need the group of every column (groups is NULL)")
    row("resp-Dx-0", lambda w: w.parts(M=3, Dx=0), BAD, b"GLM: Dx = 0: at least one coefficient is needed")
    row("resp-K-5", lambda w: w.parts(M=3, K=5), BAD, b"GLM_AUX: K = 5 must be an integer in 1..4")
    row("resp-n-0", lambda w: w.parts(M=3, n=0), BAD, b"GLM_AUX: n = 0: at least one observation is needed")
    row("resp-X-null", lambda w: w.parts(M=3, null_X=True), BAD, b"GLM_AUX: X and Y are needed")
    row("resp-c-nan", lambda w: w.parts(M=3, constants=[1.0, np.nan]), BAD, b"GLM_AUX: constant c[1] is not finite")
    row("resp-X-inf", lambda w: w.parts(M=3, X=_with(w.Xa, (2, 5), np.inf)), BAD, b"GLM_AUX: X[2, 5] is not finite")
    row("resp-source-null", lambda w: w.parts(M=3, source=None), BAD, b"GLM needs HIP source (glm_observation)")
    row("resp-tau-0", lambda w: w.parts(M=3, tau=[1, 1, 1, 1, 1, 1, 1, 1, 0]), BAD, b"GLM_AUX: prior precision tau[8] = 0 must be finite and > 0")
    row("resp-nchains-0", lambda w: w.parts(M=3, nchains=0), BAD, b"nchains = 0 out of range")
    row("resp-first-negative", lambda w: w.parts(M=3, nchains=2, first=-1), BAD, b"chain ids must fit 32 bits")
    row("resp-n-too-large", lambda w: w.parts(M=3, n=N_BIG), BAD, b"GLM_AUX: n = 1048577 observations at D = 9 exceed n_pad * L <= 2^27 (at most 1048576)")
    row("resp-M-bad-and-K-bad", lambda w: w.parts(M=0, K=0), BAD, b"GLM_AUX: K = 0 must be an integer in 1..4")
    return R


def _with(a, at, v):
    a = np.array(a, float)
    a[at] = v
    return a


ROWS = _rows()


@pytest.fixture(scope="module")
def world(idhmc):
    return World(idhmc)


def test_every_row_has_its_own_name():
    names = [r[0] for r in ROWS]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("name,call,code,message", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(world, name, call, code, message):
    idhmc = world.idhmc
    rc, msg = call(world)
    if code == OK:
        assert rc == 0 or (rc == idhmc.ERR_NO_DEVICE and b"no HIP device" in msg), (name, rc, msg)
    else:
        assert (rc, msg) == (idhmc.ERR_BAD_ARG, message), (name, rc, msg)

