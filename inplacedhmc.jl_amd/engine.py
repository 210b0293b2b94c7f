"""Engine: thin object wrapper over the C ABI (include/idhmc.h).  All compute happens in libidhmc.so's
HIP kernels; numpy arrays are only the host side of the getters/setters."""
import ctypes as C
import numpy as np

from . import _lib
from . import glm as _glm
from ._lib import (GlmBlock, GlmDesc, GlmFactors, GlmFactorValues, GlmGmrfs, GlmLocal, GlmMembers, GlmModel, GlmPairs, GlmPriors, GlmStructs,
                   ModelDesc, Options, check)

# reference TreeStatisticsNUTS (src/NUTS.jl:229-242), 32 bytes
TREE_STATS_DTYPE = np.dtype([("pi", "<f8"), ("acceptance_rate", "<f8"), ("term_left", "<i4"),
                             ("term_right", "<i4"), ("depth", "<i4"), ("steps", "<i4")])
assert TREE_STATS_DTYPE.itemsize == 32

MODEL_ISO_GAUSSIAN, MODEL_DIAG_GAUSSIAN, MODEL_DENSE_MVN, MODEL_CUSTOM, MODEL_LOGISTIC_REGRESSION, MODEL_GLM = 0, 1, 2, 3, 4, 5
MODEL_GLM_AUX = 6
EPS_PER_CHAIN, EPS_GLOBAL, EPS_PER_RESPONSE = 0, 1, 2
METRIC_PER_CHAIN, METRIC_SHARED, METRIC_POOLED, METRIC_PER_RESPONSE = 0, 1, 2, 3
GRAD_STORE, GRAD_RECOMPUTE = 0, 1
T_ADAPT_EPS, T_ACCUM_METRIC, T_ACCUM_MOMENTS, T_KEEP_P, T_USE_DIRECTIONS, T_ACCUM_DIAG = 1, 2, 4, 8, 16, 32
XCHG_DOUBLES, XCHG_ACCEPT, XCHG_LOGEPS = 4, 0, 1
POOL_SEGMENT = 1024
# status codes of include/idhmc.h (IdhmcError.code)
(ERR_BAD_ARG, ERR_HIP, ERR_EPS_UNDERFLOW, ERR_STEPSIZE_SEARCH, ERR_NONFINITE_START, ERR_NO_DEVICE, ERR_ALLOC, ERR_OPTIMIZATION,
 ERR_PEER) = range(1, 10)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def xchg_accumulate(kind, values, record=None):
    """Host side of the global-stepsize exchange (include/idhmc.h): add the fixed-point record of `values` to
    `record` (4 doubles: hi-limb sum, lo-limb sum, count, errors).  Integer-valued, so records of shards add exactly."""
    rec = np.zeros(XCHG_DOUBLES) if record is None else record
    v = np.ascontiguousarray(values, dtype=np.float64).ravel()
    check(_lib.load().idhmc_xchg_accumulate(int(kind), _dp(v), v.size, _dp(rec)))
    return rec


def xchg_mean(kind, record):
    rec = np.ascontiguousarray(record, dtype=np.float64)
    out = C.c_double()
    check(_lib.load().idhmc_xchg_mean(int(kind), _dp(rec), C.byref(out)))
    return out.value


class Model:
    """The user log density handed to the engine (reference: an AbstractProbabilityModel{D} with
    logdensity_and_gradient!, src/kinetic_energy.jl:73): a built-in device density or HIP source."""

    def __init__(self, kind, D, mu=None, tau=None, prec=None, source=None, params=None):
        self.kind, self.D = int(kind), int(D)
        self.source = None if source is None else source.encode("utf-8")
        self.params = None if params is None else np.ascontiguousarray(params, dtype=np.float64).ravel()
        self.mu = None if mu is None else np.ascontiguousarray(mu, dtype=np.float64)
        self.tau = None if tau is None else np.ascontiguousarray(tau, dtype=np.float64)
        self.prec = None if prec is None else np.ascontiguousarray(prec, dtype=np.float64)
        for name, arr, shape in (("mu", self.mu, (self.D,)), ("tau", self.tau, (self.D,)),
                                 ("prec", self.prec, (self.D, self.D))):
            if arr is not None and arr.shape != shape:
                raise ValueError("%s must have shape %s" % (name, shape))

    def glm_desc(self):
        """the descriptor of idhmc_create_glm and idhmc_create_glm_responses (a GLM with coefficient groups or several responses keeps
        X, Y and its constants as arrays; with responses Y is (M, n, K))"""
        d = GlmDesc(n=self.n, Dx=self.Dx, K=self.K, nc=self.nc, A=self.A, H=self.H, X=_dp(self.X), Y=_dp(self.Y), source=self.source)
        if self.nc:
            d.constants = _dp(self.constants)
        if self.groups is not None:
            d.groups = self.groups.ctypes.data_as(C.POINTER(C.c_int32))
        if self.mu is not None:
            d.mu = _dp(self.mu)
        if self.tau is not None:
            d.tau = _dp(self.tau)
        return d

    def glm_model(self):
        """the idhmc_glm_model of idhmc_create_glm_model: every part this model has, built once.  The part structs are kept on the
        returned struct as .parts, because a ctypes pointer field does not keep what it points to alive"""
        def i32(a):
            return a.ctypes.data_as(C.POINTER(C.c_int32))
        members = self.member_width is not None      # a table of members: factors gives F and levels only, and there are no values
        parts = {"glm": self.glm_desc()}
        if self.prior_kind is not None:
            parts["priors"] = GlmPriors(kind=i32(self.prior_kind), nu=_dp(self.prior_nu))
        if self.J > 0:
            parts["local"] = GlmLocal(local=i32(self.local), slab_scale=self.slab_scale or 0.0)
        if self.F > 0:
            parts["factors"] = GlmFactors(F=self.F, levels=i32(self.levels), index=None if members else i32(self.factor_index))
        if self.factor_has is not None:
            parts["values"] = GlmFactorValues(values=_dp(self.factor_values), has=i32(self.factor_has))
        if self.P > 0:
            parts["pairs"] = GlmPairs(P=self.P, first=i32(self.pair_first), second=i32(self.pair_second), eta=_dp(self.pair_eta))
        if self.S > 0:
            parts["structs"] = GlmStructs(S=self.S, term=i32(self.struct_term), kind=i32(self.struct_kind), eta=_dp(self.struct_eta))
        if self.G > 0:
            parts["gmrfs"] = GlmGmrfs(G=self.G, term=i32(self.gmrf_term), start=self.gmrf_start.ctypes.data_as(C.POINTER(C.c_int64)),
                                      col=i32(self.gmrf_col), val=_dp(self.gmrf_val), kappa=_dp(self.gmrf_kappa))
        if self.BK > 0:
            parts["block"] = GlmBlock(K=self.BK, term=i32(self.block_term), eta=self.block_eta)
        if members:
            parts["members"] = GlmMembers(width=i32(self.member_width), index=i32(self.member_index), values=_dp(self.member_values))
        gm = GlmModel(M=self.M if self.R is not None else 1, chains_per_response=self.R or 0, **{k: C.pointer(v) for k, v in parts.items()})
        gm.parts = parts
        return gm

    def desc(self):
        d = ModelDesc(kind=self.kind, D=self.D)
        if self.mu is not None:
            d.mu = _dp(self.mu)
        if self.tau is not None:
            d.tau = _dp(self.tau)
        if self.prec is not None:
            d.prec = _dp(self.prec)
        if self.source is not None:
            d.source = self.source
        if self.params is not None and self.params.size:
            d.params = _dp(self.params)
            d.nparams = self.params.size
        return d


def IsoGaussian(D):
    """l(q) = -1/2 |q|^2"""
    return Model(MODEL_ISO_GAUSSIAN, D)


def DiagGaussian(mu, sigma=None, tau=None):
    """l(q) = -1/2 sum (q-mu)^2 / sigma^2"""
    mu = np.asarray(mu, dtype=np.float64)
    if tau is None:
        tau = 1.0 / np.asarray(sigma, dtype=np.float64) ** 2
    return Model(MODEL_DIAG_GAUSSIAN, mu.shape[0], mu=mu, tau=tau)


def DenseMVN(mu, prec):
    """l(q) = -1/2 (q-mu)' prec (q-mu)"""
    mu = np.asarray(mu, dtype=np.float64)
    return Model(MODEL_DENSE_MVN, mu.shape[0], mu=mu, prec=prec)


def CustomDensity(D, source, params=None):
    """A user-supplied density as HIP device source (include/idhmc.h, IDHMC_MODEL_CUSTOM): `source` defines
    template <int NCH> __device__ double logdensity_and_gradient(const Vec<NCH>&, Vec<NCH>&, const UserCtx&);
    it is compiled with hipRTC against the engine's kernels when the Engine is created."""
    return Model(MODEL_CUSTOM, D, source=source, params=params)


def LogisticRegression(X, y, prior_mu=None, prior_tau=None):
    """Bayesian logistic regression (include/idhmc.h, IDHMC_MODEL_LOGISTIC_REGRESSION), the data shared by every chain:
    l(q) = sum_i [y_i z_i - softplus(z_i)] - 1/2 sum_c tau_c (q_c - mu_c)^2,  z = X q.
    X: (n, D) finite, y: (n,) of 0 and 1; prior_mu, prior_tau: (D,) or scalars, default 0 and 1, tau > 0."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be a non-empty (n, D) matrix, got shape %s" % (X.shape,))
    n, D = X.shape
    if D > 1024:
        raise ValueError("logistic regression is limited to D <= 1024 (D = %d)" % D)
    if not np.isfinite(X).all():
        raise ValueError("X must be finite")
    y = np.asarray(y)
    if y.shape != (n,):
        raise ValueError("y must have shape (%d,), got %s" % (n, y.shape))
    y = y.astype(np.float64)
    if not np.all((y == 0.0) | (y == 1.0)):
        raise ValueError("every y_i must be 0 or 1")
    mu = tau = None
    if prior_mu is not None:
        mu = np.array(np.broadcast_to(np.asarray(prior_mu, dtype=np.float64), (D,)))
        if not np.isfinite(mu).all():
            raise ValueError("prior_mu must be finite")
    if prior_tau is not None:
        tau = np.array(np.broadcast_to(np.asarray(prior_tau, dtype=np.float64), (D,)))
        if not (np.isfinite(tau).all() and (tau > 0).all()):
            raise ValueError("prior_tau must be finite and > 0")
    m = Model(MODEL_LOGISTIC_REGRESSION, D, mu=mu, tau=tau, params=np.concatenate([X.ravel(), y]))
    m.n = n
    return m


def _prior(D, prior_mu, prior_tau):
    mu = tau = None
    if prior_mu is not None:
        mu = np.array(np.broadcast_to(np.asarray(prior_mu, dtype=np.float64), (D,)))
        if not np.isfinite(mu).all():
            raise ValueError("prior_mu must be finite")
    if prior_tau is not None:
        tau = np.array(np.broadcast_to(np.asarray(prior_tau, dtype=np.float64), (D,)))
        if not (np.isfinite(tau).all() and (tau > 0).all()):
            raise ValueError("prior_tau must be finite and > 0")
    return mu, tau


def GLM(X, Y, source, constants=None, prior_mu=None, prior_tau=None, aux=0, groups=None, chains_per_response=None, prior_kind=None,
        prior_nu=None, local=None, slab_scale=None, factors=None, correlated=None, structured=None, gmrf=None):
    """A generalised linear model with the user's likelihood (include/idhmc.h, IDHMC_MODEL_GLM), the data shared by every chain:
    l(q) = sum_i log p(y_i | z_i) - 1/2 sum_c tau_c (q_c - mu_c)^2,  z = X q.
    X: (n, D) finite; Y: (n, K) or (n,) finite, K <= 4 data columns per observation; constants: up to 16 finite numbers.
    `source` defines  __device__ void glm_observation(double z, const GlmObs &o, double &r, double &v)  with v = -log p(y | z)
    and r = d log p(y | z) / dz (o.y[k], k < o.K: the observation's columns; o.c[j], j < o.nc: the constants); ready-made
    sources are in inplacedhmc_jl_amd.glm.  prior_mu, prior_tau: (D,) or scalars, default 0 and 1, tau > 0.

    aux = A (1..4): the likelihood has A sampled auxiliary parameters (IDHMC_MODEL_GLM_AUX: a scale, a shape) that every
    observation sees.  A chain's position is [beta (Dx = X.shape[1] coefficients) | a (A)], the model's D is Dx + A, all
    unconstrained; `source` defines  glm_observation(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
    with s[j] = d log p(y | z, a) / da_j, and v includes the a-dependent normalising terms.  prior_mu, prior_tau: scalars or
    length Dx + A (the Gaussian prior covers the auxiliary coordinates).  The Model exposes Dx and A.

    groups: a length-Dx integer sequence, groups[c] in {-1, 0 .. H-1} (-1: column c is in no group), H <= 4 -- a hierarchical GLM
    (idhmc_create_glm): the columns of group g share a standard deviation sigma_g = exp(omega_g) that is itself sampled, in the
    non-centred parameterisation.  A chain's position is [u (Dx) | a (A) | omega (H)], the model's D is Dx + A + H; the coefficient
    of a grouped column is beta_c = exp(omega_g) u_c, of any other u_c; z = X beta.  The Gaussian prior is on the sampled
    coordinates (prior_mu, prior_tau: scalars or length Dx + A + H): with the defaults beta_c ~ N(0, sigma_g^2) and omega_g ~ N(0, 1).
    `source` is the one the same model takes without groups.  Draws come back in the sampled coordinates:
    glm.coefficients(model, draws) gives beta, glm.group_scales(model, draws) the sigma_g.  The Model exposes H and groups.

    chains_per_response = R (a positive integer): M responses on the one design matrix (idhmc_create_glm_responses) -- Y is 3-D,
    (M, n, K), and the chain of global id g samples the posterior of Y[g // R]; X, the prior, the constants, the source and the groups
    are shared.  An Engine (or the shards of a run, through first_chain) holds at most M * R chains, with a per-chain stepsize and a
    per-chain or SHARED metric (EPS_GLOBAL and METRIC_POOLED pool over chains of different posteriors and are refused with M > 1).
    EPS_PER_RESPONSE and METRIC_PER_RESPONSE pool over the R chains of each response instead: one dual-averaging stepsize, one adapted
    diagonal metric per response (D <= 512), bit-identical to a single-response model in EPS_GLOBAL / METRIC_POOLED on those chains;
    an Engine in either mode holds whole responses (first_chain and the number of chains are multiples of R).
    Each chain's draws are bit-identical to those of a single-response model on its Y.  glm.response_of_chain, glm.by_response and
    diagnostics.rhat_by_response sort chains and draws by response.  The Model exposes M and R (1 and None without the keyword).

    prior_kind, prior_nu: scalars or length Dx + A + H -- priors beyond the Gaussian (idhmc_create_glm_priors).  A kind is one of
    glm.PRIOR_NORMAL (the default), PRIOR_STUDENT_T, PRIOR_LOG_HALF_NORMAL, PRIOR_LOG_HALF_STUDENT_T, PRIOR_LOG_EXPONENTIAL or its name;
    prior_mu and prior_tau keep their places as location and precision (Student-t: q = mu + t_nu / sqrt(tau)), the log kinds put a
    half-normal, half-t or exponential prior with scale exp(mu) on exp(q) for an auxiliary coordinate or a group scale (tau = 1 there,
    never on a coefficient), prior_nu is the degrees of freedom of the two t kinds and 0 elsewhere.  glm.priors() assembles all four
    from glm.normal, glm.student_t, glm.half_normal, glm.half_student_t and glm.exponential.  With every kind PRIOR_NORMAL the model is
    the one without the keywords.  The Model exposes prior_kind and prior_nu (None without the keywords); Engine.glm_priors() reads them back.

    local, slab_scale: per-coefficient local scales (idhmc_create_glm_local) -- the horseshoe and, with a slab, its regularised form.
    local is a length-Dx boolean or 0/1 sequence, or True for every column; the J flagged columns, in ascending column order, each get
    one more sampled coordinate lambda_k, the logarithm of the column's local scale: a chain's position is
    [u (Dx) | a (A) | omega (H) | lambda (J)], the model's D is Dx + A + H + J, and prior_mu, prior_tau, prior_kind, prior_nu are scalars
    or of that length (the log kinds apply to lambda).  A flagged column of group g has beta_c = u_c st with s = exp(omega_g)
    exp(lambda_k) (exp(lambda_k) in no group), st = s without a slab and s / sqrt(1 + s^2 / S^2) with slab_scale = S > 0 (fixed, not
    sampled; None or 0: no slab; it needs a flagged column).  glm.horseshoe() assembles groups, local, slab_scale and the priors;
    glm.coefficients, glm.group_scales and glm.local_scales read draws.  With no column flagged the model is the one without the
    keywords.  The Model exposes J, local (int32, or None) and slab_scale (None without a slab); Engine.glm_local() reads them back.

    factors: a list of up to 4 factor terms by level index (idhmc_create_glm_factors) -- a random intercept per subject, site or item,
    (1 | subject), without an indicator column per level.  Each entry is an integer array idx of shape (n,), or (idx, N); N, the number
    of levels, defaults to max(idx) + 1, and idx[i] is in 0 .. N-1.  X holds the Dd dense columns only; the columns of the model are the
    dense ones, then the levels of factor 0, of factor 1, ..: Dx = Dd + sum N_f, and groups, local, prior_mu, prior_tau, prior_kind and
    prior_nu count those Dx columns (glm.factor_columns(model, f) is the slice of factor f; glm.random_intercepts() assembles groups and
    priors).  The model is bit for bit the one with glm.expand_factors(X, factors) as its design matrix, whose indicator columns are
    never built, stored or multiplied.  An empty list is the model without the keyword.  The Model exposes Dd, F, levels (int32 (F,)) and
    factor_index (int32 (F, n)), None and 0 without factors; Engine.glm_factors() reads them back.
    An entry may also be glm.term(idx, values=None, levels=None) (idhmc_create_glm_slopes): with values, a finite number per observation,
    the term is a random slope -- z_i takes values[i] * b[off_f + idx[i]] where a term without values adds b[off_f + idx[i]] -- and its
    N columns are columns of the model like any other term's, never stored.  Two terms may share one index: a random intercept and slope
    per subject, (1 + x | subject), is factors=[subject, glm.term(subject, values=x)] with **glm.random_intercepts(Dd, [N, N]), which
    gives the intercepts and the slopes a sampled scale each, the two independent unless the terms are paired (correlated, below).
    glm.expand_factors writes the values into the term's columns, and the bits stay those of the expanded model as long as no
    product underflows to -0 (include/idhmc.h).  The Model exposes factor_has (int32 (F,)) and factor_values (float64 (F, n), rows of
    terms without values 0), None when no term has values; Engine.glm_factor_values() reads them back.
    An entry may also be glm.members(index, weights=None, levels=None) (idhmc_create_glm_multi): a term of WIDTH M in 1..4 -- index and
    weights are (n, M), observation i has the levels index[i, m] >= 0 with weights[i, m] (-1: absent; present entries first, levels
    strictly ascending) and z_i takes sum_m weights[i, m] * b[off_f + index[i, m]].  The widths of all terms sum to at most 8.  That is
    a multi-membership effect, a Bradley-Terry match (+1, -1) or a spline basis: glm.bspline(x, n_basis) is such a term of width 4, and
    GLM(X, Y, source, factors=[glm.bspline(x, 20)], **glm.smooth_effects(Dd, [20])) is y ~ 1 + s(x), a P-spline whose penalty is the
    term's GMRF prior.  The bits stay those of glm.expand_factors.  A wide term may be grouped, carry local scales, be structured or a
    GMRF term, and is in no pair and no block.  The Model exposes member_width (int32 (F,)), member_index (int32 (P, n)) and
    member_values (float64 (P, n)), None without such an entry (then every term is in the table, a plain one as a plane of 1.0, and
    factor_has is None); Engine.glm_members() reads them back.

    correlated: a list of up to 2 glm.pair(first, second, eta=2.0) (idhmc_create_glm_corr) -- correlated random effects: two distinct terms
    with equal level counts, a term in at most one pair, share a sampled correlation rho = tanh(zeta) between level k of the first and
    level k of the second.  Each pair adds one coordinate at the end: a chain's position is
    [u (Dx) | a (A) | omega (H) | lambda (J) | zeta (P)], the model's D is Dx + A + H + J + P, and the prior keywords are scalars or of that
    length.  The second term's column of level k takes rho u_first + sqrt(1 - rho^2) u_second where it took u, before the group and local
    scales: with a group per term the effects of a level are sigma .* (L u), L = [[1, 0], [rho, sqrt(1 - rho^2)]].  eta > 0 is LKJ(eta) on
    the 2 x 2 correlation, (rho + 1) / 2 ~ Beta(eta, eta), and zeta's entries in the prior keywords must be the defaults; eta = 0 lets
    them apply (PRIOR_NORMAL or PRIOR_STUDENT_T on Fisher's z; the log kinds are refused).  glm.correlated_effects() assembles groups,
    priors and correlated; glm.correlations(model, draws) gives rho, glm.coefficients applies the mix.  An empty list is the model without
    the keyword.  The Model exposes P, pairs (a list of glm.Pair, None without),
    pair_first, pair_second (int32 (P,)) and pair_eta (float64 (P,)); Engine.glm_pairs() reads them back.
    A covariance among three or four terms is a correlation block (idhmc_create_glm_block): correlated=[glm.block(terms, eta=2.0)], the
    single entry of the list -- K = 2, 3 or 4 distinct terms of equal level counts, in the row order of L; the effects of a level are
    sigma .* (L u) with L the K x K Cholesky factor of a sampled correlation matrix, built from canonical partial correlations
    z_ji = tanh(zeta_ji).  The block adds K (K - 1) / 2 coordinates, row-major, where the pairs' zetas would stand (in front of the AR(1)
    zetas).  eta > 0 is LKJ(eta) on the matrix, the zetas' prior entries at their defaults; eta = 0 lets them apply.  A block term is not
    structured and no GMRF term; more than one block, K > 4 and a block next to pairs are out of scope.  glm.block_effects() assembles
    groups, priors and correlated; glm.cholesky_factors, glm.correlation_matrix and glm.correlations read draws, glm.coefficients applies
    the mix.  The Model exposes BK (K, 0 without), Bz (the zetas), block (a glm.Block, None without), block_term (int32 (K,)) and
    block_eta; Engine.glm_block() reads them back.

    structured: a list of up to 2 glm.ar1(term, eta=2.0) or glm.rw1(term) (idhmc_create_glm_struct) -- dependence among the levels of one
    term, level k being position k of the sequence: ut_0 = u_0, ut_k = phi ut_{k-1} + c u_k takes u's place before the scales, the
    stationary unit-variance AR(1) with phi = tanh(zeta), c = sqrt(1 - phi^2), or the first-order random walk phi = c = 1.  An AR(1)
    term adds one coordinate zeta = atanh phi at the very end, behind the pairs': a chain's position is
    [u (Dx) | a (A) | omega (H) | lambda (J) | zeta_pairs (P) | zeta_ar (Sz)] and D = Dx + A + H + J + P + Sz; a random walk adds none.
    eta > 0 is (phi + 1) / 2 ~ Beta(eta, eta) with zeta's prior entries at their defaults; eta = 0 lets them apply (normal or Student-t;
    the log kinds are refused).  A structured term has at least 2 levels, is in no pair and carries no local scale; groups (the term's
    sampled scale), values, priors, responses and pairs among other terms compose.  glm.structured_effects() assembles groups, priors,
    correlated and structured; glm.autocorrelations(model, draws) gives phi, glm.coefficients applies the scan.  An empty list is the model
    without the keyword.  RW2, a sum-to-zero constraint, seasonal and spatial (ICAR) structures are `gmrf` below; AR(p) is out of scope.
    The Model exposes S, Sz, structs (a list of glm.Structure, None without), struct_term, struct_kind (int32 (S,)) and struct_eta
    (float64 (S,)); Engine.glm_structs() reads them back.

    gmrf: a list of up to 2 glm.gmrf(term, Q, sum_to_zero=0.0) (idhmc_create_glm_gmrf) -- a Gaussian Markov random field prior on the
    levels u of one term: log p(u) = -1/2 u' Q u - 1/2 kappa (sum u)^2 with a sparse symmetric precision Q (dense, or an
    (indptr, indices, data) CSR triple) and kappa = sum_to_zero, in place of the iid N(0, 1).  No coordinate is added, so D, the reported
    vector, glm.coefficients and the device summaries are those of the model without the keyword; the scale of the effect is the term's
    group scale.  glm.icar_precision, rw1_precision, rw2_precision and seasonal_precision build the common Q, glm.scale_precision
    scales one to unit typical marginal variance (INLA's scale.model, BYM2's scaling); glm.gmrf_effects() assembles groups, priors and
    gmrf.  A GMRF term is in no pair, not structured, carries no local scale and keeps the default entries of the prior arrays on its
    columns.  A Q that is only semi-definite with sum_to_zero = 0 is accepted and improper along its null space: the likelihood has to
    identify that direction.  AR(p), a sampled CAR or Leroux autocorrelation, the BYM2 mixing parameter and hard constraints are out of
    scope.  The Model exposes G, gmrfs (a list of glm.Gmrf, None without), gmrf_term (int32 (G,)), gmrf_kappa (float64 (G,)) and the
    concatenated tables gmrf_start (int64), gmrf_col (int32), gmrf_val; Engine.glm_gmrfs() reads term, kappa and the entry counts back."""
    if isinstance(aux, bool) or not isinstance(aux, (int, np.integer)) or not 0 <= aux <= 4:
        raise ValueError("aux must be an integer in 0..4 (got %r)" % (aux,))
    A = int(aux)
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be a non-empty (n, D) matrix, got shape %s" % (X.shape,))
    n, Dd = X.shape
    flev, fidx = _glm.factor_terms(factors, n)
    fhas, fval = _glm.factor_values(factors, n)
    mwidth, midx, mval = _glm.factor_members(factors, n)
    if mwidth is not None:
        fhas = fval = None                                      # (every term's values are in the table of members)
    F = 0 if flev is None else flev.size
    Dx = Dd + (int(flev.sum()) if F else 0)
    grp, H = None, 0
    if groups is not None:
        grp = np.asarray(groups)
        if grp.ndim != 1 or grp.shape[0] != Dx:
            raise ValueError("groups must have one entry per column of %s (%d), got shape %s" % ("the model" if F else "X", Dx, grp.shape))
        if grp.dtype == np.bool_ or not np.issubdtype(grp.dtype, np.integer):
            raise ValueError("groups must be integers (-1: no group), got dtype %s" % grp.dtype)
        if grp.min() < -1:
            raise ValueError("a group id is -1 (no group) or 0 .. H-1, got %d" % grp.min())
        H = int(grp.max()) + 1
        if H > 4:
            raise ValueError("at most 4 groups (ids 0..3), got id %d" % (H - 1))
        for g in range(H):
            if not (grp == g).any():
                raise ValueError("group %d has no column (the ids in use must be 0 .. H-1)" % g)
        grp = np.ascontiguousarray(grp, dtype=np.int32)
        if H == 0:
            grp = None                                          # every column ungrouped: the model without groups
    loc, J, S = _glm.local_flags(local, slab_scale, Dx)
    pfirst, psecond, peta = _glm.pair_terms(correlated, flev)
    P = 0 if pfirst is None else pfirst.size
    bterm, beta = _glm.block_terms(correlated, flev)
    BK = 0 if bterm is None else bterm.size
    Bz = BK * (BK - 1) // 2
    if mwidth is not None:
        for what, terms in (("correlated: pair", () if pfirst is None else np.r_[pfirst, psecond]), ("correlated: block", () if bterm is None else bterm)):
            for t in terms:
                if mwidth[int(t)] > 1:
                    raise ValueError("%s names term %d, a glm.members term of width %d: a term with several levels per observation is in "
                                     "no pair and no block" % (what, int(t), int(mwidth[int(t)])))
    sterm, skind, seta = _glm.struct_terms(structured, flev, correlated, loc, Dd)
    NS = 0 if sterm is None else sterm.size
    Sz = 0 if sterm is None else int((skind == _glm.STRUCT_AR1).sum())
    D = Dx + A + H + J + P + Bz + Sz
    if D > 1024:
        raise ValueError("a GLM is limited to D <= 1024 (D = %d)" % D)
    if not np.isfinite(X).all():
        raise ValueError("X must be finite")
    Y = np.asarray(Y, dtype=np.float64)
    M, R = 1, None
    if chains_per_response is not None:
        if isinstance(chains_per_response, bool) or not isinstance(chains_per_response, (int, np.integer)) or chains_per_response < 1:
            raise ValueError("chains_per_response must be a positive integer (got %r)" % (chains_per_response,))
        R = int(chains_per_response)
        if Y.ndim == 2:
            raise ValueError("with chains_per_response Y must have shape (M, n, K); a 2-D Y of shape %s could be (M, n) or (n, K): add the "
                             "K axis (Y[:, :, None] for M responses of one column, Y[None] for one response)" % (Y.shape,))
        if Y.ndim != 3 or Y.shape[0] < 1 or Y.shape[1] != n or not 1 <= Y.shape[2] <= 4:
            raise ValueError("with chains_per_response Y must have shape (M, %d, K) with M >= 1 and 1 <= K <= 4, got %s" % (n, Y.shape))
        M = Y.shape[0]
    elif Y.ndim == 1:
        Y = Y[:, None]
    if R is None and (Y.ndim != 2 or Y.shape[0] != n or not 1 <= Y.shape[1] <= 4):
        raise ValueError("Y must have shape (%d,) or (%d, K) with 1 <= K <= 4, got %s" % (n, n, Y.shape))
    if not np.isfinite(Y).all():
        raise ValueError("Y must be finite")
    c = np.zeros(0) if constants is None else np.asarray(constants, dtype=np.float64).ravel()
    if c.size > 16:
        raise ValueError("at most 16 constants (got %d)" % c.size)
    if not np.isfinite(c).all():
        raise ValueError("the constants must be finite")
    if not isinstance(source, str) or not source.strip():
        raise ValueError("a GLM needs HIP source defining glm_observation")
    mu, tau = _prior(D, prior_mu, prior_tau)
    kind, nu = _glm.prior_kinds(prior_kind, prior_nu, D, Dx, tau)
    if P:
        _glm.pair_priors(peta, D - Sz, mu, tau, kind, nu)
    if BK:
        _glm.block_priors(beta, Bz, D - Sz, mu, tau, kind, nu)
    if Sz:
        _glm.struct_priors(skind, seta, D, mu, tau, kind, nu)
    gterm, gkappa, gstart, gcol, gval = _glm.gmrf_terms(gmrf, flev, correlated, structured, loc, Dd, mu, tau, kind, nu)
    NG = 0 if gterm is None else gterm.size
    priors = kind is not None and bool(kind.any())
    K = Y.shape[-1]
    if H > 0 or R is not None or priors or J > 0 or F > 0:
        # handed over in parts (Model.glm_model, idhmc_create_glm_model): the packed params are not stretched for the groups, the
        # responses, the priors, the local scales or the factors.  No params and X, Y kept as arrays is what Engine reads as "in parts"
        m = Model(MODEL_GLM_AUX if A else MODEL_GLM, D, mu=mu, tau=tau, source=source)
        m.X, m.Y, m.constants = np.ascontiguousarray(X), np.ascontiguousarray(Y), np.ascontiguousarray(c)
    elif A == 0:
        m = Model(MODEL_GLM, D, mu=mu, tau=tau, source=source,
                  params=np.concatenate([[float(K), float(c.size)], c, X.ravel(), Y.ravel()]))
    else:
        m = Model(MODEL_GLM_AUX, D, mu=mu, tau=tau, source=source,
                  params=np.concatenate([[float(K), float(c.size), float(A)], c, X.ravel(), Y.ravel()]))
    m.n, m.K, m.nc, m.Dx, m.A, m.H, m.groups = n, K, c.size, Dx, A, H, grp
    m.M, m.R = M, R
    m.prior_kind, m.prior_nu = kind, nu
    m.J, m.local, m.slab_scale = J, loc, S
    m.Dd, m.F, m.levels, m.factor_index = Dd, F, flev, fidx
    m.factor_has, m.factor_values = fhas, fval
    m.member_width, m.member_index, m.member_values = mwidth, midx, mval
    m.P, m.pair_first, m.pair_second, m.pair_eta = P, pfirst, psecond, peta
    m.pairs = [_glm.Pair(int(a), int(b), float(e)) for a, b, e in zip(pfirst, psecond, peta)] if P else None
    m.BK, m.Bz, m.block_term, m.block_eta = BK, Bz, bterm, beta
    m.block = _glm.Block(tuple(int(t) for t in bterm), beta) if BK else None
    m.S, m.Sz, m.struct_term, m.struct_kind, m.struct_eta = NS, Sz, sterm, skind, seta
    m.structs = [_glm.Structure(int(t), int(k), float(e)) for t, k, e in zip(sterm, skind, seta)] if NS else None
    m.G, m.gmrf_term, m.gmrf_kappa, m.gmrf_start, m.gmrf_col, m.gmrf_val = NG, gterm, gkappa, gstart, gcol, gval
    m.gmrfs = list(gmrf) if NG else None
    return m


def default_options(**kw):
    o = Options()
    _lib.load().idhmc_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError("idhmc_options has no field %r" % k)
        setattr(o, k, v)
    return o


class Engine:
    """All chains of one device (one context per device, include/idhmc.h)."""

    def __init__(self, model, nchains, options=None, seed=1, first_chain=0, device=0):
        lib = _lib.load()
        opt = options if options is not None else default_options()
        h = C.c_void_p()
        if model.kind in (MODEL_GLM, MODEL_GLM_AUX) and model.params is None:
            # a GLM handed over in parts (GLM() packs no params and keeps X and Y as arrays): the one entry for all of them
            gm = model.glm_model()
            check(lib.idhmc_create_glm_model(C.byref(h), device, int(nchains), first_chain, C.byref(gm), C.byref(opt), seed))
        else:
            desc = model.desc()
            check(lib.idhmc_create(C.byref(h), device, int(nchains), first_chain, C.byref(desc), C.byref(opt), seed))
        self._set(model, h, nchains, opt)

    def _set(self, model, handle, nchains, options):
        self.lib = _lib.load()
        self.model, self.opt = model, options
        self.C, self.D = int(nchains), model.D
        self.h = handle
        self._hook = None

    @classmethod
    def _adopt(cls, model, handle, nchains, options):
        """an Engine around a context made elsewhere (a test's direct call of a creation function); it owns the handle"""
        eng = object.__new__(cls)
        eng._set(model, handle, nchains, options)
        return eng

    def close(self):
        if getattr(self, "h", None):
            self.lib.idhmc_destroy(self.h)
            self.h = None

    __del__ = close

    # ---- state ------------------------------------------------------------------------------------
    def _get_mat(self, fn):
        out = np.empty((self.C, self.D))
        check(fn(self.h, _dp(out)))
        return out

    def _get_vec(self, fn):
        out = np.empty(self.C)
        check(fn(self.h, _dp(out)))
        return out

    def _mat(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (self.C, self.D):
            raise ValueError("expected shape (%d, %d), got %s" % (self.C, self.D, a.shape))
        return a

    def set_q(self, q):
        check(self.lib.idhmc_set_q(self.h, _dp(self._mat(q))))

    def set_p(self, p):
        check(self.lib.idhmc_set_p(self.h, _dp(self._mat(p))))

    def random_position(self):
        check(self.lib.idhmc_random_position(self.h))

    def set_minv(self, minv):
        minv = np.ascontiguousarray(minv, dtype=np.float64)
        if minv.shape == (self.D,):
            check(self.lib.idhmc_set_minv(self.h, _dp(minv), 0))
        else:
            check(self.lib.idhmc_set_minv(self.h, _dp(self._mat(minv)), 1))

    def set_eps(self, eps):
        if np.ndim(eps) == 0:
            check(self.lib.idhmc_set_eps(self.h, float(eps)))
        else:
            e = np.ascontiguousarray(eps, dtype=np.float64)
            if e.shape != (self.C,):
                raise ValueError("eps must be a scalar or have shape (%d,)" % self.C)
            check(self.lib.idhmc_set_eps_per_chain(self.h, _dp(e)))

    q = property(lambda s: s._get_mat(s.lib.idhmc_get_q))
    p = property(lambda s: s._get_mat(s.lib.idhmc_get_p))
    grad = property(lambda s: s._get_mat(s.lib.idhmc_get_grad))
    minv = property(lambda s: s._get_mat(s.lib.idhmc_get_minv))
    lq = property(lambda s: s._get_vec(s.lib.idhmc_get_lq))
    eps = property(lambda s: s._get_vec(s.lib.idhmc_get_eps))

    def logdensity(self):
        return self._get_vec(self.lib.idhmc_logdensity)

    def placement_info(self):
        """(probe rate in GB/s of the placement of the state arrays that was kept, candidates tried); (0.0, 1) when not probed"""
        g, n = C.c_double(0.0), C.c_int32(0)
        check(self.lib.idhmc_placement_info(self.h, C.byref(g), C.byref(n)))
        return float(g.value), int(n.value)

    def placement_cost(self):
        """what the placement search of idhmc_create cost: dict(create_ms, peak_transient_bytes, single_array_GBps, kind)"""
        ms, pk, sg, kd = C.c_double(0.0), C.c_int64(0), C.c_double(0.0), C.c_int32(0)
        check(self.lib.idhmc_placement_cost(self.h, C.byref(ms), C.byref(pk), C.byref(sg), C.byref(kd)))
        return {"create_ms": float(ms.value), "peak_transient_bytes": int(pk.value), "single_array_GBps": float(sg.value),
                "kind": {0: "separate allocations", 3: "separate allocations found by the pair walk"}[int(kd.value)]}

    def lanes_info(self):
        """(lanes of the dense single-step sweep in use, of them on different hardware queues)"""
        a, b = C.c_int32(0), C.c_int32(0)
        check(self.lib.idhmc_lanes_info(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def leapfrog_slice_info(self):
        """(stride of the single-step leapfrog's Infinity-Cache slice in GRAD_STORE mode, in GRAD_RECOMPUTE mode); 1: every chain"""
        a, b = C.c_int32(0), C.c_int32(0)
        check(self.lib.idhmc_leapfrog_slice_info(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def device_bytes(self):
        return int(self.lib.idhmc_device_bytes(self.h))

    def padded_dim(self):
        return int(self.lib.idhmc_padded_dim(self.h))

    def glm_form(self):
        """the NUTS kernel's gradient of a logistic regression or a GLM: 0 one chain per wavefront, 1 the fp64 matrix cores;
        -1 for every other model"""
        return int(self.lib.idhmc_glm_form(self.h))

    def glm_responses(self):
        """(M, chains_per_response) of a GLM with several responses (GLM(..., chains_per_response=R)); (1, 0) for every other model"""
        m, r = C.c_int64(0), C.c_int64(0)
        check(self.lib.idhmc_glm_responses(self.h, C.byref(m), C.byref(r)))
        return int(m.value), int(r.value)

    def glm_priors(self):
        """(kind, nu) of every sampled coordinate as the context holds them (GLM(..., prior_kind=, prior_nu=)); zeros for every other model"""
        kind, nu = np.zeros(self.D, np.int32), np.zeros(self.D)
        check(self.lib.idhmc_glm_priors_get(self.h, kind.ctypes.data_as(C.POINTER(C.c_int32)), _dp(nu)))
        return kind, nu

    def glm_local(self):
        """(local int32 (Dx,), slab_scale) as the context holds them (GLM(..., local=, slab_scale=)); (None, 0.0) for a model that is not a
        GLM handed over in parts, zeros and 0.0 for one without local scales"""
        Dx = getattr(self.model, "Dx", None)
        if Dx is None:
            return None, 0.0
        loc, S = np.zeros(Dx, np.int32), C.c_double(0.0)
        check(self.lib.idhmc_glm_local_get(self.h, loc.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(S)))
        return loc, float(S.value)

    def glm_factors(self):
        """(levels int32 (F,), index int32 (F, n)) as the context holds them (GLM(..., factors=)); (None, None) for every model without
        factor terms"""
        F = C.c_int32(0)
        check(self.lib.idhmc_glm_factors_get(self.h, C.byref(F), None, None))
        if F.value == 0:
            return None, None
        lev, idx = np.zeros(F.value, np.int32), np.zeros((F.value, self.model.n), np.int32)
        check(self.lib.idhmc_glm_factors_get(self.h, C.byref(F), lev.ctypes.data_as(C.POINTER(C.c_int32)), idx.ctypes.data_as(C.POINTER(C.c_int32))))
        return lev, idx

    def glm_factor_values(self):
        """(has int32 (F,), values float64 (F, n)) as the context holds them (glm.term(..., values=)); (None, None) for every model none
        of whose factor terms has values"""
        has = np.zeros(4, np.int32)
        check(self.lib.idhmc_glm_factor_values_get(self.h, has.ctypes.data_as(C.POINTER(C.c_int32)), None))
        if not has.any():
            return None, None
        F = C.c_int32(0)
        check(self.lib.idhmc_glm_factors_get(self.h, C.byref(F), None, None))
        val = np.zeros((F.value, self.model.n))
        check(self.lib.idhmc_glm_factor_values_get(self.h, has.ctypes.data_as(C.POINTER(C.c_int32)), _dp(val)))
        return has[:F.value].copy(), val

    def glm_members(self):
        """(width int32 (F,), index int32 (P, n), values float64 (P, n)) as the context holds them (glm.members, glm.bspline); a model
        without such a term reports its F terms as planes of width 1; (None, None, None) for every model without factor terms"""
        F = C.c_int32(0)
        check(self.lib.idhmc_glm_factors_get(self.h, C.byref(F), None, None))
        if F.value == 0:
            return None, None, None
        width = np.zeros(4, np.int32)
        check(self.lib.idhmc_glm_members_get(self.h, width.ctypes.data_as(C.POINTER(C.c_int32)), None, None))
        P = int(width[:F.value].sum())
        idx, val = np.zeros((P, self.model.n), np.int32), np.zeros((P, self.model.n))
        check(self.lib.idhmc_glm_members_get(self.h, width.ctypes.data_as(C.POINTER(C.c_int32)), idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(val)))
        return width[:F.value].copy(), idx, val

    def glm_block(self):
        """(terms int32 (K,), eta) of the correlation block as the context holds it (GLM(..., correlated=[glm.block(..)])); (None, None) for
        every model without a block"""
        K = C.c_int32(0)
        check(self.lib.idhmc_glm_block_get(self.h, C.byref(K), None, None))
        if K.value == 0:
            return None, None
        t, e = np.zeros(K.value, np.int32), C.c_double(0.0)
        check(self.lib.idhmc_glm_block_get(self.h, C.byref(K), t.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(e)))
        return t, e.value

    def glm_pairs(self):
        """(first int32 (P,), second int32 (P,), eta float64 (P,)) as the context holds them (GLM(..., correlated=)); (None, None, None) for
        every model without correlated pairs"""
        P = C.c_int32(0)
        check(self.lib.idhmc_glm_pairs_get(self.h, C.byref(P), None, None, None))
        if P.value == 0:
            return None, None, None
        a, b, e = np.zeros(P.value, np.int32), np.zeros(P.value, np.int32), np.zeros(P.value)
        ip = C.POINTER(C.c_int32)
        check(self.lib.idhmc_glm_pairs_get(self.h, C.byref(P), a.ctypes.data_as(ip), b.ctypes.data_as(ip), _dp(e)))
        return a, b, e

    def glm_structs(self):
        """(term int32 (S,), kind int32 (S,), eta float64 (S,)) as the context holds them (GLM(..., structured=)); (None, None, None) for
        every model without structured terms"""
        S = C.c_int32(0)
        check(self.lib.idhmc_glm_structs_get(self.h, C.byref(S), None, None, None))
        if S.value == 0:
            return None, None, None
        t, k, e = np.zeros(S.value, np.int32), np.zeros(S.value, np.int32), np.zeros(S.value)
        ip = C.POINTER(C.c_int32)
        check(self.lib.idhmc_glm_structs_get(self.h, C.byref(S), t.ctypes.data_as(ip), k.ctypes.data_as(ip), _dp(e)))
        return t, k, e

    def glm_gmrfs(self):
        """(term int32 (G,), kappa float64 (G,), nnz int64 (G,): the entries of each precision) as the context holds them
        (GLM(..., gmrf=)); (None, None, None) for every model without a GMRF term"""
        G = C.c_int32(0)
        check(self.lib.idhmc_glm_gmrfs_get(self.h, C.byref(G), None, None, None))
        if G.value == 0:
            return None, None, None
        t, k, z = np.zeros(G.value, np.int32), np.zeros(G.value), np.zeros(G.value, np.int64)
        check(self.lib.idhmc_glm_gmrfs_get(self.h, C.byref(G), t.ctypes.data_as(C.POINTER(C.c_int32)), _dp(k),
                                           z.ctypes.data_as(C.POINTER(C.c_int64))))
        return t, k, z

    def synchronize(self):
        check(self.lib.idhmc_synchronize(self.h))

    def set_stream(self, stream_ptr):
        check(self.lib.idhmc_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- hot path ----------------------------------------------------------------------------------
    def refresh_momentum(self, it):
        check(self.lib.idhmc_refresh_momentum(self.h, it))

    def set_leapfrog_grad_mode(self, mode):
        """GRAD_STORE (0) or GRAD_RECOMPUTE (1): see idhmc_options.leapfrog_grad_mode"""
        check(self.lib.idhmc_set_leapfrog_grad_mode(self.h, int(mode)))

    def leapfrog(self, eps=None, n_steps=1):
        if eps is None:
            check(self.lib.idhmc_leapfrog_own_eps(self.h, n_steps))
        else:
            check(self.lib.idhmc_leapfrog(self.h, float(eps), n_steps))

    def nuts_transition(self, it, flags=0, directions=None):
        if directions is not None:
            d = np.ascontiguousarray(directions, dtype=np.uint32)
            if d.shape != (self.C,):
                raise ValueError("directions must have shape (%d,)" % self.C)
            check(self.lib.idhmc_set_directions(self.h, d.ctypes.data_as(C.POINTER(C.c_uint32))))
            flags |= T_USE_DIRECTIONS
        check(self.lib.idhmc_nuts_transition(self.h, it, flags))

    def nuts_transitions(self, it, n, flags=0):
        """n transitions of every chain (numbers it .. it + n - 1) in one launch; same state as n nuts_transition calls (include/idhmc.h)"""
        check(self.lib.idhmc_nuts_transitions(self.h, int(it), int(n), int(flags)))

    def fused_launch_info(self):
        """(possible on this device, used by the library's drivers) -- include/idhmc.h"""
        a, b = C.c_int32(), C.c_int32()
        check(self.lib.idhmc_fused_launch_info(self.h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def poll_abort(self, lag=0):
        """abort code (0 / IDHMC_ERR_EPS_UNDERFLOW / IDHMC_ERR_HIP) raised up to the transition `lag` launches back (include/idhmc.h)"""
        code = C.c_int32()
        check(self.lib.idhmc_poll_abort(self.h, int(lag), C.byref(code)))
        return code.value

    def tree_stats(self):
        out = np.empty(self.C, dtype=TREE_STATS_DTYPE)
        check(self.lib.idhmc_get_tree_stats(self.h, out.ctypes.data))
        return out

    def total_steps(self):
        v = C.c_int64()
        check(self.lib.idhmc_total_steps(self.h, C.byref(v)))
        return v.value

    def debug_counters(self):
        out = np.zeros(32, dtype=np.uint64)
        check(self.lib.idhmc_debug_counters(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    # ---- adaptation --------------------------------------------------------------------------------
    def find_local_optimum(self, magnitude_penalty=1e-4, iterations=50):
        check(self.lib.idhmc_find_local_optimum(self.h, float(magnitude_penalty), int(iterations)))

    def find_initial_stepsize(self, per_chain_only=False):
        """per-chain searches; in global-eps mode followed by the pooled exp(mean log eps) unless per_chain_only"""
        check((self.lib.idhmc_find_initial_stepsize_per_chain if per_chain_only else self.lib.idhmc_find_initial_stepsize)(self.h))

    def da_init(self):
        check(self.lib.idhmc_da_init(self.h))

    def da_finalize(self):
        check(self.lib.idhmc_da_finalize(self.h))

    def accept_sum(self, dev_ptr):
        check(self.lib.idhmc_accept_sum(self.h, C.c_void_p(dev_ptr)))

    def logeps_sum(self, dev_ptr):
        check(self.lib.idhmc_logeps_sum(self.h, C.c_void_p(dev_ptr)))

    def set_eps_from_logeps(self, dev_ptr):
        check(self.lib.idhmc_set_eps_from_logeps(self.h, C.c_void_p(dev_ptr)))

    def da_adapt_global(self, dev_ptr):
        check(self.lib.idhmc_da_adapt_global(self.h, C.c_void_p(dev_ptr)))

    def set_allreduce_hook(self, fn, dev_ptr):
        """fn(dev_ptr) -> None must SUM-all-reduce the XCHG_DOUBLES doubles at dev_ptr across ranks."""
        if fn is None:
            self._hook = None
            check(self.lib.idhmc_set_allreduce_hook(self.h, C.cast(None, _lib.ALLREDUCE_FN), None, None))
            return

        def _cb(buf, user):
            try:
                fn(buf)
                return 0
            except Exception:  # an exception must not unwind through C
                import traceback
                traceback.print_exc()
                return 1
        self._hook = _lib.ALLREDUCE_FN(_cb)
        check(self.lib.idhmc_set_allreduce_hook(self.h, self._hook, None, C.c_void_p(dev_ptr)))

    # native RCCL communicator for the global-eps exchange (include/idhmc.h: idhmc_comm_*)
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        check(_lib.load().idhmc_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks, rank, unique_id):
        if len(unique_id) != 128:
            raise ValueError("unique id must be 128 bytes")
        check(self.lib.idhmc_comm_init(self.h, int(nranks), int(rank), C.c_char_p(bytes(unique_id))))

    def comm_destroy(self):
        check(self.lib.idhmc_comm_destroy(self.h))

    def comm_allreduce(self, dev_ptr, n=XCHG_DOUBLES):
        check(self.lib.idhmc_comm_allreduce(self.h, C.c_void_p(dev_ptr), int(n)))

    def comm_info(self):
        """(ranks, this rank, all-reduces enqueued) of the context's RCCL communicator; zeros without one"""
        nr, r, n = C.c_int32(), C.c_int32(), C.c_int64()
        check(self.lib.idhmc_comm_info(self.h, C.byref(nr), C.byref(r), C.byref(n)))
        return nr.value, r.value, n.value

    def metric_begin(self):
        check(self.lib.idhmc_metric_begin(self.h))

    def metric_update(self, lam):
        check(self.lib.idhmc_metric_update(self.h, float(lam)))

    def pool_partials(self, pass_, dev_ptr, seg_lo, seg_hi):
        """pooled metric by hand: per-segment partial sums of a pass into a device table (include/idhmc.h)"""
        check(self.lib.idhmc_pool_partials(self.h, int(pass_), C.c_void_p(dev_ptr), int(seg_lo), int(seg_hi)))

    def pool_consume(self, pass_, dev_ptr, nseg, lam):
        check(self.lib.idhmc_pool_consume(self.h, int(pass_), C.c_void_p(dev_ptr), int(nseg), float(lam)))

    def moments_reset(self):
        check(self.lib.idhmc_moments_reset(self.h))

    def moments(self):
        mean = np.empty((self.C, self.D))
        var = np.empty((self.C, self.D))
        cnt = np.empty(self.C, dtype=np.int64)
        check(self.lib.idhmc_get_moments(self.h, _dp(mean), _dp(var), cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        return mean, var, cnt

    # ---- diagnostics reduced on the device (reference src/diagnostics.jl:28-32, 61-101) --------------
    def diag_reset(self):
        """start (or restart) the device-side diagnostics; mcmc() then adds every draw"""
        check(self.lib.idhmc_diag_reset(self.h))

    def diag_counters(self):
        """the context's integer counters (include/idhmc.h); counters of several ranks add"""
        out = np.zeros(_lib.DIAG_COUNTERS, dtype=np.uint64)
        check(self.lib.idhmc_get_diag_counters(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def tree_summary(self, counters=None):
        """reference summarize_tree_statistics from the device counters (of this context, or summed ones)"""
        from .diagnostics import summary_from_counters
        return summary_from_counters(self.diag_counters() if counters is None else counters)

    def ebfmi(self):
        out = np.empty(self.C)
        check(self.lib.idhmc_get_ebfmi(self.h, _dp(out)))
        return out

    # ---- posterior summaries reduced on the device (include/idhmc.h) ----------------
    def summary_begin(self, chains_per_group=None, bins=128):
        """open a summary: mcmc() then reduces every draw on the device, pooled over groups of chains_per_group consecutive global chain
        ids (None: the chains of a response of a many-response GLM, all chains otherwise); bins interior histogram bins, 0 for none"""
        check(self.lib.idhmc_summary_begin(self.h, 0 if chains_per_group is None else int(chains_per_group), int(bins)))

    def summary_dims(self):
        g, cpg, d, b = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        check(self.lib.idhmc_summary_dims(self.h, C.byref(g), C.byref(cpg), C.byref(d), C.byref(b)))
        return g.value, cpg.value, d.value, b.value

    def summary_set_range(self, lo=None, hi=None, span=6.0):
        """the histogram's range: arrays [groups][D], or (both None) mean -+ span sd of what has been accumulated; zeroes the histogram"""
        if (lo is None) != (hi is None):
            raise ValueError("lo and hi must both be given or both be None")
        if lo is None:
            check(self.lib.idhmc_summary_set_range(self.h, None, None, float(span)))
            return
        try:
            groups, _, D, _ = self.summary_dims()
        except _lib.IdhmcError:
            groups, D = 1, np.size(lo)      # (no summary open: let the library refuse)
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        if lo.size != groups * D or hi.size != groups * D:
            raise ValueError("expected lo, hi of shape (%d, %d)" % (groups, D))
        check(self.lib.idhmc_summary_set_range(self.h, _dp(lo), _dp(hi), float(span)))

    def summary_add_draws(self, draws):
        """reduce host draws [cnt][nchains][D] (saved earlier, or a test's) through the staging buffers and the reduction kernel"""
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim != 3 or draws.shape[1:] != (self.C, self.D):
            raise ValueError("expected shape (cnt, %d, %d), got %s" % (self.C, self.D, draws.shape))
        check(self.lib.idhmc_summary_add_draws(self.h, _dp(draws), draws.shape[0]))

    def summary(self):
        from .diagnostics import PosteriorSummary
        groups, cpg, D, bins = self.summary_dims()
        f = {k: np.empty((groups, D)) for k in ("mean", "var", "min", "max", "lo", "hi", "inv_w")}
        n, binned = np.empty(groups, dtype=np.int64), np.empty(groups, dtype=np.int64)
        pos = np.empty((groups, D), dtype=np.int64)
        counts = np.zeros((groups, D, bins + 2), dtype=np.uint32) if bins > 0 else None
        ip = C.POINTER(C.c_int64)
        check(self.lib.idhmc_get_summary(self.h, n.ctypes.data_as(ip), binned.ctypes.data_as(ip), _dp(f["mean"]), _dp(f["var"]),
                                         _dp(f["min"]), _dp(f["max"]), pos.ctypes.data_as(ip), _dp(f["lo"]), _dp(f["hi"]), _dp(f["inv_w"]),
                                         counts.ctypes.data_as(C.POINTER(C.c_uint32)) if bins > 0 else None))
        return PosteriorSummary(chains_per_group=cpg, bins=bins, n=n, binned=binned, pos=pos, counts=counts, **f)

    def summary_end(self):
        check(self.lib.idhmc_summary_end(self.h))

    def mcmc_summary(self, N, iter0, pilot=None, chains_per_group=None, bins=128, span=6.0):
        """N transitions reduced on the device, nothing stored: begin, `pilot` transitions, the range from their moments, the other
        N - pilot, summary, end.  The pilot draws count in the moments, sign counts, min and max, not in the histogram.  The default
        pilot is the smallest count with pilot * chains_per_group >= 256, at least 2 and at most N // 2: a heuristic that nobody has
        measured -- a range from few values can put tail quantiles in an end bin (quantiles() warns)."""
        N = int(N)
        self.summary_begin(chains_per_group, bins)
        try:
            if bins > 0:
                if pilot is None:
                    cpg = self.summary_dims()[1]
                    pilot = min(max(2, -(-256 // cpg)), N // 2)
                pilot = int(pilot)
                if not 1 <= pilot < N:
                    raise ValueError("pilot = %d must be at least 1 and below N = %d" % (pilot, N))
                self.mcmc(pilot, iter0, store_draws=False, store_stats=False)
                self.summary_set_range(span=span)
                self.mcmc(N - pilot, iter0 + pilot, store_draws=False, store_stats=False)
            else:
                self.mcmc(N, iter0, store_draws=False, store_stats=False)
            return self.summary()
        finally:
            self.summary_end()

    # ---- drivers -----------------------------------------------------------------------------------
    def _bufs(self, N, store_draws, store_stats):
        draws = np.empty((N, self.C, self.D)) if store_draws else None
        stats = np.empty((N, self.C), dtype=TREE_STATS_DTYPE) if store_stats else None
        return draws, stats, (_dp(draws) if store_draws else None), (stats.ctypes.data if store_stats else None)

    def tuning_stage(self, N, adapt_metric, iter0, store_draws=False, store_stats=True):
        draws, stats, dpp, sp = self._bufs(N, store_draws, store_stats)
        check(self.lib.idhmc_tuning_stage(self.h, N, int(adapt_metric), iter0, dpp, sp))
        return draws, stats

    def mcmc(self, N, iter0, store_draws=True, store_stats=True):
        draws, stats, dpp, sp = self._bufs(N, store_draws, store_stats)
        check(self.lib.idhmc_mcmc(self.h, N, iter0, dpp, sp))
        return draws, stats

    def mcmc_with_warmup(self, N, store_draws=True, store_stats=True):
        draws, stats, dpp, sp = self._bufs(N, store_draws, store_stats)
        check(self.lib.idhmc_mcmc_with_warmup(self.h, N, dpp, sp))
        return draws, stats

    # ---- measurement -------------------------------------------------------------------------------
    def time_leapfrog(self, eps, sweeps):
        ms = C.c_float()
        check(self.lib.idhmc_time_leapfrog(self.h, float(eps), sweeps, C.byref(ms)))
        return ms.value

    def time_transitions(self, n, iter0):
        ms = C.c_float()
        check(self.lib.idhmc_time_transitions(self.h, n, iter0, C.byref(ms)))
        return ms.value

    def time_transitions_fused(self, n, iter0):
        """the same n transitions as one idhmc_nuts_transitions launch"""
        ms = C.c_float()
        check(self.lib.idhmc_time_transitions_fused(self.h, n, iter0, C.byref(ms)))
        return ms.value

    def time_eps_adapt(self, n):
        """n times what the drivers enqueue between two adapting transitions in EPS_GLOBAL (three launches) or EPS_PER_RESPONSE (one):
        milliseconds in all (include/idhmc.h); moves the stepsizes, call da_init first"""
        ms = C.c_float()
        check(self.lib.idhmc_time_eps_adapt(self.h, int(n), C.byref(ms)))
        return ms.value
