// idhmc_glm.hpp -- generalised linear models on a data matrix every chain shares, DESIGN sections 10 and 11:
//   l(q) = -sum_i v(z_i, y_i) - 1/2 sum_c tau_c (q_c - mu_c)^2,   z = X q,   v = -log p(y | z) up to a data-only term
//   grad l(q) = X' r - tau .* (q - mu),   r_i = d log p(y_i | z_i) / dz_i
// The observation is a policy type Obs: Obs::K data columns per observation (1..4) and
//   static void terms(double z, const GlmObs &o, double &r, double &v)
// Two forms with one arithmetic: GlmWave (one chain per wavefront, every kernel) and GlmCoop (the NUTS kernel at L <= 256:
// 16 chains per workgroup, both products on the fp64 matrix cores).  The built-in logistic regression
// (IDHMC_MODEL_LOGISTIC_REGRESSION) is Obs = LogisticObs, instantiated ahead of time (idhmc_logistic.hip); a user's GLM
// (IDHMC_MODEL_GLM) is Obs = its glm_observation, instantiated by hipRTC (idhmc_jit.hip).  Kept out of what the hipRTC build of a
// custom density includes.
//
// The arithmetic (both forms and the tests' C restatements follow it bit for bit):
//   z_i   = fma chain over columns c ascending of X[i][c] * q_c, from +0
//   (r_i, v_i) = Obs::terms(z_i, {y_i0 .. y_i,K-1; constants})
//     logistic: s_i = y_i ? -z_i : z_i;  e_i = dexp(-|s_i|)
//               v_i = (s_i > 0 ? s_i : 0) + dlog1p(e_i)                  = softplus(z_i) - y_i z_i
//               r_i = (y_i ? 1 : -1) * ((s_i >= 0 ? 1 : e_i) / (1 + e_i)) = y_i - sigma(z_i)
//   observations i >= n: v_i = r_i = 0 (the terms are computed, then overwritten: a NaN there does not leak)
//   G_c   = fma chain over observations i ascending of X[i][c] * r_i, from +0;  g_c = dfma(-tau_c, d_c, G_c), d = q - mu
//   lane partials (residues 2l, 2l+1 of 128): T = fma chain over chunks j of (tau_c d_c) * d_c;  A = sum over observation
//   blocks ascending of v_i (plain additions, from +0);  P = dfma(2, A, T);  l = -1/2 wave_sum(P0, P1)
// A chain of fmas from +0 never holds -0, so the zero padding (columns >= D, observations >= n) leaves every chain as it is:
// the per-wave form stops at D and n, the matrix-core form runs over the padded tiles, and both give the same bits.
//
// Device layout (DevState): X [n_pad][L] (lr_x), X' [L][n_pad] (lr_xt), Y as K planes [K][n_pad] per response (lr_y), all zero-padded;
// a GLM's constants in user_params (user_nparams of them).
//
// Auxiliary coordinates (IDHMC_MODEL_GLM_AUX): Obs::A of them (0 for the policies above, 1..4), the last A of the
// D sampled coordinates, q = [beta (Dx = D - A) | a (A)].  Every observation sees them, no product with X does:
//   static void terms(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)      s[j] = d log p / d a_j
//   z_i   = the fma chain over columns c < Dx;  (r_i, v_i, s_i0 ..) from one call, all overwritten with 0 for i >= n
//   S_j[rho], rho = i mod 128: plain additions over observation blocks ascending, from +0, as A[rho] accumulates v
//   G_{Dx+j} = the canonical 128-residue tree over S_j (wave_sum, lane l holding residues 2l, 2l + 1);  g = dfma(-tau, d, G) as above
//   T runs over all D coordinates (the prior covers a), P and l unchanged.
// X has Dx columns: its device tiles hold +0 in columns >= Dx like every padded column.
//
// Coefficient groups with a sampled scale (idhmc_create_glm): Obs::H of them (0 for the policies above, 1..4),
// q = [u (Dx) | a (A) | omega (H)], grp[c] in {-1, 0 .. H-1} for every coordinate (DevState::lr_grp; -1: not in a group, and every
// coordinate >= Dx).  Non-centred: the coefficient of column c is b_c = u_c exp(omega_grp[c]).
//   e_g   = dexp(omega_g), once per gradient, the same bits in every lane (omega_g read from its owner lane)
//   b_c   = grp[c] >= 0 ? u_c * e_grp[c] : u_c (a select over the groups);  z_i = the fma chain over columns c < Dx of X[i][c] * b_c
//   G_c, S_j, A[rho] as above;  w_c = G_c * b_c for grouped c;  W_g[rho], rho = c mod 128: plain additions over chunks ascending of the
//   members' w_c, from +0 (a non-member adds +0);  G_{Dx+A+g} = the canonical 128-residue tree over W_g;  then G_c <- G_c * e_grp[c]
//   g = dfma(-tau, d, G) with d = q - mu on the sampled coordinates, T over all D, P and l unchanged.
// The per-wave form stages b instead of q (coordinates >= Dx raw: a_j is still found there); in the matrix-core form the requester
// writes b as its Q row (+0 in every column >= Dx) before barrier A and applies the chain rule to the G row it reads after barrier
// C: nothing between the barriers changes, no LDS is added.
//
// Several responses on one design matrix (idhmc_create_glm_responses): Obs::kResponses, a compile-time flag of the
// policy (false for the policies above: none of their instructions changes).  Y is M sets of K planes, [M][K][n_pad], and the chain of GLOBAL id
// g samples response g / R (DevState::lr_r), whatever context or tile it runs in.  X, X', the prior, the constants and the groups are
// shared, and for one chain the operations are those of a single-response model on its Y: only the address of y_i differs.  A kernel
// binds the chain it takes (bind_chain, idhmc_internal.hpp) before it evaluates anything: the per-wave form offsets its pointer to
// Y; in the matrix-core form the 16 rows of a tile are 16 chains of any responses, so the requester publishes its offset in
// column L of its Q row (padding: zphase, gphase and both row accesses of the requester touch columns < L only) and the Z wavefronts
// read y per accumulator row instead of once per lane.  No LDS, no tile, no barrier is added.
//
// Priors beyond the Gaussian (idhmc_create_glm_priors): Obs::kPriors, a compile-time flag of the policy (false for the
// policies above and for every model whose kinds are all 0: none of their instructions changes).  Every coordinate c carries kind_c
// (DevState::lr_pkind) and nu_c (lr_pnu) next to mu_c and tau_c; d = q_c - mu_c, and the last loop of both forms becomes, per coordinate
// (glm_prior; plain operations in the association written, dfma where written):
//   0 NORMAL               T = dfma(tau d, d, T)                                        g = dfma(-tau, d, G)          (as above)
//   1 STUDENT_T            a = tau d; s = a d;   T = T + (nu + 1) dlog1p(s / nu)          g = G + (-((nu + 1) a) / (nu + s))
//   2 LOG_HALF_NORMAL      e = dexp(2 d);        T = T + (e - 2 d)                        g = G + (1 - e)
//   3 LOG_HALF_STUDENT_T   e = dexp(2 d);        T = T + ((nu + 1) dlog1p(e / nu) - 2 d)  g = G + (1 - ((nu + 1) e) / (nu + e))
//   4 LOG_EXPONENTIAL      e = dexp(d);          T = T + 2 (e - d)                        g = G + (1 - e)
// T is -2 log prior up to a constant; the log kinds are priors on exp(q_c) with scale exp(mu_c) and carry the Jacobian of exp.  The
// order of accumulation is unchanged (chunks ascending per lane component), padded coordinates are kind 0, and everything behind T
// is as above.  The two components of a lane, and neighbouring chunks, may be of different kinds: the kinds are branches of one
// function, evaluated after barrier C in the matrix-core form, with nothing of theirs alive across multiply().  No LDS is added.
// Each kind is finite wherever its log density is, and that ends at: kind 1, tau d^2 finite (|d| < 1.3e154 / sqrt(tau)); kinds 2
// and 3, 2 d < 709.78 (every more negative d is fine: e = 0 and T = -2 d); kind 4, d < 709.08 (2 exp(d) finite).  Past those ends T is +inf (g may be
// NaN), which the engine reads as l(q) = -inf: the ordinary rejected point.
//
// Per-coefficient local scales (idhmc_create_glm_local): Obs::kLocal, a compile-time flag of the policy (false for the
// policies above and for every model without a flagged column: none of their instructions changes).  local[c] in {0, 1} per column of
// X; the J flagged columns, ascending, get local coordinates k = 0 .. J-1 and q = [u (Dx) | a (A) | omega (H) | lambda (J)], lambda_k the
// LOGARITHM of the local scale of its column col(k).  inv2 = 1 / (S S) for a fixed slab scale S > 0 (DevState::lr_inv2; 0: no slab).
// DevState::lr_lpart holds the partner of every coordinate: for a flagged column its lambda, for a lambda its column, -1 elsewhere.
//   flagged column c, local coordinate k, id = grp[c]:
//     f = dexp(lambda_k);  s = id >= 0 ? e_id * f : f
//     no slab: st = s (h unused);  slab: i = 1 / s;  nn = dfma(i, i, inv2);  st = 1 / sqrt(nn);  h = 1 - inv2 / nn
//       (st = s / sqrt(1 + s^2 / S^2), h = d log st / d log s; s = inf gives st = S, h = 0; s = 0 gives st = 0, h = 1; with s below
//        about 1.5e-154 i i overflows and st is 0 where it should be s: an absolute error below 1.5e-154 |u| in b_c)
//     b_c = u_c * st
//   every other column: as above.  z, (r, v, s), G_c, S_j, A[rho] as above, over the columns < Dx.  Then, for a flagged column:
//     w_c = G_c * b_c;  wl_c = slab ? w_c * h : w_c;  G_{Dx+A+H+k} = wl_c (no reduction: one column feeds one coordinate);
//     W_id takes wl_c where it took w_c (grouped);  G_c <- G_c * st.
//   W_g into G_{Dx+A+g} by the canonical tree and the prior loop over all D coordinates are unchanged (lambda is a coordinate >= Dx:
//   the log kinds apply to it).
// A column and its lambda live in different lanes, chunks and components in general.  Both forms read the partner through the
// wavefront-private LDS vector they already have, written and read by the same wavefront in program order (no workgroup barrier):
// GlmWave through buf -- q is staged, b is computed ONCE per gradient and kept in registers across the observation blocks (staged
// again per block as before), and st, h are computed again from q after the loop, as GlmCoop does, rather than held (two more
// vectors of registers); GlmCoop through the requester's Q row -- q, then b in its place before barrier A; after barrier C the G
// row is taken into registers, then q, then wl go through the row.  Nothing of the local scales is alive across multiply().
//
// Factor terms by level index (idhmc_create_glm_factors): Obs::kFactors, a compile-time flag of the policy (false for
// the policies above and for every model with F = 0: none of their instructions changes).  F factors, 0 <= F <= 4; factor f has
// N_f >= 1 levels and an index lvl_f[i] in 0 .. N_f-1 per observation.  With Dd >= 1 dense columns the columns of the model are
//   c < Dd: dense, X[i][c] stored      off_f = Dd + N_0 + .. + N_{f-1}      c = off_f + k: level k of factor f, not stored
//   Dx = Dd + sum N_f,   q = [u (Dx) | a (A) | omega (H) | lambda (J)],   D = Dx + A + H + J <= 1024   (unchanged)
// and b_c is as above for every c < Dx (group scale, local scale).  The arithmetic:
//   z_i  = the dfma chain over c < Dd ascending of X[i][c] b_c from +0,  then  z_i = z_i + b[off_f + lvl_f[i]]  for f = 0 .. F-1
//          ascending (plain additions)
//   (r_i, v_i, s_ij) as above; i >= n overwritten with 0 as above; padded observations carry lvl = -1 and add nothing to z
//   G_c, c < Dd: as above.   G_{off_f + k} = plain additions, from +0, of r_i over the observations i < n with lvl_f[i] = k, i ascending
// Everything after G is untouched: auxiliary scores, group chain rule, local scales, prior loop, T, A[rho], P, l.
// For finite b and r this is bit for bit the arithmetic of the same model with every level written out as an indicator column of X
// (glm.expand_factors): adding +-0 changes nothing, because a chain from +0 never holds -0 (fma(0, b, z) = z, fma(0, r, G) = G), and
// fma(1, x, y) is y + x rounded once.  It ends at the non-finite: a non-finite b of one level poisons every z of the expanded model
// (0 * inf) and here only that level's observations; both are rejected points.  A level with no observation is allowed: its G is +0
// and the prior alone moves it.
// Device layout with factors: lr_x is [n_pad][Lx] and lr_xt [Lx][n_pad], Lx = 128 ceil(Dd / 128) (the row stride of X is a run-time
// member under kFactors and the compile-time L without); lr_fidx holds the index planes, int32 [F][n_pad], -1 in the padding; the level
// lists, built on the host: per block of 128 observations lr_fpos holds 128 F bytes -- the block's observations (position in the block)
// of factor 0 sorted by level, positions ascending within a level, then factor 1's, .. -- and lr_fstart [n_pad / 128][sum N_f + 1] where
// each level's list starts in them (cumulative over the factors: entry e and e + 1 bound the list of column Dd + e).  Every walk of a
// list is clamped on the device: at most 128 trips, positions inside the block's 128 F bytes, the byte read masked to 0 .. 127, so no list,
// whatever it held, reads outside the R tile or the wavefront's vector.
// GlmWave: the z loop runs c < Dd, then adds buf[off_f + lvl] for the lane's two observations (b is staged in buf; the planes are read
// as int2, lane-offset, like y2); the G loop touches the chunks j < Lx / 128 only; after it each lane adds buf[ii] over the lists of its
// factor columns into G.c[j] (r is staged in buf[0 .. 127]).  GlmCoop: the Z wavefronts run the matrix loop over the columns
// < 32 ceil(Dd / 32), then add Q[row][off_f + lvl_f[i]] per accumulator row (the requester writes b there); a G wavefront whose tile
// starts at or beyond Dd skips the matrix loop, and a tile that holds level columns adds R[b & 1][row][i] over the column's list per
// lane, after the block's matrix steps where the tile straddles Dd.  No LDS, no tile and no barrier is added; nothing of the factors
// is alive across multiply() in the requester.
//
// Factor terms that carry a value per observation (idhmc_create_glm_slopes): random slopes, (1 + x | subject).
// Obs::kSlopes, a compile-time flag of the policy next to kFactors (false for every policy above and for every model none of whose
// terms has values: none of their instructions changes).  A term f may carry w_f[i], a finite double per observation, next to its level
// index; its columns are still off_f .. off_f + N_f - 1 of the model and are never stored.  Two terms may share one index array:
// (1 | s) and (x | s) are two terms of N columns each.  The arithmetic:
//   z_i  = the dfma chain over c < Dd (as above), then for f = 0 .. F-1 ascending:
//            term without values:  z_i = z_i + b[off_f + lvl_f[i]]                 (as above)
//            term with values:     z_i = dfma(w_f[i], b[off_f + lvl_f[i]], z_i)
//   G_{off_f + k}, term with values = the dfma chain from +0 of dfma(w_f[i], r_i, G) over the observations i < n with lvl_f[i] = k,
//            i ascending.  An observation with w = 0.0 stays in its level's list: dfma(0, r, G) is performed, as the expanded model does.
// Everything after G is untouched.  For finite b, r and w this is bit for bit the same model on glm.expand_factors(X, factors), whose
// column off_f + k holds w_f[i] where lvl_f[i] = k and 0.0 elsewhere: fma(0, x, y) = y as long as y is not -0.  The one new edge next
// to the non-finite one: a chain from +0 now CAN reach -0, which it could not above -- fma(w, b, +0) with w b negative and below half
// the smallest subnormal rounds to -0, and the expanded model's next fma(0, x, -0) is +0 for x >= 0 where this one keeps -0.  Stated
// and not engineered around.
// Under kSlopes every term reads a value: a term without values has a plane of 1.0, and fma(1, b, z) is z + b rounded once, so its
// bits are the ones above.  Device layout: lr_fval [F][n_pad] holds w (1.0 for a plain term, 0.0 in the padding, where lvl = -1 adds
// nothing anyway); lr_fwl [n_pad / 128][128 F] holds the same values a second time in the order of lr_fpos, written by the counting
// sort that builds the lists, so that the value of list entry t has an address known before the entry's byte arrives -- no second
// dependent global load behind that byte.  t is clamped as glm_list_at clamps it and the 128-trip cap holds: a bad list still cannot read
// outside the block's entries.  GlmWave: next to the int2 level read, a double2 from the value plane at the same lane offset;
// zx = dfma(w.x, bx, zx); the gather does G = dfma(wl, r[ii], G) per list entry.  GlmCoop: zphase reads w once per observation i (it
// is the same for the four rows), acc[reg] = dfma(w, bl, acc[reg]); gphase gacc[reg] = dfma(wl, R[..][ii], gacc[reg]) per entry.  No
// LDS, tile or barrier is added; nothing of the values is alive across multiply() in the requester.
//
// Correlated random effects (idhmc_create_glm_corr): Obs::kCorr, a compile-time flag of the policy next to kSlopes
// (false for every policy above and for every model without a pair: none of their instructions changes).  P pairs of factor terms,
// 0 <= P <= 2; pair p is (first_p, second_p), two distinct terms of N_p levels each, a term in at most one pair, with values or
// without, on one index array or two; level k of the first is paired with level k of the second.  Each pair adds one sampled
// coordinate zeta_p = atanh rho_p at the end:  q = [u (Dx) | a (A) | omega (H) | lambda (J) | zeta (P)],  D = Dx + A + H + J + P <= 1024.
//   per gradient and pair, the same bits in every lane (zeta_p read from its owner lane, as glm_group_scale reads omega_g):
//     s = dexp(-|zeta|);  t = s s;  d = 1 + t;  rho = copysign((1 - t) / d, zeta);  c = (2 s) / d
//     (c = sqrt(1 - rho^2) in exact arithmetic; zeta = +0: rho = +0, c = 1; past |zeta| of about 745: rho = +-1, c = 0, finite)
//   forward, k < N_p, c1 = off_first + k, c2 = off_second + k:  ut_c1 = u_c1;  ut_c2 = dfma(rho, u_c1, c u_c2);  ut = u elsewhere.
//   Everything above runs on ut where it ran on u: b_c from group and local scales, z, (r, v, s), G_c, W_g, the lambdas, the scores.
//   backward, after the chain rules above have left Gh_c = dl / dut_c in the columns and filled omega, lambda, a:
//     m_k = Gh_c2 (c dfma(c, u_c1, -(rho u_c2)));   G_c1 = dfma(rho, Gh_c2, Gh_c1);   G_c2 = c Gh_c2
//     M_p[c2 mod 128]: plain additions over chunks ascending, from +0, of the pair's m_k (a non-member adds +0)
//     G_zeta_p = the canonical tree over M_p (wave_sum), placed like a group's
//   prior: the loop runs on the raw q (the prior of u is on u).  eta_p > 0 is LKJ(eta) on the 2 x 2 correlation with the Jacobian of
//   tanh, log p(zeta) = eta log(1 - rho^2); the device's kind table holds the internal kind 5 there and eta in nu's place:
//     T = T + (4 eta) ((|zeta| + dlog1p(t)) - ln 2);   g = dfma(-2 eta, rho, G)        (ln 2 rounded to a double)
//   eta_p = 0: the coordinate's entry of the prior arrays applies (kinds 0 and 1).  The branch is compiled under kCorr only.
// DevState::lr_cpart holds, per coordinate, -1 or  partner | pair << 10 | (second ? 2048 : 0)  for a paired column; lr_cp = P.  It is
// not lr_lpart: kLocal and kCorr are independent.  Both forms read the partner through the wavefront-private LDS vector they already
// have, written and read by one wavefront in program order (no workgroup barrier): GlmWave through buf, GlmCoop through the
// requester's Q row -- q, ut from it, then b in its place before barrier A; after barrier C the G row is taken into registers, rho, c
// and ut are computed again from q (as glm_local_chain computes st again), the chain rules of the scales run on ut, and then q and Gh
// go through the row for m_k and G_c1.  No LDS, tile or barrier is added; nothing of the pairs is alive across multiply().
//
// Structured terms (idhmc_create_glm_struct): Obs::kStruct, a compile-time flag of the policy next to kCorr (false
// for every policy above and for every model without a structure: none of their instructions changes).  S structured factor terms,
// 0 <= S <= 2 (slots 0 and 1); the levels of a structured term, in index order, are an AR(1) sequence with a sampled phi = tanh(zeta),
// or a first-order random walk (phi = c = 1, no coordinate).  The zetas of the AR(1) terms are the last Sz coordinates, behind the pairs':
//   q = [u (Dx) | a (A) | omega (H) | lambda (J) | zeta_pairs (P) | zeta_ar (Sz)],   D = Dx + A + H + J + P + Sz <= 1024.
//   (phi, c) of a slot: glm_corr_factors of its zeta, read from the owner lane, the same bits in every lane.
//   forward, o the term's first column, N its levels: x_0 = u_o, x_k = c u_{o+k}; p = phi, h = 1; while h < N: every k >= h takes
//     x_k = dfma(p, x_{k-h}, x_k) from the values before the stage, then p = p p, h = 2 h; ut_{o+k} = x_k, ut = u elsewhere -- the
//     Kogge-Stone form of ut_0 = u_0, ut_k = phi ut_{k-1} + c u_k, and the definition of the bits (not the sequential recurrence).
//   Everything above runs on ut where it ran on u.  A pair's mix and a term's scan touch disjoint columns (a term is in a pair or
//   structured, never both; a structured column has no local scale), so the scan runs on the mixed vector in place.
//   backward, after the chain rules above have left Gh_c = dl / dut_c: y_k = Gh_{o+k}; p = phi, h = 1; while h < N: every k with
//     k + h < N takes y_k = dfma(p, y_{k+h}, y_k), then p = p p, h = 2 h; lambda_k = y_k; G_{u_o} = lambda_0, G_{u_{o+k}} = c lambda_k;
//     AR(1): m_k = lambda_k (c dfma(c, ut_{o+k-1}, -(phi u_{o+k}))), k >= 1; M[(o+k) mod 128] plain additions over chunks ascending
//     from +0; G_zeta = the canonical tree over M (wave_sum), placed like a group's.  The prior of zeta is a pair's (kPriorLkj).
// DevState::lr_spart holds, per coordinate, -1 or  k | slot << 10  for level k of a structured term; lr_s = S, lr_sz = Sz, lr_sn the
// slots' levels, lr_skind their kinds, lr_scz their zeta coordinates (-1: a random walk).  Values stay in registers; the exchange
// between lanes is the wavefront-private LDS vector both forms already have (GlmWave: buf; GlmCoop: the requester's Q row, at the places
// the mix and its chain run), written and read by one wavefront in program order.  The two slots share the stage loop (a slot with
// N <= h has no level left to update).  No LDS, tile or barrier is added; nothing of the structures is alive across multiply().
#pragma once
#include "idhmc_device.hpp"

namespace idhmc {

// one observation as the policy's terms() sees it
struct GlmObs {
    double y[4];             // this observation's data columns, y[k] for k < K (the rest 0)
    const double *c;         // the model's constants, c[j] for j < nc (device memory)
    int K, nc;
    int A;                   // auxiliary coordinates the model samples (0: none)
};

// Coordinate c of a chain's vector lives in lane (c & 127) >> 1, chunk c >> 7, component c & 1.  Both helpers are selects over
// the chunks: c is not known at compile time, and a register array takes no run-time index.
// the lane's component that would be coordinate c (the value in the owner lane is the coordinate)
template <int NCH>
IDHMC_DEV double glm_coord(const Vec<NCH> &q, int c)
{
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) v = (c >> 7) == j ? ((c & 1) ? q.c[j].y : q.c[j].x) : v;
    return v;
}
// G is chunk j of the lane's vector: coordinate c of it becomes x
IDHMC_DEV void glm_place(double2 &G, int j, int c, int lane, double x)
{
    const bool here = (c >> 7) == j && lane == ((c & 127) >> 1);
    G.x = here && !(c & 1) ? x : G.x;
    G.y = here && (c & 1) ? x : G.y;
}
// one call of the observation policy: with auxiliary coordinates it takes a and returns the scores s as well
template <class Obs>
IDHMC_DEV void glm_terms(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)
{
    if constexpr (Obs::A > 0) Obs::terms(z, o, a, r, v, s);
    else Obs::terms(z, o, r, v);
}

// The groups' scales e_g = dexp(omega_g), g < H <= 4, are four doubles handed around by value (those past H unused): out of an array or
// a struct the compiler makes the select over the groups an indexed load, which costs every kernel scratch or LDS.
// omega_g is coordinate c0 + g of q: read from the lane that owns it, dexp of the same bits in every lane
template <int NCH>
IDHMC_DEV double glm_group_scale(const Vec<NCH> &q, int c)
{
    return dexp(read_lane(glm_coord<NCH>(q, c), (c & 127) >> 1));
}
template <int NCH, int H>
IDHMC_DEV void glm_group_scales(const Vec<NCH> &q, int c0, double &e0, double &e1, double &e2, double &e3)
{
    e0 = glm_group_scale<NCH>(q, c0);
    if constexpr (H > 1) e1 = glm_group_scale<NCH>(q, c0 + 1);
    if constexpr (H > 2) e2 = glm_group_scale<NCH>(q, c0 + 2);
    if constexpr (H > 3) e3 = glm_group_scale<NCH>(q, c0 + 3);
}
// b of one coordinate: u e_id for a member of group id (a select over the groups), u itself for id = -1
template <int H>
IDHMC_DEV double glm_scaled(double u, int id, double e0, double e1, double e2, double e3)
{
    double s = e0;
    if constexpr (H > 1) s = id == 1 ? e1 : s;
    if constexpr (H > 2) s = id == 2 ? e2 : s;
    if constexpr (H > 3) s = id == 3 ? e3 : s;
    return id >= 0 ? u * s : u;
}
// W_g += w of a member of group G (a non-member adds +0, which leaves a sum that started at +0 as it is)
template <int G>
IDHMC_DEV void glm_group_add(double2 &W, int2 id, double wx, double wy)
{
    W.x = W.x + (id.x == G ? wx : 0.0);
    W.y = W.y + (id.y == G ? wy : 0.0);
}
// the canonical tree over W_g, into coordinate c of the lane's G
template <int NCH>
IDHMC_DEV void glm_group_place(Vec<NCH> &G, double2 W, int c, int lane)
{
    const double S = wave_sum(W.x, W.y);
#pragma unroll
    for (int j = 0; j < NCH; ++j) glm_place(G.c[j], j, c, lane, S);
}
// the chain rule on the lane's G (complete but for the log scales' coordinates c0 .. c0 + H - 1): W_g into coordinate c0 + g,
// then G_c e_grp[c] for the members.  b is computed again from q, not kept.
template <int NCH, int H>
IDHMC_DEV void glm_group_chain(Vec<NCH> &G, const Vec<NCH> &q, const int2 *grp2, int c0, int lane, double e0, double e1, double e2, double e3)
{
    double2 W0 = make_double2(0.0, 0.0), W1 = W0, W2 = W0, W3 = W0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 id = grp2[j * 64];
        const double wx = G.c[j].x * glm_scaled<H>(q.c[j].x, id.x, e0, e1, e2, e3), wy = G.c[j].y * glm_scaled<H>(q.c[j].y, id.y, e0, e1, e2, e3);
        glm_group_add<0>(W0, id, wx, wy);
        if constexpr (H > 1) glm_group_add<1>(W1, id, wx, wy);
        if constexpr (H > 2) glm_group_add<2>(W2, id, wx, wy);
        if constexpr (H > 3) glm_group_add<3>(W3, id, wx, wy);
    }
    glm_group_place<NCH>(G, W0, c0, lane);
    if constexpr (H > 1) glm_group_place<NCH>(G, W1, c0 + 1, lane);
    if constexpr (H > 2) glm_group_place<NCH>(G, W2, c0 + 2, lane);
    if constexpr (H > 3) glm_group_place<NCH>(G, W3, c0 + 3, lane);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 id = grp2[j * 64];
        G.c[j].x = glm_scaled<H>(G.c[j].x, id.x, e0, e1, e2, e3);
        G.c[j].y = glm_scaled<H>(G.c[j].y, id.y, e0, e1, e2, e3);
    }
}

// Local scales (Obs::kLocal).  st and h of a flagged column: lam its lambda, id its group; inv2 = 0: no slab (st = s, h = 1 unused)
template <int H>
IDHMC_DEV void glm_local_scale(double lam, int id, double e0, double e1, double e2, double e3, double inv2, double &st, double &h)
{
    const double s = glm_scaled<H>(dexp(lam), id, e0, e1, e2, e3);
    st = s;
    h = 1.0;
    if (inv2 != 0.0) {
        const double i = 1.0 / s;
        const double nn = dfma(i, i, inv2);
        st = 1.0 / __builtin_sqrt(nn);
        h = 1.0 - inv2 / nn;
    }
}
// the group ids of chunk j (H = 0: none)
template <int H>
IDHMC_DEV int2 glm_ids(const int2 *grp2, int j)
{
    if constexpr (H > 0) return grp2[j * 64];
    else return make_int2(-1, -1);
}
// b of every coordinate of the lane: u st for a flagged column, as glm_scaled elsewhere (coordinates >= dx raw).  vec is the
// wavefront's own LDS vector (>= 128 NCH doubles, indexed by coordinate): q is staged there and each lane reads its columns' lambdas.
template <int NCH, int H>
IDHMC_DEV void glm_local_b(Vec<NCH> &b, const Vec<NCH> &q, const int2 *grp2, const int32_t *part, double *vec, int dx, int lane,
                           double e0, double e1, double e2, double e3, double inv2)
{
    constexpr int HN = H > 0 ? H : 1;
    double2 *v2 = reinterpret_cast<double2 *>(vec) + lane;
    const int2 *part2 = reinterpret_cast<const int2 *>(part) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = q.c[j];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c0 = 128 * j + 2 * lane;
        const int2 id = glm_ids<H>(grp2, j), p = part2[j * 64];
        const bool fx = p.x >= 0 && c0 < dx, fy = p.y >= 0 && c0 + 1 < dx;
        double sx, hx, sy, hy;
        glm_local_scale<HN>(vec[fx ? p.x : 0], id.x, e0, e1, e2, e3, inv2, sx, hx);
        glm_local_scale<HN>(vec[fy ? p.y : 0], id.y, e0, e1, e2, e3, inv2, sy, hy);
        b.c[j].x = fx ? q.c[j].x * sx : glm_scaled<HN>(q.c[j].x, id.x, e0, e1, e2, e3);
        b.c[j].y = fy ? q.c[j].y * sy : glm_scaled<HN>(q.c[j].y, id.y, e0, e1, e2, e3);
    }
}
// glm_group_chain with local scales: st, h and b again from q (staged in vec), wl_c to its lambda's coordinate through vec, W_g of
// the members' wl_c into coordinate c0 + g, G_c st for the flagged columns and G_c e_grp[c] for the other members
template <int NCH, int H>
IDHMC_DEV void glm_local_chain(Vec<NCH> &G, const Vec<NCH> &q, const int2 *grp2, const int32_t *part, double *vec, int dx, int c0g,
                               int lane, double e0, double e1, double e2, double e3, double inv2)
{
    constexpr int HN = H > 0 ? H : 1;
    double2 *v2 = reinterpret_cast<double2 *>(vec) + lane;
    const int2 *part2 = reinterpret_cast<const int2 *>(part) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = q.c[j];
    Vec<NCH> wl;
    double2 W0 = make_double2(0.0, 0.0), W1 = W0, W2 = W0, W3 = W0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c0 = 128 * j + 2 * lane;
        const int2 id = glm_ids<H>(grp2, j), p = part2[j * 64];
        const bool fx = p.x >= 0 && c0 < dx, fy = p.y >= 0 && c0 + 1 < dx;
        double sx, hx, sy, hy;
        glm_local_scale<HN>(vec[fx ? p.x : 0], id.x, e0, e1, e2, e3, inv2, sx, hx);
        glm_local_scale<HN>(vec[fy ? p.y : 0], id.y, e0, e1, e2, e3, inv2, sy, hy);
        const double bx = fx ? q.c[j].x * sx : glm_scaled<HN>(q.c[j].x, id.x, e0, e1, e2, e3);
        const double by = fy ? q.c[j].y * sy : glm_scaled<HN>(q.c[j].y, id.y, e0, e1, e2, e3);
        double wx = G.c[j].x * bx, wy = G.c[j].y * by;
        wx = fx && inv2 != 0.0 ? wx * hx : wx;
        wy = fy && inv2 != 0.0 ? wy * hy : wy;
        if constexpr (H > 0) glm_group_add<0>(W0, id, wx, wy);
        if constexpr (H > 1) glm_group_add<1>(W1, id, wx, wy);
        if constexpr (H > 2) glm_group_add<2>(W2, id, wx, wy);
        if constexpr (H > 3) glm_group_add<3>(W3, id, wx, wy);
        wl.c[j] = make_double2(wx, wy);
        G.c[j].x = fx ? G.c[j].x * sx : glm_scaled<HN>(G.c[j].x, id.x, e0, e1, e2, e3);
        G.c[j].y = fy ? G.c[j].y * sy : glm_scaled<HN>(G.c[j].y, id.y, e0, e1, e2, e3);
    }
    // every lambda has been read: wl takes q's place, and each lambda's lane reads its column's
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = wl.c[j];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c0 = 128 * j + 2 * lane;
        const int2 p = part2[j * 64];
        const bool lx = p.x >= 0 && c0 >= dx, ly = p.y >= 0 && c0 + 1 >= dx;
        const double tx = vec[lx ? p.x : 0], ty = vec[ly ? p.y : 0];
        G.c[j].x = lx ? tx : G.c[j].x;
        G.c[j].y = ly ? ty : G.c[j].y;
    }
    if constexpr (H > 0) glm_group_place<NCH>(G, W0, c0g, lane);
    if constexpr (H > 1) glm_group_place<NCH>(G, W1, c0g + 1, lane);
    if constexpr (H > 2) glm_group_place<NCH>(G, W2, c0g + 2, lane);
    if constexpr (H > 3) glm_group_place<NCH>(G, W3, c0g + 3, lane);
}

// The prior of one coordinate (the table of the header comment): kind and nu select the row, d = q_c - mu_c, G the likelihood's part
// of the gradient.  Adds the coordinate's -2 log prior to T and returns g_c.
IDHMC_DEV double glm_prior(int kind, double nu, double tau, double d, double G, double &T)
{
    if (kind == 0) {
        T = dfma(tau * d, d, T);
        return dfma(-tau, d, G);
    }
    if (kind == 1) {
        const double a = tau * d, s = a * d;
        T = T + (nu + 1.0) * dlog1p(s / nu);
        return G + (-((nu + 1.0) * a) / (nu + s));
    }
    if (kind == 4) {
        const double e = dexp(d);
        T = T + 2.0 * (e - d);
        return G + (1.0 - e);
    }
    const double e = dexp(2.0 * d);
    if (kind == 2) {
        T = T + (e - 2.0 * d);
        return G + (1.0 - e);
    }
    T = T + ((nu + 1.0) * dlog1p(e / nu) - 2.0 * d);
    return G + (1.0 - ((nu + 1.0) * e) / (nu + e));
}

// Correlated pairs (Obs::kCorr).  An entry of the partner table: -1, or partner | pair << 10 | (second ? 2048 : 0)
constexpr int kCorrSecond = 2048, kCorrPair = 1024, kCorrMask = 1023;
constexpr int kPriorLkj = 5;                         // the device table's mark of a zeta with eta > 0 (eta in nu's place); never a public kind
constexpr double kLn2 = 0.69314718055994530942;
// rho and c of the pair whose zeta is coordinate cz of q: read from its owner lane, the same bits in every lane
template <int NCH>
IDHMC_DEV void glm_corr_factors(const Vec<NCH> &q, int cz, double &rho, double &c)
{
    const double z = read_lane(glm_coord<NCH>(q, cz), (cz & 127) >> 1);
    const double s = dexp(-__builtin_fabs(z));
    const double t = s * s, d = 1.0 + t;
    rho = __builtin_copysign((1.0 - t) / d, z);
    c = (2.0 * s) / d;
}
template <int NCH>
IDHMC_DEV void glm_corr_pairs(const Vec<NCH> &q, int cz0, int np, double &r0, double &c0, double &r1, double &c1)
{
    glm_corr_factors<NCH>(q, cz0, r0, c0);
    r1 = 0.0;
    c1 = 1.0;
    if (np > 1) glm_corr_factors<NCH>(q, cz0 + 1, r1, c1);
}
// ut of every coordinate of the lane: dfma(rho, u_c1, c u_c2) for a second column, q itself elsewhere.  vec is the wavefront's own
// LDS vector (>= 128 NCH doubles, indexed by coordinate): q is staged there and each second column reads its first.
template <int NCH>
IDHMC_DEV void glm_corr_mix(Vec<NCH> &ut, const Vec<NCH> &q, const int32_t *cpart, double *vec, int lane, double r0, double c0, double r1, double c1)
{
    double2 *v2 = reinterpret_cast<double2 *>(vec) + lane;
    const int2 *part2 = reinterpret_cast<const int2 *>(cpart) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = q.c[j];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 p = part2[j * 64];
        const bool sx = p.x >= 0 && (p.x & kCorrSecond), sy = p.y >= 0 && (p.y & kCorrSecond);
        const double ux = vec[sx ? p.x & kCorrMask : 0], uy = vec[sy ? p.y & kCorrMask : 0];
        const double rx = (p.x & kCorrPair) ? r1 : r0, cx = (p.x & kCorrPair) ? c1 : c0;
        const double ry = (p.y & kCorrPair) ? r1 : r0, cy = (p.y & kCorrPair) ? c1 : c0;
        ut.c[j].x = sx ? dfma(rx, ux, cx * q.c[j].x) : q.c[j].x;
        ut.c[j].y = sy ? dfma(ry, uy, cy * q.c[j].y) : q.c[j].y;
    }
}
// the chain rule of the mix on the lane's G (Gh in the columns, complete elsewhere but for the zetas): m_k into M_p and by the tree
// into coordinate cz0 + p, G_c2 = c Gh_c2, and G_c1 = dfma(rho, Gh_c2, Gh_c1) with Gh_c2 read through vec once every u_c1 has been
template <int NCH>
IDHMC_DEV void glm_corr_chain(Vec<NCH> &G, const Vec<NCH> &q, const int32_t *cpart, double *vec, int cz0, int np, int lane,
                              double r0, double c0, double r1, double c1)
{
    double2 *v2 = reinterpret_cast<double2 *>(vec) + lane;
    const int2 *part2 = reinterpret_cast<const int2 *>(cpart) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = q.c[j];
    double2 M0 = make_double2(0.0, 0.0), M1 = M0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 p = part2[j * 64];
        const bool sx = p.x >= 0 && (p.x & kCorrSecond), sy = p.y >= 0 && (p.y & kCorrSecond);
        const bool px = (p.x & kCorrPair) != 0, py = (p.y & kCorrPair) != 0;
        const double ux = vec[sx ? p.x & kCorrMask : 0], uy = vec[sy ? p.y & kCorrMask : 0];
        const double rx = px ? r1 : r0, cx = px ? c1 : c0, ry = py ? r1 : r0, cy = py ? c1 : c0;
        const double mx = G.c[j].x * (cx * dfma(cx, ux, -(rx * q.c[j].x))), my = G.c[j].y * (cy * dfma(cy, uy, -(ry * q.c[j].y)));
        M0.x = M0.x + (sx && !px ? mx : 0.0);
        M0.y = M0.y + (sy && !py ? my : 0.0);
        M1.x = M1.x + (sx && px ? mx : 0.0);
        M1.y = M1.y + (sy && py ? my : 0.0);
    }
    // every u has been read: Gh takes q's place, and each first column's lane reads its second's
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = G.c[j];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 p = part2[j * 64];
        const bool ax = p.x >= 0, ay = p.y >= 0;
        const bool sx = ax && (p.x & kCorrSecond), sy = ay && (p.y & kCorrSecond);
        const double gx = vec[ax && !sx ? p.x & kCorrMask : 0], gy = vec[ay && !sy ? p.y & kCorrMask : 0];
        const double rx = (p.x & kCorrPair) ? r1 : r0, cx = (p.x & kCorrPair) ? c1 : c0;
        const double ry = (p.y & kCorrPair) ? r1 : r0, cy = (p.y & kCorrPair) ? c1 : c0;
        G.c[j].x = sx ? cx * G.c[j].x : ax ? dfma(rx, gx, G.c[j].x) : G.c[j].x;
        G.c[j].y = sy ? cy * G.c[j].y : ay ? dfma(ry, gy, G.c[j].y) : G.c[j].y;
    }
    glm_group_place<NCH>(G, M0, cz0, lane);
    if (np > 1) glm_group_place<NCH>(G, M1, cz0 + 1, lane);
}
// glm_prior with the LKJ row: d is zeta itself (its mu is 0), nu holds eta
IDHMC_DEV double glm_prior_corr(int kind, double nu, double tau, double d, double G, double &T)
{
    if (kind == kPriorLkj) {
        const double z = __builtin_fabs(d);
        const double s = dexp(-z);
        const double t = s * s;
        const double rho = __builtin_copysign((1.0 - t) / (1.0 + t), d);
        T = T + (4.0 * nu) * ((z + dlog1p(t)) - kLn2);
        return dfma(-2.0 * nu, rho, G);
    }
    return glm_prior(kind, nu, tau, d, G, T);
}
template <bool CORR>
IDHMC_DEV double glm_prior_of(int kind, double nu, double tau, double d, double G, double &T)
{
    if constexpr (CORR) return glm_prior_corr(kind, nu, tau, d, G, T);
    else return glm_prior(kind, nu, tau, d, G, T);
}
// a when B, else b: the vector the scales and the products run on
template <bool B, class T>
IDHMC_DEV const T &glm_pick(const T &a, const T &b)
{
    if constexpr (B) return a;
    else return b;
}

// Structured terms (Obs::kStruct).  An entry of the level table: -1, or k | slot << 10 for level k of the term in slot 0 or 1
constexpr int kStructSlot = 1024, kStructMask = 1023;
// what both forms take from DevState: the slots' levels (n1 = 0 with one slot) and zeta coordinates (-1: a random walk, phi = c = 1)
struct GlmStruct {
    const int32_t *spart;
    int n0, n1, cz0, cz1;
    template <class State>
    IDHMC_DEV void init(const State &s)
    {
        spart = s.lr_spart;
        n0 = s.lr_sn[0];
        n1 = s.lr_s > 1 ? s.lr_sn[1] : 0;
        cz0 = s.lr_scz[0];
        cz1 = s.lr_s > 1 ? s.lr_scz[1] : -1;
    }
};
// (phi, c) of the slots: glm_corr_factors of the slot's zeta, the constants (1, 1) for a random walk and for a slot that is not there
template <int NCH>
IDHMC_DEV void glm_struct_factors(const Vec<NCH> &q, const GlmStruct &st, double &f0, double &c0, double &f1, double &c1)
{
    f0 = c0 = f1 = c1 = 1.0;
    if (st.cz0 >= 0) glm_corr_factors<NCH>(q, st.cz0, f0, c0);
    if (st.cz1 >= 0) glm_corr_factors<NCH>(q, st.cz1, f1, c1);
}
// The forward scan, in place on ut (u in the structured columns on entry, whatever the caller has elsewhere): x_0 = u_o, x_k = c u_{o+k},
// then per stage h = 1, 2, 4, .. < N every k >= h takes dfma(p, x_{k-h}, x_k) from the values before the stage, p = phi^h by squaring.
// Values stay in registers; vec, the wavefront's own LDS vector (>= 128 NCH doubles, indexed by coordinate), is the exchange, written
// and read by this wavefront alone in program order.  Both slots share the stage loop: a slot with N <= h has no k >= h left.
template <int NCH>
IDHMC_DEV void glm_struct_scan(Vec<NCH> &ut, const GlmStruct &st, double *vec, int lane, double f0, double c0, double f1, double c1)
{
    double2 *v2 = reinterpret_cast<double2 *>(vec) + lane;
    const int2 *part2 = reinterpret_cast<const int2 *>(st.spart) + lane;
    int2 e[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        e[j] = part2[j * 64];
        const bool mx = e[j].x >= 0 && (e[j].x & kStructMask) >= 1, my = e[j].y >= 0 && (e[j].y & kStructMask) >= 1;
        ut.c[j].x = mx ? ((e[j].x & kStructSlot) ? c1 : c0) * ut.c[j].x : ut.c[j].x;
        ut.c[j].y = my ? ((e[j].y & kStructSlot) ? c1 : c0) * ut.c[j].y : ut.c[j].y;
    }
    const int nm = st.n0 > st.n1 ? st.n0 : st.n1;
    double p0 = f0, p1 = f1;
    for (int h = 1; h < nm; h <<= 1) {
#pragma unroll
        for (int j = 0; j < NCH; ++j) v2[j * 64] = ut.c[j];
        asm volatile("" ::: "memory");                        // (the stage's reads stay behind its writes, and ahead of the next stage's)
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c = 128 * j + 2 * lane;
            const bool ax = e[j].x >= 0 && (e[j].x & kStructMask) >= h, ay = e[j].y >= 0 && (e[j].y & kStructMask) >= h;
            const double nx = vec[ax ? c - h : 0], ny = vec[ay ? c + 1 - h : 0];
            ut.c[j].x = ax ? dfma((e[j].x & kStructSlot) ? p1 : p0, nx, ut.c[j].x) : ut.c[j].x;
            ut.c[j].y = ay ? dfma((e[j].y & kStructSlot) ? p1 : p0, ny, ut.c[j].y) : ut.c[j].y;
        }
        asm volatile("" ::: "memory");
        p0 = p0 * p0;
        p1 = p1 * p1;
    }
}
// The chain rule of the scan on the lane's G (Gh = dl / dut in the structured columns, complete elsewhere but for their zetas): the
// mirror-image scan y_k <- dfma(p, y_{k+h}, y_k) for k + h < N gives lambda; m_k = lambda_k (c dfma(c, ut_{k-1}, -(phi u_k))), k >= 1,
// into M_slot and by the tree into the slot's zeta; G_{u_o} = lambda_0, G_{u_{o+k}} = c lambda_k.  ut: the forward scan's result.
template <int NCH>
IDHMC_DEV void glm_struct_chain(Vec<NCH> &G, const Vec<NCH> &q, const Vec<NCH> &ut, const GlmStruct &st, double *vec, int lane,
                                double f0, double c0, double f1, double c1)
{
    double2 *v2 = reinterpret_cast<double2 *>(vec) + lane;
    const int2 *part2 = reinterpret_cast<const int2 *>(st.spart) + lane;
    int2 e[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) e[j] = part2[j * 64];
    const int nm = st.n0 > st.n1 ? st.n0 : st.n1;
    double p0 = f0, p1 = f1;
    for (int h = 1; h < nm; h <<= 1) {
#pragma unroll
        for (int j = 0; j < NCH; ++j) v2[j * 64] = G.c[j];
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int c = 128 * j + 2 * lane;
            const bool ax = e[j].x >= 0 && (e[j].x & kStructMask) + h < ((e[j].x & kStructSlot) ? st.n1 : st.n0);
            const bool ay = e[j].y >= 0 && (e[j].y & kStructMask) + h < ((e[j].y & kStructSlot) ? st.n1 : st.n0);
            const double nx = vec[ax ? c + h : 0], ny = vec[ay ? c + 1 + h : 0];
            G.c[j].x = ax ? dfma((e[j].x & kStructSlot) ? p1 : p0, nx, G.c[j].x) : G.c[j].x;
            G.c[j].y = ay ? dfma((e[j].y & kStructSlot) ? p1 : p0, ny, G.c[j].y) : G.c[j].y;
        }
        asm volatile("" ::: "memory");
        p0 = p0 * p0;
        p1 = p1 * p1;
    }
    // ut goes through the vector: level k reads ut of level k - 1
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = ut.c[j];
    asm volatile("" ::: "memory");
    double2 M0 = make_double2(0.0, 0.0), M1 = M0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = 128 * j + 2 * lane;
        const bool ax = e[j].x >= 0 && (e[j].x & kStructMask) >= 1, ay = e[j].y >= 0 && (e[j].y & kStructMask) >= 1;
        const bool sx = (e[j].x & kStructSlot) != 0, sy = (e[j].y & kStructSlot) != 0;
        const double ux = vec[ax ? c - 1 : 0], uy = vec[ay ? c : 0];
        const double fx = sx ? f1 : f0, cx = sx ? c1 : c0, fy = sy ? f1 : f0, cy = sy ? c1 : c0;
        const double mx = G.c[j].x * (cx * dfma(cx, ux, -(fx * q.c[j].x))), my = G.c[j].y * (cy * dfma(cy, uy, -(fy * q.c[j].y)));
        M0.x = M0.x + (ax && !sx ? mx : 0.0);
        M0.y = M0.y + (ay && !sy ? my : 0.0);
        M1.x = M1.x + (ax && sx ? mx : 0.0);
        M1.y = M1.y + (ay && sy ? my : 0.0);
        G.c[j].x = ax ? cx * G.c[j].x : G.c[j].x;
        G.c[j].y = ay ? cy * G.c[j].y : G.c[j].y;
    }
    asm volatile("" ::: "memory");
    if (st.cz0 >= 0) glm_group_place<NCH>(G, M0, st.cz0, lane);
    if (st.cz1 >= 0) glm_group_place<NCH>(G, M1, st.cz1, lane);
}

// Factor terms (Obs::kFactors): what both forms take from DevState
struct GlmFactors {
    const int32_t *idx, *start;      // lr_fidx [F][n_pad], lr_fstart [n_pad / 128][cols + 1]
    const unsigned char *pos;        // lr_fpos [n_pad / 128][128 F]
    int F, dd, lx, cols;             // factors, dense columns, row stride of X and rows of X', sum N_f
    int off[4];                      // off_f: the column of level 0 of factor f
    template <class State>
    IDHMC_DEV void init(const State &s)
    {
        idx = s.lr_fidx;
        start = s.lr_fstart;
        pos = s.lr_fpos;
        F = s.lr_f;
        dd = s.lr_dd;
        lx = s.lr_lx;
        cols = s.lr_fcols;
#pragma unroll
        for (int f = 0; f < 4; ++f) off[f] = s.lr_foff[f];
    }
};
// the list of level column dd + e in block b: entries s0 .. s0 + cnt - 1 of the block's bytes, cnt clamped to 0 .. 128 (has: the
// lane's column is a level column at all)
IDHMC_DEV void glm_list(const GlmFactors &f, int b, int e, bool has, int &s0, int &cnt)
{
    s0 = 0;
    cnt = 0;
    if (has) {
        const int32_t *st = f.start + (size_t)b * (size_t)(f.cols + 1) + e;
        s0 = st[0];
        cnt = st[1] - s0;
    }
    cnt = cnt > 128 ? 128 : cnt;
}
// entry t of block b's bytes (t clamped into them): an observation's place in the block, 0 .. 127
IDHMC_DEV int glm_list_at(const GlmFactors &f, int b, int t)
{
    const int last = 128 * f.F - 1;
    t = t < 0 ? 0 : t > last ? last : t;
    return f.pos[(size_t)b * (size_t)(128 * f.F) + t] & 127;
}
// G of one level column in the per-wave form: plain additions of the block's r (staged in r[0 .. 127]) over the column's list
IDHMC_DEV void glm_gather(double &G, const GlmFactors &f, int b, int e, bool has, const double *r)
{
    int s0, cnt;
    glm_list(f, b, e, has, s0, cnt);
    for (int k = 0; k < cnt; ++k) G = G + r[glm_list_at(f, b, s0 + k)];
}
// Values on factor terms (Obs::kSlopes): the value planes and the values in list order
struct GlmSlopes {
    const double *val, *wl;          // lr_fval [F][n_pad], lr_fwl [n_pad / 128][128 F]
    template <class State>
    IDHMC_DEV void init(const State &s)
    {
        val = s.lr_fval;
        wl = s.lr_fwl;
    }
};
// the value of entry t of block b (t clamped as glm_list_at clamps it): its address does not wait for the entry's byte
IDHMC_DEV double glm_list_value(const GlmSlopes &v, const GlmFactors &f, int b, int t)
{
    const int last = 128 * f.F - 1;
    t = t < 0 ? 0 : t > last ? last : t;
    return v.wl[(size_t)b * (size_t)(128 * f.F) + t];
}
// glm_gather for terms that read a value: the dfma chain of w r over the column's list
IDHMC_DEV void glm_gather(double &G, const GlmSlopes &v, const GlmFactors &f, int b, int e, bool has, const double *r)
{
    int s0, cnt;
    glm_list(f, b, e, has, s0, cnt);
    for (int k = 0; k < cnt; ++k) G = dfma(glm_list_value(v, f, b, s0 + k), r[glm_list_at(f, b, s0 + k)], G);
}

// v_i and r_i of one observation (y is 0 or 1)
IDHMC_DEV void logistic_terms(double z, double y, double &r, double &v)
{
    const double s = y != 0.0 ? -z : z;
    const double e = dexp(-__builtin_fabs(s));
    v = (s > 0.0 ? s : 0.0) + dlog1p(e);
    const double sg = (s >= 0.0 ? 1.0 : e) / (1.0 + e);
    r = y != 0.0 ? sg : -sg;
}

// Bernoulli with the logit link: IDHMC_MODEL_LOGISTIC_REGRESSION
struct LogisticObs {
    static constexpr int K = 1, A = 0, H = 0;
    static constexpr bool kResponses = false, kPriors = false, kLocal = false, kFactors = false, kSlopes = false, kCorr = false, kStruct = false;
    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v) { logistic_terms(z, o.y[0], r, v); }
};

// One chain per wavefront.  Observations in blocks of 128, lane l owning observations 128 b + 2 l, 128 b + 2 l + 1: z from
// coalesced rows of X' against q broadcast from the wavefront's LDS vector, then r is staged in that vector and g accumulates
// over the block's observations from coalesced rows of X.  X and X' stream from L2 once per gradient.
template <int NCH, class Obs>
struct GlmWave {
    static constexpr bool kHasParams = true;
    static constexpr bool kSeparable = false;
    static constexpr bool kCooperative = false;
    static constexpr bool kBindsChain = Obs::kResponses;
    static constexpr int AN = Obs::A > 0 ? Obs::A : 1;
    static constexpr int HN = Obs::H > 0 ? Obs::H : 1;
    const double *x, *xt;    // [npad][L], [L][npad], device
    const double2 *y2;       // [K][npad], lane-offset (Obs::kResponses: of the bound chain's response)
    const double2 *mu2, *tau2;   // lane-offset, device
    const double *cst;       // the constants, device
    const int2 *grp2;        // the group ids, lane-offset, device (Obs::H > 0)
    const int2 *kind2;       // the priors' kinds and their nu, lane-offset, device (Obs::kPriors)
    const double2 *nu2;
    const int32_t *part;     // the partner of every coordinate, device (Obs::kLocal)
    double inv2;             // 1 / slab_scale^2, 0 without a slab (Obs::kLocal)
    GlmFactors fac;          // the factor terms (Obs::kFactors)
    GlmSlopes slo;           // their values (Obs::kSlopes)
    const int32_t *cpart;    // the partner table of the paired columns, device (Obs::kCorr)
    int cz0, ncp;            // the coordinate of zeta_0 and the pairs (Obs::kCorr)
    GlmStruct stc;           // the structured terms (Obs::kStruct)
    double *buf;             // this wavefront's LDS vector, L doubles
    int D, n, npad, nc, lane;    // D: the columns of X (then Obs::A auxiliary coordinates, Obs::H log scales, the log local scales)
    template <class State>
    IDHMC_DEV void init(const State &s, double *lds_vec, int lane_)
    {
        x = s.lr_x;
        xt = s.lr_xt;
        y2 = reinterpret_cast<const double2 *>(s.lr_y) + lane_;
        mu2 = reinterpret_cast<const double2 *>(s.mu) + lane_;
        tau2 = reinterpret_cast<const double2 *>(s.tau) + lane_;
        cst = s.user_params;
        if constexpr (Obs::H > 0) grp2 = reinterpret_cast<const int2 *>(s.lr_grp) + lane_;
        if constexpr (Obs::kPriors) {
            kind2 = reinterpret_cast<const int2 *>(s.lr_pkind) + lane_;
            nu2 = reinterpret_cast<const double2 *>(s.lr_pnu) + lane_;
        }
        buf = lds_vec;
        D = s.D - Obs::A - Obs::H;
        if constexpr (Obs::kLocal) {
            part = s.lr_lpart;
            inv2 = s.lr_inv2;
            D -= s.lr_j;
        }
        if constexpr (Obs::kFactors) fac.init(s);
        if constexpr (Obs::kSlopes) slo.init(s);
        if constexpr (Obs::kCorr) {
            cpart = s.lr_cpart;
            ncp = s.lr_cp;
            cz0 = s.D - s.lr_cp;
            D -= s.lr_cp;
        }
        if constexpr (Obs::kStruct) {
            stc.init(s);
            D -= s.lr_sz;
            if constexpr (Obs::kCorr) cz0 -= s.lr_sz;          // (the pairs' zetas come first)
        }
        n = s.lr_n;
        npad = s.lr_npad;
        nc = (int)s.user_nparams;
        lane = lane_;
    }
    // Obs::kResponses: the chain of global id gc is evaluated next
    template <class State>
    IDHMC_DEV void bind_chain(const State &s, uint32_t gc)
    {
        const uint32_t resp = gc / s.lr_r;
        y2 = reinterpret_cast<const double2 *>(s.lr_y) + lane + (size_t)resp * (size_t)(Obs::K * (npad >> 1));
    }
    IDHMC_DEV double grad(const Vec<NCH> &q, Vec<NCH> &g) const
    {
        constexpr int L = 128 * NCH;
        Vec<NCH> G = vfill<NCH>(0.0);
        double a0 = 0.0, a1 = 0.0;
        double s0[AN], s1[AN];                                 // lane partials of the auxiliary scores, next to a0 / a1
        if constexpr (Obs::A > 0) {
#pragma unroll
            for (int j = 0; j < AN; ++j) s0[j] = s1[j] = 0.0;
        }
        double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;         // the groups' scales
        if constexpr (Obs::H > 0) glm_group_scales<NCH, HN>(q, D + Obs::A, e0, e1, e2, e3);
        double cr0 = 0.0, cc0 = 1.0, cr1 = 0.0, cc1 = 1.0;     // Obs::kCorr: rho and c of the pairs
        Vec<NCH> qm;                                           // and ut in the columns, q elsewhere
        if constexpr (Obs::kCorr) {
            glm_corr_pairs<NCH>(q, cz0, ncp, cr0, cc0, cr1, cc1);
            glm_corr_mix<NCH>(qm, q, cpart, buf, lane, cr0, cc0, cr1, cc1);
        }
        double sf0 = 1.0, sc0 = 1.0, sf1 = 1.0, sc1 = 1.0;     // Obs::kStruct: phi and c of the slots; the scan runs on qm, after the mix
        if constexpr (Obs::kStruct) {                          // (disjoint columns)
            if constexpr (!Obs::kCorr) qm = q;
            glm_struct_factors<NCH>(q, stc, sf0, sc0, sf1, sc1);
            glm_struct_scan<NCH>(qm, stc, buf, lane, sf0, sc0, sf1, sc1);
        }
        const Vec<NCH> &u = glm_pick<Obs::kCorr || Obs::kStruct>(qm, q);       // what the scales and the products run on
        Vec<NCH> bq;                                           // Obs::kLocal: b, once per gradient
        if constexpr (Obs::kLocal) glm_local_b<NCH, Obs::H>(bq, u, grp2, part, buf, D, lane, e0, e1, e2, e3, inv2);
        double2 *b2 = reinterpret_cast<double2 *>(buf) + lane;
        const int nb = npad >> 7;
        for (int b = 0; b < nb; ++b) {
            // q is staged again every block: r overwrites the first 128 doubles of the vector
            // (with groups b = u e is staged, computed again per block rather than kept: ids -1 past the columns of X leave a raw)
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                if constexpr (Obs::kLocal) {
                    b2[j * 64] = bq.c[j];
                } else if constexpr (Obs::H > 0) {
                    const int2 id = grp2[j * 64];
                    b2[j * 64] = make_double2(glm_scaled<HN>(u.c[j].x, id.x, e0, e1, e2, e3), glm_scaled<HN>(u.c[j].y, id.y, e0, e1, e2, e3));
                } else {
                    b2[j * 64] = u.c[j];
                }
            }
            const double2 *xtp = reinterpret_cast<const double2 *>(xt + 128 * b) + lane;
            double zx = 0.0, zy = 0.0;
            int dz = D;                                        // the stored columns
            if constexpr (Obs::kFactors) dz = fac.dd;
#pragma unroll 4
            for (int c = 0; c < dz; ++c) {
                const double qc = buf[c];                      // LDS broadcast
                const double2 xv = xtp[(size_t)c * (npad / 2)];
                zx = dfma(xv.x, qc, zx);
                zy = dfma(xv.y, qc, zy);
            }
            if constexpr (Obs::kFactors) {
                // the level columns: b of the observation's level, factors ascending (lvl = -1, the padding, adds nothing)
                const int2 *lv2 = reinterpret_cast<const int2 *>(fac.idx) + lane + b * 64;
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    if (f < fac.F) {
                        const int2 lv = lv2[(size_t)f * (npad >> 1)];
                        const double bx = buf[fac.off[f] + (lv.x > 0 ? lv.x : 0)], by = buf[fac.off[f] + (lv.y > 0 ? lv.y : 0)];
                        if constexpr (Obs::kSlopes) {
                            // the term's value plane at the same lane offset (1.0 for a term without values)
                            const double2 w = (reinterpret_cast<const double2 *>(slo.val) + lane + b * 64)[(size_t)f * (npad >> 1)];
                            zx = lv.x >= 0 ? dfma(w.x, bx, zx) : zx;
                            zy = lv.y >= 0 ? dfma(w.y, by, zy) : zy;
                        } else {
                            zx = lv.x >= 0 ? zx + bx : zx;
                            zy = lv.y >= 0 ? zy + by : zy;
                        }
                    }
                }
            }
            // the K planes of Y (written out: a loop over the planes costs the logistic kernels their register assignment)
            const double2 p0 = y2[b * 64];
            const double2 p1 = Obs::K > 1 ? y2[(npad >> 1) + b * 64] : make_double2(0.0, 0.0);
            const double2 p2 = Obs::K > 2 ? y2[2 * (npad >> 1) + b * 64] : make_double2(0.0, 0.0);
            const double2 p3 = Obs::K > 3 ? y2[3 * (npad >> 1) + b * 64] : make_double2(0.0, 0.0);
            const GlmObs ox{{p0.x, p1.x, p2.x, p3.x}, cst, Obs::K, nc, Obs::A}, oy{{p0.y, p1.y, p2.y, p3.y}, cst, Obs::K, nc, Obs::A};
            const int i0 = 128 * b + 2 * lane;
            double rx, vx, ry, vy;
            double av[AN], ux[AN], uy[AN];
            if constexpr (Obs::A > 0) {
#pragma unroll
                for (int j = 0; j < AN; ++j) av[j] = buf[D + j];   // LDS broadcast: q is still staged
            }
            glm_terms<Obs>(zx, ox, av, rx, vx, ux);
            glm_terms<Obs>(zy, oy, av, ry, vy, uy);
            if (i0 >= n) { rx = 0.0; vx = 0.0; }
            if (i0 + 1 >= n) { ry = 0.0; vy = 0.0; }
            a0 = a0 + vx;
            a1 = a1 + vy;
            if constexpr (Obs::A > 0) {
#pragma unroll
                for (int j = 0; j < AN; ++j) {
                    s0[j] = s0[j] + (i0 >= n ? 0.0 : ux[j]);
                    s1[j] = s1[j] + (i0 + 1 >= n ? 0.0 : uy[j]);
                }
            }
            b2[0] = make_double2(rx, ry);
            const int m = n - 128 * b < 128 ? n - 128 * b : 128;
            if constexpr (Obs::kFactors) {
                // rows of Lx doubles: the chunks that hold a stored column, then each level column's list
                const double2 *xr = reinterpret_cast<const double2 *>(x + (size_t)128 * b * fac.lx) + lane;
                const int nchx = fac.lx >> 7, xs = fac.lx >> 1;
#pragma unroll 2
                for (int ii = 0; ii < m; ++ii) {
                    const double ri = buf[ii];                 // LDS broadcast
#pragma unroll
                    for (int j = 0; j < NCH; ++j) {
                        if (j < nchx) {
                            const double2 xv = xr[(size_t)ii * xs + j * 64];
                            G.c[j].x = dfma(xv.x, ri, G.c[j].x);
                            G.c[j].y = dfma(xv.y, ri, G.c[j].y);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    if (128 * j + 128 > fac.dd && 128 * j < D) {               // the chunk holds a level column
                        const int c0 = 128 * j + 2 * lane, e = c0 - fac.dd;
                        if constexpr (Obs::kSlopes) {
                            glm_gather(G.c[j].x, slo, fac, b, e, e >= 0 && c0 < D, buf);
                            glm_gather(G.c[j].y, slo, fac, b, e + 1, e + 1 >= 0 && c0 + 1 < D, buf);
                        } else {
                            glm_gather(G.c[j].x, fac, b, e, e >= 0 && c0 < D, buf);
                            glm_gather(G.c[j].y, fac, b, e + 1, e + 1 >= 0 && c0 + 1 < D, buf);
                        }
                    }
                }
            } else {
                const double2 *xr = reinterpret_cast<const double2 *>(x + (size_t)128 * b * L) + lane;
#pragma unroll 2
                for (int ii = 0; ii < m; ++ii) {
                    const double ri = buf[ii];                 // LDS broadcast
#pragma unroll
                    for (int j = 0; j < NCH; ++j) {
                        const double2 xv = xr[(size_t)ii * (L / 2) + j * 64];
                        G.c[j].x = dfma(xv.x, ri, G.c[j].x);
                        G.c[j].y = dfma(xv.y, ri, G.c[j].y);
                    }
                }
            }
        }
        if constexpr (Obs::A > 0) {
            // G of an auxiliary coordinate: the tree over its 128 residues, into the lane that owns the coordinate
#pragma unroll
            for (int jx = 0; jx < AN; ++jx) {
                const double S = wave_sum(s0[jx], s1[jx]);
#pragma unroll
                for (int j = 0; j < NCH; ++j) glm_place(G.c[j], j, D + jx, lane, S);
            }
        }
        // (with local scales b was held across the blocks, not ut: it is mixed again from q)
        if constexpr (Obs::kCorr && Obs::kLocal) glm_corr_mix<NCH>(qm, q, cpart, buf, lane, cr0, cc0, cr1, cc1);
        if constexpr (Obs::kStruct && Obs::kLocal) {
            if constexpr (!Obs::kCorr) qm = q;
            glm_struct_scan<NCH>(qm, stc, buf, lane, sf0, sc0, sf1, sc1);
        }
        if constexpr (Obs::kLocal) glm_local_chain<NCH, Obs::H>(G, u, grp2, part, buf, D, D + Obs::A, lane, e0, e1, e2, e3, inv2);
        else if constexpr (Obs::H > 0) glm_group_chain<NCH, HN>(G, u, grp2, D + Obs::A, lane, e0, e1, e2, e3);
        if constexpr (Obs::kCorr) glm_corr_chain<NCH>(G, q, cpart, buf, cz0, ncp, lane, cr0, cc0, cr1, cc1);
        if constexpr (Obs::kStruct) glm_struct_chain<NCH>(G, q, u, stc, buf, lane, sf0, sc0, sf1, sc1);
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const double2 m = mu2[j * 64], t = tau2[j * 64];
            const double dx = q.c[j].x - m.x, dy = q.c[j].y - m.y;
            if constexpr (Obs::kPriors) {
                const int2 k = kind2[j * 64];
                const double2 nu = nu2[j * 64];
                g.c[j].x = glm_prior_of<Obs::kCorr || Obs::kStruct>(k.x, nu.x, t.x, dx, G.c[j].x, t0);
                g.c[j].y = glm_prior_of<Obs::kCorr || Obs::kStruct>(k.y, nu.y, t.y, dy, G.c[j].y, t1);
            } else {
                t0 = dfma(t.x * dx, dx, t0);
                t1 = dfma(t.y * dy, dy, t1);
                g.c[j] = make_double2(dfma(-t.x, dx, G.c[j].x), dfma(-t.y, dy, G.c[j].y));
            }
        }
        const double lq = -0.5 * wave_sum(dfma(2.0, a0, t0), dfma(2.0, a1, t1));
        return dfinite(lq) ? lq : -kInf;
    }
};

// The same density for the NUTS kernel at L <= 256, evaluated COOPERATIVELY by the 16 wavefronts of a workgroup on the fp64
// matrix cores, one 16-chain v_mfma_f64_16x16x4_f64 tile (the round protocol is DenseMvnCoop's, CoopRounds).  A round:
//   (1) the requester writes q as its row of the [16][L + 2] Q tile;                                      -- barrier A --
//   (2) per block b of 128 observations: the Z wavefronts (the last 8, one 16-observation column tile each) form
//       Z = Q X'[:, block] (k = columns ascending), apply the observation's terms, r into R tile b & 1 and v into registers;
//   (3) the G wavefronts (the first L / 16, one 16-column tile of X each) accumulate G += R[b & 1] X[block, :] (k =
//       observations ascending, the accumulators carried across blocks);
//       Z of block b + 1 runs between the same barriers as G of block b (two R tiles): one barrier per block;
//   (4) G goes into the Q tile, the per-residue sums of v into the free R tile;                            -- barrier C --
//   (5) the requester reads its row of each: g = dfma(-tau, d, G), P = dfma(2, A, T).
// X' and X stream through L1 once per 16 gradients instead of once per gradient.  LDS: 16 (L + 2) + 2 * 16 * 130 doubles,
// 49.9 KB at L = 128, 66.3 KB at L = 256.
// Auxiliary coordinates (Obs::A > 0): A further [16][129] planes, one per coordinate.  (1) the requester writes +0 into the
// auxiliary columns of its Q row (they take no part in Z) and a_j into the padding column 128 of its row of plane j, which
// nothing else writes; (2) the Z wavefronts read a of the chain behind each accumulator row from there and add the scores into
// columns 0..127 of the planes, each (chain, residue) slot owned by one lane of one Z wavefront across the blocks (block 0 stores
// 0 + s: the sum starts from +0) -- in LDS, not in registers: the kernel has 128 registers per lane and 4 A accumulators more
// would spill; (5) the requester reduces its row of each with wave_sum.  16.5 KB per auxiliary coordinate; which (L, A, metric) fit a CU is glm_coop's table (idhmc_logistic.hip).
template <int NCH, class Obs>
struct GlmCoop : CoopRounds<GlmCoop<NCH, Obs>> {
    static constexpr bool kHasParams = true;
    static constexpr bool kSeparable = false;
    static constexpr bool kCooperative = true;
    static constexpr bool kBindsChain = Obs::kResponses;
    static constexpr int L = 128 * NCH, DS = L + 2, RS = 130, KB = L / 4;
    static constexpr int kZT = 8, kGT = L / 16;        // Z column tiles per block (wavefronts 8..15), G column tiles (0..L/16-1)
    static constexpr int kQ = 0, kR = 16 * DS;         // Q / G tile, then the two R tiles
    static constexpr int AN = Obs::A > 0 ? Obs::A : 1;
    static constexpr int HN = Obs::H > 0 ? Obs::H : 1;
    static constexpr int kS = kR + 2 * 16 * RS;        // then the Obs::A score planes, [16][PS]: 128 residues and the slot of a_j
    static constexpr int PS = 129;                     // (one padding column, not RS's two: the 1 KB saved decides two rows of glm_coop's table)
    static constexpr int kLdsDoubles = 16 * DS + 2 * 16 * RS + Obs::A * 16 * PS;
    struct Prefetch {};                                 // nothing is requested ahead of barrier A
    using CoopRounds<GlmCoop<NCH, Obs>>::alive;
    using CoopRounds<GlmCoop<NCH, Obs>>::lane;
    using CoopRounds<GlmCoop<NCH, Obs>>::wv;
    const double *x, *xt, *y;
    const double2 *mu2, *tau2;   // lane-offset, device
    const double *cst;           // the constants, device
    const int2 *grp2;            // the group ids, lane-offset, device (Obs::H > 0)
    const int2 *kind2;           // the priors' kinds and their nu, lane-offset, device (Obs::kPriors)
    const double2 *nu2;
    const int32_t *part;         // the partner of every coordinate, device (Obs::kLocal)
    double inv2;                 // 1 / slab_scale^2, 0 without a slab (Obs::kLocal)
    GlmFactors fac;              // the factor terms (Obs::kFactors)
    GlmSlopes slo;               // their values (Obs::kSlopes)
    const int32_t *cpart;        // the partner table of the paired columns, device (Obs::kCorr)
    int cz0, ncp;                // the coordinate of zeta_0 and the pairs (Obs::kCorr)
    GlmStruct stc;               // the structured terms (Obs::kStruct)
    double *tile;
    int n, npad, nc, dx;         // dx: the columns of X (then Obs::A auxiliary coordinates, Obs::H log scales, the log local scales)
    template <class State>
    IDHMC_DEV void init(const State &s, double *tile_, int *alive_, int lane_, int wv_)
    {
        dx = s.D - Obs::A - Obs::H;
        if constexpr (Obs::kLocal) {
            part = s.lr_lpart;
            inv2 = s.lr_inv2;
            dx -= s.lr_j;
        }
        if constexpr (Obs::H > 0) grp2 = reinterpret_cast<const int2 *>(s.lr_grp) + lane_;
        if constexpr (Obs::kPriors) {
            kind2 = reinterpret_cast<const int2 *>(s.lr_pkind) + lane_;
            nu2 = reinterpret_cast<const double2 *>(s.lr_pnu) + lane_;
        }
        if constexpr (Obs::kFactors) fac.init(s);
        if constexpr (Obs::kSlopes) slo.init(s);
        if constexpr (Obs::kCorr) {
            cpart = s.lr_cpart;
            ncp = s.lr_cp;
            cz0 = s.D - s.lr_cp;
            dx -= s.lr_cp;
        }
        if constexpr (Obs::kStruct) {
            stc.init(s);
            dx -= s.lr_sz;
            if constexpr (Obs::kCorr) cz0 -= s.lr_sz;          // (the pairs' zetas come first)
        }
        x = s.lr_x;
        xt = s.lr_xt;
        y = s.lr_y;
        mu2 = reinterpret_cast<const double2 *>(s.mu) + lane_;
        tau2 = reinterpret_cast<const double2 *>(s.tau) + lane_;
        cst = s.user_params;
        tile = tile_;
        n = s.lr_n;
        npad = s.lr_npad;
        nc = (int)s.user_nparams;
        alive = alive_;
        lane = lane_;
        wv = wv_;
        // a row that never holds a chain is still multiplied: its offset into Y must be a valid one (the kernel's first barrier follows)
        if constexpr (Obs::kResponses) { if (lane == 0) *yslot(wv) = 0; }
    }
    // Obs::kResponses: row's offset into Y (doubles), kept in the padding column L of its Q row
    IDHMC_DEV int *yslot(int row) const { return reinterpret_cast<int *>(tile + kQ + row * DS + L); }
    // the chain of global id gc is this wavefront's next requester.  Called between rounds (every wavefront of the workgroup is in
    // every round, so none reads the slot now), ahead of barrier A of the chain's first request.
    template <class State>
    IDHMC_DEV void bind_chain(const State &s, uint32_t gc)
    {
        const uint32_t resp = gc / s.lr_r;
        if (lane == 0) *yslot(wv) = (int)(resp * (uint32_t)(Obs::K * npad));      // M K n_pad <= 2^27
    }
    IDHMC_DEV double *rtile(int b) const { return tile + kR + (b & 1) * (16 * RS); }
    IDHMC_DEV double *splane(int j) const { return tile + kS + j * (16 * PS); }
    IDHMC_DEV void prefetch(Prefetch &) const {}
    // (2) for block b: Z tile zt, r into R[b & 1], v added to vacc, the auxiliary scores to their planes
    IDHMC_DEV void zphase(int b, int zt, int kk, int jj, double (&vacc)[4]) const
    {
        const __amdgpu_buffer_rsrc_t rX = buf_rsrc(xt + 128 * b + 16 * zt);
        const int vo = (kk * npad + jj) * 8;                  // B[kk][jj] = X'[4 kb + kk][128 b + 16 zt + jj]
        const double *ap = tile + kQ + jj * DS + kk;          // A[jj][kk] = Q[chain jj][4 kb + kk]
        v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
        int kbn = KB;
        if constexpr (Obs::kFactors) kbn = 8 * ((fac.dd + 31) >> 5);      // the stored columns, in the loop's steps of 32 (<= Lx / 4)
#pragma unroll 1
        for (int kb0 = 0; kb0 < kbn; kb0 += 8) {
            double bv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                bv[u] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rX, vo + 4 * (kb0 + u) * npad * 8, 0, 0));
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * (kb0 + u)], bv[u], acc, 0, 0, 0);
        }
        const int i = 128 * b + 16 * zt + jj;
        if constexpr (Obs::kFactors) {
            // the level columns: b of observation i's level from each row's Q, factors ascending (lvl = -1, the padding, adds nothing)
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                if (f < fac.F) {
                    const int lv = fac.idx[(size_t)f * npad + i];
                    const double *qp = tile + kQ + kk * DS + fac.off[f] + (lv > 0 ? lv : 0);
                    double w = 0.0;                            // the observation's value, the same for the four rows (Obs::kSlopes)
                    if constexpr (Obs::kSlopes) w = slo.val[(size_t)f * npad + i];
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const double bl = qp[4 * reg * DS];
                        if constexpr (Obs::kSlopes)
                            acc[reg] = lv >= 0 ? dfma(w, bl, acc[reg]) : acc[reg];
                        else
                            acc[reg] = lv >= 0 ? acc[reg] + bl : acc[reg];
                    }
                }
            }
        }
        GlmObs o;
        if constexpr (!Obs::kResponses) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o.y[k] = k < Obs::K ? y[k * npad + i] : 0.0;
        }
        o.c = cst;
        o.K = Obs::K;
        o.nc = nc;
        o.A = Obs::A;
        double *rt = rtile(b) + 16 * zt + jj;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {                  // row kk + 4 reg (chain), column jj (observation)
            double r, v;
            double av[AN], u[AN];
            if constexpr (Obs::kResponses) {
                const double *yr = y + *yslot(kk + 4 * reg) + i;                             // Y of this row's chain
#pragma unroll
                for (int k = 0; k < 4; ++k) o.y[k] = k < Obs::K ? yr[k * npad] : 0.0;
            }
            if constexpr (Obs::A > 0) {
#pragma unroll
                for (int j = 0; j < AN; ++j) av[j] = splane(j)[(kk + 4 * reg) * PS + 128];   // a_j of this row's chain
            }
            glm_terms<Obs>(acc[reg], o, av, r, v, u);
            if (i >= n) { r = 0.0; v = 0.0; }
            vacc[reg] = vacc[reg] + v;
            if constexpr (Obs::A > 0) {
#pragma unroll
                for (int j = 0; j < AN; ++j) {
                    double *sp = splane(j) + (kk + 4 * reg) * PS + 16 * zt + jj;
                    *sp = (b == 0 ? 0.0 : *sp) + (i >= n ? 0.0 : u[j]);
                }
            }
            rt[(kk + 4 * reg) * RS] = r;
        }
    }
    // (3) for block b: G tile wv += R[b & 1] X[block, 16 wv ..]
    IDHMC_DEV void gphase(int b, int kk, int jj, v4d &gacc) const
    {
        if constexpr (Obs::kFactors) {
            // rows of Lx doubles; a tile at or beyond Dd has no stored column and skips the matrix steps
            if (16 * wv < fac.dd) {
                const __amdgpu_buffer_rsrc_t rX = buf_rsrc(x + (size_t)128 * b * fac.lx + 16 * wv);
                const int vo = (kk * fac.lx + jj) * 8;
                const double *ap = rtile(b) + jj * RS + kk;
#pragma unroll 1
                for (int kb0 = 0; kb0 < 32; kb0 += 8) {
                    double bv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        bv[u] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rX, vo + 4 * (kb0 + u) * fac.lx * 8, 0, 0));
#pragma unroll
                    for (int u = 0; u < 8; ++u) gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * (kb0 + u)], bv[u], gacc, 0, 0, 0);
                }
            }
            // the tile's level columns: lane (kk, jj) holds column 16 wv + jj of rows kk + 4 reg and adds their r over the column's list
            if (16 * wv + 16 > fac.dd && 16 * wv < dx) {
                const int c = 16 * wv + jj, e = c - fac.dd;
                int s0, cnt;
                glm_list(fac, b, e, e >= 0 && c < dx, s0, cnt);
                const double *rp = rtile(b) + kk * RS;
                for (int k = 0; k < cnt; ++k) {
                    const int ii = glm_list_at(fac, b, s0 + k);
                    if constexpr (Obs::kSlopes) {
                        const double wl = glm_list_value(slo, fac, b, s0 + k);
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) gacc[reg] = dfma(wl, rp[4 * reg * RS + ii], gacc[reg]);
                    } else {
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) gacc[reg] = gacc[reg] + rp[4 * reg * RS + ii];
                    }
                }
            }
            return;
        }
        const __amdgpu_buffer_rsrc_t rX = buf_rsrc(x + (size_t)128 * b * L + 16 * wv);
        const int vo = (kk * L + jj) * 8;                     // B[kk][jj] = X[128 b + 4 kb + kk][16 wv + jj]
        const double *ap = rtile(b) + jj * RS + kk;           // A[jj][kk] = R[chain jj][4 kb + kk]
#pragma unroll 1
        for (int kb0 = 0; kb0 < 32; kb0 += 8) {
            double bv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                bv[u] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rX, vo + 4 * (kb0 + u) * L * 8, 0, 0));
#pragma unroll
            for (int u = 0; u < 8; ++u) gacc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * (kb0 + u)], bv[u], gacc, 0, 0, 0);
        }
    }
    // steps (2)-(4) of a round; entered after barrier A by all 16 wavefronts, left after barrier C
    IDHMC_DEV void multiply(Prefetch &) const
    {
        static_assert(kGT <= 16, "one 16-column tile of G per wavefront: L <= 256");
        int ln = lane;
        asm volatile("" : "+v"(ln));                          // see DenseMvnCoop::multiply
        const int kk = ln >> 4, jj = ln & 15;
        const int nb = npad >> 7;
        const bool zw = wv >= 16 - kZT, gw = wv < kGT;
        const int zt = wv - (16 - kZT);
        v4d gacc = v4d{0.0, 0.0, 0.0, 0.0};
        double vacc[4] = {0.0, 0.0, 0.0, 0.0};
        if (zw) zphase(0, zt, kk, jj, vacc);
        __syncthreads();                                      // R[0] complete
        for (int b = 0; b < nb; ++b) {
            if (gw) gphase(b, kk, jj, gacc);
            if (zw && b + 1 < nb) zphase(b + 1, zt, kk, jj, vacc);
            if (b + 1 < nb) __syncthreads();                  // R[b + 1] complete, R[b] consumed
        }
        // the last Z phase ran before the last barrier, so the Q tile is free; R[nb & 1] is not the one G reads now
        if (gw) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) tile[kQ + (kk + 4 * reg) * DS + 16 * wv + jj] = gacc[reg];
        }
        if (zw) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) rtile(nb)[(kk + 4 * reg) * RS + 16 * zt + jj] = vacc[reg];
        }
        __syncthreads();                                      // barrier C
    }
    IDHMC_DEV double grad(const Vec<NCH> &q, Vec<NCH> &g) const
    {
        double l0, l1;
        grad_partial(q, g, l0, l1);
        const double lq = -0.5 * wave_sum(l0, l1);
        return dfinite(lq) ? lq : -kInf;
    }
    // l = -1/2 wave_sum(l0, l1), as DenseMvnCoop's
    IDHMC_DEV void grad_partial(const Vec<NCH> &q, Vec<NCH> &g, double &l0, double &l1) const
    {
        Prefetch pf;
        double2 *row = reinterpret_cast<double2 *>(tile + kQ + wv * DS) + lane;
        double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;        // the groups' scales
        double cr0 = 0.0, cc0 = 1.0, cr1 = 0.0, cc1 = 1.0;    // Obs::kCorr: rho and c of the pairs
        Vec<NCH> qm;                                          // and ut in the columns, q elsewhere (q goes through the row for it)
        if constexpr (Obs::kCorr) {
            glm_corr_pairs<NCH>(q, cz0, ncp, cr0, cc0, cr1, cc1);
            glm_corr_mix<NCH>(qm, q, cpart, tile + kQ + wv * DS, lane, cr0, cc0, cr1, cc1);
        }
        double sf0 = 1.0, sc0 = 1.0, sf1 = 1.0, sc1 = 1.0;    // Obs::kStruct: phi and c of the slots; the scan runs on qm through the row
        if constexpr (Obs::kStruct) {
            if constexpr (!Obs::kCorr) qm = q;
            glm_struct_factors<NCH>(q, stc, sf0, sc0, sf1, sc1);
            glm_struct_scan<NCH>(qm, stc, tile + kQ + wv * DS, lane, sf0, sc0, sf1, sc1);
        }
        const Vec<NCH> &u = glm_pick<Obs::kCorr || Obs::kStruct>(qm, q);      // what the scales and the products run on
        if constexpr (Obs::kLocal) {
            // q goes through the row first (each column reads its lambda there), then b takes its place, +0 in every column >= dx
            if constexpr (Obs::H > 0) glm_group_scales<NCH, HN>(q, dx + Obs::A, e0, e1, e2, e3);
            Vec<NCH> bq;
            glm_local_b<NCH, Obs::H>(bq, u, grp2, part, tile + kQ + wv * DS, dx, lane, e0, e1, e2, e3, inv2);
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c0 = 128 * j + 2 * lane;
                row[j * 64] = make_double2(c0 >= dx ? 0.0 : bq.c[j].x, c0 + 1 >= dx ? 0.0 : bq.c[j].y);
            }
        } else if constexpr (Obs::H > 0) {
            // the Q row is b = u e, +0 in every column that is not one of X (the auxiliary ones and the log scales)
            glm_group_scales<NCH, HN>(q, dx + Obs::A, e0, e1, e2, e3);
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c0 = 128 * j + 2 * lane;
                const int2 id = grp2[j * 64];
                row[j * 64] = make_double2(c0 >= dx ? 0.0 : glm_scaled<HN>(u.c[j].x, id.x, e0, e1, e2, e3), c0 + 1 >= dx ? 0.0 : glm_scaled<HN>(u.c[j].y, id.y, e0, e1, e2, e3));
            }
        } else if constexpr (Obs::A > 0 || Obs::kCorr || Obs::kStruct) {
            // (the zetas are coordinates behind the columns like the auxiliary ones: +0 in the row)
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c0 = 128 * j + 2 * lane;
                row[j * 64] = make_double2(c0 >= dx ? 0.0 : u.c[j].x, c0 + 1 >= dx ? 0.0 : u.c[j].y);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NCH; ++j) row[j * 64] = q.c[j];
        }
        if constexpr (Obs::A > 0) {
#pragma unroll
            for (int jx = 0; jx < AN; ++jx) {
                const double a = glm_coord<NCH>(q, dx + jx);
                if (lane == (((dx + jx) & 127) >> 1)) splane(jx)[wv * PS + 128] = a;
            }
        }
        __syncthreads();                                      // barrier A
        multiply(pf);
        const double2 A = reinterpret_cast<const double2 *>(rtile(npad >> 7) + wv * RS)[lane];
        double S[AN];
        if constexpr (Obs::A > 0) {
#pragma unroll
            for (int jx = 0; jx < AN; ++jx) {
                const double *sp = splane(jx) + wv * PS + 2 * lane;      // a row of 129 doubles is not 16-byte aligned: two loads
                S[jx] = wave_sum(sp[0], sp[1]);
            }
        }
        Vec<NCH> Gh;                                          // with groups, local scales or pairs: the whole G row, for the chain rule
        if constexpr (Obs::H > 0 || Obs::kLocal || Obs::kCorr || Obs::kStruct) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                Gh.c[j] = row[j * 64];
                if constexpr (Obs::A > 0) {
#pragma unroll
                    for (int jx = 0; jx < AN; ++jx) glm_place(Gh.c[j], j, dx + jx, lane, S[jx]);
                }
            }
            // the scales again, from q: eight registers held across the round made the matrix loops of multiply() spill
            int c0 = dx + Obs::A;
            asm volatile("" : "+s"(c0));                      // (not the value of before barrier A kept alive)
            if constexpr (Obs::H > 0) glm_group_scales<NCH, HN>(q, c0, e0, e1, e2, e3);
            // (pairs: rho, c and ut again from q, through the row, which is the requester's own until barrier A now that G is in registers)
            int cz = 0;
            if constexpr (Obs::kCorr) {
                cz = cz0;
                asm volatile("" : "+s"(cz));
                glm_corr_pairs<NCH>(q, cz, ncp, cr0, cc0, cr1, cc1);
                glm_corr_mix<NCH>(qm, q, cpart, tile + kQ + wv * DS, lane, cr0, cc0, cr1, cc1);
            }
            // (structured terms: phi, c and the forward scan again from q, through the row, as the pairs above)
            GlmStruct st2;
            if constexpr (Obs::kStruct) {
                st2 = stc;
                asm volatile("" : "+s"(st2.cz0), "+s"(st2.cz1));
                if constexpr (!Obs::kCorr) qm = q;
                glm_struct_factors<NCH>(q, st2, sf0, sc0, sf1, sc1);
                glm_struct_scan<NCH>(qm, st2, tile + kQ + wv * DS, lane, sf0, sc0, sf1, sc1);
            }
            // (local scales: the G row is in registers now, so q and then wl go through the row, which is the requester's own until barrier A)
            if constexpr (Obs::kLocal) glm_local_chain<NCH, Obs::H>(Gh, u, grp2, part, tile + kQ + wv * DS, dx, c0, lane, e0, e1, e2, e3, inv2);
            else if constexpr (Obs::H > 0) glm_group_chain<NCH, HN>(Gh, u, grp2, c0, lane, e0, e1, e2, e3);
            if constexpr (Obs::kCorr) glm_corr_chain<NCH>(Gh, q, cpart, tile + kQ + wv * DS, cz, ncp, lane, cr0, cc0, cr1, cc1);
            if constexpr (Obs::kStruct) glm_struct_chain<NCH>(Gh, q, u, st2, tile + kQ + wv * DS, lane, sf0, sc0, sf1, sc1);
        }
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const double2 m = mu2[j * 64], t = tau2[j * 64];
            double2 G;
            if constexpr (Obs::H > 0 || Obs::kLocal || Obs::kCorr || Obs::kStruct) {
                G = Gh.c[j];
            } else {
                G = row[j * 64];
                if constexpr (Obs::A > 0) {
#pragma unroll
                    for (int jx = 0; jx < AN; ++jx) glm_place(G, j, dx + jx, lane, S[jx]);
                }
            }
            const double dx = q.c[j].x - m.x, dy = q.c[j].y - m.y;
            if constexpr (Obs::kPriors) {
                // kinds and nu are read here, after barrier C: nothing of the prior is alive across multiply()
                const int2 k = kind2[j * 64];
                const double2 nu = nu2[j * 64];
                g.c[j].x = glm_prior_of<Obs::kCorr || Obs::kStruct>(k.x, nu.x, t.x, dx, G.x, t0);
                g.c[j].y = glm_prior_of<Obs::kCorr || Obs::kStruct>(k.y, nu.y, t.y, dy, G.y, t1);
            } else {
                t0 = dfma(t.x * dx, dx, t0);
                t1 = dfma(t.y * dy, dy, t1);
                g.c[j] = make_double2(dfma(-t.x, dx, G.x), dfma(-t.y, dy, G.y));
            }
        }
        l0 = dfma(2.0, A.x, t0);
        l1 = dfma(2.0, A.y, t1);
    }
};

// the built-in logistic regression
template <int NCH>
using LogisticRegression = GlmWave<NCH, LogisticObs>;
template <int NCH>
using LogisticRegressionCoop = GlmCoop<NCH, LogisticObs>;

}  // namespace idhmc
