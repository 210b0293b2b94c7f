// idhmc_glm_coords.hpp -- the arithmetic of a generalised linear model on a data matrix every chain shares, and the part of it that does
// not depend on how a kernel evaluates it.  The two forms that do (GlmWave, GlmCoop) and what is theirs alone are in idhmc_glm.hpp.
//   l(q) = -sum_i v(z_i, y_i) + log prior(q),   v = -log p(y | z) up to a data-only term,   r_i = d log p(y_i | z_i) / dz_i
// The observation is a policy type Obs: Obs::K data columns per observation (1..4), Obs::A auxiliary coordinates, Obs::H groups, the
// compile-time flags kResponses, kPriors, kLocal, kFactors, kSlopes, kCorr, kStruct, kGmrf, kBlock, kMulti, and
//   static void terms(double z, const GlmObs &o, double &r, double &v)                                             (A = 0)
//   static void terms(double z, const GlmObs &o, const double *a, double &r, double &v, double *s)    s[j] = d log p / d a_j
// A flag that is false (A, H = 0) takes its stage out at compile time: none of the instructions of a model without it changes.  Each
// feature's record is its DESIGN section (10-27); this comment is the full model in evaluation order, every stage tagged with its
// flag, and both forms and the tests' C restatements follow it bit for bit.  dfma is one fused multiply-add; every other operation
// is a plain one in the association written.
//
// COORDINATES.   q = [u (Dx) | a (A) | omega (H) | lambda (J) | zeta_pairs (P) | zeta_ar (Sz)],   D = Dx + A + H + J + P + Sz <= 1024
//   ([kBlock] the K (K - 1) / 2 zetas of the block stand where the pairs' stand: a model has pairs or a block, kCorr && kBlock is never built)
//   u       the Dx columns of the model.  [kFactors] Dd >= 1 dense columns, stored in X, then the levels of F <= 4 factor terms, never
//           stored: off_f = Dd + N_0 + .. + N_{f-1}, column off_f + k is level k of term f (N_f >= 1), Dx = Dd + sum N_f.  Without
//           factors Dd = Dx.  [kSlopes] a term may carry a finite value w_f[i] per observation next to its level index lvl_f[i]; two
//           terms may share one index array ((1 | s) and (x | s) are two terms of N columns each).  [kMulti] term f has a WIDTH M_f in
//           1..4: observation i has M_f entries (lvl_{f,m}[i], w_{f,m}[i]), m < M_f, the planes P = sum M_f <= 8.  An entry may be absent
//           (lvl = -1, the value ignored): the present entries of an observation come first and within a term their levels are strictly
//           ascending, hence distinct; an observation with no present entry in a term is allowed.  The columns are what they were,
//           off_f .. off_f + N_f - 1, and a wide term is in no pair and no block.
//   a       [A > 0] auxiliary coordinates: every observation sees them, no product with X does.
//   omega   [H > 0] log scales of the coefficient groups; grp[c] in {-1, 0 .. H-1} (DevState::lr_grp; -1: not in a group, and every
//           coordinate >= Dx).
//   lambda  [kLocal] local[c] in {0, 1} per column; the J flagged columns, ascending, get lambda_k, the LOGARITHM of the local scale of
//           col(k).  lr_lpart holds the partner of every coordinate: for a flagged column its lambda, for a lambda its column, -1
//           elsewhere.  inv2 = 1 / (S S) for a fixed slab scale S > 0 (lr_inv2; 0: no slab).
//   zeta_p  [kCorr] P <= 2 pairs (first_p, second_p) of distinct factor terms of N_p levels each, a term in at most one pair, with values
//           or without, on one index array or two; level k of the first is paired with level k of the second; zeta_p = atanh rho_p.
//           lr_cpart holds per coordinate -1 or  partner | pair << 10 | (second ? 2048 : 0);  lr_cp = P.  Not lr_lpart: kLocal and kCorr
//           are independent.
//   zeta_b  [kBlock] ONE block of K in {2, 3, 4} distinct factor terms t_0 .. t_{K-1} of N levels each, in the user's order, which is the row
//           order of L; with values or without, on one index array or several; level k of every term belongs together,
//           c_j = off_{t_j} + k.  zeta_ji = atanh z_ji, 1 <= j < K, 0 <= i < j, is coordinate cz0 + j (j - 1) / 2 + i (row-major), z the
//           canonical partial correlations of R = L L'.  lr_bpart holds per coordinate -1 or  k | row << 10;  lr_bk = K, lr_boff the rows'
//           first columns.  A block term is neither structured nor a GMRF term.
//   zeta_ar [kStruct] S <= 2 structured factor terms (slots 0, 1): the levels in index order are an AR(1) sequence with a sampled
//           phi = tanh(zeta) -- the Sz such zetas come behind the pairs' -- or a first-order random walk (phi = c = 1, no coordinate).
//           lr_spart holds per coordinate -1 or  k | slot << 10;  lr_s = S, lr_sz = Sz, lr_sn the slots' levels, lr_skind their kinds,
//           lr_scz their zeta coordinates (-1: a random walk).  A term is in a pair or structured, never both, and a structured column
//           has no local scale.
//   gmrf    [kGmrf] up to two GMRF terms (slots 0, 1), no coordinate of their own.  Each names a factor term f with N = N_f levels and
//           first column o = off_f, a symmetric N x N precision Q in CSR form -- start[N+1], col[], val[], columns ascending within a row,
//           the diagonal present in every row and > 0, at most 128 entries per row -- and a fixed kappa >= 0.  The term's levels u get
//           log p(u) = -1/2 u'Qu - 1/2 kappa (sum u)^2 in place of the iid N(0, 1) (PRIOR row 6); the scale of the effect is the term's
//           group scale, b = exp(omega_g) u, as for every term.  lr_gpart holds per coordinate -1 or  k | slot << 10;  lr_g the slots.
//           A GMRF term is in no pair and not structured, its columns carry no local scale and the default entries of the prior arrays.
//   Coordinate c of a chain's vector lives in lane (c & 127) >> 1, chunk c >> 7, component c & 1.
//
// FORWARD, per gradient.
//  1 factors, from q, each read from its owner lane, so the same bits in every lane:
//      [H]        e_g = dexp(omega_g)
//      [kCorr]    per pair  s = dexp(-|zeta|); t = s s; d = 1 + t; rho = copysign((1 - t) / d, zeta); c = (2 s) / d      (glm_corr_factors)
//                 (c = sqrt(1 - rho^2) in exact arithmetic; zeta = +0: rho = +0, c = 1; past |zeta| of about 745: rho = +-1, c = 0, finite)
//      [kBlock]   (z_ji, c_ji) = glm_corr_factors(zeta_ji).  coef(j, m, .) for -1 <= m < j, row j "behind column m":  s = 1; for i = m+1 .. j-1:
//                 coef(j,m,i) = z_ji s, then s = s c_ji; coef(j,m,j) = s -- and where s is still the initial 1 the other factor is taken
//                 itself, no multiplication.  L_ji = coef(j, -1, i), L_00 = 1:  L_j0 = z_j0, L_j1 = z_j1 c_j0, L_j2 = z_j2 (c_j0 c_j1),
//                 L_jj = ((c_j0 c_j1) c_j2).  r_jm = c_j0 .. c_j,m-1 left to right, r_j0 = 1.              (glm_block_factors, glm_block_coef)
//      [kStruct]  per slot  (phi, c) = glm_corr_factors of its zeta; the constants (1, 1) for a random walk and for a slot that is not there
//  2 mix [kCorr], k < N_p, c1 = off_first + k, c2 = off_second + k:   ut_c1 = u_c1;   ut_c2 = dfma(rho, u_c1, c u_c2);   ut = u elsewhere
//    [kBlock] ut_{c_0} = u_{c_0};  j >= 1:  x = L_jj u_{c_j};  for i = 0 .. j-1 ascending  x = dfma(L_ji, u_{c_i}, x);  ut_{c_j} = x   (glm_block_mix)
//      THE ASSOCIATION: the diagonal product first, then the partners' fmas with the column ascending.  At K = 2 this is the pair's
//      dfma(rho, u_c1, c u_c2) bit for bit, and every line of the block below is the pair's at K = 2 (coef is 1 or c, r = 1).
//  3 scan [kStruct], o the term's first column, N its levels: x_0 = u_o, x_k = c u_{o+k}; p = phi, h = 1; while h < N: every k >= h takes
//      x_k = dfma(p, x_{k-h}, x_k) from the values before the stage, then p = p p, h = 2 h; ut_{o+k} = x_k -- the Kogge-Stone form of
//      ut_0 = u_0, ut_k = phi ut_{k-1} + c u_k, and the definition of the bits (not the sequential recurrence).  Mix and scan touch disjoint
//      columns, so the scan runs on the mixed vector in place; the two slots share the stage loop (a slot with N <= h has no level left).
//  4 scales, b_c of every column c < Dx, on ut where the stages above exist and on u where not:
//      [H]        b_c = grp[c] >= 0 ? ut_c * e_grp[c] : ut_c   (a select over the groups)
//      [kLocal]   flagged column c, local coordinate k, id = grp[c]:   f = dexp(lambda_k);  s = id >= 0 ? e_id * f : f
//                 no slab: st = s (h unused);   slab: i = 1 / s;  nn = dfma(i, i, inv2);  st = 1 / sqrt(nn);  h = 1 - inv2 / nn
//                 (st = s / sqrt(1 + s^2 / S^2), h = d log st / d log s; s = inf gives st = S, h = 0; s = 0 gives st = 0, h = 1; with s below
//                  about 1.5e-154 i i overflows and st is 0 where it should be s: an absolute error below 1.5e-154 |u| in b_c -- the
//                  overflow itself sits at 7.5e-155.  h is a difference: accurate to about 1e-16 absolutely and, where s >> S and
//                  h -> 0, to no relative bound, so the likelihood's part of the gradient in
//                  lambda and omega, u st h, carries an absolute error of about 1e-16 |u| st there; their priors' part does not)
//                 b_c = ut_c * st;   every other column as under [H];   neither: b = ut
//  5 z_i = the dfma chain over the stored columns c < Dd ascending of X[i][c] b_c, from +0; then [kFactors] for f = 0 .. F-1 ascending
//        z_i = z_i + b[off_f + lvl_f[i]]  (plain addition),   [kSlopes]  z_i = dfma(w_f[i], b[off_f + lvl_f[i]], z_i)
//      Padded observations carry lvl = -1 and add nothing.  Under kSlopes EVERY term reads a value: a term without values has a plane of
//      1.0, and fma(1, b, z) is z + b rounded once, so its bits are those of the plain addition.
//      [kMulti] for f ascending and within f for m = 0 .. M_f-1 ascending:  z_i = dfma(w_{f,m}[i], b[off_f + lvl_{f,m}[i]], z_i)  for the
//      present entries.  Every plane reads a value, as under kSlopes (a term given without values has planes of 1.0).
//  6 (r_i, v_i, s_i0 ..) = Obs::terms(z_i, {y_i0 .. y_i,K-1; constants}, a), one call; for i >= n all are overwritten with 0 (the terms are
//      computed, then overwritten: a NaN there does not leak).  [kResponses] Y is M sets of K planes, [M][K][n_pad], and the chain of
//      GLOBAL id g samples response g / R (lr_r), whatever context or tile it runs in: only the address of y_i differs, and a kernel binds
//      the chain it takes (bind_chain, idhmc_internal.hpp) before it evaluates anything.
//      logistic (LogisticObs): s_i = y_i ? -z_i : z_i;  e_i = dexp(-|s_i|);  v_i = (s_i > 0 ? s_i : 0) + dlog1p(e_i) = softplus(z_i) - y_i z_i;
//                 r_i = (y_i ? 1 : -1) * ((s_i >= 0 ? 1 : e_i) / (1 + e_i)) = y_i - sigma(z_i)
//
// G, the gradient of the likelihood in b.
//  7 stored columns c < Dd:  G_c = dfma chain over observations i ascending of X[i][c] r_i, from +0
//  8 [kFactors] level columns:  G_{off_f + k} = plain additions, from +0, of r_i over the observations i < n with lvl_f[i] = k, i ascending;
//      [kSlopes] the dfma chain from +0 of dfma(w_f[i], r_i, G) over them.  An observation with w = 0.0 stays in its level's list:
//      dfma(0, r, G) is performed, as the expanded model does.  A level with no observation is allowed: its G is +0 and the prior alone
//      moves it.
//      [kMulti] the same chain over the observations i < n that have level k in ANY plane of term f, i ascending, each with the w of the
//      plane that names k.  Levels are distinct within an observation, so it appears at most once per level: a level's list in a block of
//      128 still has at most 128 entries and the clamps below stay valid.  A w of exactly 0.0 stays in its list.
//  9 [A] scores:  S_j[rho], rho = i mod 128: plain additions over observation blocks ascending, from +0;  G_{Dx+j} = the canonical
//      128-residue tree over S_j (wave_sum, lane l holding residues 2l, 2l + 1).   A[rho] accumulates v_i the same way.
//
// BACKWARD, the chain rules on G, in this order.
// 10 [kLocal] or else [H] (glm_local_chain, glm_group_chain; b, st, h again from ut):   w_c = G_c * b_c for a grouped or flagged c;
//      flagged c: wl_c = slab ? w_c * h : w_c;  G_{Dx+A+H+k} = wl_c (no reduction: one column feeds one coordinate);
//      W_g[rho], rho = c mod 128: plain additions over chunks ascending, from +0, of the members' w_c -- wl_c for a flagged member -- (a
//      non-member adds +0);  G_{Dx+A+g} = the canonical tree over W_g;   then G_c <- G_c * st (flagged), G_c * e_grp[c] (other members).
//      This leaves Gh_c = dl / dut_c in the columns.
// 11 [kCorr] (glm_corr_chain):  m_k = Gh_c2 (c dfma(c, u_c1, -(rho u_c2)));   G_c1 = dfma(rho, Gh_c2, Gh_c1);   G_c2 = c Gh_c2
//      M_p[c2 mod 128]: plain additions over chunks ascending, from +0, of the pair's m_k (a non-member adds +0);  G_zeta_p = the tree over M_p
//    [kBlock] (glm_block_chain), per zeta_jm:  w = coef(j,m,j) u_{c_j} (u_{c_j} itself when j = m + 1);  for i = m+1 .. j-1 ascending
//      w = dfma(coef(j,m,i), u_{c_i}, w);  e = c_jm dfma(c_jm, u_{c_m}, -(z_jm w));  m >= 1: e = r_jm e;  m_k = Gh_{c_j} e
//      (Gh_j dut_j / dzeta_jm with dut_j / dzeta_jm = r_jm c_jm (c_jm u_m - z_jm w));  M_jm[c_j mod 128]: plain additions over chunks
//      ascending, from +0 (a non-member adds +0);  G_zeta_jm = the tree over M_jm.  Then, from the Gh before any is overwritten:
//      G_{c_i} = (i == 0 ? Gh_{c_0} : L_ii Gh_{c_i});  for j = i+1 .. K-1 ascending  G_{c_i} = dfma(L_ji, Gh_{c_j}, G_{c_i}).
// 12 [kStruct] (glm_struct_chain):  y_k = Gh_{o+k}; p = phi, h = 1; while h < N: every k with k + h < N takes y_k = dfma(p, y_{k+h}, y_k),
//      then p = p p, h = 2 h; lambda_k = y_k;  G_{u_o} = lambda_0, G_{u_{o+k}} = c lambda_k;   AR(1): m_k = lambda_k (c dfma(c, ut_{o+k-1},
//      -(phi u_{o+k}))), k >= 1; M[(o+k) mod 128] plain additions over chunks ascending from +0;  G_zeta = the tree over M.
//
// PRIOR, before the loop, [kGmrf] per slot with kappa > 0: Sr per lane component = the plain additions over chunks ascending, from +0, of
// the member u_c (a non-member adds +0);  S = wave_sum(Sr.x, Sr.y), the canonical tree (glm_gmrf_sums).
// PRIOR (the last loop of both forms; glm_prior_of), on the raw q (the prior of u is on u), over all D coordinates: d = q_c - mu_c; per lane component T = the sum
// over chunks ascending of the coordinate's -2 log prior up to a constant, g_c from G_c.  [kPriors] kind_c (lr_pkind) and nu_c (lr_pnu)
// select the row, without the flag every row is 0; padded coordinates are kind 0:
//   0 NORMAL               T = dfma(tau d, d, T)                                        g = dfma(-tau, d, G)
//   1 STUDENT_T            a = tau d; s = a d;   T = T + (nu + 1) dlog1p(s / nu)          g = G + (-((nu + 1) a) / (nu + s))
//   2 LOG_HALF_NORMAL      e = dexp(2 d);        T = T + (e - 2 d)                        g = G + (1 - e)
//   3 LOG_HALF_STUDENT_T   e = dexp(2 d);        T = T + ((nu + 1) dlog1p(e / nu) - 2 d)  g = G + (1 - ((nu + 1) e) / (nu + e))
//   4 LOG_EXPONENTIAL      e = dexp(d);          T = T + 2 (e - d)                        g = G + (1 - e)
//   5 (internal, [kCorr], [kStruct] or [kBlock] only: a zeta with eta > 0, eta in nu's place; LKJ(eta) on the 2 x 2 correlation with the Jacobian of
//      tanh, log p(zeta) = eta log(1 - rho^2))   t as in stage 1:
//                          T = T + (4 eta) ((|zeta| + dlog1p(t)) - ln 2)                g = dfma(-2 eta, rho, G)      (ln 2 rounded to a double)
//      eta = 0: the coordinate's entry of the prior arrays applies (kinds 0 and 1).
//      [kBlock] LKJ(eta) on the K x K matrix is separable in the partial correlations: the host marks every zeta_ji with this row and puts
//      beta_ji = eta + (K - 2 - i) / 2 (i the COLUMN) in nu's place; the row itself is unchanged.
//   6 (internal, [kGmrf] only, like row 5; glm_gmrf_row)  a member c = o + k, u_c = q_c:
//                          s = kappa > 0 ? kappa * S : +0;   for e = start[k] .. start[k+1]-1 ascending:  s = dfma(val[e], u_{o + col[e]}, s)
//                          T = dfma(u_c, s, T)                                          g = G - s
//      This states log p(u) = -1/2 u'Qu - 1/2 kappa (sum u)^2, since sum_c u_c (Qu)_c = u'Qu and sum_c u_c kappa S = kappa S^2.  The row
//      REPLACES the coordinate's entry of the prior arrays and sits inside the loop, in chunk order: with Q = I and kappa = 0 it gives
//      the bits of row 0 with mu = 0, tau = 1 at every L, for u and G that are not -0.  The u_{o+col} are read from vec, which holds
//      the raw q for the duration of the loop.  Every walk is clamped as the level lists are: at most 128 trips per row, col masked
//      into 0 .. N-1, entry positions inside the term's table -- a bad table cannot read outside vec or the table.
// The log kinds are priors on exp(q_c) with scale exp(mu_c) and carry the Jacobian of exp (a lambda is a coordinate like any other: they
// apply to it).  The two components of a lane, and neighbouring chunks, may be of different kinds: the kinds are branches of one function.
// Each kind is finite wherever its log density is, and that ends at: kind 1, tau d^2 finite (|d| < 1.3e154 / sqrt(tau)); kinds 2 and 3,
// 2 d < 709.78 (every more negative d is fine: e = 0 and T = -2 d); kind 4, d < 709.08 (2 exp(d) finite).  Past those ends T is +inf (g may
// be NaN), which the engine reads as l(q) = -inf: the ordinary rejected point.  The two t kinds also end where nu leaves what their
// arithmetic holds: s / nu or e / nu overflowing makes T +inf where the density is finite (nu below tau d^2 / 1.8e308), and g is finite
// while (nu + 1) a, (nu + 1) e are: kind 3's g ends at 2 d < 709.78 - log(nu + 1), before its T does.  Row 5's T is computed as a
// difference of terms of size |zeta| + ln 2 and is accurate to about 1e-16 eta absolutely; at small zeta, where the true T is
// 2 eta zeta^2, its relative error is unbounded (its sign included) and g = -2 eta rho, which does not cancel, is what moves the chain.
// tests/test_glm_terms_edges_cpu.py holds every row to mpmath over these ranges and asserts each end.
//
// P AND l.   Per lane component (residues 2l, 2l+1 of 128):  P = dfma(2, A, T);   l = -1/2 wave_sum(P0, P1), -inf where that is not finite.
//
// EDGES.  A chain of fmas from +0 never holds -0, so the zero padding (columns >= Dx, observations >= n) leaves every chain as it is:
// a form may stop at Dx and n or run over padded tiles, and both give the same bits.  For finite b and r the level columns are bit for
// bit the same model with every level written out as an indicator column of X (glm.expand_factors): adding +-0 changes nothing
// (fma(0, b, z) = z, fma(0, r, G) = G), and fma(1, x, y) is y + x rounded once.  It ends at the non-finite: a non-finite b of one level
// poisons every z of the expanded model (0 * inf) and here only that level's observations; both are rejected points.  With values the
// expanded column off_f + k holds w_f[i] where lvl_f[i] = k and 0.0 elsewhere, and there is one more edge: a chain from +0 now CAN reach
// -0 -- fma(w, b, +0) with w b negative and below half the smallest subnormal rounds to -0, and the expanded model's next fma(0, x, -0)
// is +0 for x >= 0 where this one keeps -0.  Stated and not engineered around.  [kMulti] the expanded column off_f + k holds w_{f,m}[i]
// where lvl_{f,m}[i] = k and 0.0 elsewhere, and it is the ascending levels that keep the bits: the expanded chain of z_i meets the
// columns of a term in ascending order, which is then the order of the planes, and everything between two of them is fma(0, b, z) = z.
// The same conditions, the same two edges.
//
// DEVICE LAYOUT (DevState).  X [n_pad][Lx] (lr_x), X' [Lx][n_pad] (lr_xt), Y as K planes [K][n_pad] per response (lr_y), all zero-padded
// (+0 in every column >= Dd); a GLM's constants in user_params (user_nparams of them).  Lx = 128 ceil(Dd / 128) is a run-time member
// under kFactors (lr_lx) and the compile-time L without.  [kFactors] lr_fidx holds the index planes, int32 [F][n_pad], -1 in the padding;
// the level lists, built on the host: per block of 128 observations lr_fpos holds 128 F bytes -- the block's observations (position in the
// block) of factor 0 sorted by level, positions ascending within a level, then factor 1's, .. -- and lr_fstart [n_pad / 128][sum N_f + 1]
// where each level's list starts in them (cumulative over the factors: entry e and e + 1 bound the list of column Dd + e).  Every walk of
// a list is clamped on the device: at most 128 trips, positions inside the block's 128 F bytes, the byte read masked to 0 .. 127, so no
// list, whatever it held, reads outside the R tile or the wavefront's vector.  [kGmrf] lr_gstart [sum N + 1] (int32, cumulative over the
// slots: the rows of slot 0, then those of slot 1), lr_gcol (int32) and lr_gval (double) hold the precisions' entries, lr_gnz the slots'
// entry counts, lr_gkappa, lr_go, lr_gn their kappa, first column and levels.  [kSlopes] lr_fval [F][n_pad] holds w (1.0 for a plain
// term, 0.0 in the padding, where lvl = -1 adds nothing anyway); lr_fwl [n_pad / 128][128 F] holds the same values a second time in the
// order of lr_fpos, written by the counting sort that builds the lists, so that the value of list entry t has an address known before
// the entry's byte arrives -- no second dependent global load behind that byte.  t is clamped as glm_list_at clamps it and the 128-trip
// cap holds: a bad list still cannot read outside the block's entries.  [kMulti] (lr_mp = P > 0) the layout goes by PLANE, the planes of
// term 0 first: lr_fidx and lr_fval [P][n_pad] (-1 and 0.0 where an entry is absent), lr_fpos and lr_fwl with 128 P entries per block --
// the counting sort puts every present entry of every plane of a term into that term's level lists, places ascending within a level, the
// entry's value into lr_fwl at the same position -- and eight more int32 behind the last row of lr_fstart: the first column of the term
// each plane belongs to (GlmMulti::poff; uniform, so a scalar load).  lr_fstart stays per column and lr_foff per TERM: pairs, blocks,
// structures and GMRF slots index it as before.  The reason lr_fwl exists applies unchanged.
//
// EXCHANGE BETWEEN LANES.  A column and its lambda, the two columns of a pair, and neighbouring levels of a structured term live in
// different lanes, chunks and components in general; so do the up to three partners of a block's column.  The helpers of stages 2-4 and 10-12 take vec, a wavefront-private LDS vector
// (>= 128 NCH doubles, indexed by coordinate), written and read by one wavefront in program order, no workgroup barrier; values stay
// in registers.  Which vector that is, and when each stage runs, is the form's (idhmc_glm.hpp).
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
// A correlation block (Obs::kBlock).  An entry of the level table: -1, or k | row << 10 for level k of the term in row 0 .. K-1 of L
constexpr int kBlockRow = 10, kBlockMask = 1023;
// what both forms take from DevState: the rows' first columns, K, the zetas nz = K (K - 1) / 2 and the coordinate of zeta_10
struct GlmBlock {
    const int32_t *bpart;
    int K, nz, cz0;
    int off[4];
    template <class State>
    IDHMC_DEV void init(const State &s)
    {
        bpart = s.lr_bpart;
        K = s.lr_bk;
        nz = (K * (K - 1)) >> 1;
        cz0 = s.D - s.lr_sz - nz;                              // (the block's zetas come first, the AR(1) zetas last)
#pragma unroll
        for (int r = 0; r < 4; ++r) off[r] = s.lr_boff[r];
    }
};
// (z_ji, c_ji) of the block at index j (j - 1) / 2 + i, the same bits in every lane; the constants (0, 1) for a zeta that is not there.
// The indices are compile-time constants everywhere: the twelve doubles are registers, never an indexed array.
struct GlmBlockZ {
    double z[6], c[6];
};
constexpr int glm_bz(int j, int i) { return ((j * (j - 1)) >> 1) + i; }
template <int NCH>
IDHMC_DEV void glm_block_factors(const Vec<NCH> &q, const GlmBlock &bk, GlmBlockZ &f)
{
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        f.z[e] = 0.0;
        f.c[e] = 1.0;
        if (e < bk.nz) glm_corr_factors<NCH>(q, bk.cz0 + e, f.z[e], f.c[e]);
    }
}
// coef(J, M, I) of the header comment, M < I <= J (M = -1: L_JI); where s is still the initial 1 the other factor is taken itself
template <int J, int M, int I>
IDHMC_DEV double glm_block_coef(const GlmBlockZ &f)
{
    double s = 1.0;
    bool one = true;
#pragma unroll
    for (int i = M + 1; i < I; ++i) {
        s = one ? f.c[glm_bz(J, i)] : s * f.c[glm_bz(J, i)];
        one = false;
    }
    if constexpr (I == J) return s;
    else return one ? f.z[glm_bz(J, I)] : f.z[glm_bz(J, I)] * s;
}
// L_JI for the row j the lane's column is in (a select over the rows; I <= j)
template <int I>
IDHMC_DEV double glm_block_lcol(const GlmBlockZ &f, int j)
{
    // rows J > I hold L_JI below the diagonal, row I the diagonal
    double l = 1.0;
    if constexpr (I == 0) l = j == 1 ? glm_block_coef<1, -1, 0>(f) : j == 2 ? glm_block_coef<2, -1, 0>(f) : glm_block_coef<3, -1, 0>(f);
    if constexpr (I == 1) l = j == 1 ? glm_block_coef<1, -1, 1>(f) : j == 2 ? glm_block_coef<2, -1, 1>(f) : glm_block_coef<3, -1, 1>(f);
    if constexpr (I == 2) l = j == 2 ? glm_block_coef<2, -1, 2>(f) : glm_block_coef<3, -1, 2>(f);
    if constexpr (I == 3) l = glm_block_coef<3, -1, 3>(f);
    return l;
}
// ut of one column: u its own coordinate, row j >= 1, p0 .. p2 the partners u_{c_0} .. u_{c_2} (those at or past j unused)
IDHMC_DEV double glm_block_mix1(const GlmBlockZ &f, int j, double u, double p0, double p1, double p2)
{
    const double ljj = j == 1 ? glm_block_lcol<1>(f, 1) : j == 2 ? glm_block_lcol<2>(f, 2) : glm_block_lcol<3>(f, 3);
    double x = ljj * u;
    x = dfma(glm_block_lcol<0>(f, j), p0, x);
    x = j > 1 ? dfma(glm_block_lcol<1>(f, j), p1, x) : x;
    x = j > 2 ? dfma(glm_block_lcol<2>(f, j), p2, x) : x;
    return x;
}
// the partners' values of the column with table entry e (row j): vec[off_i + k] for the rows i < j, vec[0] (unused) elsewhere
IDHMC_DEV void glm_block_partners(const GlmBlock &bk, const double *vec, int e, double &p0, double &p1, double &p2)
{
    const int j = e >= 0 ? e >> kBlockRow : 0, k = e & kBlockMask;
    p0 = vec[j > 0 ? bk.off[0] + k : 0];
    p1 = vec[j > 1 ? bk.off[1] + k : 0];
    p2 = vec[j > 2 ? bk.off[2] + k : 0];
}
// ut of every coordinate of the lane: stage 2 for a column of the rows 1 .. K-1, q itself elsewhere.  vec as for glm_corr_mix: q is
// staged there and each column reads up to three partners.
template <int NCH>
IDHMC_DEV void glm_block_mix(Vec<NCH> &ut, const Vec<NCH> &q, const GlmBlock &bk, double *vec, int lane, const GlmBlockZ &f)
{
    double2 *v2 = reinterpret_cast<double2 *>(vec) + lane;
    const int2 *part2 = reinterpret_cast<const int2 *>(bk.bpart) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = q.c[j];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 e = part2[j * 64];
        double a0, a1, a2, b0, b1, b2;
        glm_block_partners(bk, vec, e.x, a0, a1, a2);
        glm_block_partners(bk, vec, e.y, b0, b1, b2);
        const bool mx = e.x >= (1 << kBlockRow), my = e.y >= (1 << kBlockRow);
        ut.c[j].x = mx ? glm_block_mix1(f, e.x >> kBlockRow, q.c[j].x, a0, a1, a2) : q.c[j].x;
        ut.c[j].y = my ? glm_block_mix1(f, e.y >> kBlockRow, q.c[j].y, b0, b1, b2) : q.c[j].y;
    }
}
// e of zeta_JM for a column of row J: u its own coordinate, p[i] = u_{c_i}; m_k = Gh e
template <int J, int M>
IDHMC_DEV double glm_block_e(const GlmBlockZ &f, double u, double p0, double p1, double p2)
{
    double w = u;
    if constexpr (J > M + 1) w = glm_block_coef<J, M, J>(f) * u;
    if constexpr (M + 1 <= 1 && 1 < J) w = dfma(glm_block_coef<J, M, 1>(f), p1, w);
    if constexpr (M + 1 <= 2 && 2 < J) w = dfma(glm_block_coef<J, M, 2>(f), p2, w);
    const double um = M == 0 ? p0 : M == 1 ? p1 : p2;
    const double cm = f.c[glm_bz(J, M)];
    double e = cm * dfma(cm, um, -(f.z[glm_bz(J, M)] * w));
    if constexpr (M == 1) e = f.c[glm_bz(J, 0)] * e;
    if constexpr (M == 2) e = (f.c[glm_bz(J, 0)] * f.c[glm_bz(J, 1)]) * e;
    return e;
}
// G_{c_i} of the column with table entry e (row i, level k): g its own Gh, the Gh of the rows j > i read from vec
IDHMC_DEV double glm_block_back1(const GlmBlock &bk, const GlmBlockZ &f, const double *vec, int e, double g)
{
    const bool in = e >= 0;
    const int i = in ? e >> kBlockRow : 4, k = e & kBlockMask;
    const double g1 = vec[i < 1 ? bk.off[1] + k : 0];
    const double g2 = vec[i < 2 && bk.K > 2 ? bk.off[2] + k : 0];
    const double g3 = vec[i < 3 && bk.K > 3 ? bk.off[3] + k : 0];
    const double lii = i == 1 ? glm_block_lcol<1>(f, 1) : i == 2 ? glm_block_lcol<2>(f, 2) : glm_block_lcol<3>(f, 3);
    double x = i == 0 ? g : lii * g;
    x = i < 1 ? dfma(glm_block_coef<1, -1, 0>(f), g1, x) : x;
    const double l2 = i == 0 ? glm_block_coef<2, -1, 0>(f) : glm_block_coef<2, -1, 1>(f);
    x = i < 2 && bk.K > 2 ? dfma(l2, g2, x) : x;
    const double l3 = i == 0 ? glm_block_coef<3, -1, 0>(f) : i == 1 ? glm_block_coef<3, -1, 1>(f) : glm_block_coef<3, -1, 2>(f);
    x = i < 3 && bk.K > 3 ? dfma(l3, g3, x) : x;
    return in ? x : g;
}
template <int J, int M>
IDHMC_DEV void glm_block_madd(double2 &Mz, const GlmBlockZ &f, int jx, int jy, const double2 &Gh, const double2 &u, double a0, double a1, double a2,
                              double b0, double b1, double b2)
{
    const double mx = Gh.x * glm_block_e<J, M>(f, u.x, a0, a1, a2), my = Gh.y * glm_block_e<J, M>(f, u.y, b0, b1, b2);
    Mz.x = Mz.x + (jx == J ? mx : 0.0);
    Mz.y = Mz.y + (jy == J ? my : 0.0);
}
// the chain rule of the block on the lane's G (Gh in the columns, complete elsewhere but for the zetas): m_k into M_jm and by the tree
// into coordinate cz0 + j (j - 1) / 2 + m, then G_{c_i} from the Gh of the rows j >= i, read through vec once every u has been
template <int NCH>
IDHMC_DEV void glm_block_chain(Vec<NCH> &G, const Vec<NCH> &q, const GlmBlock &bk, double *vec, int lane, const GlmBlockZ &f)
{
    double2 *v2 = reinterpret_cast<double2 *>(vec) + lane;
    const int2 *part2 = reinterpret_cast<const int2 *>(bk.bpart) + lane;
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = q.c[j];
    double2 M10 = make_double2(0.0, 0.0), M20 = M10, M21 = M10, M30 = M10, M31 = M10, M32 = M10;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 e = part2[j * 64];
        double a0, a1, a2, b0, b1, b2;
        glm_block_partners(bk, vec, e.x, a0, a1, a2);
        glm_block_partners(bk, vec, e.y, b0, b1, b2);
        const int jx = e.x >= 0 ? e.x >> kBlockRow : 0, jy = e.y >= 0 ? e.y >> kBlockRow : 0;
        glm_block_madd<1, 0>(M10, f, jx, jy, G.c[j], q.c[j], a0, a1, a2, b0, b1, b2);
        if (bk.K > 2) {
            glm_block_madd<2, 0>(M20, f, jx, jy, G.c[j], q.c[j], a0, a1, a2, b0, b1, b2);
            glm_block_madd<2, 1>(M21, f, jx, jy, G.c[j], q.c[j], a0, a1, a2, b0, b1, b2);
        }
        if (bk.K > 3) {
            glm_block_madd<3, 0>(M30, f, jx, jy, G.c[j], q.c[j], a0, a1, a2, b0, b1, b2);
            glm_block_madd<3, 1>(M31, f, jx, jy, G.c[j], q.c[j], a0, a1, a2, b0, b1, b2);
            glm_block_madd<3, 2>(M32, f, jx, jy, G.c[j], q.c[j], a0, a1, a2, b0, b1, b2);
        }
    }
    // every u has been read: Gh takes q's place, and each column reads the Gh of the rows below its own
#pragma unroll
    for (int j = 0; j < NCH; ++j) v2[j * 64] = G.c[j];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 e = part2[j * 64];
        G.c[j].x = glm_block_back1(bk, f, vec, e.x, G.c[j].x);
        G.c[j].y = glm_block_back1(bk, f, vec, e.y, G.c[j].y);
    }
    glm_group_place<NCH>(G, M10, bk.cz0, lane);
    if (bk.K > 2) {
        glm_group_place<NCH>(G, M20, bk.cz0 + 1, lane);
        glm_group_place<NCH>(G, M21, bk.cz0 + 2, lane);
    }
    if (bk.K > 3) {
        glm_group_place<NCH>(G, M30, bk.cz0 + 3, lane);
        glm_group_place<NCH>(G, M31, bk.cz0 + 4, lane);
        glm_group_place<NCH>(G, M32, bk.cz0 + 5, lane);
    }
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

// GMRF terms (Obs::kGmrf).  An entry of the level table: -1, or k | slot << 10 for level k of the term in slot 0 or 1
constexpr int kGmrfSlot = 1024, kGmrfMask = 1023;
constexpr int kPriorGmrf = 6;                        // the device table's mark of a member of a GMRF term; never a public kind
// what both forms take from DevState: the slots' tables (n1 = z1 = 0 with one slot); z: the entries of a slot's precision
struct GlmGmrf {
    const int32_t *gpart, *start, *col;
    const double *val;
    double k0, k1;
    int o0, o1, n0, n1, z0, z1;
    template <class State>
    IDHMC_DEV void init(const State &s)
    {
        gpart = s.lr_gpart;
        start = s.lr_gstart;
        col = s.lr_gcol;
        val = s.lr_gval;
        const bool two = s.lr_g > 1;
        k0 = s.lr_gkappa[0];
        k1 = two ? s.lr_gkappa[1] : 0.0;
        o0 = s.lr_go[0];
        o1 = two ? s.lr_go[1] : 0;
        n0 = s.lr_gn[0];
        n1 = two ? s.lr_gn[1] : 0;
        z0 = s.lr_gnz[0];
        z1 = two ? s.lr_gnz[1] : 0;
    }
};
// S of the slots with kappa > 0 (+0 for the others): the members' u per lane component, chunks ascending from +0, then the tree
template <int NCH>
IDHMC_DEV void glm_gmrf_sums(const Vec<NCH> &q, const GlmGmrf &gm, int lane, double &S0, double &S1)
{
    const int2 *part2 = reinterpret_cast<const int2 *>(gm.gpart) + lane;
    double2 R0 = make_double2(0.0, 0.0), R1 = R0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int2 e = part2[j * 64];
        const bool ax = e.x >= 0, ay = e.y >= 0, sx = (e.x & kGmrfSlot) != 0, sy = (e.y & kGmrfSlot) != 0;
        R0.x = R0.x + (ax && !sx ? q.c[j].x : 0.0);
        R0.y = R0.y + (ay && !sy ? q.c[j].y : 0.0);
        R1.x = R1.x + (ax && sx ? q.c[j].x : 0.0);
        R1.y = R1.y + (ay && sy ? q.c[j].y : 0.0);
    }
    S0 = S1 = 0.0;
    if (gm.k0 > 0.0) S0 = wave_sum(R0.x, R0.y);
    if (gm.k1 > 0.0) S1 = wave_sum(R1.x, R1.y);
}
// PRIOR row 6 for the member with table entry e >= 0 (u its coordinate, G the likelihood's part of its gradient): adds u (Qu + kappa S)
// to T and returns g.  vec: the wavefront's own LDS vector holding the raw q, indexed by coordinate.  The walk is clamped: at most 128
// trips, entry positions inside the slot's part of the table, col into 0 .. N-1, so vec is read inside the term's columns only.
IDHMC_DEV double glm_gmrf_row(const GlmGmrf &gm, int e, const double *vec, double u, double S0, double S1, double G, double &T)
{
    const bool s1 = (e & kGmrfSlot) != 0;
    const int k = e & kGmrfMask;
    const int N = s1 ? gm.n1 : gm.n0, o = s1 ? gm.o1 : gm.o0;
    const int lo = s1 ? gm.z0 : 0, hi = s1 ? gm.z0 + gm.z1 : gm.z0;
    const double kap = s1 ? gm.k1 : gm.k0;
    double s = kap > 0.0 ? kap * (s1 ? S1 : S0) : 0.0;
    const int32_t *st = gm.start + (s1 ? gm.n0 : 0) + (k < N ? k : 0);
    const int e0 = st[0];
    int cnt = st[1] - e0;
    cnt = cnt > 128 ? 128 : cnt;
    cnt = hi > lo && N > 0 ? cnt : 0;
    for (int t = 0; t < cnt; ++t) {
        int p = e0 + t;
        p = p < lo ? lo : p > hi - 1 ? hi - 1 : p;
        int c = gm.col[p];
        c = c < 0 ? 0 : c > N - 1 ? N - 1 : c;
        s = dfma(gm.val[p], vec[o + c], s);
    }
    T = dfma(u, s, T);
    return G - s;
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
// Terms with several weighted levels per observation (Obs::kMulti, with kFactors and kSlopes): the index planes, the value planes and
// the blocks' bytes and values are laid out by PLANE -- lr_fidx and lr_fval [P][n_pad], lr_fpos and lr_fwl 128 P entries per block --
// and the plane's first column comes from a table of eight entries in device memory, which stands behind lr_fstart's last row.  The
// address is uniform: a scalar load, no register held across the gradient.  lr_fstart itself stays per column.
struct GlmMulti {
    const int32_t *poff;             // [8] the column of level 0 of the term plane p belongs to (planes >= P: that of the last plane)
    int P;                           // planes, sum M_f <= 8
    template <class State>
    IDHMC_DEV void init(const State &s)
    {
        poff = s.lr_fstart + (size_t)(s.lr_npad >> 7) * (size_t)(s.lr_fcols + 1);
        P = s.lr_mp;
    }
};
// glm_list_at and glm_list_value over blocks of 128 P entries: t clamped into the block's entries, the byte masked to 0 .. 127
IDHMC_DEV int glm_list_at(const GlmMulti &m, const GlmFactors &f, int b, int t)
{
    const int last = 128 * m.P - 1;
    t = t < 0 ? 0 : t > last ? last : t;
    return f.pos[(size_t)b * (size_t)(128 * m.P) + t] & 127;
}
IDHMC_DEV double glm_list_value(const GlmMulti &m, const GlmSlopes &v, int b, int t)
{
    const int last = 128 * m.P - 1;
    t = t < 0 ? 0 : t > last ? last : t;
    return v.wl[(size_t)b * (size_t)(128 * m.P) + t];
}
// Four entries of a list at a time: the lists of a wide term are M times as long as a plain term's, and walked one entry at a time each
// trip waits for its byte.  The bytes and values of entries t .. t + 3 have addresses known from t alone, so the eight loads go out
// together; an entry past the list's end is read (clamped into the block's entries, as ever) and not used.
constexpr int kListBatch = 4;
struct GlmListBatch {
    int ii[kListBatch];
    double wl[kListBatch];
};
IDHMC_DEV void glm_list_batch(GlmListBatch &q, const GlmMulti &m, const GlmSlopes &v, const GlmFactors &f, int b, int t)
{
#pragma unroll
    for (int u = 0; u < kListBatch; ++u) {
        q.ii[u] = glm_list_at(m, f, b, t + u);
        q.wl[u] = glm_list_value(m, v, b, t + u);
    }
}
// glm_gather over them: an observation is in a level's list once (its levels are distinct), so the list still has at most 128 entries.
// The chain is the list's order, entry by entry, as written in stage 8.
IDHMC_DEV void glm_gather(double &G, const GlmMulti &m, const GlmSlopes &v, const GlmFactors &f, int b, int e, bool has, const double *r)
{
    int s0, cnt;
    glm_list(f, b, e, has, s0, cnt);
    for (int k = 0; k < cnt; k += kListBatch) {
        GlmListBatch q;
        glm_list_batch(q, m, v, f, b, s0 + k);
#pragma unroll
        for (int u = 0; u < kListBatch; ++u) G = k + u < cnt ? dfma(q.wl[u], r[q.ii[u]], G) : G;
    }
}

}  // namespace idhmc
