// idhmc_glm.hpp -- the two forms that evaluate a generalised linear model (DESIGN sections 10-27).  The arithmetic, stage by stage for
// the full model, the device layout and every helper that does not depend on the form are in idhmc_glm_coords.hpp; the stage numbers
// below are that header's.  Two forms with one arithmetic: GlmWave (one chain per wavefront, every kernel) and GlmCoop (the NUTS kernel
// at L <= 256: 16 chains per workgroup, both products on the fp64 matrix cores).  The built-in logistic regression
// (IDHMC_MODEL_LOGISTIC_REGRESSION) is Obs = LogisticObs, instantiated ahead of time (idhmc_logistic.hip); a user's GLM
// (IDHMC_MODEL_GLM) is Obs = its glm_observation, instantiated by hipRTC (idhmc_jit.hip).  Kept out of what the hipRTC build of a
// custom density includes.
// What a form decides: which wavefront-private LDS vector the lanes exchange through, when the factors, ut and b (stages 1-4) are made
// and made again, and how the two products (5, 7, 8) are laid out.  What both keep: the four group scales are handed around as four
// scalars (glm_group_scales), and no feature adds LDS, a tile or a barrier to either form.
#pragma once
#include "idhmc_glm_coords.hpp"

namespace idhmc {

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
    static constexpr bool kResponses = false, kPriors = false, kLocal = false, kFactors = false, kSlopes = false, kCorr = false, kStruct = false,
                          kGmrf = false, kBlock = false, kMulti = false;
    IDHMC_DEV static void terms(double z, const GlmObs &o, double &r, double &v) { logistic_terms(z, o.y[0], r, v); }
};

// One chain per wavefront.  Observations in blocks of 128, lane l owning observations 128 b + 2 l, 128 b + 2 l + 1: z from
// coalesced rows of X' against q broadcast from the wavefront's LDS vector, then r is staged in that vector and g accumulates
// over the block's observations from coalesced rows of X.  X and X' stream from L2 once per gradient.
// The exchange vector is buf, the wavefront's LDS vector of L doubles.  Stages 1-3 run once per gradient and the factors and ut are held
// across the observation blocks.  b is staged in buf instead of q, again for every block because r overwrites buf[0 .. 127]; coordinates
// >= Dx are staged raw (a_j is read there).  [H] b is computed again per block rather than held.  [kLocal] q goes through buf for the
// lambdas, b is computed ONCE per gradient and held in registers across the blocks; ut is then not held: after the loop the mix and the
// scan run again from q, and st, h are computed again by the chain rule (two more vectors of registers otherwise).  [kResponses]
// bind_chain offsets the pointer to Y.  [kFactors] the z loop runs c < Dd, then adds buf[off_f + lvl] for the lane's two observations
// (the planes are read as int2, lane-offset, like y2; [kSlopes] a double2 from the value plane at the same offset, zx = dfma(w.x, bx,
// zx)); the stored-column loop touches the chunks j < Lx / 128 only -- one loop, whose stride and chunk bound are compile-time constants
// without factors --; after it each lane walks the lists of its level columns over r staged in buf[0 .. 127] (glm_gather: G + r[ii],
// [kSlopes] dfma(wl, r[ii], G)).  [kGmrf] once every chain rule has run, the raw q is staged in buf a last time and stays there for the
// prior loop: row 6 of a member reads its neighbours' u from it.  [kBlock] the block's factors and its mix take the pairs' places
// (a model has one or the other): the twelve factors are held across the blocks like the pairs' four.
// [kMulti] the z loop's level stage runs over the planes p < P instead of the terms: index and value of plane p at the lane offset, b
// from buf[poff_p + lvl], the planes' loads independent of z and of each other; the lists are walked with the planes' block size, four
// entries per trip (glm_gather's overload for GlmMulti).
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
    GlmMulti mul;            // the planes of terms with several levels per observation (Obs::kMulti)
    const int32_t *cpart;    // the partner table of the paired columns, device (Obs::kCorr)
    int cz0, ncp;            // the coordinate of zeta_0 and the pairs (Obs::kCorr)
    GlmBlock blk;            // the correlation block (Obs::kBlock)
    GlmStruct stc;           // the structured terms (Obs::kStruct)
    GlmGmrf gm;              // the GMRF terms (Obs::kGmrf)
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
        if constexpr (Obs::kMulti) {
            static_assert(Obs::kFactors && Obs::kSlopes, "every plane of a wide term reads a value");
            mul.init(s);
        }
        if constexpr (Obs::kCorr) {
            cpart = s.lr_cpart;
            ncp = s.lr_cp;
            cz0 = s.D - s.lr_cp;
            D -= s.lr_cp;
        }
        if constexpr (Obs::kBlock) {
            static_assert(!Obs::kCorr, "a model has pairs or a block");
            blk.init(s);
            D -= blk.nz;
        }
        if constexpr (Obs::kStruct) {
            stc.init(s);
            D -= s.lr_sz;
            if constexpr (Obs::kCorr) cz0 -= s.lr_sz;          // (the pairs' zetas come first)
        }
        if constexpr (Obs::kGmrf) gm.init(s);
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
        GlmBlockZ bz;                                          // Obs::kBlock: z and c of the block's zetas
        if constexpr (Obs::kBlock) {
            glm_block_factors<NCH>(q, blk, bz);
            glm_block_mix<NCH>(qm, q, blk, buf, lane, bz);
        }
        double sf0 = 1.0, sc0 = 1.0, sf1 = 1.0, sc1 = 1.0;     // Obs::kStruct: phi and c of the slots; the scan runs on qm, after the mix
        if constexpr (Obs::kStruct) {                          // (disjoint columns)
            if constexpr (!Obs::kCorr && !Obs::kBlock) qm = q;
            glm_struct_factors<NCH>(q, stc, sf0, sc0, sf1, sc1);
            glm_struct_scan<NCH>(qm, stc, buf, lane, sf0, sc0, sf1, sc1);
        }
        const Vec<NCH> &u = glm_pick<Obs::kCorr || Obs::kStruct || Obs::kBlock>(qm, q);    // what the scales and the products run on
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
            if constexpr (Obs::kMulti) {
                // the level columns by plane, terms ascending and within a term its planes ascending: every plane reads a value, and an
                // absent entry (lvl = -1, the padding too) adds nothing.  The index and the value of a plane wait for nothing but the
                // block, so the loads of four planes go out together ahead of their LDS reads.
                const int2 *lv2 = reinterpret_cast<const int2 *>(fac.idx) + lane + b * 64;
                const double2 *w2 = reinterpret_cast<const double2 *>(slo.val) + lane + b * 64;
                const int np = mul.P < 8 ? mul.P : 8;
#pragma unroll 4
                for (int p = 0; p < np; ++p) {
                    const int o = mul.poff[p];
                    const int2 lv = lv2[(size_t)p * (npad >> 1)];
                    const double2 w = w2[(size_t)p * (npad >> 1)];
                    const double bx = buf[o + (lv.x > 0 ? lv.x : 0)], by = buf[o + (lv.y > 0 ? lv.y : 0)];
                    zx = lv.x >= 0 ? dfma(w.x, bx, zx) : zx;
                    zy = lv.y >= 0 ? dfma(w.y, by, zy) : zy;
                }
            } else if constexpr (Obs::kFactors) {
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
            // the stored columns: rows of lx doubles, the chunks j < lx / 128 (all NCH of them without factors, at compile time)
            int lx = L;
            if constexpr (Obs::kFactors) lx = fac.lx;
            const double2 *xr = reinterpret_cast<const double2 *>(x + (size_t)128 * b * lx) + lane;
            const int nchx = lx >> 7, xs = lx >> 1;
#pragma unroll 2
            for (int ii = 0; ii < m; ++ii) {
                const double ri = buf[ii];                     // LDS broadcast
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    if (j < nchx) {
                        const double2 xv = xr[(size_t)ii * xs + j * 64];
                        G.c[j].x = dfma(xv.x, ri, G.c[j].x);
                        G.c[j].y = dfma(xv.y, ri, G.c[j].y);
                    }
                }
            }
            if constexpr (Obs::kFactors) {
                // then each level column's list
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    if (128 * j + 128 > fac.dd && 128 * j < D) {               // the chunk holds a level column
                        const int c0 = 128 * j + 2 * lane, e = c0 - fac.dd;
                        if constexpr (Obs::kMulti) {
                            glm_gather(G.c[j].x, mul, slo, fac, b, e, e >= 0 && c0 < D, buf);
                            glm_gather(G.c[j].y, mul, slo, fac, b, e + 1, e + 1 >= 0 && c0 + 1 < D, buf);
                        } else if constexpr (Obs::kSlopes) {
                            glm_gather(G.c[j].x, slo, fac, b, e, e >= 0 && c0 < D, buf);
                            glm_gather(G.c[j].y, slo, fac, b, e + 1, e + 1 >= 0 && c0 + 1 < D, buf);
                        } else {
                            glm_gather(G.c[j].x, fac, b, e, e >= 0 && c0 < D, buf);
                            glm_gather(G.c[j].y, fac, b, e + 1, e + 1 >= 0 && c0 + 1 < D, buf);
                        }
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
        if constexpr (Obs::kBlock && Obs::kLocal) glm_block_mix<NCH>(qm, q, blk, buf, lane, bz);
        if constexpr (Obs::kStruct && Obs::kLocal) {
            if constexpr (!Obs::kCorr && !Obs::kBlock) qm = q;
            glm_struct_scan<NCH>(qm, stc, buf, lane, sf0, sc0, sf1, sc1);
        }
        if constexpr (Obs::kLocal) glm_local_chain<NCH, Obs::H>(G, u, grp2, part, buf, D, D + Obs::A, lane, e0, e1, e2, e3, inv2);
        else if constexpr (Obs::H > 0) glm_group_chain<NCH, HN>(G, u, grp2, D + Obs::A, lane, e0, e1, e2, e3);
        if constexpr (Obs::kCorr) glm_corr_chain<NCH>(G, q, cpart, buf, cz0, ncp, lane, cr0, cc0, cr1, cc1);
        if constexpr (Obs::kBlock) glm_block_chain<NCH>(G, q, blk, buf, lane, bz);
        if constexpr (Obs::kStruct) glm_struct_chain<NCH>(G, q, u, stc, buf, lane, sf0, sc0, sf1, sc1);
        double gs0 = 0.0, gs1 = 0.0;                           // Obs::kGmrf: S of the slots; the raw q stays in buf for the loop
        if constexpr (Obs::kGmrf) {
            glm_gmrf_sums<NCH>(q, gm, lane, gs0, gs1);
#pragma unroll
            for (int j = 0; j < NCH; ++j) b2[j * 64] = q.c[j];
            asm volatile("" ::: "memory");                     // (the rows' reads stay behind the writes)
        }
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const double2 m = mu2[j * 64], t = tau2[j * 64];
            const double dx = q.c[j].x - m.x, dy = q.c[j].y - m.y;
            if constexpr (Obs::kPriors && Obs::kGmrf) {
                // (a member takes row 6, from its table entry; kind2 holds kPriorGmrf there)
                const int2 k = kind2[j * 64], ge = (reinterpret_cast<const int2 *>(gm.gpart) + lane)[j * 64];
                const double2 nu = nu2[j * 64];
                g.c[j].x = ge.x >= 0 ? glm_gmrf_row(gm, ge.x, buf, q.c[j].x, gs0, gs1, G.c[j].x, t0)
                                     : glm_prior_of<Obs::kCorr || Obs::kStruct || Obs::kBlock>(k.x, nu.x, t.x, dx, G.c[j].x, t0);
                g.c[j].y = ge.y >= 0 ? glm_gmrf_row(gm, ge.y, buf, q.c[j].y, gs0, gs1, G.c[j].y, t1)
                                     : glm_prior_of<Obs::kCorr || Obs::kStruct || Obs::kBlock>(k.y, nu.y, t.y, dy, G.c[j].y, t1);
            } else if constexpr (Obs::kPriors) {
                const int2 k = kind2[j * 64];
                const double2 nu = nu2[j * 64];
                g.c[j].x = glm_prior_of<Obs::kCorr || Obs::kStruct || Obs::kBlock>(k.x, nu.x, t.x, dx, G.c[j].x, t0);
                g.c[j].y = glm_prior_of<Obs::kCorr || Obs::kStruct || Obs::kBlock>(k.y, nu.y, t.y, dy, G.c[j].y, t1);
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
// would spill; (5) the requester reduces its row of each with wave_sum.  16.5 KB per auxiliary coordinate; which (L, A, metric)
// fit a CU is glm_coop's table (idhmc_logistic.hip).
// The transform (stages 1-4, 10-12) is the requester's work, and its exchange vector is its own Q row: before barrier A q goes
// through the row (the mix, the scan, then the lambdas read there), and b takes its place, +0 in every coordinate >= Dx -- the
// auxiliary ones, the log scales, the lambdas and the zetas take no part in Z.  After barrier C the G row is taken into registers
// with the scores placed, and the row is the requester's own again until the next barrier A: the factors, ut, st and h are all
// computed AGAIN from q through it, then wl and Gh go through it for the chain rules.  Held across the round instead, they made
// the matrix loops of multiply() spill; the coordinates they are read from are laundered through an empty asm so that the
// compiler does not keep the values of before barrier A alive.  Nothing of a feature is alive across multiply(); the prior's
// tables are read after barrier C too.  [kGmrf] the G row is taken into registers as for the chain rules, and once they have run the
// raw q goes into the row, which is the requester's own, and stays there for the prior loop: row 6 reads its neighbours' u from it.
// [kBlock] as the pairs: the factors live for the mix only before barrier A and are made again from q after barrier C.
// [kResponses] the 16 rows of a tile are 16 chains of any responses: the requester publishes its offset into Y in column L of its
// Q row (padding: zphase, gphase and both row accesses of the requester touch columns < L only) and the Z wavefronts read y per
// accumulator row instead of once per lane.
// [kFactors] the Z wavefronts run the matrix loop over the columns < 32 ceil(Dd / 32), then add Q[row][off_f + lvl_f[i]] per
// accumulator row ([kSlopes] w is read once per observation i, the same for the four rows: acc[reg] = dfma(w, bl, acc[reg])).  A
// G wavefront whose tile starts at or beyond Dd skips the matrix loop; gphase spells that loop out twice, with the run-time
// stride Lx and with the compile-time L.  A tile that holds level columns adds R[b & 1][row][i] over the column's list per lane
// ([kSlopes] gacc[reg] = dfma(wl, R[..][ii], gacc[reg])), after the block's matrix steps where the tile straddles Dd.
// [kMulti] the Z wavefronts add Q[row][poff_p + lvl_p[i]] per plane p < P, w_p[i] read once per observation; the G wavefronts walk the
// lists with the planes' block size, four entries per trip, the chain in list order.
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
    GlmMulti mul;                // the planes of terms with several levels per observation (Obs::kMulti)
    const int32_t *cpart;        // the partner table of the paired columns, device (Obs::kCorr)
    int cz0, ncp;                // the coordinate of zeta_0 and the pairs (Obs::kCorr)
    GlmBlock blk;                // the correlation block (Obs::kBlock)
    GlmStruct stc;               // the structured terms (Obs::kStruct)
    GlmGmrf gm;                  // the GMRF terms (Obs::kGmrf)
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
        if constexpr (Obs::kMulti) {
            static_assert(Obs::kFactors && Obs::kSlopes, "every plane of a wide term reads a value");
            mul.init(s);
        }
        if constexpr (Obs::kCorr) {
            cpart = s.lr_cpart;
            ncp = s.lr_cp;
            cz0 = s.D - s.lr_cp;
            dx -= s.lr_cp;
        }
        if constexpr (Obs::kBlock) {
            static_assert(!Obs::kCorr, "a model has pairs or a block");
            blk.init(s);
            dx -= blk.nz;
        }
        if constexpr (Obs::kStruct) {
            stc.init(s);
            dx -= s.lr_sz;
            if constexpr (Obs::kCorr) cz0 -= s.lr_sz;          // (the pairs' zetas come first)
        }
        if constexpr (Obs::kGmrf) gm.init(s);
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
        if constexpr (Obs::kMulti) {
            // the level columns by plane, terms ascending and within a term its planes ascending: b of observation i's level from each
            // row's Q, the observation's value the same for the four rows (an absent entry, lvl = -1, adds nothing)
            const int np = mul.P < 8 ? mul.P : 8;
#pragma unroll 4
            for (int p = 0; p < np; ++p) {
                const int lv = fac.idx[(size_t)p * npad + i];
                const double w = slo.val[(size_t)p * npad + i];
                const double *qp = tile + kQ + kk * DS + mul.poff[p] + (lv > 0 ? lv : 0);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const double bl = qp[4 * reg * DS];
                    acc[reg] = lv >= 0 ? dfma(w, bl, acc[reg]) : acc[reg];
                }
            }
        } else if constexpr (Obs::kFactors) {
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
            // (the matrix loop is spelled out a second time below with the compile-time stride L: written once with the stride chosen by
            // if constexpr, its address arithmetic came out in another order under kFactors)
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
                if constexpr (Obs::kMulti) {
                    // (the block's entries are 128 P: the list is walked with the planes' clamps, four entries at a time)
                    for (int k = 0; k < cnt; k += kListBatch) {
                        GlmListBatch q;
                        glm_list_batch(q, mul, slo, fac, b, s0 + k);
#pragma unroll
                        for (int u = 0; u < kListBatch; ++u) {
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg) gacc[reg] = k + u < cnt ? dfma(q.wl[u], rp[4 * reg * RS + q.ii[u]], gacc[reg]) : gacc[reg];
                        }
                    }
                    return;
                }
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
        if constexpr (Obs::kBlock) {                          // Obs::kBlock: z and c of the block's zetas live for the mix only
            GlmBlockZ bz;
            glm_block_factors<NCH>(q, blk, bz);
            glm_block_mix<NCH>(qm, q, blk, tile + kQ + wv * DS, lane, bz);
        }
        double sf0 = 1.0, sc0 = 1.0, sf1 = 1.0, sc1 = 1.0;    // Obs::kStruct: phi and c of the slots; the scan runs on qm through the row
        if constexpr (Obs::kStruct) {
            if constexpr (!Obs::kCorr && !Obs::kBlock) qm = q;
            glm_struct_factors<NCH>(q, stc, sf0, sc0, sf1, sc1);
            glm_struct_scan<NCH>(qm, stc, tile + kQ + wv * DS, lane, sf0, sc0, sf1, sc1);
        }
        const Vec<NCH> &u = glm_pick<Obs::kCorr || Obs::kStruct || Obs::kBlock>(qm, q);   // what the scales and the products run on
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
        } else if constexpr (Obs::A > 0 || Obs::kCorr || Obs::kStruct || Obs::kBlock) {
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
        if constexpr (Obs::H > 0 || Obs::kLocal || Obs::kCorr || Obs::kStruct || Obs::kGmrf || Obs::kBlock) {
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
            // (a block: z, c and ut again from q, through the row, as the pairs above)
            GlmBlock bk2;
            GlmBlockZ bz;
            if constexpr (Obs::kBlock) {
                bk2 = blk;
                asm volatile("" : "+s"(bk2.cz0));
                glm_block_factors<NCH>(q, bk2, bz);
                glm_block_mix<NCH>(qm, q, bk2, tile + kQ + wv * DS, lane, bz);
            }
            // (structured terms: phi, c and the forward scan again from q, through the row, as the pairs above)
            GlmStruct st2;
            if constexpr (Obs::kStruct) {
                st2 = stc;
                asm volatile("" : "+s"(st2.cz0), "+s"(st2.cz1));
                if constexpr (!Obs::kCorr && !Obs::kBlock) qm = q;
                glm_struct_factors<NCH>(q, st2, sf0, sc0, sf1, sc1);
                glm_struct_scan<NCH>(qm, st2, tile + kQ + wv * DS, lane, sf0, sc0, sf1, sc1);
            }
            // (local scales: the G row is in registers now, so q and then wl go through the row, which is the requester's own until barrier A)
            if constexpr (Obs::kLocal) glm_local_chain<NCH, Obs::H>(Gh, u, grp2, part, tile + kQ + wv * DS, dx, c0, lane, e0, e1, e2, e3, inv2);
            else if constexpr (Obs::H > 0) glm_group_chain<NCH, HN>(Gh, u, grp2, c0, lane, e0, e1, e2, e3);
            if constexpr (Obs::kCorr) glm_corr_chain<NCH>(Gh, q, cpart, tile + kQ + wv * DS, cz, ncp, lane, cr0, cc0, cr1, cc1);
            if constexpr (Obs::kBlock) glm_block_chain<NCH>(Gh, q, bk2, tile + kQ + wv * DS, lane, bz);
            if constexpr (Obs::kStruct) glm_struct_chain<NCH>(Gh, q, u, st2, tile + kQ + wv * DS, lane, sf0, sc0, sf1, sc1);
        }
        double gs0 = 0.0, gs1 = 0.0;                          // Obs::kGmrf: S of the slots; the raw q stays in the row for the loop
        if constexpr (Obs::kGmrf) {
            glm_gmrf_sums<NCH>(q, gm, lane, gs0, gs1);
#pragma unroll
            for (int j = 0; j < NCH; ++j) row[j * 64] = q.c[j];
            asm volatile("" ::: "memory");                    // (the rows' reads stay behind the writes)
        }
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const double2 m = mu2[j * 64], t = tau2[j * 64];
            double2 G;
            if constexpr (Obs::H > 0 || Obs::kLocal || Obs::kCorr || Obs::kStruct || Obs::kGmrf || Obs::kBlock) {
                G = Gh.c[j];
            } else {
                G = row[j * 64];
                if constexpr (Obs::A > 0) {
#pragma unroll
                    for (int jx = 0; jx < AN; ++jx) glm_place(G, j, dx + jx, lane, S[jx]);
                }
            }
            const double dx = q.c[j].x - m.x, dy = q.c[j].y - m.y;
            if constexpr (Obs::kPriors && Obs::kGmrf) {
                // (a member takes row 6, from its table entry; kind2 holds kPriorGmrf there)
                const int2 k = kind2[j * 64], ge = (reinterpret_cast<const int2 *>(gm.gpart) + lane)[j * 64];
                const double2 nu = nu2[j * 64];
                g.c[j].x = ge.x >= 0 ? glm_gmrf_row(gm, ge.x, tile + kQ + wv * DS, q.c[j].x, gs0, gs1, G.x, t0)
                                     : glm_prior_of<Obs::kCorr || Obs::kStruct || Obs::kBlock>(k.x, nu.x, t.x, dx, G.x, t0);
                g.c[j].y = ge.y >= 0 ? glm_gmrf_row(gm, ge.y, tile + kQ + wv * DS, q.c[j].y, gs0, gs1, G.y, t1)
                                     : glm_prior_of<Obs::kCorr || Obs::kStruct || Obs::kBlock>(k.y, nu.y, t.y, dy, G.y, t1);
            } else if constexpr (Obs::kPriors) {
                // kinds and nu are read here, after barrier C: nothing of the prior is alive across multiply()
                const int2 k = kind2[j * 64];
                const double2 nu = nu2[j * 64];
                g.c[j].x = glm_prior_of<Obs::kCorr || Obs::kStruct || Obs::kBlock>(k.x, nu.x, t.x, dx, G.x, t0);
                g.c[j].y = glm_prior_of<Obs::kCorr || Obs::kStruct || Obs::kBlock>(k.y, nu.y, t.y, dy, G.y, t1);
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
