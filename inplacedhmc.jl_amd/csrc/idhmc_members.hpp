// idhmc_members.hpp -- the host side of the factor terms' level lists (DESIGN sections 20, 21, 27): the check of a table of members
// (idhmc_create_glm_multi) and the counting sort that lays the index planes, the value planes and the blocks' lists out for the device.
// Plain C++ with no device call, so that tools/members_check.cpp can run both under the host sanitizers; idhmc_create.hip is their
// one user in the library.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace idhmc {

constexpr int kMaxPlanes = 8;      // sum of the terms' widths
constexpr int kMaxWidth = 4;       // levels an observation has in one term

// The planes of a model's factor terms in the device's order: the planes of term 0 first.  A plain term is one plane.
struct Planes {
    int P = 0;
    int32_t term[kMaxPlanes] = {};              // the term plane p belongs to, ascending
    const int32_t *idx[kMaxPlanes] = {};        // [n] levels, -1: absent
    const double *val[kMaxPlanes] = {};         // [n] values, or null: 1.0 on every present entry
};
// what upload_regression copies to the device (the names are DevState's)
struct LevelLists {
    std::vector<int32_t> fidx;         // [P][n_pad], -1 in the padding
    std::vector<int32_t> fstart;       // [n_pad / 128][cols + 1], then `tail` more entries left 0 for the caller
    std::vector<unsigned char> fpos;   // [n_pad / 128][128 P]
    std::vector<double> fval, fwl;     // [P][n_pad] (0.0 where absent) and [n_pad / 128][128 P]; empty without values
};

// Every check of idhmc_glm_members against the terms' levels: widths, the plane limit, and per entry the level's range, absent entries
// last, levels strictly ascending within an observation, a finite value on a present entry.  Returns false with the message in msg.
// *planes: sum of the widths;  *wide: some term has a width > 1 (false: the table is F plain index rows).
inline bool check_members(int F, const int32_t *levels, int64_t n, const int32_t *width, const int32_t *index, const double *values,
                          int *planes, bool *wide, char *msg, size_t cap)
{
    *planes = 0;
    *wide = false;
    if (!width || !index) {
        snprintf(msg, cap, "GLM: members need width and index (%s is NULL)", width ? "index" : "width");
        return false;
    }
    int P = 0;
    for (int f = 0; f < F; ++f) {
        if (width[f] < 1 || width[f] > kMaxWidth) {
            snprintf(msg, cap, "GLM: members: width[%d] = %d of term %d must be in 1..%d", f, width[f], f, kMaxWidth);
            return false;
        }
        P += width[f];
        if (width[f] > 1) *wide = true;
    }
    if (P > kMaxPlanes) {
        snprintf(msg, cap, "GLM: members: the widths sum to P = %d planes: at most %d", P, kMaxPlanes);
        return false;
    }
    for (int f = 0, p0 = 0; f < F; p0 += width[f], ++f)
        for (int64_t i = 0; i < n; ++i) {
            int32_t prev = -1;
            bool absent = false;
            for (int m = 0; m < width[f]; ++m) {
                const int p = p0 + m;
                const int32_t v = index[(int64_t)p * n + i];
                if (v < -1 || v >= levels[f]) {
                    snprintf(msg, cap, "GLM: members: term %d, plane %d, observation %lld: level %d is outside -1..%d", f, p, (long long)i, v, levels[f] - 1);
                    return false;
                }
                if (v < 0) {
                    if (width[f] == 1) {
                        snprintf(msg, cap, "GLM: members: term %d, plane %d, observation %lld: an absent entry (-1) in a term of width 1", f, p, (long long)i);
                        return false;
                    }
                    absent = true;
                    continue;
                }
                if (absent) {
                    snprintf(msg, cap, "GLM: members: term %d, plane %d, observation %lld: a present entry (level %d) behind an absent one", f, p, (long long)i, v);
                    return false;
                }
                if (v <= prev) {
                    snprintf(msg, cap, "GLM: members: term %d, plane %d, observation %lld: level %d after level %d: the levels of an observation "
                             "must be strictly ascending", f, p, (long long)i, v, prev);
                    return false;
                }
                prev = v;
                if (values && !std::isfinite(values[(int64_t)p * n + i])) {
                    snprintf(msg, cap, "GLM: members: term %d, plane %d, observation %lld: the value is not finite", f, p, (long long)i);
                    return false;
                }
            }
        }
    *planes = P;
    return true;
}

// The device layout of the planes: the index (and value) planes zero-padded to n_pad, and per block of 128 observations the level lists
// -- a counting sort by term, level, place: every present entry of every plane of a term goes into that term's lists, places ascending
// within a level (an observation's levels in a term are distinct, so a list holds a place once and at most 128 entries), the entry's
// value into fwl at the same position.  Levels must have passed check_members or validate_factors: -1 .. N_f-1.
inline void build_level_lists(const Planes &pl, int F, const int32_t *levels, int64_t n, bool with_values, int tail, LevelLists *out)
{
    const int64_t npad = (n + 127) / 128 * 128, nb = npad / 128, P = pl.P;
    int64_t off[5] = {0, 0, 0, 0, 0};                       // the first list of term f (cumulative levels)
    for (int f = 0; f < F; ++f) off[f + 1] = off[f] + levels[f];
    const int64_t cols = off[F];
    out->fidx.assign((size_t)(P * npad), -1);
    out->fstart.assign((size_t)(nb * (cols + 1) + tail), 0);
    out->fpos.assign((size_t)(nb * 128 * P), 0);
    out->fval.clear();
    out->fwl.clear();
    if (with_values) {
        out->fval.assign((size_t)(P * npad), 0.0);
        out->fwl.assign((size_t)(nb * 128 * P), 0.0);
    }
    for (int64_t p = 0; p < P; ++p)
        for (int64_t i = 0; i < n; ++i) {
            const int32_t v = pl.idx[p][i];
            out->fidx[(size_t)(p * npad + i)] = v;
            if (with_values && v >= 0) out->fval[(size_t)(p * npad + i)] = pl.val[p] ? pl.val[p][i] : 1.0;
        }
    std::vector<int32_t> cur((size_t)cols, 0);
    for (int64_t b = 0; b < nb; ++b) {
        int32_t *st = &out->fstart[(size_t)(b * (cols + 1))];
        const int64_t m = n - 128 * b < 128 ? n - 128 * b : 128;
        for (int64_t p = 0; p < P; ++p)
            for (int64_t ii = 0; ii < m; ++ii) {
                const int32_t v = pl.idx[p][128 * b + ii];
                if (v >= 0) ++st[off[pl.term[p]] + v + 1];
            }
        for (int64_t e = 0; e < cols; ++e) { st[e + 1] += st[e]; cur[(size_t)e] = st[e]; }
        // places ascending within a level: the place is the outer loop of a term, its planes the inner one
        for (int64_t p0 = 0; p0 < P;) {
            int64_t p1 = p0;
            while (p1 < P && pl.term[p1] == pl.term[p0]) ++p1;
            for (int64_t ii = 0; ii < m; ++ii)
                for (int64_t p = p0; p < p1; ++p) {
                    const int32_t v = pl.idx[p][128 * b + ii];
                    if (v < 0) continue;
                    const int64_t t = b * 128 * P + cur[(size_t)(off[pl.term[p0]] + v)]++;
                    out->fpos[(size_t)t] = (unsigned char)ii;
                    if (with_values) out->fwl[(size_t)t] = out->fval[(size_t)(p * npad + 128 * b + ii)];
                }
            p0 = p1;
        }
    }
}

}  // namespace idhmc
