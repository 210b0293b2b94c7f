// members_check.cpp -- the host side of the level lists (inplacedhmc.jl_amd/csrc/idhmc_members.hpp: check_members and build_level_lists)
// as a stand-alone program, so that it runs under the host sanitizers without a device and without Python:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinplacedhmc.jl_amd/csrc tools/members_check.cpp -o members_check && ./members_check
// It builds the lists for the shapes the device tests use -- n in {1, 128, 130}, widths (4, 4), (4, 2, 1, 1) and (3,), a level nobody has,
// a level that holds a whole block through two planes, observations with 0, 1 and M entries -- checks every list against a direct
// scan, and hands check_members tables it must refuse.  Exit status 0 and "members_check ok" when all holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include "idhmc_members.hpp"

using namespace idhmc;

static int failures = 0;
#define EXPECT(c)                                                                  \
    do {                                                                           \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

struct Table {
    int F;
    std::vector<int32_t> levels, width, index;   // index, values: P x n
    std::vector<double> values;
    int64_t n;
    int P;
};

// a valid table: per observation and term a random number of present entries (0 .. M; a term of width 1 always 1), levels ascending
static Table make(int64_t n, std::vector<int32_t> width, std::vector<int32_t> levels, unsigned seed, int special)
{
    Table t;
    t.F = (int)width.size();
    t.width = width;
    t.levels = levels;
    t.n = n;
    t.P = 0;
    for (int w : width) t.P += w;
    t.index.assign((size_t)(t.P * n), -1);
    t.values.assign((size_t)(t.P * n), 0.0);
    std::mt19937 rng(seed);
    for (int f = 0, p0 = 0; f < t.F; p0 += width[f], ++f)
        for (int64_t i = 0; i < n; ++i) {
            const int M = width[f], N = levels[f];
            int cnt = M == 1 ? 1 : (int)(rng() % (unsigned)(M + 1));
            if (cnt > N - 1) cnt = N - 1 > 0 ? N - 1 : (M == 1 ? 1 : 0);      // (the last level stays empty: a level nobody has)
            if (M == 1 && N == 1) cnt = 1;
            // cnt distinct levels of 0 .. N-2 (N-1 when N = 1), ascending
            std::vector<int32_t> pick;
            const int top = N > 1 ? N - 1 : 1;
            for (int k = 0; k < top && (int)pick.size() < cnt; ++k)
                if ((int)(rng() % (unsigned)(top - k)) < cnt - (int)pick.size()) pick.push_back(k);
            if (special == 1 && f == 0 && M >= 2) {
                // level 1 holds every observation: even ones by plane 0, odd ones by plane 1 (behind level 0)
                pick.clear();
                if (i & 1) pick.push_back(0);
                pick.push_back(1);
            }
            for (size_t m = 0; m < pick.size(); ++m) {
                t.index[(size_t)((p0 + (int)m) * n + i)] = pick[m];
                t.values[(size_t)((p0 + (int)m) * n + i)] = (rng() % 5 == 0) ? 0.0 : (double)((int)(rng() % 17) - 8) / 4.0;
            }
        }
    return t;
}

static void check_lists(const Table &t, bool with_values)
{
    char msg[320];
    int P = 0;
    bool wide = false;
    EXPECT(check_members(t.F, t.levels.data(), t.n, t.width.data(), t.index.data(), with_values ? t.values.data() : nullptr, &P, &wide, msg, sizeof msg));
    EXPECT(P == t.P);
    Planes pl;
    for (int f = 0; f < t.F; ++f)
        for (int m = 0; m < t.width[f]; ++m, ++pl.P) {
            pl.term[pl.P] = f;
            pl.idx[pl.P] = t.index.data() + (int64_t)pl.P * t.n;
            pl.val[pl.P] = with_values ? t.values.data() + (int64_t)pl.P * t.n : nullptr;
        }
    LevelLists ll;
    build_level_lists(pl, t.F, t.levels.data(), t.n, true, kMaxPlanes, &ll);
    const int64_t npad = (t.n + 127) / 128 * 128, nb = npad / 128;
    int64_t cols = 0;
    for (int32_t N : t.levels) cols += N;
    EXPECT((int64_t)ll.fidx.size() == P * npad && (int64_t)ll.fpos.size() == nb * 128 * P && (int64_t)ll.fwl.size() == nb * 128 * P);
    EXPECT((int64_t)ll.fstart.size() == nb * (cols + 1) + kMaxPlanes);
    for (int64_t b = 0; b < nb; ++b) {
        const int32_t *st = &ll.fstart[(size_t)(b * (cols + 1))];
        EXPECT(st[0] == 0 && st[cols] <= 128 * P);
        int64_t e = 0;
        for (int f = 0, p0 = 0; f < t.F; p0 += t.width[f], ++f)
            for (int32_t k = 0; k < t.levels[f]; ++k, ++e) {
                // the list of level k of term f against a direct scan: places ascending, the value of the plane that names the level
                int32_t at = st[e];
                EXPECT(st[e + 1] - st[e] <= 128);
                for (int64_t ii = 0; ii < 128 && 128 * b + ii < t.n; ++ii)
                    for (int m = 0; m < t.width[f]; ++m) {
                        const int64_t g = (int64_t)(p0 + m) * t.n + 128 * b + ii;
                        if (t.index[(size_t)g] != k) continue;
                        EXPECT(at < st[e + 1]);
                        if (at >= st[e + 1]) continue;
                        EXPECT(ll.fpos[(size_t)(b * 128 * P + at)] == ii);
                        EXPECT(ll.fwl[(size_t)(b * 128 * P + at)] == (with_values ? t.values[(size_t)g] : 1.0));
                        ++at;
                    }
                EXPECT(at == st[e + 1]);
            }
    }
    for (int p = 0; p < P; ++p)
        for (int64_t i = 0; i < npad; ++i) {
            const int32_t want = i < t.n ? t.index[(size_t)(p * t.n + i)] : -1;
            EXPECT(ll.fidx[(size_t)(p * npad + i)] == want);
            EXPECT(ll.fval[(size_t)(p * npad + i)] == (want < 0 ? 0.0 : with_values ? t.values[(size_t)(p * t.n + i)] : 1.0));
        }
}

static void refused(Table t, const char *what, int p, int64_t i, int32_t v, double val = 1.0)
{
    char msg[320] = "";
    int P = 0;
    bool wide = false;
    if (p >= 0) {
        t.index[(size_t)(p * t.n + i)] = v;
        t.values[(size_t)(p * t.n + i)] = val;
    }
    const bool ok = check_members(t.F, t.levels.data(), t.n, t.width.data(), t.index.data(), t.values.data(), &P, &wide, msg, sizeof msg);
    EXPECT(!ok);
    EXPECT(strstr(msg, what) != nullptr);
    if (ok || !strstr(msg, what)) printf("  wanted \"%s\", got \"%s\"\n", what, msg);
}

int main()
{
    const std::vector<std::vector<int32_t>> widths = {{4, 4}, {4, 2, 1, 1}, {3}};
    const std::vector<std::vector<int32_t>> levels = {{7, 130}, {9, 3, 5, 1}, {24}};
    unsigned seed = 1;
    for (int64_t n : {1, 128, 130})
        for (size_t w = 0; w < widths.size(); ++w)
            for (int special : {0, 1})
                for (bool with_values : {true, false}) check_lists(make(n, widths[w], levels[w], seed++, special), with_values);
    // tables the validation must refuse, each naming term, plane and observation
    Table t = make(130, {4, 2, 1, 1}, {9, 3, 5, 1}, 99, 1);
    refused(t, "term 0, plane 1, observation 129: level 9 is outside -1..8", 1, 129, 9);
    refused(t, "term 0, plane 0, observation 0: level -2 is outside -1..8", 0, 0, -2);
    refused(t, "term 1, plane 4, observation 7: level 1000000 is outside -1..2", 4, 7, 1000000);
    refused(t, "term 2, plane 6, observation 128: an absent entry (-1) in a term of width 1", 6, 128, -1);
    refused(t, "term 0, plane 1, observation 5: a present entry (level 1) behind an absent one", 0, 5, -1);
    refused(t, "term 0, plane 1, observation 5: level 0 after level 0", 1, 5, 0);
    refused(t, "term 0, plane 1, observation 5: the value is not finite", 1, 5, 1, std::nan(""));
    Table u = t;
    u.width[0] = 5;
    refused(u, "width[0] = 5 of term 0 must be in 1..4", -1, 0, 0);
    u.width = {4, 4, 1, 1};
    refused(u, "the widths sum to P = 10 planes", -1, 0, 0);
    if (failures) {
        printf("members_check: %d failures\n", failures);
        return 1;
    }
    printf("members_check ok\n");
    return 0;
}
