// idhmc_place.hip -- where the state arrays of a context go (place_state, called once from context creation).
#include "idhmc_host.hpp"

// The state arrays q, p, grad l (and a per-chain M^-1): what the single-step leapfrog streams, element i of each at the same time.
// Where the allocator puts them decides how their streams fall on the HBM channels: the same kernel runs at 5.65 to 6.38 TB/s
// depending on nothing else (profiles/r02_state_layout.log; alternating between successive contexts of one process).  So large
// contexts try a few placements -- every candidate set stays allocated while the next one is made, which is what moves it --
// time the access pattern on each (k_placement_probe, ~0.5 ms per launch at configs[1]) and keep the fastest.
// What "good" means is measured in the same call, not assumed: one array alone streams at the same rate in good and bad
// placements (5.0-5.1 TB/s on MI355X), a good set of nvec arrays together 13-17 % above that, a bad one 0-3 % -- a candidate
// is taken at once when it reaches kGoodRatio x the single-array rate; otherwise the best of the candidates tried wins.
// Bounds (round 3): every exit path frees what it does not keep (CandidateSets below); the bytes held at any one time stay below
// IDHMC_PLACEMENT_MAX_BYTES (default 16 GiB) and a quarter of the free memory, the kept set included; at most
// IDHMC_PLACEMENT_TRIES candidates (default 32, at most 48, 1 = take what comes); no candidate starts after kSearchMs of the call.  The wall time and the peak are reported by
// idhmc_placement_cost.  IDHMC_PLACEMENT_VERBOSE=1 prints the candidates.
// Candidates: the pair walk below, then ordinary sets of nvec hipMallocs (DESIGN.md 2 has the kinds tried before and why they went).
namespace {
constexpr int kMaxTries = 48;
constexpr double kGoodRatio = 1.10;
// no new candidate set after this much wall time of place_state (the pair walk included).  After a pair walk that found nothing, every
// candidate of the walk over whole sets took 0.1-0.25 s (alone the same walk tries 8-12 in 30-50 ms): idhmc_create took 0.4-2.6 s with
// 1-9 candidates, 0.55-0.62 s with this bound, every set kept at 1.13-1.18 x one array alone either way
constexpr double kSearchMs = 500.0;
// the candidate sets of one place_state call; whatever is still here when the call returns -- on any path -- is freed
struct CandidateSets {
    double *arr[kMaxTries][4] = {};
    float ms[kMaxTries] = {};
    int64_t held[kMaxTries] = {};        // device bytes the set occupies
    int n = 0;
    int64_t held_now = 0, held_peak = 0;
    void drop(int t, int nvec)
    {
        for (int k = 0; k < nvec; ++k) if (arr[t][k]) (void)hipFree(arr[t][k]);
        for (int k = 0; k < 4; ++k) arr[t][k] = nullptr;
        held_now -= held[t];
        held[t] = 0;
    }
    int nvec_ = 0;
    ~CandidateSets() { for (int t = 0; t < n; ++t) if (held[t]) drop(t, nvec_); }
};
// what the phases of one place_state call share
struct Search {
    idhmc_ctx *c;
    double **out;
    int nvec;
    int64_t C;
    int L;
    std::chrono::steady_clock::time_point t_begin;
    size_t bytes;                        // of one array
    int64_t set_bytes;
    int tries;
    bool verbose;
    double single_Bps = 0.0;             // one array alone, measured on the first candidate
    int best = -1;
    double elapsed_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); }
    bool pair_walk();
    int set_walk(CandidateSets &cs, int64_t budget);
    int choose_pair(CandidateSets &cs);
};
// bytes per second of a probe that took `ms` over `narrays` arrays of `bytes` each (4 launches, every element read and written)
double probe_rate(int narrays, size_t bytes, float ms) { return 2.0 * narrays * (double)bytes * 4 / (ms * 1e-3); }
// a byte budget, never more than 1 / `part` of the free memory
int64_t clamp_to_free(int64_t budget, int part)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (int64_t)(free_b / part) < budget) budget = (int64_t)(free_b / part);
    return budget;
}
}  // namespace
static int probe_ms(idhmc_ctx *c, double *const *v, int nvec, int64_t C, int L, float *ms)
{
    HIPCHK(launch_placement_probe(v, nvec, C, L, c->stream));           // warm-up (TLB, clocks)
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    for (int r = 0; r < 4; ++r) HIPCHK(launch_placement_probe(v, nvec, C, L, c->stream));
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev1));
    HIPCHK(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return IDHMC_OK;
}
// (P) first of all, the PAIR WALK.  Round 3, last measurements (profiles/r03_state_layout.log, tools/ubench/placement_*.hip): whether
// arrays stream well together is not a matter of their offsets (no offset inside one allocation changes anything) nor of how their
// physical chunks are ordered (an array of mapped chunks pairs the same in any order): arrays fall into two CLASSES by where in
// HBM their memory lies, two arrays of different classes stream at 1.12-1.17 x one array alone, two of the same class at 0.97-1.02 x,
// a set is good exactly when it mixes the classes -- and the class changes in RUNS along the order in which the allocator hands
// memory out: consecutive hipMallocs share it for anything from 2 to over 100 GiB.  On a device in such a stretch 28 consecutive
// candidate sets inside the 16 GiB budget were all bad (1.165e8 leapfrog-steps/s instead of 1.30e8).  So: one reference array,
// then single arrays further and further along -- spacers of growing size are held in between, untouched -- each probed as a PAIR
// with the reference until one of the other class turns up; the set is the reference, that partner and the rejected ones.
// Bounded by IDHMC_PLACEMENT_WALK_BYTES (default 64 GiB, never more than half of the free memory; with 128 GiB one walk that found nothing took 4 s, with 64 GiB 33 ms) and by
// 250 ms of wall time held at one time, all of it
// given back before the call returns.  IDHMC_PLACEMENT_PAIRS=0 goes straight to the walk over whole sets below.
// True when it placed the set (the context's record is then complete).
bool Search::pair_walk()
{
    const int64_t walk_budget = clamp_to_free(c->place.walk_bytes, 2);
    if (!(tries > 1 && c->place.pairs && walk_budget >= 2 * set_bytes)) return false;
    std::vector<void *> spacer_blocks;
    std::vector<double *> same;             // arrays of the reference's class, in the order found
    std::vector<double *> other;            // arrays of the other class
    double *ref = nullptr;
    int64_t held = 0, peak = 0;
    int steps = 0;
    double one = 0.0;
    auto give_back = [&]() {
        (void)hipStreamSynchronize(c->stream);
        for (void *p : spacer_blocks) (void)hipFree(p);
        for (double *p : same) (void)hipFree(p);
        for (double *p : other) (void)hipFree(p);
        if (ref) (void)hipFree(ref);
        spacer_blocks.clear(); same.clear(); other.clear(); ref = nullptr;
    };
    auto take = [&](size_t nbytes, bool touch) -> void * {
        void *p = nullptr;
        if (held + (int64_t)nbytes > walk_budget || hipMalloc(&p, nbytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (touch && hipMemsetAsync(p, 0, nbytes, c->stream) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); return nullptr; }
        held += (int64_t)nbytes;
        if (held > peak) peak = held;
        return p;
    };
    bool ok = (ref = (double *)take(bytes, true)) != nullptr;
    if (ok) {
        float ms1 = 0.f;
        double *v1[1] = {ref};
        ok = probe_ms(c, v1, 1, C, L, &ms1) == IDHMC_OK && ms1 > 0.f;
        if (ok) one = probe_rate(1, bytes, ms1);
    }
    const int need_other = nvec >= 4 ? 2 : 1, max_steps = tries > 40 ? 40 : tries;
    int64_t jump = 0;
    while (ok && (int)other.size() < need_other && steps < max_steps && elapsed_ms() < 250.0) {
        if (jump > 0) {
            void *sp = take((size_t)jump, false);
            if (!sp) break;
            spacer_blocks.push_back(sp);
        }
        double *x = (double *)take(bytes, true);
        if (!x) break;
        float ms2 = 0.f;
        double *v2[2] = {ref, x};
        if (probe_ms(c, v2, 2, C, L, &ms2) != IDHMC_OK || !(ms2 > 0.f)) { (void)hipFree(x); ok = false; break; }
        const double r2 = probe_rate(2, bytes, ms2);
        ++steps;
        if (verbose) fprintf(stderr, "idhmc placement pair walk step %d (%.1f GiB held): %.1f GB/s = %.3f x one array alone (%.1f GB/s) at %p\n", steps,
                             held / 1073741824.0, r2 / 1e9, r2 / one, one / 1e9, (void *)x);
        if (r2 >= kGoodRatio * one) other.push_back(x); else same.push_back(x);
        // further along every time nothing turned up: 0, 0, 1, 2, 4, 8, 16, 16, ... GiB of untouched memory in between
        if (other.empty()) jump = steps < 2 ? 0 : (jump == 0 ? ((int64_t)1 << 30) : (jump < ((int64_t)16 << 30) ? jump * 2 : jump));
        else jump = 0;
    }
    if (ok && !other.empty()) {
        // q: the reference; p: the partner; grad: one of the reference's class (a rejected one, else new); a per-chain M^-1: the other class.
        // Invariant (both walks): out[0], out[1] -- q and p -- are a pair of DIFFERENT classes, because the default single-step
        // sweep streams those two alone (IDHMC_GRAD_RECOMPUTE) and a same-class pair runs at the rate of one array
        double *setv[4] = {ref, other[0], nullptr, nullptr};
        auto pick = [&](std::vector<double *> &from) -> double * {
            if (!from.empty()) { double *p = from.back(); from.pop_back(); return p; }
            return (double *)take(bytes, true);
        };
        other.erase(other.begin());
        if (nvec >= 3) setv[2] = pick(same);
        if (nvec >= 4) setv[3] = pick(other.empty() ? same : other);
        bool have = true;
        for (int k = 0; k < nvec; ++k) have = have && setv[k] != nullptr;
        float msn = 0.f;
        if (have && probe_ms(c, setv, nvec, C, L, &msn) == IDHMC_OK && msn > 0.f && probe_rate(nvec, bytes, msn) >= kGoodRatio * one) {
            ref = nullptr;                                  // kept: not given back
            for (int k = 0; k < nvec; ++k) { out[k] = setv[k]; c->allocs.push_back(setv[k]); }
            give_back();
            c->bytes += set_bytes;
            c->placement_kind = 3;
            c->placement_GBps = probe_rate(nvec, bytes, msn) / 1e9;
            c->placement_tries = steps;
            c->placement_single_GBps = one / 1e9;
            c->placement_peak_bytes = peak;
            c->placement_ms = elapsed_ms();
            if (verbose) fprintf(stderr, "idhmc placement pair walk: set of %d at %.1f GB/s = %.3f x one array alone after %d steps, %.1f GiB held at most\n", nvec,
                                 c->placement_GBps, c->placement_GBps * 1e9 / one, steps, peak / 1073741824.0);
            return true;
        }
        for (int k = 1; k < nvec; ++k) if (setv[k]) spacer_blocks.push_back(setv[k]);      // (given back with the rest)
    }
    give_back();
    return false;
}
// the walk over whole sets: candidates of nvec ordinary hipMallocs, `best` the one to keep (-1: none)
int Search::set_walk(CandidateSets &cs, int64_t budget)
{
    for (int t = 0; t < tries; ++t) {
        if (t > 0 && cs.held_now + set_bytes > budget) break;       // the budget is what bounds the walk ...
        if (t > 0 && elapsed_ms() >= kSearchMs) break;   // ... and the clock
        bool ok = true;
        for (int k = 0; k < nvec && ok; ++k) {
            void *p = nullptr;
            ok = hipMalloc(&p, bytes) == hipSuccess && hipMemsetAsync(p, 0, bytes, c->stream) == hipSuccess;
            cs.arr[t][k] = (double *)p;
        }
        cs.held[t] = set_bytes;
        if (!ok) {                                    // out of memory: what we have is what we get
            (void)hipGetLastError();
            cs.n = t + 1;
            cs.held_now += cs.held[t];
            cs.drop(t, nvec);
            cs.n = t;
            if (best < 0) return fail(IDHMC_ERR_ALLOC, "hipMalloc(%zu bytes) failed for the chain state", bytes);
            break;
        }
        cs.n = t + 1;
        cs.held_now += cs.held[t];
        if (cs.held_now > cs.held_peak) cs.held_peak = cs.held_now;
        if (tries == 1) { best = t; break; }
        if (single_Bps == 0.0) {
            float ms1 = 0.f;
            if (int rc = probe_ms(c, cs.arr[t], 1, C, L, &ms1)) return rc;
            single_Bps = probe_rate(1, bytes, ms1);
        }
        if (int rc = probe_ms(c, cs.arr[t], nvec, C, L, &cs.ms[t])) return rc;
        const double rate = probe_rate(nvec, bytes, cs.ms[t]);
        if (verbose) {
            fprintf(stderr, "idhmc placement candidate %d (sets): %.1f GB/s = %.3f x one array alone (%.1f GB/s), holding %.2f GiB  at", t,
                    rate / 1e9, rate / single_Bps, single_Bps / 1e9, cs.held_now / 1073741824.0);
            for (int k = 0; k < nvec; ++k) fprintf(stderr, " %p", (void *)cs.arr[t][k]);
            fprintf(stderr, "\n");
        }
        if (best < 0 || cs.ms[t] < cs.ms[best]) best = t;
        if (rate >= kGoodRatio * single_Bps) { best = t; break; }      // a good one: stop looking
        // a candidate that is not the best so far only has to keep the allocator from handing the same memory out again: one of its
        // arrays (a spacer) does that (the next set then pairs the two freed blocks with a new one) -- three times as many candidates
        // inside the same byte budget.  Measured after allocator churn (profiles/r03_state_layout.log): 6 of 6 contexts found a good
        // placement (3 to 16 candidates, <= 10 GiB held) where whole sets, as rounds 2-3 held them, ran out of the 16 GiB budget after
        // 10 candidates in 2 of 6
        for (int u = 0; u <= t; ++u) {
            if (u == best || !cs.held[u] || cs.held[u] <= (int64_t)bytes) continue;
            for (int k = 1; k < nvec; ++k) if (cs.arr[u][k]) { (void)hipFree(cs.arr[u][k]); cs.arr[u][k] = nullptr; }
            cs.held_now -= cs.held[u] - (int64_t)bytes;
            cs.held[u] = (int64_t)bytes;
        }
    }
    if (best < 0) return fail(IDHMC_ERR_ALLOC, "no placement for the chain state (%zu bytes per array)", bytes);
    for (int t = 0; t < cs.n; ++t) if (t != best && cs.held[t]) cs.drop(t, nvec);
    return IDHMC_OK;
}
// (R) the set to keep is known; which of its arrays become q and p is not indifferent: the default single-step sweep streams q and p
// alone, and a mixed set of three holds one pair of the same class (0.97-1.02 x one array alone) and two pairs of different classes.
// Allocation order may make q, p the same-class pair, so the three pairs are probed (3 x 5 launches) and the fastest becomes out[0],
// out[1], the remaining array grad l; a per-chain M^-1 keeps its slot.  Only pointers the holder owns are permuted.
int Search::choose_pair(CandidateSets &cs)
{
    if (nvec >= 3 && cs.ms[best] > 0.f) {
        static const int kPair[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};
        float pms[3] = {0.f, 0.f, 0.f};
        int fastest = 0;
        for (int i = 0; i < 3; ++i) {
            double *v2[2] = {cs.arr[best][kPair[i][0]], cs.arr[best][kPair[i][1]]};
            if (int rc = probe_ms(c, v2, 2, C, L, &pms[i])) return rc;       // (the holder frees every set, this one included)
            if (pms[i] < pms[fastest]) fastest = i;
        }
        double *const a[3] = {cs.arr[best][kPair[fastest][0]], cs.arr[best][kPair[fastest][1]], cs.arr[best][kPair[fastest][2]]};
        if (verbose) {
            fprintf(stderr, "idhmc placement pairs of the kept set: (0,1) %.1f (0,2) %.1f (1,2) %.1f GB/s, one array alone %.1f GB/s: q, p = arrays %d, %d, grad = array %d\n",
                    probe_rate(2, bytes, pms[0]) / 1e9, probe_rate(2, bytes, pms[1]) / 1e9, probe_rate(2, bytes, pms[2]) / 1e9, single_Bps / 1e9,
                    kPair[fastest][0], kPair[fastest][1], kPair[fastest][2]);
        }
        for (int k = 0; k < 3; ++k) cs.arr[best][k] = a[k];
    }
    return IDHMC_OK;
}
int idhmc::place_state(idhmc_ctx *c, double **out, int nvec, int64_t n, int64_t C, int L)
{
    Search S{c, out, nvec, C, L, std::chrono::steady_clock::now(), (size_t)n * sizeof(double), 0, c->place.tries, c->place.verbose};
    S.set_bytes = (int64_t)nvec * (int64_t)S.bytes;
    if (S.bytes < ((size_t)64 << 20)) S.tries = 1;       // small arrays: latency, not channels
    if (S.tries > kMaxTries) S.tries = kMaxTries;
    if (S.tries < 1) S.tries = 1;
    int64_t budget = clamp_to_free(c->place.max_bytes, 4);              // bytes held at any one time, the kept set included
    if (budget < S.set_bytes) { budget = S.set_bytes; S.tries = 1; }
    auto CS = std::unique_ptr<CandidateSets>(new (std::nothrow) CandidateSets());
    if (!CS) return fail(IDHMC_ERR_ALLOC, "out of host memory");
    CandidateSets &cs = *CS;
    cs.nvec_ = nvec;
    if (S.pair_walk()) return IDHMC_OK;
    if (int rc = S.set_walk(cs, budget)) return rc;
    if (int rc = S.choose_pair(cs)) return rc;
    const int best = S.best;
    c->placement_tries = cs.n;
    c->placement_GBps = (cs.n > 1 || cs.ms[best] > 0.f) && cs.ms[best] > 0.f ? probe_rate(nvec, S.bytes, cs.ms[best]) / 1e9 : 0.0;
    c->placement_single_GBps = S.single_Bps / 1e9;
    c->placement_peak_bytes = cs.held_peak;
    for (int k = 0; k < nvec; ++k) { out[k] = cs.arr[best][k]; c->allocs.push_back(cs.arr[best][k]); }
    c->placement_kind = 0;
    c->bytes += cs.held[best];
    cs.held[best] = 0;                  // kept: not the holder's to free any more
    c->placement_ms = S.elapsed_ms();
    return IDHMC_OK;
}
