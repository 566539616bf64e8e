// envelope_knots_ranges_test.cc — the interval arithmetic of horizon envelopes (longtermplanner_amd/csrc/ltp_intervals.hpp) on the
// host, as k_envelope_knots runs it: a lane's walk over random cut lists of up to 20 runs (runs of one sample, cuts that coincide
// with edges) against edge lists both inside the contract and BREAKING it (decreasing, negative, INT_MAX). Valid grids: the
// stretches of interval w unite to exactly [a_w, min(b_w, len - 1)], in order, each inside one run, and at most one interval is
// carried across a cut. All grids: every index in [0, M), every pair written exactly once, only g[0 .. M] read, the steps of a
// walk bounded by M + the number of runs. A stand-alone program; tests/test_envelope_knots_cpu.py compiles and runs it, once more
// under -fsanitize=address,undefined.
#include "ltp_intervals.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failures <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                  \
    } while (0)

// a grid that reports every index it is read at
struct CheckedGrid {
    const std::vector<int>& g;
    mutable bool outside = false;
    int operator[](int i) const
    {
        if (i < 0 || i >= (int)g.size()) { outside = true; return 0; }
        return g[(size_t)i];
    }
};

std::vector<int> staged(const std::vector<int>& raw)
{
    std::vector<int> s(raw.size());
    for (size_t w = 0; w < raw.size(); ++w) s[w] = ltp::knot_clamp(raw[w]);
    return s;
}

struct Stretch { int run, s0, s1; };
struct Walk {
    std::vector<std::vector<Stretch>> of;      // per interval: its stretches in the order they were handed over
    std::vector<int> stored;                   // per interval: 1 = completed inside a run, 2 = carried out of the walk, 3 = past the end
    std::vector<int> writes;
    long long steps = 0;
    bool carried = false;                      // an interval was open at a cut
    bool index_outside = false, w_shrank = false, stopped_early = false;
};

// the kernel's walk: the runs [cuts[r], cuts[r + 1]) of a trajectory of len samples from the start k (as given; clamped here)
Walk walk(const std::vector<int>& g, int M, int closed, int k_given, const std::vector<int>& cuts)
{
    const int len = cuts.back();
    const int k = k_given < 0 ? 0 : (k_given > len ? len : k_given);
    const CheckedGrid G{g};
    Walk out;
    out.of.resize((size_t)M);
    out.stored.assign((size_t)M, 0);
    out.writes.assign((size_t)M, 0);
    ltp::IntervalCursor cu;
    int last_w = 0;
    auto index = [&](int w) {
        if (w < 0 || w >= M) { out.index_outside = true; return false; }
        return true;
    };
    for (size_t r = 0; r + 1 < cuts.size(); ++r) {
        const int b = cuts[r], e = cuts[r + 1];
        if (cu.w >= M) { out.stopped_early = true; break; }
        if (ltp::run_before_intervals(G, M, k, e, cu)) continue;
        const bool done = ltp::intervals_in_run(G, M, closed, k, b, e, cu, [&](int w, int s0, int s1, bool complete) {
            ++out.steps;
            if (!index(w)) return;
            if (s0 <= s1) out.of[(size_t)w].push_back(Stretch{(int)r, s0, s1});
            if (complete) { ++out.writes[(size_t)w]; out.stored[(size_t)w] = 1; }
        });
        if (cu.w < last_w) out.w_shrank = true;
        last_w = cu.w;
        out.carried = out.carried || cu.open;
        if (done && cu.w < M) out.index_outside = true;          // "every interval stored" with one left
    }
    ltp::intervals_after_walk(M, cu, [&](int w) { if (index(w)) { ++out.writes[(size_t)w]; out.stored[(size_t)w] = 2; } },
                              [&](int w) { if (index(w)) { ++out.writes[(size_t)w]; out.stored[(size_t)w] = 3; } });
    if (cu.w < last_w) out.w_shrank = true;
    CHECK(!G.outside, "an index outside g[0 .. M]");
    return out;
}

// up to 20 runs: cut points 0 = c0 < c1 < ... = len, with runs of one sample, some cuts moved onto k + an edge
std::vector<int> random_cuts(std::mt19937& rng, const std::vector<int>& g, int k)
{
    const int runs = 1 + (int)(rng() % 20);
    std::vector<int> cuts{0};
    for (int r = 0; r < runs; ++r) {
        const unsigned kind = rng() % 4;
        const int step = kind == 0 ? 1 : kind == 1 ? 1 + (int)(rng() % 4) : 1 + (int)(rng() % 60);
        int next = cuts.back() + step;
        if (kind == 3) {                                         // the next edge behind the last cut, if there is one nearby
            for (int v : g) {
                const long long at = (long long)(k < 0 ? 0 : k) + v;
                if (at > cuts.back() && at <= cuts.back() + 200) { next = (int)at; break; }
            }
        }
        cuts.push_back(next);
    }
    return cuts;
}

void all_grids_properties(const Walk& w, int M, size_t runs, const char* what)
{
    CHECK(!w.index_outside, "%s: an index outside [0, M)", what);
    CHECK(!w.w_shrank, "%s: w went back", what);
    for (int i = 0; i < M; ++i) CHECK(w.writes[(size_t)i] == 1, "%s: pair %d of %d written %d times", what, i, M, w.writes[(size_t)i]);
    CHECK(w.steps <= (long long)M + (long long)runs, "%s: %lld steps for M %d and %zu runs", what, w.steps, M, runs);
}

void valid_grids()
{
    std::mt19937 rng(2024);
    long long walks = 0, carried_walks = 0, early = 0, past = 0;
    for (int round = 0; round < 4000; ++round) {
        const int M = round % 50 == 0 ? ltp::kMaxKnots - 1 : 1 + (int)(rng() % 40);
        const int variant = round % 5;         // 0: w; 1: steps 0..3 (duplicates); 2: starts above 0, steps 0..9; 3: all equal; 4: steps 0..40
        std::vector<int> g((size_t)M + 1);
        int at = variant == 2 ? (int)(rng() % 40) : 0;
        for (int w = 0; w <= M; ++w) {
            if (w > 0) at += variant == 0 ? 1 : variant == 1 ? (int)(rng() % 4) : variant == 2 ? (int)(rng() % 10) : variant == 3 ? 0 : (int)(rng() % 41);
            g[(size_t)w] = at;
        }
        CHECK(*ltp::intervals_refusal(M, g.data()) == 0, "a valid grid is refused: %s", ltp::intervals_refusal(M, g.data()));
        CHECK(staged(g) == g, "the clamp changes a grid inside the contract");
        for (int closed = 0; closed < 2; ++closed) {
            const int k_given = (int)(rng() % 120) - 10;
            const std::vector<int> cuts = random_cuts(rng, g, k_given);
            const int len = cuts.back();
            const long long k = k_given < 0 ? 0 : (k_given > len ? len : k_given);
            const Walk w = walk(g, M, closed, k_given, cuts);
            ++walks;
            carried_walks += w.carried;
            early += w.stopped_early;
            all_grids_properties(w, M, cuts.size() - 1, "valid grid");
            // at most one interval has samples on both sides of a cut
            std::vector<int> across(cuts.size(), 0);
            for (int i = 0; i < M; ++i) {
                const auto& st = w.of[(size_t)i];
                if (!st.empty())
                    for (int c = st.front().run + 1; c <= st.back().run; ++c) ++across[(size_t)c];
            }
            for (size_t c = 0; c < across.size(); ++c) CHECK(across[c] <= 1, "%d intervals carried across cut %zu", across[c], c);
            for (int i = 0; i < M; ++i) {
                const long long a = k + g[(size_t)i], z = std::max(a, k + g[(size_t)i + 1] - 1 + closed);
                const auto& st = w.of[(size_t)i];
                if (a >= len) {                                  // starts at or past the end: the last position twice, no stretch
                    ++past;
                    CHECK(st.empty() && w.stored[(size_t)i] == 3, "interval %d past the end: %zu stretches, stored %d", i, st.size(), w.stored[(size_t)i]);
                    continue;
                }
                const long long last = std::min(z, (long long)len - 1);
                CHECK(!st.empty() && w.stored[(size_t)i] == (z < len ? 1 : 2), "interval %d [%lld, %lld] of len %d: %zu stretches, stored %d", i, a, z,
                      len, st.size(), w.stored[(size_t)i]);
                if (st.empty()) continue;
                CHECK(st.front().s0 == a && st.back().s1 == last, "interval %d covers [%d, %d], not [%lld, %lld]", i, st.front().s0, st.back().s1, a, last);
                for (size_t x = 0; x < st.size(); ++x) {
                    CHECK(st[x].s0 <= st[x].s1 && st[x].s0 >= cuts[(size_t)st[x].run] && st[x].s1 < cuts[(size_t)st[x].run + 1],
                          "interval %d: stretch [%d, %d] is not inside run %d", i, st[x].s0, st[x].s1, st[x].run);
                    if (x > 0) CHECK(st[x].s0 == st[x - 1].s1 + 1 && st[x].run > st[x - 1].run, "interval %d: stretches out of order or with a gap", i);
                }
            }
        }
    }
    CHECK(carried_walks > walks / 4 && early > walks / 20 && past > 0, "the draw does not reach the cases: %lld carried, %lld early, %lld past of %lld",
          carried_walks, early, past, walks);
    std::printf("valid grids: %lld walks, %lld with a carried interval, %lld stopped early, %lld intervals past the end\n", walks, carried_walks, early, past);
}

void broken_grids()
{
    std::mt19937 rng(777);
    const int specials[] = {INT_MIN, -1, 0, 1, ltp::kKnotOffsetMax, ltp::kKnotOffsetMax + 1, INT_MAX};
    long long grids = 0, refused = 0;
    for (int round = 0; round < 2000; ++round) {
        const int M = round % 40 == 0 ? ltp::kMaxKnots - 1 : 1 + (int)(rng() % 60);
        std::vector<int> raw((size_t)M + 1);
        const int kind = round % 4;                              // 0: decreasing, 1: any ints, 2: specials mixed in, 3: noisy ramp
        for (int w = 0; w <= M; ++w) {
            const int r = (int)rng();
            raw[(size_t)w] = kind == 0 ? 300 - 3 * w - (int)(rng() % 3) : kind == 1 ? r : kind == 2 ? (rng() % 3 ? w * 5 : specials[rng() % 7]) : w * 4 + (int)(rng() % 41) - 20;
        }
        if (kind == 3) raw[(size_t)(rng() % (unsigned)(M + 1))] = -1;
        if (kind == 2) raw[(size_t)(rng() % (unsigned)(M + 1))] = INT_MAX;
        if (kind == 1) raw[0] = INT_MIN;
        ++grids;
        refused += *ltp::intervals_refusal(M, raw.data()) != 0;
        const std::vector<int> s = staged(raw);
        for (int v : s) CHECK(v >= 0 && v <= ltp::kKnotOffsetMax, "a staged edge %d", v);
        for (int closed = 0; closed < 2; ++closed) {
            const int k_given = round % 7 == 0 ? INT_MAX : round % 11 == 0 ? INT_MIN : (int)(rng() % 400) - 20;
            const std::vector<int> cuts = random_cuts(rng, s, k_given < 0 ? 0 : (k_given > 1000 ? 0 : k_given));
            const Walk w = walk(s, M, closed, k_given, cuts);
            all_grids_properties(w, M, cuts.size() - 1, "broken grid");
            for (int i = 0; i < M; ++i)
                for (const Stretch& st : w.of[(size_t)i])
                    CHECK(st.s0 >= cuts[(size_t)st.run] && st.s1 < cuts[(size_t)st.run + 1], "broken grid: a stretch outside its run");
        }
    }
    CHECK(refused == grids, "%lld of %lld contract-breaking grids pass intervals_refusal", grids - refused, grids);
    const int two[2] = {0, 1};
    CHECK(*ltp::intervals_refusal(0, two) != 0 && *ltp::intervals_refusal(-1, two) != 0 && *ltp::intervals_refusal(ltp::kMaxKnots, two) != 0 &&
              *ltp::intervals_refusal(1, nullptr) != 0 && *ltp::intervals_refusal(1, two) == 0,
          "the length rule: 2 .. LTP_MAX_KNOTS edges");
    std::printf("broken grids: %lld grids\n", grids);
}

}  // namespace

int main()
{
    valid_grids();
    broken_grids();
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
