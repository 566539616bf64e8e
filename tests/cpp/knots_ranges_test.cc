// knots_ranges_test.cc — the arithmetic of knot-grid horizons (longtermplanner_amd/csrc/ltp_knots.hpp) on the host, as the kernel
// runs it: knots_below against a linear count on valid grids, and, for grids that BREAK the contract (decreasing, negative,
// INT_MAX), the memory-safety half of ltp_sample_knots_batch's contract: every index the search forms is inside the grid, every
// count is in [0, N], every staged offset is in [0, 2^30]. A stand-alone program; tests/test_knots_cpu.py compiles and runs it, once
// more under -fsanitize=address,undefined.
#include "ltp_knots.hpp"

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
    mutable long long reads = 0;
    mutable bool outside = false;
    int operator[](int i) const
    {
        ++reads;
        if (i < 0 || i >= (int)g.size()) { outside = true; return 0; }
        return g[(size_t)i];
    }
};

// the kernel's staging: every entry through knot_clamp
std::vector<int> staged(const std::vector<int>& raw)
{
    std::vector<int> s(raw.size());
    for (size_t w = 0; w < raw.size(); ++w) s[w] = ltp::knot_clamp(raw[w]);
    return s;
}

int linear_below(const std::vector<int>& g, int x)
{
    int c = 0;
    for (int v : g) c += v < x;
    return c;
}

void valid_grids()
{
    std::mt19937 rng(12345);
    const int sizes[] = {1, 2, 3, 31, 32, 33, 511, 512};
    long long compared = 0;
    for (int n : sizes) {
        const int steps = ltp::knots_steps(n);
        CHECK((1ll << steps) >= n + 1 && (steps == 0 || (1ll << (steps - 1)) < n + 1), "steps %d for n %d", steps, n);
        for (int variant = 0; variant < 4; ++variant) {
            // 0: w; 1: random steps of 0..3 (duplicates); 2: starts above 0, steps 0..9; 3: all equal
            std::vector<int> g((size_t)n);
            int at = variant == 2 ? 37 : 0;
            for (int w = 0; w < n; ++w) {
                if (w > 0) at += variant == 0 ? 1 : variant == 1 ? (int)(rng() % 4) : variant == 2 ? (int)(rng() % 10) : 0;
                g[(size_t)w] = at;
            }
            CHECK(*ltp::knots_refusal(n, g.data()) == 0, "a valid grid is refused: %s", ltp::knots_refusal(n, g.data()));
            const std::vector<int> s = staged(g);
            CHECK(s == g, "the clamp changes a grid inside the contract (n %d)", n);
            const CheckedGrid cg{s};
            for (int x = -3; x <= g.back() + 3; ++x) {
                const int got = ltp::knots_below(cg, n, steps, x), want = linear_below(g, x);
                CHECK(got == want, "n %d variant %d x %d: %d, linear count %d", n, variant, x, got, want);
                ++compared;
            }
            CHECK(!cg.outside, "n %d variant %d: an index outside the grid", n, variant);
            CHECK(cg.reads <= (long long)steps * (g.back() + 7), "n %d: more reads than steps", n);
        }
    }
    // the largest admitted offsets
    std::vector<int> far = {0, 1 << 29, ltp::kKnotOffsetMax, ltp::kKnotOffsetMax};
    CHECK(*ltp::knots_refusal(4, far.data()) == 0, "2^30 is refused");
    CHECK(ltp::knots_below(far, 4, ltp::knots_steps(4), ltp::kKnotOffsetMax) == 2 && ltp::knots_below(far, 4, ltp::knots_steps(4), INT_MAX) == 4,
          "counts at 2^30");
    std::printf("valid grids: %lld counts compared\n", compared);
}

void broken_grids()
{
    std::mt19937 rng(777);
    const int specials[] = {INT_MIN, -1, 0, 1, ltp::kKnotOffsetMax, ltp::kKnotOffsetMax + 1, INT_MAX};
    const int xs[] = {INT_MIN, -5, 0, 1, 2, 1000, ltp::kKnotOffsetMax, ltp::kKnotOffsetMax + 1, INT_MAX};
    long long counts = 0, refused = 0, grids = 0;
    for (int round = 0; round < 400; ++round) {
        const int n = 1 + (int)(rng() % ltp::kMaxKnots);
        std::vector<int> raw((size_t)n);
        const int kind = round % 4;                              // 0: decreasing, 1: any ints, 2: specials mixed in, 3: noisy ramp
        for (int w = 0; w < n; ++w) {
            const int r = (int)rng();
            raw[(size_t)w] = kind == 0 ? 5000 - 3 * w - (int)(rng() % 3) : kind == 1 ? r : kind == 2 ? (rng() % 3 ? w * 5 : specials[rng() % 7]) : w * 4 + (int)(rng() % 41) - 20;
        }
        if (kind == 3) raw[(size_t)(rng() % (unsigned)n)] = -1;  // a noisy ramp of one knot may be in order: make it break the contract
        if (kind == 2) raw[(size_t)(rng() % (unsigned)n)] = INT_MAX;
        if (kind == 0 && n == 1) raw[0] = -7;
        if (kind == 1) raw[0] = INT_MIN;
        ++grids;
        refused += *ltp::knots_refusal(n, raw.data()) != 0;
        const std::vector<int> s = staged(raw);
        for (int v : s) CHECK(v >= 0 && v <= ltp::kKnotOffsetMax, "a staged offset %d", v);
        const CheckedGrid cg{s};
        const int steps = ltp::knots_steps(n);
        auto count_at = [&](int x) {
            const int c = ltp::knots_below(cg, n, steps, x);
            CHECK(c >= 0 && c <= n, "count %d of n %d at x %d", c, n, x);
            ++counts;
        };
        for (int x : xs) count_at(x);
        for (int i = 0; i < 200; ++i) count_at((int)(rng() % 6000) - 500);
        for (int i = 0; i < 50; ++i) count_at((int)rng());
        CHECK(!cg.outside, "round %d: an index outside the grid", round);
    }
    CHECK(refused == grids, "%lld of %lld contract-breaking grids pass knots_refusal", grids - refused, grids);
    // n_knots itself
    const int one = 0;
    CHECK(*ltp::knots_refusal(0, &one) != 0 && *ltp::knots_refusal(-1, &one) != 0 && *ltp::knots_refusal(ltp::kMaxKnots + 1, &one) != 0,
          "n_knots outside 1 .. LTP_MAX_KNOTS passes");
    std::printf("broken grids: %lld grids, %lld counts\n", grids, counts);
}

}  // namespace

int main()
{
    static_assert(ltp::knots_steps(1) == 1 && ltp::knots_steps(2) == 2 && ltp::knots_steps(3) == 2 && ltp::knots_steps(511) == 9 && ltp::knots_steps(512) == 10,
                  "ceil(log2(n + 1))");
    static_assert(ltp::knot_clamp(INT_MIN) == 0 && ltp::knot_clamp(INT_MAX) == (1 << 30) && ltp::knot_clamp(17) == 17, "the clamp");
    valid_grids();
    broken_grids();
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
