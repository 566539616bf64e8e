// ltp_knots.hpp — the arithmetic of knot-grid horizons (ltp_sample_knots_batch, include/ltp_hip.h; k_sample_window's knots mode,
// ltp_window.hip): the clamp every offset passes when the grid is staged, the count "how many knots lie below trajectory offset x",
// and the host entries' check of a grid. Host logic without HIP headers: tests/cpp/knots_ranges_test.cc pins it, the half of the
// contract that speaks of grids which BREAK it included (every count in [0, n], every staged offset in [0, 2^30], no index outside
// the grid).
#pragma once
#include "../../include/ltp_hip.h"

#if defined(__HIPCC__)
#define LTP_KNOTS_HD __host__ __device__
#else
#define LTP_KNOTS_HD
#endif

namespace ltp {

constexpr int kMaxKnots = LTP_MAX_KNOTS;
constexpr int kKnotOffsetMax = 1 << 30;    // the kernel's sample indices are ints: k + g[w] with k <= traj_len stays below 2^31

// what the kernel stages of a grid entry: inside the contract the entry itself
LTP_KNOTS_HD constexpr int knot_clamp(int g) { return g < 0 ? 0 : g > kKnotOffsetMax ? kKnotOffsetMax : g; }

// steps of knots_below over n knots: ceil(log2(n + 1)), so that the steps' sizes 2^(steps-1), ..., 2, 1 sum to at least n
LTP_KNOTS_HD constexpr int knots_steps(int n)
{
    int s = 0;
    while (s < 31 && (1ll << s) < (long long)n + 1) ++s;
    return s;
}

// The number of w in [0, n) with g[w] < x, for a non-decreasing g: 0 for x <= 0, else a lower bound in a FIXED number of steps
// (steps = knots_steps(n)): no trip count depends on the data. pos knots are known to lie below x; a step of size `bit` is taken
// if it stays inside the grid and the knot it lands on lies below x too. Whatever g holds, only g[0 .. n) is read and the result
// is in [0, n].
template <class Grid>
LTP_KNOTS_HD inline int knots_below(const Grid& g, int n, int steps, int x)
{
    if (x <= 0) return 0;
    int pos = 0;
    for (int bit = steps > 0 ? 1 << (steps - 1) : 0; bit > 0; bit >>= 1) {
        const int probe = pos + bit;
        const int at = (probe <= n ? probe : n) - 1;      // an index inside the grid whether the step is or not (n >= 1)
        pos = probe <= n && g[at] < x ? probe : pos;
    }
    return pos;
}

// what the entries that SEE the grid (host memory) have against it: "" for a grid inside the contract
inline const char* knots_refusal(int n_knots, const int* g)
{
    if (n_knots < 1 || n_knots > kMaxKnots) return "n_knots must be in 1 .. LTP_MAX_KNOTS";
    if (!g) return "null knot_offsets";
    for (int w = 0; w < n_knots; ++w) {
        if (g[w] < 0) return "knot_offsets holds a negative offset";
        if (g[w] > kKnotOffsetMax) return "knot_offsets holds an offset beyond 2^30";
        if (w > 0 && g[w] < g[w - 1]) return "knot_offsets decreases";
    }
    return "";
}

}  // namespace ltp
