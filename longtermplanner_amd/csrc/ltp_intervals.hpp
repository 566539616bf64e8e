// ltp_intervals.hpp — the arithmetic of horizon envelopes (ltp_envelope_knots_batch, include/ltp_hip.h; k_envelope_knots,
// ltp_consumers.hip): which samples interval w of a staged edge list holds, and the loop that lays the intervals over one run of
// a lane's walk. Host logic without HIP headers, in the manner of ltp_knots.hpp: tests/cpp/envelope_knots_ranges_test.cc runs the
// same functions the kernel runs, the half of the contract that speaks of grids which BREAK it included (the cursor only grows,
// every index is in [0, M), every pair is written exactly once, the steps of a whole walk are bounded by M + the number of runs).
//
// Everything is counted in OFFSETS from the plan's start k (already clamped to [0, traj_len]): the staged edges g[0 .. M] lie in
// [0, 2^30] (knot_clamp), a run [b, e) of the trajectory is [b - k, e - k), and neither forms a signed overflow. Interval w holds
// the offsets interval_first .. interval_last: g[w] .. max(g[w], g[w + 1] - 1 + closed).
#pragma once
#include "ltp_knots.hpp"

namespace ltp {

template <class Grid>
LTP_KNOTS_HD inline int interval_first(const Grid& g, int w) { return g[w]; }
template <class Grid>
LTP_KNOTS_HD inline int interval_last(const Grid& g, int w, int closed)
{
    const int a = g[w], z = g[w + 1] - 1 + closed;
    return z > a ? z : a;
}

// Where a lane's walk stands among its M intervals: w is the first one that is not stored yet; open: it already holds samples of
// earlier runs. For a grid inside the contract interval_first(w + 1) >= interval_last(w) in both modes, so at most ONE interval
// straddles a run boundary and one carried [lo, hi] is enough.
struct IntervalCursor {
    int w = 0;
    bool open = false;
};

// the run that ends at trajectory sample e (exclusive) ends at or before the first sample of the first interval not stored yet:
// it holds nothing of any interval, and the walk steps over it
template <class Grid>
LTP_KNOTS_HD inline bool run_before_intervals(const Grid& g, int M, int k, int e, const IntervalCursor& cu)
{
    return cu.w < M && e - k <= interval_first(g, cu.w);
}

// The intervals that meet the run [b, e) of the trajectory, in order: stretch(w, s0, s1, complete) receives the trajectory samples
// s0 .. s1 of interval w that lie in this run (s0 > s1: none — only a grid outside the contract gets there) and whether the
// interval ends inside the run; a complete interval is to be stored and the carried [lo, hi] emptied, an incomplete one is carried
// into the next run. Returns true once every interval is stored: the walk may stop. Whatever g holds, cu.w only grows, only
// g[0 .. M] is read, and a call makes at most (intervals completed) + 1 steps.
template <class Grid, class Stretch>
LTP_KNOTS_HD inline bool intervals_in_run(const Grid& g, int M, int closed, int k, int b, int e, IntervalCursor& cu, Stretch&& stretch)
{
    const int rb = b - k, re = e - k;
    while (cu.w < M) {
        const int a = interval_first(g, cu.w);
        if (a >= re) break;                                   // starts behind this run
        const int z = interval_last(g, cu.w, closed);
        const bool complete = z < re;
        const int s0 = a > rb ? a : rb, s1 = complete ? z : re - 1;
        stretch(cu.w, s0 + k, s1 + k, complete);
        cu.open = !complete;
        if (!complete) break;
        ++cu.w;
    }
    return cu.w >= M;
}

// After the last run: the interval the trajectory ended in holds the samples that exist (carried(w)); every one behind it starts
// at or past traj_len and holds the last position twice (rest(w)).
template <class Carried, class Rest>
LTP_KNOTS_HD inline void intervals_after_walk(int M, IntervalCursor& cu, Carried&& carried, Rest&& rest)
{
    if (cu.w < M && cu.open) {
        carried(cu.w);
        cu.open = false;
        ++cu.w;
    }
    for (; cu.w < M; ++cu.w) rest(cu.w);
}

// what the entries that SEE the edges (host memory) have against them: "" for a grid inside the contract
inline const char* intervals_refusal(int n_intervals, const int* edges)
{
    if (n_intervals < 1 || n_intervals > kMaxKnots - 1) return "n_intervals must be in 1 .. LTP_MAX_KNOTS - 1 (at least 2 edges)";
    if (!edges) return "null edge_offsets";
    return knots_refusal(n_intervals + 1, edges);
}

}  // namespace ltp
