// ltp_consumers.hip — everything that reads a planned batch without writing dense rows, gfx950: the table pass
// (k_build_tables: the packed run tables of include/ltp_run_tables.hpp, for the library's own short-row sampler / envelope consumer
// and, through ltp_build_tables_batch, for USER consumers), the envelope consumer (k_envelope, k_envelope_walk; on the intervals of a
// knot grid from a start per plan: k_envelope_knots), the receding-horizon restart states
// (k_state_at, k_replan_states) and the end-limit verdict without rows (k_end_limit).
#include "ltp_sampler_lds.hpp"
#include "ltp_intervals.hpp"
#include "ltp_extremes.hpp"
#include "ltp_crossings.hpp"

namespace ltp {

// The analytic envelope forms (k_envelope<.., ANALYTIC>, k_envelope_walk, k_envelope_knots, k_envelope_knots_arrays): inside a run
// q(m) is ONE cubic in the run-local index m, q(m) = c4[0] + c4[1] m + c4[2] m^2 + c4[3] m^3 (run_eval_q). The real roots of
// q'(m) = c1 + 2 c2 m + 3 c3 m^2 (qprime_roots) and the candidate rule (fold_candidates) are ltp_extremes.hpp's, which the host runs too.
using QPrimeRoots = StretchRoots;
// Folds the extreme samples of the stretch m0 .. m1 of a run into [lo, hi]: its two end samples and, for m1 - m0 > 1 (the only
// stretches whose roots are read), the samples either side of a root. Every candidate is run_eval_q: a sample of the row, bit for bit.
template <class Roots>
LTP_DEV void fold_stretch(const double* c4, Roots&& roots_of_run, int m0, int m1, double& lo, double& hi)
{
    fold_candidates(m0, m1, roots_of_run, [&](int m) {
        const double q = run_eval_q(c4, m);
        lo = __builtin_fmin(lo, q);
        hi = __builtin_fmax(hi, q);
    });
}

// ---------------------------------------------------------------------------------------
// On-device consumer: position envelopes instead of dense rows. A caller that only needs to
// know where each joint can be during each time window of the plan (reachability / limit / collision checks of a
// safety shield, reference README.md:10-13) gets, per plan and joint, [min q, max q] over the samples of each of
// n_windows windows of `window` samples — 16 bytes per window instead of 32 bytes per sample, so nothing the size
// of the dense trajectories ever exists. The values are the minimum and maximum of exactly the q samples k_sample
// would have stored (same run tables, same run_eval expression). Windows that start after the end of the trajectory
// hold its last position (the joint rests there); plans without a trajectory (traj_len 0) get NaN.
// Item = plan x joint group as in k_sample; lane -> (joint, window) task, each walking its samples in order.
// ---------------------------------------------------------------------------------------
// ANALYTIC (ltp_set_envelope_mode(p, LTP_ENVELOPE_ANALYTIC), round 5): inside a run q(m) is ONE cubic in the run-local index m, so its
// extreme samples over a stretch of the run are the stretch's two end samples or the samples either side of a real root of
// q'(m) = c1 + 2 c2 m + 3 c3 m^2. The task evaluates those <= 6 candidates per (run, window) stretch — with run_eval_q, i.e. they ARE
// samples of the row, bit for bit — instead of every sample. What it can miss is a sample that undercuts its neighbour by rounding
// alone: the result is within a few ulps of q (~1e-15) of the exhaustive form's, not bit-identical, which is why the exhaustive form
// stays the default (tests: 1e-12 against the exhaustive form, 1e-9 against the CPU checker's reduced rows).
template <bool PROBE, bool TABLES, bool ANALYTIC = false>
__global__ void __launch_bounds__(kSampleThreads, kSampleBlocksPerCU)
k_envelope(long long first, long long count, long long base_first, int dof, double t_sample, PlanLimits lim, Queries in, Records rec, int window,
           int n_windows, int lg, double* __restrict__ env, unsigned long long* __restrict__ next_item,
           unsigned long long* __restrict__ probe_buf /* diagnostic, PROBE only: 16 stamps per item */,
           const unsigned long long* __restrict__ tables)
{
    __shared__ SegTable tab;
    __shared__ unsigned long long s_item;
    const int ngroups = (dof + kSampleJointGroup - 1) / kSampleJointGroup;
    const unsigned long long total = (unsigned long long)count * ngroups;
    constexpr int kChunk = 4;                      // items per queue draw (see k_sample)
    unsigned long long chunk_base = 0ull;
    int chunk_i = 0;
    for (;;) {
        __syncthreads();
        unsigned long long t_top = 0ull;
        if constexpr (PROBE) t_top = wall_clock64();
        if (threadIdx.x == 0) {
            if (chunk_i == 0) chunk_base = atomicAdd(next_item, (unsigned long long)kChunk);
            s_item = chunk_base + (unsigned long long)chunk_i;
        }
        chunk_i = (chunk_i + 1) & (kChunk - 1);
        __syncthreads();
        const unsigned long long item = s_item;
        if (item >= total) break;
        unsigned long long* probe = nullptr;
        if constexpr (PROBE) {
            probe = probe_buf + item * 16;
            if (threadIdx.x == 0) { probe[0] = t_top; probe[1] = wall_clock64(); }
        }
        const int group = (int)(item % ngroups);
        const long long local = (long long)(item / ngroups);
        const long long p = first + local;
        const int j0 = group * kSampleJointGroup;
        const int nj = (dof - j0) < kSampleJointGroup ? (dof - j0) : kSampleJointGroup;
        const int len = rec.traj_len[p];
        const int tasks = nj * n_windows;
        double2_t* const dst = reinterpret_cast<double2_t*>(env) + ((unsigned long long)(p - base_first) * dof + j0) * n_windows;
        if (len <= 0) {
            const double nan = __builtin_nan("");
            for (int task = threadIdx.x; task < tasks; task += kSampleThreads) dst[task] = double2_t{nan, nan};
            continue;
        }
        if constexpr (PROBE) { if (threadIdx.x == 0) probe[2] = wall_clock64(); }
        const ItemRegs<TABLES> regs = fetch_item<TABLES>(p, j0, nj, dof, lim, in, rec, nullptr, tables, first);
        if constexpr (TABLES) install_run_tables(tab.jt, nj, regs.w, t_sample);
        else {
            build_run_tables<PROBE>(tab, p, j0, nj, len, t_sample, plan_limits(lim, p, dof), rec, regs.pa, regs.pb, probe);
            __syncthreads();
        }
        if constexpr (PROBE) { if (threadIdx.x == 0) probe[9] = wall_clock64(); }
        // g lanes share one (joint, window) task (g = 2^lg divides 64, chosen by the host so that the block has
        // work for all its lanes); lane r of the task takes samples b + r, b + r + g, ... and the g partial results
        // meet in a butterfly. Minimum and maximum do not depend on the order, so any g gives the same bits.
        const int g = 1 << lg;
        for (int base = 0; base < tasks * g; base += kSampleThreads) {
            const int idx = base + (int)threadIdx.x;
            const int task = idx >> lg, r = idx & (g - 1);
            const bool live = task < tasks;
            double lo = __builtin_huge_val(), hi = -__builtin_huge_val();
            if (live) {
                // (through the public consumer interface, include/ltp_run_tables.hpp: JointTable in LDS, RunCursor, run_eval_q)
                const int jl = task / n_windows, w = task - jl * n_windows;
                const JointTable& jt = tab.jt[jl];
                const long long b = (long long)w * window;
                const bool past = b >= (long long)len;                            // past the end: the last sample only
                int i = past ? len - 1 + r : (int)b + r;
                const int e = (b + window < (long long)len) ? (int)(b + window) : len;
                RunCursor cu(jt);
                // the four q coefficients of the current run stay in registers; they are re-read at a run boundary only
                double c4[4] = {jt.c[0][0], jt.c[0][1], jt.c[0][2], jt.c[0][3]};
                if constexpr (ANALYTIC) {
                    // (one lane per task: the host launches this form with lg = 0)
                    const int e_task = past ? len : e;
                    while (i < e_task) {
                        if (cu.advance(jt, i)) {
#pragma unroll
                            for (int x = 0; x < 4; ++x) c4[x] = jt.c[cu.run][x];
                        }
                        const int stretch_end = cu.nxt < e_task ? cu.nxt : e_task;     // samples [i, stretch_end) lie in this run
                        const int m0 = i - cu.cur + 1, m1 = stretch_end - cu.cur;      // their run-local positions m0 .. m1
                        // (a task meets a run in one stretch: the roots are formed once per run, and only where they are read)
                        fold_stretch(c4, [&] { return qprime_roots(c4); }, m0, m1, lo, hi);
                        i = stretch_end;
                    }
                } else
                for (; i < e; i += g) {
                    if (cu.advance(jt, i)) {
#pragma unroll
                        for (int x = 0; x < 4; ++x) c4[x] = jt.c[cu.run][x];
                    }
                    const double q = run_eval_q(c4, i - cu.cur + 1);
                    lo = __builtin_fmin(lo, q);
                    hi = __builtin_fmax(hi, q);
                }
            }
            for (int d = 1; d < g; d <<= 1) {
                lo = __builtin_fmin(lo, __shfl_xor(lo, d));
                hi = __builtin_fmax(hi, __shfl_xor(hi, d));
            }
            if (live && r == 0) dst[task] = double2_t{lo, hi};
        }
        if constexpr (PROBE) {
            __syncthreads();
            if (threadIdx.x == 0) probe[10] = wall_clock64();
        }
    }
}

// The analytic envelopes WITHOUT run tables (round 5): lane = (plan, joint) walks its runs in registers — the walk of k_state_at /
// k_end_limit — and while a run lasts folds the candidates of each window it crosses: the two end samples of the stretch and the
// samples either side of the real roots of q'(m) (computed once per run: they do not depend on the window), evaluated with
// run_eval_q on the coefficients for_each_run hands over, i.e. the values k_envelope's analytic form folds, bit for bit. A window
// is stored (16 bytes) when the walk leaves it; the walk goes on to the last sample, which also gives planTrajectory's end-limit
// verdict (cc:59-61) and the content of the windows past the end. No table pass, no workspace, no LDS, no per-item latency: what
// the block-cooperative kernel spends on fetching and installing seven joints' tables per plan (E7.4) is not there.
template <int SEM>
__global__ void __launch_bounds__(256)
k_envelope_walk(PlanRange r, long long base_first, int window, int n_windows, double* __restrict__ env)
{
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long p = l.p;
    const int j = l.j, dof = r.dof;
    double2_t* const dst = reinterpret_cast<double2_t*>(env) + ((unsigned long long)(p - base_first) * dof + j) * n_windows;
    const int len = r.rec.traj_len[p];
    if (len <= 0) {
        const double nan = __builtin_nan("");
        for (int w = 0; w < n_windows; ++w) dst[w] = double2_t{nan, nan};
        return;
    }
    double q, v, a;
    l.start(r.in, q, v, a);
    const Limits L = plan_limits(r.lim, p, dof);
    int w = 0;                                                  // the window under construction: samples [w_end - window, w_end)
    long long w_end = window;
    double lo = __builtin_huge_val(), hi = -__builtin_huge_val();
    for_each_run<SEM>(L, r.rec, p * dof + j, j, len, r.t_sample, q, v, a, [&](int b, int e, const RunCoef& rc) {
        if (w >= n_windows) return false;                       // every window written: the walk only continues for the end-limit verdict
        const QPrimeRoots roots = qprime_roots(rc.c);           // once per run: they do not depend on the window
        int i = b;
        while (i < e && w < n_windows) {
            const int stretch_end = (long long)e < w_end ? e : (int)w_end;      // samples [i, stretch_end) of this run lie in window w
            fold_stretch(rc.c, [&] { return roots; }, i - b + 1, stretch_end - b, lo, hi);
            i = stretch_end;
            if ((long long)i == w_end) {                                        // the window is complete
                dst[w] = double2_t{lo, hi};
                ++w;
                w_end += window;
                lo = __builtin_huge_val();
                hi = -__builtin_huge_val();
            }
        }
        return false;
    }, j == dof - 1);
    // q now holds the last trajectory sample. A window the trajectory ended in holds the samples that exist; windows that start at or
    // after the end hold the last position twice (as k_envelope)
    if (w < n_windows && lo <= hi) { dst[w] = double2_t{lo, hi}; ++w; }
    for (; w < n_windows; ++w) dst[w] = double2_t{q, q};
    if constexpr (SEM == kSemCpp) {
        if (beyond_end_limits(q, L.q_min[j], L.q_max[j])) atomicOr(&r.rec.status[p], kStatusEndLimit);
    }
}

// The start k of the horizon kernels (k_envelope_knots_arrays, k_first_exit; k_envelope_knots writes it out) for a plan of len > 0
// samples, k per plan or the same for all: below 0 is 0; from k > traj_len everything is past the end, as from traj_len
LTP_DEV int horizon_start(const int* __restrict__ first_sample, int uniform_first, long long local, int len)
{
    const int k = first_sample ? first_sample[local] : uniform_first;
    return k < 0 ? 0 : (k > len ? len : k);
}

// Horizon envelopes (ltp_envelope_knots_batch): k_envelope_walk's fold on the intervals between the edges k + g[w] of a knot grid,
// counted from a start k per plan — [min q, max q] of joint j between knot w and knot w + 1 of a horizon, from where each robot is
// now. The block stages the M + 1 edges in LDS through knot_clamp (<= 2 KB); the barrier is passed before any lane may return, and
// there is none after it. The lane then walks its runs in registers; ltp_intervals.hpp lays the intervals over each run (the same
// functions the host test runs): a run that ends before the first open interval is stepped over, an interval that ends inside
// the run is stored (16 bytes), the one that straddles the run's end is carried in lo / hi — for a grid inside the contract there
// is at most one. This call forms no end-limit verdict, so the walk STOPS when the last interval is stored. Candidates and values
// are k_envelope_walk's: with k = 0 and g[w] = w * window the two kernels fold the same stretches. No table pass, no scratch.
template <int SEM>
__global__ void __launch_bounds__(256)
k_envelope_knots(PlanRange r, int M, int closed, const int* __restrict__ edges, const int* __restrict__ first_sample, int uniform_first,
                 int* __restrict__ valid, double* __restrict__ env)
{
    __shared__ int G[kMaxKnots];                                // M + 1 <= kMaxKnots edges (the entry's rule)
    for (int w = (int)threadIdx.x; w <= M; w += (int)blockDim.x) G[w] = knot_clamp(edges[w]);
    __syncthreads();
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long p = l.p;
    const int j = l.j, dof = r.dof;
    double2_t* const dst = reinterpret_cast<double2_t*>(env) + ((unsigned long long)l.local * dof + j) * M;
    const int len = r.rec.traj_len[p];
    if (len <= 0) {
        const double nan = __builtin_nan("");
        for (int w = 0; w < M; ++w) dst[w] = double2_t{nan, nan};
        if (valid && j == 0) valid[l.local] = 0;
        return;
    }
    // horizon_start written out: through the helper two independent moves of this kernel change places (the other two users keep
    // their code to the byte), and this code object is the one the q-only call's time is held against (profiles/r22_horizon_rules.txt)
    int k = first_sample ? first_sample[l.local] : uniform_first;
    k = k < 0 ? 0 : (k > len ? len : k);
    if (valid && j == 0) valid[l.local] = knots_below(G, M, knots_steps(M), len - k);   // the w in [0, M) with k + g[w] < traj_len
    double q, v, a;
    l.start(r.in, q, v, a);
    const Limits L = plan_limits(r.lim, p, dof);
    IntervalCursor cu;
    double lo = __builtin_huge_val(), hi = -__builtin_huge_val();
    for_each_run<SEM>(L, r.rec, p * dof + j, j, len, r.t_sample, q, v, a, [&](int b, int e, const RunCoef& rc) {
        if (cu.w >= M) return true;
        if (run_before_intervals(G, M, k, e, cu)) return false;
        const QPrimeRoots roots = qprime_roots(rc.c);           // once per run: they do not depend on the interval
        return intervals_in_run(G, M, closed, k, b, e, cu, [&](int w, int s0, int s1, bool complete) {
            if (s0 <= s1) fold_stretch(rc.c, [&] { return roots; }, s0 - b + 1, s1 - b + 1, lo, hi);
            if (complete) {
                dst[w] = double2_t{lo, hi};
                lo = __builtin_huge_val();
                hi = -__builtin_huge_val();
            }
        });
    }, j == dof - 1);
    // the walk ended with intervals left: it went to the last sample, which q now holds
    intervals_after_walk(M, cu, [&](int w) { dst[w] = double2_t{lo, hi}; }, [&](int w) { dst[w] = double2_t{q, q}; });
}

// Horizon envelopes of q, v, a and j (ltp_envelope_knots_arrays_batch): k_envelope_knots' walk with one [lo, hi] per selected array.
// mask (LTP_ENV_*) is a kernel argument, so every test of it is a scalar branch the whole wave takes alike; the four accumulators
// are eight named doubles. Plane x of plan i — the rank of the array among the selected ones, in the order q, v, a, j — starts at
// pair ((i * A + x) * dof + j) * M, A = popcount(mask) (1 .. 4, the entry's rule); the interval index of every store is the cursor's,
// which ltp_intervals.hpp keeps in [0, M). Candidates per (run, interval) stretch (ltp_extremes.hpp): q as k_envelope_knots; v the
// two end samples and the samples either side of the root of v'(m); a the two end samples (exhaustive: one rounding of a monotone
// function of m); j the run's jerk. Every value is what run_eval gives the sampler, bit for bit. Past the end the sampler's rows
// hold +0.0 in v, a and j: the interval the trajectory ends in (intervals_after_walk's carried one: it always reaches past the last
// sample) also folds +0.0 into those three, the intervals behind it hold {0, 0}. With mask == LTP_ENV_Q: k_envelope_knots' stores.
template <int SEM>
__global__ void __launch_bounds__(256)
k_envelope_knots_arrays(PlanRange r, int M, int closed, int mask, const int* __restrict__ edges, const int* __restrict__ first_sample,
                        int uniform_first, int* __restrict__ valid, double* __restrict__ env)
{
    __shared__ int G[kMaxKnots];                                // M + 1 <= kMaxKnots edges (the entry's rule)
    for (int w = (int)threadIdx.x; w <= M; w += (int)blockDim.x) G[w] = knot_clamp(edges[w]);
    __syncthreads();
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long p = l.p;
    const int j = l.j, dof = r.dof;
    const bool want_q = (mask & LTP_ENV_Q) != 0, want_v = (mask & LTP_ENV_V) != 0, want_a = (mask & LTP_ENV_A) != 0, want_j = (mask & LTP_ENV_J) != 0;
    const int x_v = (int)want_q, x_a = x_v + (int)want_v, x_j = x_a + (int)want_a, A = x_j + (int)want_j;   // ranks < A <= 4
    // plane x of this lane: pairs [0, M) behind ((local * A + x) * dof + j) * M
    auto plane = [&](int x) {
        return reinterpret_cast<double2_t*>(env) + (((unsigned long long)l.local * A + x) * dof + j) * M;
    };
    double2_t* const dst_q = plane(0);
    double2_t* const dst_v = plane(x_v);
    double2_t* const dst_a = plane(x_a);
    double2_t* const dst_j = plane(x_j);                        // (a plane that is not selected is never stored through)
    auto store = [&](int w, double2_t pq, double2_t pv, double2_t pa, double2_t pj) {
        if (want_q) dst_q[w] = pq;
        if (want_v) dst_v[w] = pv;
        if (want_a) dst_a[w] = pa;
        if (want_j) dst_j[w] = pj;
    };
    const int len = r.rec.traj_len[p];
    if (len <= 0) {
        const double nan = __builtin_nan("");
        const double2_t none{nan, nan};
        for (int w = 0; w < M; ++w) store(w, none, none, none, none);
        if (valid && j == 0) valid[l.local] = 0;
        return;
    }
    const int k = horizon_start(first_sample, uniform_first, l.local, len);
    if (valid && j == 0) valid[l.local] = knots_below(G, M, knots_steps(M), len - k);   // the w in [0, M) with k + g[w] < traj_len
    double q, v, a;
    l.start(r.in, q, v, a);
    const Limits L = plan_limits(r.lim, p, dof);
    IntervalCursor cu;
    const double top = __builtin_huge_val();
    double q_lo = top, q_hi = -top, v_lo = top, v_hi = -top, a_lo = top, a_hi = -top, j_lo = top, j_hi = -top;
    for_each_run<SEM>(L, r.rec, p * dof + j, j, len, r.t_sample, q, v, a, [&](int b, int e, const RunCoef& rc) {
        if (cu.w >= M) return true;
        if (run_before_intervals(G, M, k, e, cu)) return false;
        // once per run: the roots do not depend on the interval
        StretchRoots q_roots{0.0, 0.0}, v_roots{0.0, 0.0};
        if (want_q) q_roots = qprime_roots(rc.c);
        if (want_v) v_roots = vprime_root(rc.c);
        return intervals_in_run(G, M, closed, k, b, e, cu, [&](int w, int s0, int s1, bool complete) {
            if (s0 <= s1) {
                const int m0 = s0 - b + 1, m1 = s1 - b + 1;
                if (want_q) fold_stretch(rc.c, [&] { return q_roots; }, m0, m1, q_lo, q_hi);
                if (want_v)
                    fold_candidates(m0, m1, [&] { return v_roots; }, [&](int m) {
                        const double vm = run_eval_v(rc.c + 4, m);
                        v_lo = __builtin_fmin(v_lo, vm);
                        v_hi = __builtin_fmax(v_hi, vm);
                    });
                if (want_a)
                    fold_ends(m0, m1, [&](int m) {
                        const double am = run_eval_a(rc.c + 7, m);
                        a_lo = __builtin_fmin(a_lo, am);
                        a_hi = __builtin_fmax(a_hi, am);
                    });
                if (want_j) {
                    j_lo = __builtin_fmin(j_lo, rc.c[9]);                                                   // the j line of run_eval
                    j_hi = __builtin_fmax(j_hi, rc.c[9]);
                }
            }
            if (complete) {
                store(w, double2_t{q_lo, q_hi}, double2_t{v_lo, v_hi}, double2_t{a_lo, a_hi}, double2_t{j_lo, j_hi});
                q_lo = v_lo = a_lo = j_lo = top;
                q_hi = v_hi = a_hi = j_hi = -top;
            }
        });
    }, j == dof - 1);
    // the walk ended with intervals left: it went to the last sample, which q now holds. The carried interval reaches past it.
    intervals_after_walk(M, cu, [&](int w) {
        store(w, double2_t{q_lo, q_hi}, double2_t{__builtin_fmin(v_lo, 0.0), __builtin_fmax(v_hi, 0.0)},
              double2_t{__builtin_fmin(a_lo, 0.0), __builtin_fmax(a_hi, 0.0)}, double2_t{__builtin_fmin(j_lo, 0.0), __builtin_fmax(j_hi, 0.0)});
    }, [&](int w) {
        const double2_t rest{0.0, 0.0};
        store(w, double2_t{q, q}, rest, rest, rest);
    });
}

// First exits (ltp_first_exit_batch): per plan, selected array X of q, v, a, j and joint the smallest trajectory sample t in
// [k, k + H) whose S_X(t) — k_envelope_knots_arrays' values: the sampler's bits for t < traj_len, past the end the last position
// for q and +0.0 for v, a, j — lies outside the box [lo, hi] (x < lo || x > hi: a NaN sample never exits), LTP_EXIT_NONE for none,
// LTP_EXIT_NO_PLAN for traj_len == 0. The lane walks its runs in registers (for_each_run) and, per run that reaches into [k, k + H)
// and per array still open, folds the candidates of the stretch (ltp_crossings.hpp: first_outside_candidate, the envelope fold with
// two compares per sample). A stretch with a candidate outside CLOSES its array: the lane keeps that array's own coefficients of the
// run (4 + 3 + 2 + 1 = the ten of a RunCoef between the four arrays), the stretch and the candidate, and the walk goes on for the
// other arrays; it stops when every selected array is closed or the run reaches k + H. The bisection (locate_outside: <= 31
// evaluations) runs BEHIND the walk, at most once per (lane, array): the lanes of a wave take that divergent tail together instead
// of inside each other's runs. Past the end only sample traj_len can be a new exit: for v, a and j where the box excludes 0, for q
// where the walk started there (k == traj_len: the last position). mask (LTP_ENV_*) is a kernel argument: scalar branches. One int
// store per selected array and at most one atomicMin (unsigned: LTP_EXIT_NONE > LTP_EXIT_NO_PLAN > every index) per lane; no LDS, no
// barrier, no scratch.
struct ExitBoxes {             // ltp_first_exit_opts' boxes: element (local plan i, joint j) of a given array at ptr[i * sq + j * sj]
    const double* lo[4];
    const double* hi[4];
    long long sq, sj;
};
struct ExitStretch {           // the stretch m0 .. m1 of the run that starts at sample b whose candidate `bad` lies outside
    int b, m0, m1, bad;
};
template <int SEM>
__global__ void __launch_bounds__(256)
k_first_exit(PlanRange r, int mask, int horizon, const int* __restrict__ first_sample, int uniform_first, ExitBoxes box,
             int* __restrict__ exit_sample, unsigned* __restrict__ first_any)
{
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long p = l.p;
    const int j = l.j, dof = r.dof;
    // k_envelope_knots_arrays' decode, written out in both: handed over in one value type it cost this kernel 1 - 3 % on several
    // lines of its benchmark (three shapes tried, none kept the code object; profiles/r22_horizon_rules.txt)
    const bool want_q = (mask & LTP_ENV_Q) != 0, want_v = (mask & LTP_ENV_V) != 0, want_a = (mask & LTP_ENV_A) != 0, want_j = (mask & LTP_ENV_J) != 0;
    const int x_v = (int)want_q, x_a = x_v + (int)want_v, x_j = x_a + (int)want_a, A = x_j + (int)want_j;   // ranks < A <= 4
    int* const dst = exit_sample + ((unsigned long long)l.local * A) * dof + j;                             // plane x at dst[x * dof]
    auto store = [&](int tq, int tv, int ta, int tj) {
        if (want_q) dst[0] = tq;
        if (want_v) dst[(long long)x_v * dof] = tv;
        if (want_a) dst[(long long)x_a * dof] = ta;
        if (want_j) dst[(long long)x_j * dof] = tj;
    };
    const int len = r.rec.traj_len[p];
    if (len <= 0) {
        store(LTP_EXIT_NO_PLAN, LTP_EXIT_NO_PLAN, LTP_EXIT_NO_PLAN, LTP_EXIT_NO_PLAN);
        if (first_any) atomicMin(first_any + l.local, (unsigned)LTP_EXIT_NO_PLAN);
        return;
    }
    const int k = horizon_start(first_sample, uniform_first, l.local, len);
    const long long reach = (long long)k + horizon;             // the horizon is [k, reach); horizon <= 2^30 (the entry's rule)
    const int end_in = reach < (long long)len ? (int)reach : len;   // ... and [k, end_in) of it lies inside the trajectory
    const Limits L = plan_limits(r.lim, p, dof);
    // the boxes, once per lane: a given side from the caller's array, else the plan's own limit on that side
    const long long bx = l.local * box.sq + (long long)j * box.sj;
    double q_lo = 0.0, q_hi = 0.0, v_lo = 0.0, v_hi = 0.0, a_lo = 0.0, a_hi = 0.0, j_lo = 0.0, j_hi = 0.0;
    if (want_q) { q_lo = box.lo[0] ? box.lo[0][bx] : L.q_min[j]; q_hi = box.hi[0] ? box.hi[0][bx] : L.q_max[j]; }
    if (want_v) { v_lo = box.lo[1] ? box.lo[1][bx] : -L.v_max[j]; v_hi = box.hi[1] ? box.hi[1][bx] : L.v_max[j]; }
    if (want_a) { a_lo = box.lo[2] ? box.lo[2][bx] : -L.a_max[j]; a_hi = box.hi[2] ? box.hi[2][bx] : L.a_max[j]; }
    if (want_j) { j_lo = box.lo[3] ? box.lo[3][bx] : -L.j_max[j]; j_hi = box.hi[3] ? box.hi[3][bx] : L.j_max[j]; }
    double q, v, a;
    l.start(r.in, q, v, a);
    bool open_q = want_q, open_v = want_v, open_a = want_a, open_j = want_j;
    ExitStretch at_q{0, 0, 0, kNoCandidate}, at_v = at_q, at_a = at_q;
    double cq[4] = {0.0, 0.0, 0.0, 0.0}, cv[3] = {0.0, 0.0, 0.0}, ca[2] = {0.0, 0.0};   // the closed array's own coefficients
    int t_j = LTP_EXIT_NONE;
    for_each_run<SEM>(L, r.rec, p * dof + j, j, len, r.t_sample, q, v, a, [&](int b, int e, const RunCoef& rc) {
        if (e <= k) return false;                               // a run that ends at or before k
        if (b >= end_in) return true;
        const int s0 = b > k ? b : k, s1 = (e < end_in ? e : end_in) - 1;   // samples s0 .. s1 of the horizon lie in this run
        const int m0 = s0 - b + 1, m1 = s1 - b + 1;
        if (open_q) {
            const int bad = first_outside_candidate(m0, m1, [&] { return qprime_roots(rc.c); }, [&](int m) { return run_eval_q(rc.c, m); }, q_lo, q_hi);
            if (bad != kNoCandidate) {
                open_q = false;
                at_q = ExitStretch{b, m0, m1, bad};
#pragma unroll
                for (int x = 0; x < 4; ++x) cq[x] = rc.c[x];
            }
        }
        if (open_v) {
            const int bad = first_outside_candidate(m0, m1, [&] { return vprime_root(rc.c); }, [&](int m) { return run_eval_v(rc.c + 4, m); }, v_lo, v_hi);
            if (bad != kNoCandidate) {
                open_v = false;
                at_v = ExitStretch{b, m0, m1, bad};
#pragma unroll
                for (int x = 0; x < 3; ++x) cv[x] = rc.c[4 + x];
            }
        }
        if (open_a) {
            const int bad = first_outside_candidate(m0, m1, [] { return no_roots(); }, [&](int m) { return run_eval_a(rc.c + 7, m); }, a_lo, a_hi);
            if (bad != kNoCandidate) {
                open_a = false;
                at_a = ExitStretch{b, m0, m1, bad};
                ca[0] = rc.c[7];
                ca[1] = rc.c[8];
            }
        }
        if (open_j && outside_box(rc.c[9], j_lo, j_hi)) {       // the j line of run_eval: the run's constant
            open_j = false;
            t_j = s0;
        }
        return !(open_q || open_v || open_a || open_j) || e >= end_in;
    }, j == dof - 1);
    // behind the walk: the one sample past the end that can be a new exit, then the bisections of the closed arrays
    const bool past = reach > (long long)len;                   // sample traj_len lies in the horizon
    int t_q = LTP_EXIT_NONE, t_v = LTP_EXIT_NONE, t_a = LTP_EXIT_NONE;
    // (k == traj_len: no run was visited, the walk went to the last sample, which q now holds)
    if (open_q && k == len && outside_box(q, q_lo, q_hi)) t_q = len;
    if (open_v && past && outside_box(0.0, v_lo, v_hi)) t_v = len;
    if (open_a && past && outside_box(0.0, a_lo, a_hi)) t_a = len;
    if (open_j && past && outside_box(0.0, j_lo, j_hi)) t_j = len;
    if (want_q && !open_q)
        t_q = at_q.b - 1 + locate_outside(at_q.m0, at_q.m1, [&] { return qprime_roots(cq); }, [&](int m) { return run_eval_q(cq, m); }, q_lo, q_hi, at_q.bad);
    if (want_v && !open_v) {
        // (vprime_root reads c[5], c[6] of a RunCoef: cv[1], cv[2])
        t_v = at_v.b - 1 + locate_outside(at_v.m0, at_v.m1, [&] { return linear_root(2.0 * cv[2], cv[1]); }, [&](int m) { return run_eval_v(cv, m); }, v_lo, v_hi, at_v.bad);
    }
    if (want_a && !open_a)
        t_a = at_a.b - 1 + locate_outside(at_a.m0, at_a.m1, [] { return no_roots(); }, [&](int m) { return run_eval_a(ca, m); }, a_lo, a_hi, at_a.bad);
    store(t_q, t_v, t_a, t_j);
    if (first_any) {
        unsigned best = (unsigned)LTP_EXIT_NONE;
        if (want_q) best = (unsigned)t_q < best ? (unsigned)t_q : best;
        if (want_v) best = (unsigned)t_v < best ? (unsigned)t_v : best;
        if (want_a) best = (unsigned)t_a < best ? (unsigned)t_a : best;
        if (want_j) best = (unsigned)t_j < best ? (unsigned)t_j : best;
        if (best != (unsigned)LTP_EXIT_NONE) atomicMin(first_any + l.local, best);
    }
}

// Settling (ltp_settle_batch): k_first_exit's question read from the other end — per plan, selected array and joint the sample from
// which S_X(t) is inside its box and STAYS inside for the rest of [k, k + H): max(O) + 1 for O = the outside samples of the horizon,
// k for none, LTP_SETTLE_NOT_YET when sample k + H - 1 is in O, LTP_EXIT_NO_PLAN for traj_len == 0. Same lane, same walk, same
// boxes and values as k_first_exit. Per run that reaches into [k, end_in) and per selected array the lane runs
// last_outside_candidate (ltp_crossings.hpp) on the stretch; a stretch with an outside candidate OVERWRITES that array's saved
// stretch and its own coefficients, so the later run wins, and the walk cannot stop at a find: it stops at end_in, and where the
// horizon reaches past the trajectory it goes to the last sample, which q then holds. No tail run is stepped over (a tail run that
// is also a constant-velocity run still moves: ADVICE.md, first finding). Behind the walk: for reach > traj_len the resting state
// decides LTP_SETTLE_NOT_YET alone (the last position for q, +0.0 for v, a, j); otherwise at most one locate_last_outside per (lane,
// array), which the lanes of a wave take together. mask (LTP_ENV_*) is a kernel argument: scalar branches. One int store per
// selected array and at most one atomicMax (unsigned: LTP_EXIT_NO_PLAN > LTP_SETTLE_NOT_YET > every index, over a fill of 0) per
// lane; no LDS, no barrier, no scratch. Every address derives from l.local, j, dof, A and the mask's ranks alone — k_first_exit's
// expressions — and a plane that is not selected is never stored through.
template <int SEM>
__global__ void __launch_bounds__(256)
k_settle(PlanRange r, int mask, int horizon, const int* __restrict__ first_sample, int uniform_first, ExitBoxes box,
         int* __restrict__ settle_sample, unsigned* __restrict__ settle_all)
{
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long p = l.p;
    const int j = l.j, dof = r.dof;
    const bool want_q = (mask & LTP_ENV_Q) != 0, want_v = (mask & LTP_ENV_V) != 0, want_a = (mask & LTP_ENV_A) != 0, want_j = (mask & LTP_ENV_J) != 0;
    const int x_v = (int)want_q, x_a = x_v + (int)want_v, x_j = x_a + (int)want_a, A = x_j + (int)want_j;   // ranks < A <= 4
    int* const dst = settle_sample + ((unsigned long long)l.local * A) * dof + j;                           // plane x at dst[x * dof]
    auto store = [&](int tq, int tv, int ta, int tj) {
        if (want_q) dst[0] = tq;
        if (want_v) dst[(long long)x_v * dof] = tv;
        if (want_a) dst[(long long)x_a * dof] = ta;
        if (want_j) dst[(long long)x_j * dof] = tj;
    };
    const int len = r.rec.traj_len[p];
    if (len <= 0) {
        store(LTP_EXIT_NO_PLAN, LTP_EXIT_NO_PLAN, LTP_EXIT_NO_PLAN, LTP_EXIT_NO_PLAN);
        if (settle_all) atomicMax(settle_all + l.local, (unsigned)LTP_EXIT_NO_PLAN);
        return;
    }
    const int k = horizon_start(first_sample, uniform_first, l.local, len);
    const long long reach = (long long)k + horizon;             // the horizon is [k, reach); horizon <= 2^30 (the entry's rule)
    const bool past = reach > (long long)len;                   // the resting state lies in the horizon, and is its last sample
    const int end_in = past ? len : (int)reach;                 // [k, end_in) of the horizon lies inside the trajectory
    const Limits L = plan_limits(r.lim, p, dof);
    // the boxes, once per lane: a given side from the caller's array, else the plan's own limit on that side
    const long long bx = l.local * box.sq + (long long)j * box.sj;
    double q_lo = 0.0, q_hi = 0.0, v_lo = 0.0, v_hi = 0.0, a_lo = 0.0, a_hi = 0.0, j_lo = 0.0, j_hi = 0.0;
    if (want_q) { q_lo = box.lo[0] ? box.lo[0][bx] : L.q_min[j]; q_hi = box.hi[0] ? box.hi[0][bx] : L.q_max[j]; }
    if (want_v) { v_lo = box.lo[1] ? box.lo[1][bx] : -L.v_max[j]; v_hi = box.hi[1] ? box.hi[1][bx] : L.v_max[j]; }
    if (want_a) { a_lo = box.lo[2] ? box.lo[2][bx] : -L.a_max[j]; a_hi = box.hi[2] ? box.hi[2][bx] : L.a_max[j]; }
    if (want_j) { j_lo = box.lo[3] ? box.lo[3][bx] : -L.j_max[j]; j_hi = box.hi[3] ? box.hi[3][bx] : L.j_max[j]; }
    double q, v, a;
    l.start(r.in, q, v, a);
    ExitStretch at_q{0, 0, 0, kNoLastCandidate}, at_v = at_q, at_a = at_q;   // the LATEST stretch with an outside candidate
    double cq[4] = {0.0, 0.0, 0.0, 0.0}, cv[3] = {0.0, 0.0, 0.0}, ca[2] = {0.0, 0.0};   // ... and that array's own coefficients of its run
    int last_j = -1;                                            // the last sample of the latest run whose jerk is outside
    for_each_run<SEM>(L, r.rec, p * dof + j, j, len, r.t_sample, q, v, a, [&](int b, int e, const RunCoef& rc) {
        if (e <= k) return false;                               // a run that ends at or before k
        if (b >= end_in) return true;
        const int s0 = b > k ? b : k, s1 = (e < end_in ? e : end_in) - 1;   // samples s0 .. s1 of the horizon lie in this run
        const int m0 = s0 - b + 1, m1 = s1 - b + 1;
        if (want_q) {
            const int bad = last_outside_candidate(m0, m1, [&] { return qprime_roots(rc.c); }, [&](int m) { return run_eval_q(rc.c, m); }, q_lo, q_hi);
            if (bad != kNoLastCandidate) {
                at_q = ExitStretch{b, m0, m1, bad};
#pragma unroll
                for (int x = 0; x < 4; ++x) cq[x] = rc.c[x];
            }
        }
        if (want_v) {
            const int bad = last_outside_candidate(m0, m1, [&] { return vprime_root(rc.c); }, [&](int m) { return run_eval_v(rc.c + 4, m); }, v_lo, v_hi);
            if (bad != kNoLastCandidate) {
                at_v = ExitStretch{b, m0, m1, bad};
#pragma unroll
                for (int x = 0; x < 3; ++x) cv[x] = rc.c[4 + x];
            }
        }
        if (want_a) {
            const int bad = last_outside_candidate(m0, m1, [] { return no_roots(); }, [&](int m) { return run_eval_a(rc.c + 7, m); }, a_lo, a_hi);
            if (bad != kNoLastCandidate) {
                at_a = ExitStretch{b, m0, m1, bad};
                ca[0] = rc.c[7];
                ca[1] = rc.c[8];
            }
        }
        if (want_j && outside_box(rc.c[9], j_lo, j_hi)) last_j = s1;   // the j line of run_eval: the run's constant
        // a horizon that ends inside the trajectory ends the walk; one that reaches past it walks on to the last sample, for q
        return !past && e >= end_in;
    }, j == dof - 1);
    // behind the walk. With `past` the walk went to the last sample, which q now holds, and the resting state is sample reach - 1;
    // without it sample reach - 1 = end_in - 1 is a trajectory sample, outside exactly where it is the last outside one.
    const bool rest_q = want_q && past && outside_box(q, q_lo, q_hi);
    const bool rest_v = want_v && past && outside_box(0.0, v_lo, v_hi);
    const bool rest_a = want_a && past && outside_box(0.0, a_lo, a_hi);
    const bool rest_j = want_j && past && outside_box(0.0, j_lo, j_hi);
    auto settled = [&](int s) { return !past && s == end_in - 1 ? LTP_SETTLE_NOT_YET : s + 1; };   // s: the last outside sample
    int t_q = k, t_v = k, t_a = k, t_j = k;
    if (rest_q) t_q = LTP_SETTLE_NOT_YET;
    else if (want_q && at_q.bad != kNoLastCandidate)
        t_q = settled(at_q.b - 1 + locate_last_outside(at_q.m0, at_q.m1, [&] { return qprime_roots(cq); }, [&](int m) { return run_eval_q(cq, m); }, q_lo, q_hi, at_q.bad));
    if (rest_v) t_v = LTP_SETTLE_NOT_YET;
    else if (want_v && at_v.bad != kNoLastCandidate) {
        // (vprime_root reads c[5], c[6] of a RunCoef: cv[1], cv[2])
        t_v = settled(at_v.b - 1 + locate_last_outside(at_v.m0, at_v.m1, [&] { return linear_root(2.0 * cv[2], cv[1]); }, [&](int m) { return run_eval_v(cv, m); }, v_lo, v_hi, at_v.bad));
    }
    if (rest_a) t_a = LTP_SETTLE_NOT_YET;
    else if (want_a && at_a.bad != kNoLastCandidate)
        t_a = settled(at_a.b - 1 + locate_last_outside(at_a.m0, at_a.m1, [] { return no_roots(); }, [&](int m) { return run_eval_a(ca, m); }, a_lo, a_hi, at_a.bad));
    if (rest_j) t_j = LTP_SETTLE_NOT_YET;
    else if (last_j >= 0) t_j = settled(last_j);
    store(t_q, t_v, t_a, t_j);
    if (settle_all) {
        unsigned best = 0u;
        if (want_q) best = (unsigned)t_q > best ? (unsigned)t_q : best;
        if (want_v) best = (unsigned)t_v > best ? (unsigned)t_v : best;
        if (want_a) best = (unsigned)t_a > best ? (unsigned)t_a : best;
        if (want_j) best = (unsigned)t_j > best ? (unsigned)t_j : best;
        if (best != 0u) atomicMax(settle_all + l.local, best);
    }
}

// ---------------------------------------------------------------------------------------
// Receding horizon (reference README.md:10-13): the start state of the next plan is the state
// at sample k of the previous trajectory, gathered on the device without a host round trip.
// ---------------------------------------------------------------------------------------
// Stored sample k of a plan that has n of them, k per plan or the same for all: below 0 is sample 0, beyond the end the last one
LTP_DEV int clamped_sample(const int* __restrict__ sample_index, int uniform_index, long long local, int n)
{
    const int k = sample_index ? sample_index[local] : uniform_index;
    return k < 0 ? 0 : (k >= n ? n - 1 : k);
}

// A plan the sampler left out of the tile, so that the restart state is the start state carried over and nothing outside the tile is
// read: no trajectory, flagged by the sampler as not fitting its tile, or rows that would end beyond the tile — the test every
// sampler applies before it sets that flag (plan_beyond_tile, ltp_sampler_policy.hpp). slen: stored_len of the plan;
// rel, stride: where its rows start in the tile and their padded length.
LTP_DEV bool sampler_skipped(const PlanRange& r, long long p, int slen, const unsigned long long* __restrict__ offsets, unsigned long long capacity,
                             unsigned long long& rel, unsigned long long& stride)
{
    stride = row_stride((unsigned long long)slen);
    rel = offsets[p] - offsets[r.first];
    return slen <= 0 || (r.rec.status[p] & kStatusOverflow) || plan_beyond_tile(rel, slen, r.dof, capacity);
}

template <typename T>
__global__ void __launch_bounds__(256)
k_replan_states(PlanRange r, RowSpec rows, const unsigned long long* __restrict__ offsets, const T* __restrict__ tile, unsigned long long capacity,
                const int* __restrict__ sample_index, int uniform_index,
                double* __restrict__ q_0, double* __restrict__ v_0, double* __restrict__ a_0, long long sq, long long sj)
{
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long dst = l.local * sq + (long long)l.j * sj;
    const int slen = stored_len(r.rec.traj_len[l.p], rows);
    unsigned long long rel, stride;
    if (sampler_skipped(r, l.p, slen, offsets, capacity, rel, stride)) {
        l.start(r.in, q_0[dst], v_0[dst], a_0[dst]);
        return;
    }
    const int k = clamped_sample(sample_index, uniform_index, l.local, slen);
    const T* row = tile + rel + (unsigned long long)l.j * stride + k;
    const unsigned long long arr = (unsigned long long)r.dof * stride;
    q_0[dst] = (double)row[0];
    v_0[dst] = (double)row[arr];
    a_0[dst] = (double)row[2 * arr];
}

// Receding horizon without any sampled rows: the state (q, v, a) at trajectory sample k of every plan straight from
// the switching-time records. A caller that only needs the restart state pays neither the table build of a sampler
// item (~15 us of latency per plan) nor a byte of trajectory traffic. The result has the bits of the row element the
// sampler would have stored at k.
template <int SEM>
__global__ void __launch_bounds__(256)
k_state_at(PlanRange r, const int* __restrict__ sample_index, int uniform_index,
           double* __restrict__ q_0, double* __restrict__ v_0, double* __restrict__ a_0, long long sq, long long sj)
{
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long p = l.p;
    const int j = l.j, dof = r.dof;
    const long long dst = l.local * sq + (long long)j * sj;
    double q, v, a;
    l.start(r.in, q, v, a);
    const int len = r.rec.traj_len[p];
    if (len > 0) {
        const int k = clamped_sample(sample_index, uniform_index, l.local, len);
        for_each_run<SEM>(plan_limits(r.lim, p, dof), r.rec, p * dof + j, j, len, r.t_sample, q, v, a, [&](int b, int e, const RunCoef& rc) {
            if (k >= e) return false;
            double jj;
            run_eval(rc.c, k + 1 - b, q, v, a, jj);
            return true;
        }, j == dof - 1);
    }
    q_0[dst] = q;
    v_0[dst] = v;
    a_0[dst] = a;
}

// ltp_replan_states_batch for float64 tiles: the restart state = STORED sample k of the rows ltp_sample_batch wrote. Those rows hold
// run_eval(run_coef(..)) of the run walk below, bit for bit, so the state is recomputed from the records (k_state_at's walk, ~0.1 ms
// per 1 M plans) instead of being gathered from the tile by 21 M scattered 8-byte reads (0.385 ms, at the rate of DRAM sectors):
// the tile is not read at all. Plans the sampler skipped (sampler_skipped) keep their start state, as in k_replan_states.
template <int SEM>
__global__ void __launch_bounds__(256)
k_replan_walk(PlanRange r, RowSpec rows, const unsigned long long* __restrict__ offsets, unsigned long long capacity,
              const int* __restrict__ sample_index, int uniform_index,
              double* __restrict__ q_0, double* __restrict__ v_0, double* __restrict__ a_0, long long sq, long long sj)
{
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long p = l.p;
    const int j = l.j, dof = r.dof;
    const long long dst = l.local * sq + (long long)j * sj;
    double q, v, a;
    l.start(r.in, q, v, a);
    const int len = r.rec.traj_len[p];
    const int slen = stored_len(len, rows);
    unsigned long long rel, stride;
    if (!sampler_skipped(r, p, slen, offsets, capacity, rel, stride)) {
        const int k = clamped_sample(sample_index, uniform_index, l.local, slen);
        const int kt = k * (rows.stride > 1 ? rows.stride : 1);   // stored sample k is trajectory sample k * stride (< len)
        for_each_run<SEM>(plan_limits(r.lim, p, dof), r.rec, p * dof + j, j, len, r.t_sample, q, v, a, [&](int b, int e, const RunCoef& rc) {
            if (kt >= e) return false;
            double jj;
            run_eval(rc.c, kt + 1 - b, q, v, a, jj);
            return true;
        }, j == dof - 1);
    }
    q_0[dst] = q;
    v_0[dst] = v;
    a_0[dst] = a;
}

// planTrajectory's end-limit check (cc:59-61) without sampled rows: lane = (plan, joint) walks its runs to the last
// trajectory sample — the bits k_sample would have stored at traj_len-1, which is also what build_run_tables step (5)
// tests — and flags the plan if that position lies outside the joint range. (walk_may_stop_at: the two or three one-sample runs
// behind s6 need not be walked.)
__global__ void __launch_bounds__(256)
k_end_limit(PlanRange r)
{
    const PlanLane l = plan_lane(r);
    if (!l.live) return;
    const long long p = l.p;
    const int j = l.j;
    const int len = r.rec.traj_len[p];
    if (len <= 0) return;                                     // failed before sampling: the reference never gets to cc:59
    double q, v, a;
    l.start(r.in, q, v, a);
    const Limits L = plan_limits(r.lim, p, r.dof);
    for_each_run(L, r.rec, p * r.dof + j, j, len, r.t_sample, q, v, a, [](int, int, const RunCoef& rc) { return walk_may_stop_at(rc); });
    if (beyond_end_limits(q, L.q_min[j], L.q_max[j])) atomicOr(&r.rec.status[p], kStatusEndLimit);
}

// The table pass: the run tables of plans [first, first + count) as a kernel of its own, lane = (plan, joint), everything
// in registers (the walk of k_state_at), written word for word in the JointTable layout. A sampler item then costs one
// (prefetched) table read instead of a cooperative build of ~8 us of latency — what short rows, the envelope consumer and
// receding-horizon rows are bound by. 912 bytes per joint (packed): worth it when a plan's rows are not much longer than that.
// Also applies the end-limit check of cc:59-61 (the sampler variants that read tables no longer do).
template <int SEM>
__global__ void __launch_bounds__(256)
k_build_tables(PlanRange r, int needed_end /* runs that start at or after this sample are not stored (capped rows) */,
               const unsigned long long* __restrict__ offsets /* nullptr: no row offsets wanted */, long long base_first,
               unsigned long long* __restrict__ tables)
{
    // (plan_lane, its start state and beyond_end_limits written out: with any one of them the C++-semantics instantiation takes one
    // more VGPR, profiles/r11_readers_refactor.txt)
    const int dof = r.dof;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= r.count * dof) return;
    const long long local = idx / dof;
    const int j = (int)(idx - local * dof);
    const long long p = r.first + local;
    const Records& rec = r.rec;
    const unsigned long long lane_id = (unsigned long long)idx;
    auto word = [&](int w) -> unsigned long long* { return tables + table_word_index(lane_id, w); };
    const int len = rec.traj_len[p];
    typedef double pair_t __attribute__((ext_vector_type(2)));
    auto store_pair = [&](int w, double lo, double hi) {        // 16 bytes per lane: a full 1 KiB line per wave instruction
        pair_t v2;
        v2[0] = lo;
        v2[1] = hi;
        __builtin_nontemporal_store(v2, reinterpret_cast<pair_t*>(word(w)));
    };
    if (len <= 0) { *word(0) = 0ull; return; }                 // nseg 0: the sampler skips such plans anyway
    const long long ix = p * r.in.sq + (long long)j * r.in.sj;
    double q = r.in.q_0[ix], v = r.in.v_0[ix], a = r.in.a_0[ix];
    store_pair(12, rec.v_drive[p * dof + j] * rec.dir[p * dof + j], 0.0);   // vsnap, as for_each_run forms it (cc:823)
    const Limits L = plan_limits(r.lim, p, dof);
    // Packed runs: five words each, stored as word pairs two runs at a time. A lane whose runs are past the cap stores zeros as
    // long as a neighbour still stores: the lanes of a wave are the lanes of one table tile, and a 1 KiB line written whole costs
    // HBM half of what the same line written by some of its lanes does (measured: 1.53 -> 1.1 ms for the same tables).
    int run = 0, slots = 0;
    int last_b = len;
    double ha = 0.0, hv = 0.0, hq = 0.0, hj = 0.0, hm = 0.0;     // the even run of a pair, until its odd partner arrives
    auto as_word = [](int mode) { return __builtin_bit_cast(double, (unsigned long long)(unsigned)mode); };
    for_each_run<SEM>(L, rec, p * dof + j, j, len, r.t_sample, q, v, a, [&](int b, int, const RunCoef& rc) {
        const bool mine = b < needed_end;
        if (__builtin_amdgcn_ballot_w64(mine) != 0ull) {
            // q, v, a still hold the state before this run: for_each_run advances them after the visit
            const double sa = mine ? a : 0.0, sv = mine ? v : 0.0, sq = mine ? q : 0.0, sj = mine ? rc.c[9] : 0.0;
            const double sm = mine ? as_word(rc.mode) : 0.0;
            if (mine) {
                reinterpret_cast<int*>(word(1 + (run >> 1)))[run & 1] = b;
                ++run;
            }
            if (slots & 1) {
                const int w0 = kPackedHeaderWords + (slots - 1) * kPackedRunWords;   // even: a pair boundary
                store_pair(w0, ha, hv); store_pair(w0 + 2, hq, hj); store_pair(w0 + 4, hm, sa); store_pair(w0 + 6, sv, sq); store_pair(w0 + 8, sj, sm);
            } else {
                ha = sa; hv = sv; hq = sq; hj = sj; hm = sm;
            }
            ++slots;
        }
        if (!mine && last_b == len) last_b = b;                  // first run that is not stored: it ends the last stored one
        return false;                                          // the walk still goes to the last sample: end-limit check
    }, j == dof - 1);
    if (slots & 1) {
        const int w0 = kPackedHeaderWords + (slots - 1) * kPackedRunWords;
        store_pair(w0, ha, hv); store_pair(w0 + 2, hq, hj); store_pair(w0 + 4, hm, 0.0);
    }
    static_assert(kPackedHeaderWords % 2 == 0 && (2 * kPackedRunWords) % 2 == 0, "two runs start on a word pair");
    reinterpret_cast<int*>(word(1 + (run >> 1)))[run & 1] = last_b;
    *word(0) = (unsigned long long)(unsigned)run | ((unsigned long long)(unsigned)len << 32);
    // where the plan's rows start inside the range the sampler is called for: what k_sample_tab's loader would otherwise
    // have to load per item (plan sizes are multiples of kRowAlign elements)
    // (saturated: an offset that does not fit 32 bits is beyond any tile, and the sampler then flags the plan as not fitting)
    if (offsets) {
        const unsigned long long rel = (offsets[p] - offsets[base_first]) / kRowAlign;
        reinterpret_cast<unsigned*>(word(1 + (kMaxSegments + 1) / 2))[(kMaxSegments + 1) & 1] = rel > 0xffffffffull ? 0xffffffffu : (unsigned)rel;
    }
    if constexpr (SEM == kSemCpp) {                            // LTPlanner.m has no position limits, hence no end-limit check
        if (q < L.q_min[j] || q > L.q_max[j]) atomicOr(&rec.status[p], kStatusEndLimit);   // cc:59-61: q is sample len-1
    }
}

int envelope_resident_blocks(int device)
{
    int cus = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_envelope<false, false>, kSampleThreads, 0);
    if (e != hipSuccess || per_cu <= 0) per_cu = 4;
    return cus * per_cu;
}

unsigned long long table_bytes(long long lanes) { return run_table_bytes(lanes); }

void launch_build_tables(hipStream_t s, const PlanRange& r, RowSpec rows, bool whole_trajectory, const unsigned long long* offsets, long long base_first,
                         unsigned long long* tables)
{
    // capped rows only touch the samples before max_samples * stride
    long long needed = 0x7fffffffll;
    if (!whole_trajectory && rows.max_samples > 0) needed = (long long)rows.max_samples * (rows.stride > 1 ? rows.stride : 1);
    if (needed > 0x7fffffffll) needed = 0x7fffffffll;
    dispatch_semantics(r.semantics, [&](auto v) { launch_lanes(s, r, k_build_tables<decltype(v)::value>, (int)needed, offsets, base_first, tables); });
}

void launch_envelope(hipStream_t s, const PlanRange& r, long long base_first, int window, int n_windows, double* env, unsigned long long* next_item,
                     int resident_blocks, unsigned long long* probe, const unsigned long long* tables, bool analytic)
{
    if (r.count <= 0 || n_windows <= 0) return;
    const int dof = r.dof;
    const int ngroups = (dof + kSampleJointGroup - 1) / kSampleJointGroup;
    long long blocks = resident_blocks > 0 ? resident_blocks : 1536;
    if (blocks > r.count * ngroups) blocks = r.count * ngroups;
    // lanes per (joint, window) task: the largest power of two <= 64 that still gives every lane of a block a task
    const long long tasks = (long long)(dof < kSampleJointGroup ? dof : kSampleJointGroup) * n_windows;
    int lg = 0;
    while (lg < 6 && (tasks << (lg + 1)) <= kSampleThreads && (2 << lg) <= window) ++lg;
    auto launch = [&](auto kernel, int lanes_lg) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kSampleThreads), 0, s, r.first, r.count, base_first, dof, r.t_sample, r.lim, r.in, r.rec,
                           window, n_windows, lanes_lg, env, next_item, probe, tables);
    };
    // the analytic form looks at a handful of samples per run and window: one lane per (joint, window) task
    if (analytic && !probe) tables ? launch(k_envelope<false, true, true>, 0) : launch(k_envelope<false, false, true>, 0);
    else if (probe) launch(k_envelope<true, false>, lg);
    else tables ? launch(k_envelope<false, true>, lg) : launch(k_envelope<false, false>, lg);
}

void launch_envelope_walk(hipStream_t s, const PlanRange& r, long long base_first, int window, int n_windows, double* env)
{
    if (n_windows <= 0) return;
    dispatch_semantics(r.semantics, [&](auto v) { launch_lanes(s, r, k_envelope_walk<decltype(v)::value>, base_first, window, n_windows, env); });
}

void launch_envelope_knots(hipStream_t s, const PlanRange& r, int n_intervals, int closed, const int* edges, const int* first_sample,
                           int uniform_first, int* valid, double* env)
{
    if (n_intervals < 1 || n_intervals > kMaxKnots - 1) return;
    dispatch_semantics(r.semantics, [&](auto v) {
        launch_lanes(s, r, k_envelope_knots<decltype(v)::value>, n_intervals, closed, edges, first_sample, uniform_first, valid, env);
    });
}

void launch_envelope_knots_arrays(hipStream_t s, const PlanRange& r, int n_intervals, int closed, int arrays, const int* edges,
                                  const int* first_sample, int uniform_first, int* valid, double* env)
{
    if (n_intervals < 1 || n_intervals > kMaxKnots - 1 || arrays < 1 || arrays > 15) return;
    dispatch_semantics(r.semantics, [&](auto v) {
        launch_lanes(s, r, k_envelope_knots_arrays<decltype(v)::value>, n_intervals, closed, arrays, edges, first_sample, uniform_first, valid, env);
    });
}

// launch_first_exit and launch_settle behind their two names: the arguments are checked, the fold (first_any / settle_all), where
// given, is set to its start value by the reader's fill kernel, and the reader's kernel of the plans' semantics — kernel_of(v), v
// dispatch_semantics' tag — fills the table.
template <class FoldInit, class KernelOf>
static void launch_box_reader(hipStream_t s, const PlanRange& r, int arrays, int horizon, const int* first_sample, int uniform_first,
                              const double* const (&lo)[4], const double* const (&hi)[4], long long box_query_stride, long long box_joint_stride,
                              int* table, int* fold, FoldInit fold_init, KernelOf kernel_of)
{
    if (arrays < 1 || arrays > 15 || horizon < 1 || horizon > kKnotOffsetMax || r.count <= 0 || r.dof <= 0) return;
    if (fold) hipLaunchKernelGGL(fold_init, dim3((unsigned)((r.count + 255) / 256)), dim3(256), 0, s, r.count, fold);
    ExitBoxes box;
    for (int x = 0; x < 4; ++x) { box.lo[x] = lo[x]; box.hi[x] = hi[x]; }
    box.sq = box_query_stride;
    box.sj = box_joint_stride;
    dispatch_semantics(r.semantics, [&](auto v) {
        launch_lanes(s, r, kernel_of(v), arrays, horizon, first_sample, uniform_first, box, table, reinterpret_cast<unsigned*>(fold));
    });
}

// first_any starts from LTP_EXIT_NONE in every plan. A kernel, not a memset: the memset node of a captured graph did not write its
// value on a second replay (profiles/r21_first_exit.txt), a kernel node does.
__global__ void __launch_bounds__(256)
k_first_any_init(long long count, int* __restrict__ first_any)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) first_any[i] = LTP_EXIT_NONE;
}

void launch_first_exit(hipStream_t s, const PlanRange& r, int arrays, int horizon, const int* first_sample, int uniform_first,
                       const double* const (&lo)[4], const double* const (&hi)[4], long long box_query_stride, long long box_joint_stride,
                       int* exit_sample, int* first_any)
{
    launch_box_reader(s, r, arrays, horizon, first_sample, uniform_first, lo, hi, box_query_stride, box_joint_stride, exit_sample, first_any,
                      k_first_any_init, [](auto v) { return k_first_exit<decltype(v)::value>; });
}

// settle_all starts from 0 in every plan, below every answer but "inside throughout from sample 0". A kernel, not a memset: see
// k_first_any_init.
__global__ void __launch_bounds__(256)
k_settle_all_init(long long count, int* __restrict__ settle_all)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) settle_all[i] = 0;
}

void launch_settle(hipStream_t s, const PlanRange& r, int arrays, int horizon, const int* first_sample, int uniform_first,
                   const double* const (&lo)[4], const double* const (&hi)[4], long long box_query_stride, long long box_joint_stride,
                   int* settle_sample, int* settle_all)
{
    launch_box_reader(s, r, arrays, horizon, first_sample, uniform_first, lo, hi, box_query_stride, box_joint_stride, settle_sample, settle_all,
                      k_settle_all_init, [](auto v) { return k_settle<decltype(v)::value>; });
}

void launch_replan_states(hipStream_t s, const PlanRange& r, RowSpec rows, const unsigned long long* offsets, const void* tile, bool f32,
                          unsigned long long capacity, const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                          long long sq, long long sj)
{
    if (f32)      // float rows hold ROUNDED values: the caller gets what the tile holds
        launch_lanes(s, r, k_replan_states<float>, rows, offsets, (const float*)tile, capacity, sample_index, uniform_index, q_0, v_0, a_0, sq, sj);
    else
        dispatch_semantics(r.semantics, [&](auto v) {
            launch_lanes(s, r, k_replan_walk<decltype(v)::value>, rows, offsets, capacity, sample_index, uniform_index, q_0, v_0, a_0, sq, sj);
        });
}

void launch_end_limit(hipStream_t s, const PlanRange& r) { launch_lanes(s, r, k_end_limit); }

void launch_state_at(hipStream_t s, const PlanRange& r, const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                     long long sq, long long sj)
{
    dispatch_semantics(r.semantics, [&](auto v) { launch_lanes(s, r, k_state_at<decltype(v)::value>, sample_index, uniform_index, q_0, v_0, a_0, sq, sj); });
}

}  // namespace ltp
