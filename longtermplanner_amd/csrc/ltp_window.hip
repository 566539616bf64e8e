// ltp_window.hip — horizon windows (ltp_sample_window_batch, include/ltp_hip.h), gfx950: for every plan of a planned batch the
// N trajectory samples [k, k + N) of all four arrays, k per plan, in a FIXED layout — local plan i at out + i * 4 * dof * R,
// [q,v,a,j][joint][R], R = ltp_row_stride(N) — so that nothing of the offsets scan, the status or the handle's workspace is read or
// written. What a controller that follows existing plans needs every control period (reference README.md:10-13).
//
// The arithmetic is the other consumers': the lane-per-(plan, joint) run walk of ltp_runs.hpp (for_each_run -> run_coef) and
// run_eval(c, t + 1 - b) of include/ltp_run_tables.hpp, k_state_at's form, so every real sample has the bits ltp_sample_batch stores
// at trajectory sample t of that row. Samples at or past traj_len hold the last position with v = a = j = +0.0 (the robot rests
// there); plans without a trajectory get NaN in all four arrays.
//
// Shape: autonomous waves. A block is ONE wave; it owns 64 consecutive (plan, joint) lanes (lane index = local * dof + j) and talks
// to nobody — no queue, no flag, no atomic.
//   walk    per lane, divergent: the lane walks its runs, skips those that end at or before its next sample, and parks the next
//           <= kWindowRuns runs that overlap the window in LDS: the run's first sample inside the window, the offset that turns a
//           window sample into the run position m, and the ten RunCoef words; plus where its hold (or NaN) samples start and end.
//           Nothing wave-level sits inside the visit callback.
//   stream  converged: the wave goes through its 64 rows; for a row lane l takes samples l, l + 64, ..., finds the parked run that
//           holds its sample (the runs' first samples are read at one LDS address each: broadcasts), reads that run's coefficients
//           and evaluates: the stores of one instruction are consecutive elements of one row (512 bytes for float64), on a
//           64-element grid of the row, however short the runs are. For N <= 32 the two halves of the wave take two rows at once.
// A window that overlaps more than kWindowRuns runs of a lane (wide windows: N = 4096 holds whole trajectories) takes further
// walk + stream passes, each from where the lane's previous pass stopped; the pass loop is wave-uniform (a ballot outside the
// callback) and bounded by window_passes_bound(runs) = ceil(kMaxSegments / runs).
//
// Strided horizons (ltp_sample_horizon_batch): element w of a row is trajectory sample k + w * stride. Everything a pass keeps is
// then in window ELEMENTS: a run [b, e) delivers the elements [ceil((b - k) / stride), ceil((e - k) / stride)) — compared in the
// run-relative coordinates b - k and e - k, k + N * stride is never formed — and a run that holds no element is not parked: it
// takes none of the kWindowRuns slots, so the ranges of the parked runs still follow one another without a gap and the pass loop
// keeps its bound. The dense mode is the window call: stride 1 at compile time, so its walk holds no division.
//
// Knot grids (ltp_sample_knots_batch): element w is trajectory sample k + g[w], g one non-decreasing list of <= LTP_MAX_KNOTS offsets
// per call. The two places the stride entered are the two places the grid enters: "how many elements lie below trajectory offset x"
// is knots_below (ltp_knots.hpp: a lower bound over the grid in a fixed, wave-uniform number of steps, so the visit callback still
// holds nothing wave-level and no data-dependent loop), and "the trajectory offset of element s" is a load of g[s]. The block
// stages the grid in LDS once, before the first walk, clamped to [0, 2^30]: whatever the caller's list holds, every count is in
// [0, N] and every element range is clamped to [from, N] as before, so a grid that breaks the contract changes values, never an
// address. A run without a knot is not parked, so the pass bound stands; the hold elements start at knots_below(traj_len - k).
// On such a grid the counts need not grow from run to run: within a pass `cover` can move backwards and the parked sb are no longer
// ordered, so the parked ranges need not tile [pf, hb). Memory safety does NOT rely on that order — only the values do: every sb
// and se is clamped to [from, N], a parked run has se > sb >= from (the pass loop, bounded by window_passes_bound anyway, moves on),
// and the stream phase takes s from [pf, N) only and reads G[s] and the slots [0, np) of its row, whatever sb they hold.
//
// Stop horizons (ltp_stop_knots_batch: k_stop_knots): the knots mode with another sink. The walk and the stream phase are stated ONCE,
// in window_passes(); what a kernel does with element s of a row — (q, v, a, j) as the knots mode stores them — is its sink, called
// where the rows were stored, lane = element. k_sample_window's sink is window_store; k_stop_knots' sink clamps (or checks) the
// acceleration against the row's a_max, calls opt_braking and stores q + qb and the sum of the three braking phases in two planes,
// [count][{q_stop, t_stop}][dof][R]. Each lane parks the four limit words opt_braking reads for its (plan, joint) — a_max, j_max and
// tj, tj^3 of its LimPow — in LDS before the first walk; the stream phase reads them at one address per row.
#include "ltp_knots.hpp"
#include "ltp_runs.hpp"

namespace ltp {

constexpr int kWindowRuns = 6;                                                   // runs parked per lane and pass (k_sample_window)
constexpr int window_passes_bound(int runs) { return (kMaxSegments + runs - 1) / runs; }   // every pass but the last parks `runs` runs
constexpr int kWindowLanes = 64;                                                 // one wave per block

// [..][lane]: a lane's own words are 64 words apart, so the walk's stores are conflict-free and the stream's reads of one row are
// one address per parked run; a run's coefficient block is two words longer than 10 x 64, which puts the blocks of different runs
// on different banks (lanes of one row that sit in different runs read their coefficients without a conflict)
constexpr int kWindowCoefStride = kRunCoefs * kWindowLanes + 2;
template <int RUNS>
struct WindowLds {
    double c[RUNS * kWindowCoefStride];           // word x of parked run r of lane l at r * kWindowCoefStride + x * 64 + l
    int sb[RUNS][kWindowLanes];                   // first element of the parked run inside the window; the runs follow one another
    int mo[RUNS][kWindowLanes];                   // m = w * stride + mo: position of window element w in the run (k + 1 - b)
    double hold_q[kWindowLanes];                  // position of samples [hb, he): the last sample's, or NaN
    double hold_z[kWindowLanes];                  // their v, a, j: +0.0, or NaN
    unsigned long long base[kWindowLanes];        // element offset of the q row of this (plan, joint) in `out`
    int np[kWindowLanes];                         // runs parked in this pass
    int pf[kWindowLanes];                         // first window element this pass delivers: the parked runs cover [pf, hb)
    int hb[kWindowLanes], he[kWindowLanes];       // window elements past the end (or of a plan without a trajectory) in this pass
};
static_assert(sizeof(WindowLds<kWindowRuns>) * 4 <= 160 * 1024, "four blocks per compute unit (160 KiB of LDS)");
static_assert((sizeof(WindowLds<kWindowRuns>) + kMaxKnots * sizeof(int)) * 4 <= 160 * 1024, "four blocks per compute unit with a staged knot grid too");

// How element w of a row maps to a trajectory sample. The fourth-last kernel argument is the stride (an int, read by the strided
// mode only) or, in the knots mode, the grid.
enum WindowMode { kWindowDense = 0, kWindowStrided = 1, kWindowKnots = 2 };
template <int MODE> struct WindowGridArg { using type = int; };
template <> struct WindowGridArg<kWindowKnots> { using type = const int*; };

// the staged grid: LDS that exists in the knots instantiations only
template <int MODE>
LTP_DEV int* window_knots_lds()
{
    if constexpr (MODE == kWindowKnots) {
        __shared__ int g[kMaxKnots];
        return g;
    } else {
        return nullptr;
    }
}

template <typename T>
LTP_DEV void window_store(T* __restrict__ out, unsigned long long at, unsigned long long plane, double q, double v, double a, double j)
{
    __builtin_nontemporal_store((T)q, out + at);
    __builtin_nontemporal_store((T)v, out + at + plane);
    __builtin_nontemporal_store((T)a, out + at + 2 * plane);
    __builtin_nontemporal_store((T)j, out + at + 3 * plane);
}

// elements of a grid of step s (from 0) below x: ceil(x / s) for x > 0, else 0; x + s is never formed
LTP_DEV int window_grid_below(int x, int s) { return x > 0 ? (int)((unsigned)(x - 1) / (unsigned)s) + 1 : 0; }

// The walk + stream passes of one block over its 64 (plan, joint) rows: every kernel of this file is this function with its own sink.
// PLANES: arrays per plan in the kernel's buffer (a row of array x of local plan i starts at ((i * PLANES + x) * dof + j) * R). RUNS: runs
// parked per lane and pass. park(p, j): called once by every live lane before the first walk (what the sink wants in LDS per row; the
// barrier that ends the first walk orders it). sink(row, at, q, v, a, j): element at - base of block row `row`, `at` its offset in
// array 0; called in the stream phase, lane = element, by the lanes whose element this pass delivers.
template <int SEM, int MODE, int PLANES, int RUNS, class Park, class Sink>
LTP_DEV void window_passes(long long first, long long count, int dof, double t_sample, const PlanLimits& lim, const Queries& in,
                           const Records& rec, int N, int R, typename WindowGridArg<MODE>::type grid_arg,
                           const int* __restrict__ first_sample, int uniform_first, int* __restrict__ valid, Park park, Sink sink)
{
    constexpr bool STRIDED = MODE == kWindowStrided, KNOTS = MODE == kWindowKnots;
    int stride = 1;                                            // wave-uniform; element w is trajectory sample k + w * stride
    if constexpr (STRIDED) stride = grid_arg;
    __shared__ WindowLds<RUNS> S;
    const int l = (int)threadIdx.x;
    // knots: element w is trajectory sample k + G[w]; N <= kMaxKnots (the entry's rule). Staged once, 64 offsets per load
    int* const G = window_knots_lds<MODE>();
    int steps = 0;                                             // of every knots_below: wave-uniform
    if constexpr (KNOTS) {
        steps = knots_steps(N);
        for (int w = l; w < N; w += kWindowLanes) G[w] = knot_clamp(grid_arg[w]);
        __syncthreads();
    }
    // elements below trajectory offset x: those w with w * stride < x, or G[w] < x
    auto below = [&](int x) {
        if constexpr (KNOTS) return knots_below(G, N, steps, x);
        else if constexpr (STRIDED) return window_grid_below(x, stride);
        else return x;
    };
    const long long total = count * dof;
    const long long idx = (long long)blockIdx.x * kWindowLanes + l;
    const bool live = idx < total;

    long long p = 0;
    int j = 0, len = 0, k = 0;
    if (live) {
        const long long local = idx / dof;
        j = (int)(idx - local * dof);
        p = first + local;
        len = rec.traj_len[p];
        k = first_sample ? first_sample[local] : uniform_first;
        k = k < 0 ? 0 : k;
        if (len > 0 && k > len) k = len;                      // every sample of such a window is past the end, as from k = len
        if (valid && j == 0) {
            const int left = len > 0 ? below(len - k) : 0;
            valid[local] = left < N ? left : N;
        }
        S.base[l] = ((unsigned long long)local * (unsigned long long)PLANES * (unsigned long long)dof + (unsigned long long)j) * (unsigned long long)R;
        park(p, j);
    }
    // rows of this block, and how the wave is laid over them: all 64 lanes on one row, or 32 on each of two (N <= 32)
    const long long rows_left = total - (long long)blockIdx.x * kWindowLanes;
    const int rows = rows_left < kWindowLanes ? (int)rows_left : kWindowLanes;
    const int wshift = N <= 32 ? 5 : 6;
    const int width = 1 << wshift;
    const int sub = l & (width - 1);

    int from = live ? 0 : N;                                   // next window element this lane has to deliver
    for (int pass = 0; pass < window_passes_bound(RUNS); ++pass) {
        // ---- walk (per lane) ----
        int np = 0, cover = from;                              // parked runs deliver elements [from, cover)
        int stop = 0;                                          // why the walk ended: 0 = the trajectory did, 1 = the window did, 2 = no room left
        double hq = __builtin_nan(""), hz = hq;
        [[maybe_unused]] int seen_e = -0x7fffffff - 1, seen_we = 0;   // knots: the end of the last visited run and the knots below it
        if (from < N && len > 0) {
            const long long ix = p * in.sq + (long long)j * in.sj;
            double q = in.q_0[ix], v = in.v_0[ix], a = in.a_0[ix];
            for_each_run<SEM>(plan_limits(lim, p, dof), rec, p * dof + j, j, len, t_sample, q, v, a, [&](int b, int e, const RunCoef& rc) {
                // the run's elements [sb, se): those w with b <= k + w * stride (or k + G[w]) < e that are still to deliver
                int wb, we;
                if constexpr (KNOTS) {
                    // one search per run: the runs follow one another, so the count at this run's start is the one found at the
                    // last run's end; none for a run that starts past the grid (the walk ends there, `we` is not looked at)
                    wb = b == seen_e ? seen_we : below(b - k);
                    we = wb < N ? below(e - k) : N;
                    seen_e = e;
                    seen_we = we;
                } else {
                    wb = below(b - k);
                    we = below(e - k);
                }
                const int sb = wb > from ? wb : from, se = we < N ? we : N;
                if (sb >= N) { stop = 1; return true; }        // the run starts past the window: so does every later one
                if (se <= sb) return false;                    // delivered already, before the window, or between two grid samples
                if (np == RUNS) { stop = 2; return true; }
                S.sb[np][l] = sb;
                S.mo[np][l] = k + 1 - b;
#pragma unroll
                for (int x = 0; x < kRunCoefs; ++x) S.c[np * kWindowCoefStride + x * kWindowLanes + l] = rc.c[x];
                cover = se;
                ++np;
                return false;
            }, j == dof - 1);
            hq = q;                                            // a walk that came to its end leaves the last sample's position
            hz = 0.0;
        }
        // what follows the parked runs in this pass: the hold samples if the walk reached the end of the trajectory (or the plan
        // has none), nothing if it stopped at the window's end or for want of room
        const int he = (from < N && stop == 0) ? N : cover;
        S.np[l] = np;
        S.pf[l] = from;
        S.hb[l] = cover;
        S.he[l] = he;
        S.hold_q[l] = hq;
        S.hold_z[l] = hz;
        from = stop == 2 ? cover : N;
        __syncthreads();

        // ---- stream (converged) ----
        for (int row0 = 0; row0 < rows; row0 += kWindowLanes >> wshift) {
            const int row = row0 + (l >> wshift);
            if (row >= rows) continue;
            const unsigned long long base = S.base[row];
            const int rnp = S.np[row], pf = S.pf[row], hb = S.hb[row], rhe = S.he[row];
            const double hq = S.hold_q[row], hz = S.hold_z[row];
            // lane = element: every store instruction covers `width` consecutive elements of the row, whatever the runs' lengths
            for (int s = (pf & ~(width - 1)) + sub; s < rhe; s += width) {
                if (s < pf || s >= N) continue;
                double q = hq, v = hz, a = hz, jj = hz;
                if (s < hb) {
                    int r = 0;                                 // the parked run that holds s: the last one that starts at or before it
                    for (int x = 1; x < rnp; ++x) r = s >= S.sb[x][row] ? x : r;
                    const double* cw = S.c + r * kWindowCoefStride + row;
                    double c[kRunCoefs];
#pragma unroll
                    for (int x = 0; x < kRunCoefs; ++x) c[x] = cw[x * kWindowLanes];
                    int at = s;                                // trajectory offset of element s
                    if constexpr (KNOTS) at = G[s];
                    else if constexpr (STRIDED) at = s * stride;
                    run_eval(c, at + S.mo[r][row], q, v, a, jj);
                }
                sink(row, base + (unsigned long long)s, q, v, a, jj);
            }
        }
        __syncthreads();
        if (__builtin_amdgcn_ballot_w64(from < N) == 0ull) break;
    }
}

template <int SEM, typename T, int MODE>
__global__ void __launch_bounds__(kWindowLanes)
k_sample_window(long long first, long long count, int dof, double t_sample, PlanLimits lim, Queries in, Records rec, int N, int R,
                typename WindowGridArg<MODE>::type grid_arg, const int* __restrict__ first_sample, int uniform_first,
                int* __restrict__ valid, T* __restrict__ out)
{
    const unsigned long long plane = (unsigned long long)dof * (unsigned long long)R;   // elements between the arrays of a plan
    window_passes<SEM, MODE, 4, kWindowRuns>(first, count, dof, t_sample, lim, in, rec, N, R, grid_arg, first_sample, uniform_first, valid,
        [](long long, int) {},
        [&](int, unsigned long long at, double q, double v, double a, double jj) { window_store(out, at, plane, q, v, a, jj); });
}

// ltp_stop_knots_batch: the knots mode with the braking sink. SEM is the pow rule alone (kSemCpp | kPowLibm: the entry refuses MATLAB
// semantics); the walk is the C++ reference's. Five parked runs under the libm rule: with the pow tables (5 120 B) and the limit words
// (2 048 B) six would put a block at 45 664 B of LDS, three blocks per compute unit; five is 40 016 B and keeps four. The exact rule
// stages no tables and keeps six (40 544 B).
#ifndef LTP_STOP_KNOTS_LIBM_RUNS
#define LTP_STOP_KNOTS_LIBM_RUNS 5      // (-DLTP_STOP_KNOTS_LIBM_RUNS=6: the A/B build with three blocks per compute unit)
#endif
constexpr int stop_knots_runs(int sem) { return sem_libm(sem) ? LTP_STOP_KNOTS_LIBM_RUNS : 6; }
constexpr int kStopKnotsStrict = 1;     // LTP_STOP_ACCEL_STRICT; 0 is LTP_STOP_ACCEL_CLAMP (the entry admits nothing else)
template <int SEM, int RUNS>
__global__ void __launch_bounds__(kWindowLanes)
k_stop_knots(long long first, long long count, int dof, double t_sample, PlanLimits lim, Queries in, Records rec, int N, int R,
             const int* __restrict__ grid, const int* __restrict__ first_sample, int uniform_first, int* __restrict__ valid, int accel,
             double* __restrict__ out)
{
    static_assert(!sem_matlab(SEM), "stop horizons follow the C++ reference's sampler only");
    static_assert((sizeof(WindowLds<RUNS>) + kMaxKnots * sizeof(int) + 4 * kWindowLanes * sizeof(double) + (sem_libm(SEM) ? 5120 : 0))
                          * (LTP_STOP_KNOTS_LIBM_RUNS == 5 ? 4 : 3) <= 160 * 1024, "four blocks per compute unit");
    if constexpr (sem_libm(SEM)) libm::stage_tables();        // the block's LDS copy of glibc's pow tables (ltp_libm_pow.hpp)
    // what opt_braking reads of a row's limits: a_max, j_max and, of its LimPow, tj and tj^3 (pw3_tj; the other five words are timeScaling's)
    __shared__ double s_am[kWindowLanes], s_jm[kWindowLanes], s_tj[kWindowLanes], s_tj3[kWindowLanes];
    const unsigned long long plane = (unsigned long long)dof * (unsigned long long)R;   // q_stop to t_stop of a plan
    const double nan = __builtin_nan("");
    window_passes<kSemCpp, kWindowKnots, 2, RUNS>(first, count, dof, t_sample, lim, in, rec, N, R, grid, first_sample, uniform_first, valid,
        [&](long long p, int j) {
            const Limits L = plan_limits(lim, p, dof);
            const int l = (int)threadIdx.x;
            s_am[l] = L.a_max[j];
            s_jm[l] = L.j_max[j];
            s_tj[l] = L.pw[(long long)j * kLimPowN];
            s_tj3[l] = L.pw[(long long)j * kLimPowN + 1];
        },
        [&](int row, unsigned long long at, double q, double v, double a, double) {
            const double am = s_am[row];
            const LimPow P{s_tj[row], s_tj3[row], 0.0, 0.0, 0.0, 0.0, 0.0};
            const bool beyond = dabs(a) > am;                  // LTP_STOP_CHECK_BRAKING's comparison, per (plan, joint, knot)
            const double ab = accel == kStopKnotsStrict ? a : (a > am ? am : (a < -am ? -am : a));   // a NaN passes (torch.clamp)
            double r[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[7];
            double qb = 0.0, dir = 0.0;
            MatlabCtx mc;
            opt_braking<SEM>(am, s_jm[row], P, t_sample, v, ab, qb, r, dir, mc);
            cumsum7(r, t);
            const bool refused = accel == kStopKnotsStrict && beyond;
            __builtin_nontemporal_store(refused ? nan : q + qb, out + at);            // one addition, as in k_stop
            __builtin_nontemporal_store(refused ? nan : t[6], out + at + plane);
        });
}

void launch_stop_knots(hipStream_t s, const PlanRange& r, int n_knots, int row_stride, const int* knots, const int* first_sample,
                       int uniform_first, int* valid, int accel, int variant, double* out)
{
    if (r.count <= 0 || r.dof <= 0 || n_knots <= 0 || n_knots > kMaxKnots || !knots) return;
    const unsigned blocks = (unsigned)((r.count * r.dof + kWindowLanes - 1) / kWindowLanes);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kWindowLanes), 0, s, r.first, r.count, r.dof, r.t_sample, r.lim, r.in, r.rec, n_knots,
                           row_stride, knots, first_sample, uniform_first, valid, accel, out);
    };
    if (variant & kPowLibm) launch(k_stop_knots<kPowLibm, stop_knots_runs(kPowLibm)>);
    else launch(k_stop_knots<kSemCpp, stop_knots_runs(kSemCpp)>);
}

void launch_sample_window(hipStream_t s, const PlanRange& r, int n_samples, int row_stride, int stride, const int* knots,
                          const int* first_sample, int uniform_first, int* valid, void* out, bool f32)
{
    if (r.count <= 0 || r.dof <= 0 || n_samples <= 0 || stride <= 0 || (knots && n_samples > kMaxKnots)) return;
    const unsigned blocks = (unsigned)((r.count * r.dof + kWindowLanes - 1) / kWindowLanes);
    auto launch = [&](auto kernel, auto grid, auto* rows) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kWindowLanes), 0, s, r.first, r.count, r.dof, r.t_sample, r.lim, r.in, r.rec, n_samples,
                           row_stride, grid, first_sample, uniform_first, valid, rows);
    };
    dispatch_semantics(r.semantics, [&](auto v) {
        constexpr int SEM = decltype(v)::value;
        // a grid (every ltp_sample_knots_batch call, the uniform ones included) has its own instantiation: the only one with the
        // grid's LDS; stride 1 (every ltp_sample_window_batch call) keeps its own too: no division in its walk
        if (knots) {
            if (f32) launch(k_sample_window<SEM, float, kWindowKnots>, knots, (float*)out);
            else launch(k_sample_window<SEM, double, kWindowKnots>, knots, (double*)out);
        } else if (stride == 1) {
            if (f32) launch(k_sample_window<SEM, float, kWindowDense>, stride, (float*)out);
            else launch(k_sample_window<SEM, double, kWindowDense>, stride, (double*)out);
        } else {
            if (f32) launch(k_sample_window<SEM, float, kWindowStrided>, stride, (float*)out);
            else launch(k_sample_window<SEM, double, kWindowStrided>, stride, (double*)out);
        }
    });
}

}  // namespace ltp
