// ltp_kernels.hpp — gfx950 kernels of the batched planner (declarations + shared structs).
//
// Pipeline for one batch (reference src/long_term_planner.cc:7-63, one query = one call):
//   k_opt_fast       stage 1 (checkInputs + optSwitchTimes per (query, joint)) without the quartic
//                    sites; lanes that reach them are compacted into queue A
//   k_opt_slow       queue A, densely, with the root finder
//   k_reduce_scale   slowest-joint reduction in LDS + the two closed-form timeScaling cases;
//                    lanes that need the polynomial cases are compacted into queue B
//   k_scaling_slow   queue B, densely: all eight timeScaling cases + reset
//   k_finalize_lens  padded row stride, per-plan output size, block sums for the offsets scan (the lengths,
//                    cc:716-719, come from the two kernels above; k_finalize forms them itself for records
//                    planned elsewhere)
//   k_scan_top / k_scan_apply   exclusive scan -> packed trajectory offsets
//   k_sample         getTrajectory (cc:706-841) + end-limit check (cc:59-61), HBM-write bound
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/ltp_run_tables.hpp"   // kMaxSegments, the packed run-table format (public)
#include "ltp_sampler_policy.hpp"               // RowSpec, kRowAlign, the sampler's row predicates

namespace ltp {

// status bits (planTrajectory's bool == (status == 0))
enum : int {
    kStatusInvalidInput = 1,   // checkInputs false (cc:14-15)
    kStatusOptFailed = 2,      // optSwitchTimes false for a joint (cc:29)
    kStatusNoSlowest = 4,      // slowest_joint == -1 (cc:39)
    kStatusEndLimit = 8,       // last q sample outside [q_min,q_max] (cc:59-61); trajectory is filled
    kStatusNonFinite = 16,     // DEFINED: non-finite switching times -> traj_len 0 (reference: UB)
    kStatusOverflow = 32,      // trajectory does not fit the caller's output tile; not sampled
    kStatusGoalOutside = 64,   // NEW, opt-in: q_goal outside [q_min,q_max]; rejected before planning (reference: unchecked)
    kStatusMatlabError = 128,  // MATLAB semantics only: LTPlanner.m would have raised an error; rejected, traj_len 0
    kStatusMatlabComplex = 256,// MATLAB semantics only, informational: LTPlanner.m would have carried a complex intermediate
                               // value; the plan continues with the real part and IS delivered
    kStatusBadLimitSet = 512,  // ltp_bind_limit_sets: the query's set index lies outside [0, n_sets); traj_len 0, slowest -1
};

constexpr int kQueriesPerBlock = 64;   // one wave = 64 queries of one joint
constexpr int kMaxJointSlots = 8;      // blockDim.y of k_switch_times
constexpr int kSampleJointGroup = 8;   // joints handled by one k_sample block
constexpr int kSampleThreads = 256;
#ifndef LTP_SAMPLE_BLOCKS_PER_CU
#define LTP_SAMPLE_BLOCKS_PER_CU 5
#endif
constexpr int kSampleBlocksPerCU = LTP_SAMPLE_BLOCKS_PER_CU;   // register budget of k_sample (512 / this many VGPRs); measured best of 4..7
constexpr int kSampleSpread = 64;      // default block->plan interleave of k_sample
constexpr int kScanBlock = 1024;       // plans per finalize/scan block

struct Limits {            // one set of joint limits: device pointers, [dof] each
    const double* q_min;
    const double* q_max;
    const double* v_max;
    const double* a_max;
    const double* j_max;
    const double* pw;      // [dof][kLimPowN]: LimPow of every joint under the handle's pow rule (k_limit_powers)
};
constexpr int kLimPowN = 7;

// Where the plans of a batch read their limits (ltp_set_limit_sets / ltp_bind_limit_sets): without an index, the handle's own set
// above for every plan; with one, plan p reads set set_index[p] of the set table. plan_limits() (ltp_device.hpp) is the one place
// that decides. A derived struct, so that the kernels that never read a binding (the stage kernels' one-set instantiations, the
// one-lane mirrors, the generator, k_plan_small) keep their argument layout.
struct PlanLimits : Limits {
    const int* set_index;  // [n] per plan of the batch, or null
    int n_sets;
    long long set_rows;    // rows each of the five arrays below has room for (the table's capacity: stable while it is reused)
    const double* sets;    // [5][set_rows]: q_min, q_max, v_max, a_max, j_max; row s * dof + j is joint j of set s
    const double* set_pw;  // [set_rows][kLimPowN] under the handle's pow rule
};

struct Queries {           // element (query p, joint j) at ptr[p * sq + j * sj]
    const double* q_goal;
    const double* q_0;
    const double* v_0;
    const double* a_0;
    long long sq, sj;
};

struct Records {           // query-major outputs of stages 1-3
    double* t_opt;         // [n][dof][7]
    double* t_scaled;      // [n][dof][7]
    double* dir;           // [n][dof]
    double* v_drive;       // [n][dof]
    signed char* mod;      // [n][dof]
    double* t_required;    // [n]
    int* slowest;          // [n]
    int* traj_len;         // [n]
    int* status;           // [n]
};

// Plans [first, first + count) of a planned batch and what every reader needs of them. ltp_capi::plan_range (ltp_handle.hpp) builds
// one from the handle and the caller's ltp_queries / ltp_records; every reader launcher below takes (stream, range, what is its own).
struct PlanRange {
    long long first, count;
    int dof;
    double t_sample;
    PlanLimits lim;
    Queries in;
    Records rec;
    int semantics;         // kSemCpp | kSemMatlab (dispatch_semantics)
};

// items per work-queue draw of the persistent samplers: 1 for whole trajectories; for capped rows as many as keep a draw at
// >= ~256 KB of rows, at most 8
inline int queue_draw_chunk(RowSpec rows, bool f32, int joints_per_item)
{
    if (rows.max_samples <= 0) return 1;
    const long long item_bytes = 4ll * (f32 ? 4 : 8) * rows.max_samples * joints_per_item;
    int k = 1;
    while (k < 8 && item_bytes * (2 * k) <= 262144) k *= 2;
    return k;
}

// variant = semantics (bit 0: 0 = the C++ reference, 1 = LTPlanner.m) | kPowLibm (bit 1: the pow rule LTP_POW_LIBM); the template
// parameter SEM of ltp_profile.hpp and of the stage kernels. f is called with std::integral_constant<int, variant>.
template <class F>
inline void dispatch_variant(int variant, F&& f)
{
    switch (variant & 3) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
    }
}
// f is called with std::integral_constant<int, kSemCpp | kSemMatlab>: the template parameter SEM of the run walk (ltp_runs.hpp)
template <class F>
inline void dispatch_semantics(int semantics, F&& f)
{
    if (semantics == kSemMatlab) f(std::integral_constant<int, kSemMatlab>{});
    else f(std::integral_constant<int, kSemCpp>{});
}
// a lane-per-(plan, joint) kernel (plan_lane, ltp_device.hpp) over the count * dof lanes of r in blocks of 256; its arguments are
// (r, args...). Nothing is launched for an empty range.
template <class... KArgs, class... Args>
inline void launch_lanes(hipStream_t s, const PlanRange& r, void (*kernel)(PlanRange, KArgs...), Args... args)
{
    if (r.count <= 0 || r.dof <= 0) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((r.count * r.dof + 255) / 256)), dim3(256), 0, s, r, args...);
}
// The stage kernels' variant adds kStageSets (bit 2: per-plan limit sets, ltp_bind_limit_sets). Only the two C++-semantics variants
// have a sets twin (4, 6); the caller refuses a binding in MATLAB semantics.
constexpr int kStageSets = 4;
constexpr bool sem_sets(int sem) { return (sem & kStageSets) != 0; }
template <class F>
inline void dispatch_stage_variant_cpp(int variant, F&& f)   // the C++-semantics variants alone (0, 2, 4, 6): bit 0 is not read
{
    if (variant & kStageSets) {
        if (variant & 2) f(std::integral_constant<int, 6>{});
        else f(std::integral_constant<int, 4>{});
    } else {
        if (variant & 2) f(std::integral_constant<int, 2>{});
        else f(std::integral_constant<int, 0>{});
    }
}
template <class F>
inline void dispatch_stage_variant(int variant, F&& f)
{
    if ((variant & (1 | kStageSets)) != 1) dispatch_stage_variant_cpp(variant, f);
    else if (variant & 2) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 1>{});
}

long long queue_segment(long long n, int dof);   // entries per queue shard; a batch needs 2 * 8 * this many u64
void launch_switch_times(hipStream_t s, long long n, int dof, double t_sample, int goal_check, PlanLimits lim, Queries in,
                         Records out, signed char* lane_flags, unsigned long long* queue_items, unsigned long long* counts,
                         int variant = 0 /* semantics | pow rule << 1 | sets << 2 (dispatch_stage_variant) */);
// finalize + k_scan_top + k_scan_apply -> offsets[n + 1]. lens_ready: traj_len / status are formed (k_finalize_lens; keep_status: the
// status bits that do not drop a plan), else k_finalize forms them from t_scaled
void launch_offsets(hipStream_t s, long long n, int dof, double t_sample, Records rec,
                    unsigned long long* block_sums, unsigned long long* offsets, bool lens_ready, RowSpec rows,
                    int keep_status = kStatusMatlabComplex);
// ltp_retime_batch (include/ltp_hip.h): what a planned batch is retimed to. Every pointer is device memory or null.
struct RetimeRequest {
    const double* t_target;    // [n] requested duration per query, or null
    double t_uniform;          // requested duration of every query, 0 = none (finite, >= 0: checked by the caller)
    const int* group;          // [n] group id per query, or null; ids outside [0, n_groups) = no group
    int n_groups;
    double* group_time;        // [n_groups], zeroed by the caller on the same stream (with group)
};
// k_group_time (with group), k_retime + queue B (k_scaling_slow), then the offsets scan (k_finalize_lens with the mask of a retimed
// batch). queue_items / counts as for launch_switch_times (counts zeroed by the caller on the same stream). C++ semantics only
// (dispatch_stage_variant_cpp): either pow rule, with or without limit sets.
void launch_retime(hipStream_t s, long long n, int dof, double t_sample, PlanLimits lim, Queries in, Records rec, RetimeRequest req,
                   unsigned long long* queue_items, unsigned long long* counts, unsigned long long* block_sums,
                   unsigned long long* offsets, RowSpec rows, int variant);
// ltp_plan_stop_batch (ltp_stop.hip: k_stop): every joint of every query brakes to rest by optBraking; all nine record fields are
// written, traj_len and status included (launch_offsets(..., lens_ready = true) follows). in.q_goal is not read. q_stop: null, or
// the standstill positions laid out like the queries. check: LTP_STOP_CHECK_*. C++ semantics only (variant: pow rule | sets).
void launch_stop(hipStream_t s, long long n, int dof, double t_sample, PlanLimits lim, Queries in, Records out, double* q_stop,
                 int check, int variant);
// ---- the readers of a planned batch: every launcher takes (stream, the PlanRange, what is its own) ----
// Run tables: built inside the sampler / envelope kernel by the item's block, or by the table pass: launch_build_tables leaves
// table_bytes(count * dof) bytes in `tables` (912 bytes per plan and joint: the packed form, which the consumer expands with
// run_coef()) for launch_sample_tab / launch_envelope(tables != nullptr). base_first: the plan whose offset is the origin of out / env
// (== first unless a range is processed in pieces that share one table buffer).
unsigned long long table_bytes(long long lanes /* plans * dof */);
void launch_build_tables(hipStream_t s, const PlanRange& r, RowSpec rows, bool whole_trajectory /* false: only the runs capped rows touch */,
                         const unsigned long long* offsets /* or nullptr */, long long base_first /* row offsets relative to this plan */,
                         unsigned long long* tables);
// interleave: SamplePolicy::interleave (0 = kSampleSpread)
void launch_sample(hipStream_t s, const PlanRange& r, const unsigned long long* offsets, void* out, bool f32, unsigned long long capacity,
                   bool nontemporal, bool dry, int interleave, RowSpec rows, unsigned long long* next_item /* zeroed on the same stream */,
                   int resident_blocks, unsigned long long* stamps = nullptr);
// (reads r.rec and the tables alone; r.t_sample: the one the tables were built with)
void launch_sample_tab(hipStream_t s, const PlanRange& r, long long base_first, const unsigned long long* offsets, void* out, bool f32,
                       unsigned long long capacity, bool nontemporal, int interleave, RowSpec rows,
                       unsigned long long* next_item /* zeroed on the same stream */, int resident_blocks, const unsigned long long* tables,
                       unsigned long long* stamps = nullptr /* diagnostic: 8 per (plan, joint group) item */);
// Rows without any table traffic (every row format, both semantics, any number of joints; taken by itself for capped, float32 and
// sparse rows and in MATLAB semantics): a builder wave per block walks the runs into LDS, five streaming waves write the rows
// (ltp_sampler_walk.hip). walk_kernel: choose_sampler's pick (walk_kernel_index, ltp_sampler_policy.hpp), which carries the semantics.
int sample_walk_resident_blocks(int device, bool f32);
void launch_sample_walk(hipStream_t s, const PlanRange& r, const unsigned long long* offsets, void* out, unsigned long long capacity,
                        int walk_kernel, int interleave, RowSpec rows, unsigned long long* next_item /* zeroed on the same stream */,
                        int resident_blocks, int auto_cus /* autonomous form: sample_walk_auto_prepare(device) */);
// per device, once, outside stream capture: dynamic-LDS limit of the autonomous-wave kernels (checked) -> compute units (0: *err)
int sample_walk_auto_prepare(int device, hipError_t* err);
int sample_tab_resident_blocks(int device, bool f32);
int sample_resident_blocks(int device, bool f32);
int envelope_resident_blocks(int device);
// the analytic envelopes by a lane-per-(plan, joint) register walk: no run tables, no workspace (ltp_consumers.hip: k_envelope_walk)
void launch_envelope_walk(hipStream_t s, const PlanRange& r, long long base_first, int window, int n_windows, double* env);
// horizon envelopes (ltp_consumers.hip: k_envelope_knots): per plan and joint [min q, max q] between the edges k + edges[w] and
// k + edges[w + 1] of one grid (device int[n_intervals + 1], n_intervals <= LTP_MAX_KNOTS - 1), k = first_sample[i] (or uniform_first);
// env[((i * dof + j) * n_intervals + w) * 2], valid (or null) receives the w with k + edges[w] < traj_len. Nothing but the kernel is enqueued.
void launch_envelope_knots(hipStream_t s, const PlanRange& r, int n_intervals, int closed, const int* edges, const int* first_sample,
                           int uniform_first, int* valid, double* env);
// horizon envelopes of q, v, a and j (ltp_consumers.hip: k_envelope_knots_arrays): the call above per selected array, arrays a non-empty
// subset of LTP_ENV_Q | _V | _A | _J; env[((((i * A + x) * dof + j) * n_intervals + w) * 2], A = popcount(arrays), x the array's rank
// among the selected ones. Nothing but the kernel is enqueued.
void launch_envelope_knots_arrays(hipStream_t s, const PlanRange& r, int n_intervals, int closed, int arrays, const int* edges,
                                  const int* first_sample, int uniform_first, int* valid, double* env);
// first exits (ltp_consumers.hip: k_first_exit): per plan, selected array (arrays: a non-empty subset of LTP_ENV_Q | _V | _A | _J) and
// joint the first trajectory sample of [k, k + horizon) outside the box [lo, hi] of that (plan, joint, array), k = first_sample[i] (or
// uniform_first); exit_sample[(i * A + x) * dof + j]. lo[x] / hi[x]: device arrays read at [i * box_query_stride + j *
// box_joint_stride], or null = the plan's own limit. first_any: null, or device int[count], which a fill kernel sets to LTP_EXIT_NONE
// before the lanes fold into it. Nothing but the one or two kernels is enqueued.
void launch_first_exit(hipStream_t s, const PlanRange& r, int arrays, int horizon, const int* first_sample, int uniform_first,
                       const double* const (&lo)[4], const double* const (&hi)[4], long long box_query_stride, long long box_joint_stride,
                       int* exit_sample, int* first_any);
// settling (ltp_consumers.hip: k_settle): launch_first_exit's arguments; settle_sample[(i * A + x) * dof + j] is the sample from which
// the array stays inside its box for the rest of [k, k + horizon), LTP_SETTLE_NOT_YET where the horizon's last sample is outside.
// settle_all: null, or device int[count], which a fill kernel sets to 0 before the lanes fold their maximum into it. Nothing but the
// one or two kernels is enqueued.
void launch_settle(hipStream_t s, const PlanRange& r, int arrays, int horizon, const int* first_sample, int uniform_first,
                   const double* const (&lo)[4], const double* const (&hi)[4], long long box_query_stride, long long box_joint_stride,
                   int* settle_sample, int* settle_all);
void launch_envelope(hipStream_t s, const PlanRange& r, long long base_first, int window, int n_windows, double* env,
                     unsigned long long* next_item /* zeroed on the same stream */, int resident_blocks,
                     unsigned long long* probe = nullptr /* diagnostic: 16 stamps per item */, const unsigned long long* tables = nullptr,
                     bool analytic = false /* extreme samples from the roots of q'(m) per run instead of every sample: 1e-15, not bit-identical */);
// float64 tiles: the states are recomputed from the records, same bits
void launch_replan_states(hipStream_t s, const PlanRange& r, RowSpec rows, const unsigned long long* offsets, const void* tile, bool f32,
                          unsigned long long capacity, const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                          long long sq, long long sj);
void launch_end_limit(hipStream_t s, const PlanRange& r);
void launch_state_at(hipStream_t s, const PlanRange& r, const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                     long long sq, long long sj);
// Horizon windows (ltp_window.hip: k_sample_window): the n_samples trajectory samples k, k + stride, ... from k = first_sample[i]
// (or uniform_first) on of the range's plans in the fixed layout [count][q,v,a,j][dof][row_stride]; valid (or null) receives the real samples per plan.
// knots != null (device int[n_samples], n_samples <= LTP_MAX_KNOTS; stride is then not read): the samples k + knots[w] instead.
// Autonomous waves: no workspace, no queue head, nothing but the kernel is enqueued.
void launch_sample_window(hipStream_t s, const PlanRange& r, int n_samples, int row_stride, int stride, const int* knots,
                          const int* first_sample, int uniform_first, int* valid, void* out, bool f32);
// Stop horizons (ltp_window.hip: k_stop_knots): the knots mode above with the braking sink — per element (q, v, a) of the knot grid
// opt_braking under the plan's limits; out [count][{q_stop, t_stop}][dof][row_stride], float64. accel: LTP_STOP_ACCEL_*; variant: the
// pow rule (kPowLibm or 0; C++ semantics only). Nothing but the kernel is enqueued.
void launch_stop_knots(hipStream_t s, const PlanRange& r, int n_knots, int row_stride, const int* knots, const int* first_sample,
                       int uniform_first, int* valid, int accel, int variant, double* out);
// planTrajectory for n queries with n * dof <= small_batch_pairs() in one launch of one block; every pointer may be host
// memory the device can address (pinned). rows == nullptr: no sampling (status still carries the end-limit verdict).
// *done becomes 1 when all results are visible to the host, 2 if the rows did not fit `capacity` (then nothing was sampled).
// The grid has small_batch_blocks() blocks (one per joint when rows are written); end_flags: [blocks][n] ints the host ORs into
// status; arrivals: one zeroed device word.
int small_batch_pairs();
int small_batch_blocks(int dof, bool with_rows);
void launch_plan_small(hipStream_t s, int n, int dof, double t_sample, int goal_check, RowSpec rows, Limits lim, const double* const in[4],
                       Records rec, unsigned long long* offsets, double* out_rows, unsigned long long capacity, int* end_flags,
                       unsigned int* arrivals, volatile int* done,
                       bool records_given = false /* getTrajectory: t_scaled, dir, mod, v_drive of `rec` are inputs */,
                       bool libm_pow = false /* the pow rule LTP_POW_LIBM */,
                       bool host_inputs = false /* in[] is host memory this thread may read now: a few queries then ride in the kernel arguments */);
void launch_generate(hipStream_t s, long long n, int dof, Limits lim, unsigned long long seed, long long first_query,
                     double* q_goal, double* q_0, double* v_0, double* a_0, long long sq, long long sj);

// LimPow tables of dof joints under both pow rules ([dof][kLimPowN] each), from the device copies of a_max / j_max
void launch_limit_powers(hipStream_t s, int dof, const double* a_max, const double* j_max, double* out_exact, double* out_libm);
void launch_check_inputs(hipStream_t s, int dof, Limits lim, const double* q_0, const double* v_0, const double* a_0, int* ok, int variant = 0);
// single-joint mirrors of the protected methods (one lane); io[11] receives the lane's MATLAB flags (kMatlabComplex | kMatlabError)
void launch_single_opt_braking(hipStream_t s, int joint, double t_sample, Limits lim, double v_0, double a_0, double* out10, int variant = 0);
void launch_single_opt_switch(hipStream_t s, int joint, double t_sample, Limits lim, double q_goal, double q_0, double v_0,
                              double a_0, double v_drive, double* io10, int variant = 0);
void launch_single_time_scaling(hipStream_t s, int joint, double t_sample, Limits lim, double q_goal, double q_0, double v_0,
                                double a_0, double dir, double t_required, double* out11, int variant = 0);
// MATLAB's roots() on the device (ltp_roots_matlab.hpp): n polynomials of `degree` <= 6, [n][degree+1] coefficients; re, im
// [n][degree] in MATLAB's output order, nroots [n], status [n] (0 ok, 1 no convergence, 2 NaN / Inf)
void launch_roots_matlab(hipStream_t s, long long n, int degree, const double* coef, double* re, double* im, int* nroots, int* status);
void launch_math_probe(hipStream_t s, long long n, const double* x, const double* y, double* out);
void launch_libm_pow_probe(hipStream_t s, long long n, const double* x, const double* y, double* out);   // out[i] = the restated glibc pow(x[i], y[i])
void launch_roots_probe(hipStream_t s, long long n, int degree, const double* coef, double* root);
void launch_roots_all(hipStream_t s, long long n, int degree, bool f32, const void* coef, void* re, void* im);

}  // namespace ltp
