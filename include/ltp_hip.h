/*
 * ltp_hip.h — C ABI of libltp_hip.so, the MI355X (gfx950) batched planner.
 *
 * This is the drop-in boundary for the reference's hot path
 * LongTermPlanner::planTrajectory and the member functions under it. The
 * reference has no FFI layer of its own (it is one C++ class:
 * /root/reference/include/long_term_planner/long_term_planner.h:61-308), so each
 * entry point below names the reference member it replaces; the drop-in C++
 * class in include/long_term_planner/long_term_planner.h forwards to exactly
 * these symbols and INTEGRATION.md shows the binding.
 *
 * Conventions: plain C, opaque handle, caller-owned buffers, `int` return
 * (0 = LTP_OK, otherwise an ltp_error and ltp_last_error() has the text), no
 * exceptions cross the boundary. `stream` is a hipStream_t (NULL = the default
 * stream). Functions ending in _batch take DEVICE pointers and only enqueue
 * work; functions ending in _host take host pointers and are synchronous.
 * All arithmetic is IEEE binary64, as in the reference.
 *
 * Streams. A handle owns ONE device workspace (compaction queues, lane flags, scan scratch) that
 * ltp_plan_switch_times_batch uses. Calls on one stream are ordered by the stream. When a call arrives on a
 * different stream than the handle's previous workspace user, the library inserts the dependency itself (an event
 * recorded after the previous call, waited for by the new stream), so two streams of one handle — e.g. a
 * double-buffered pipeline — serialise on the workspace instead of racing. For concurrency use one handle per
 * stream (handles are cheap: ~1 MB plus the workspace). A stream that is being captured into a hipGraph is exempt
 * (events cannot cross a capture): do not replay such a graph concurrently with other work of the same handle.
 *
 * Batch geometry. dof, t_sample, max_samples and sample_stride are captured when a batch is planned
 * (ltp_plan_switch_times_batch, ltp_plan_stop_batch) and define its records, offsets and row strides. The calls that consume a planned
 * batch (ltp_sample_batch*, ltp_envelope_batch, ltp_build_tables_batch, ltp_replan_states*_batch, ltp_state_at_batch,
 * ltp_sample_window_batch, ltp_end_limit_batch) return LTP_ERR_INVALID_ARGUMENT if one of them was changed on the handle in between.
 * The same holds for the limit sets (ltp_bind_limit_sets): the bound index pointer, n_sets and the generation that every
 * ltp_set_limit_sets increments are captured too, and a consumer call (ltp_retime_batch included) fails if any of them changed.
 */
#ifndef LTP_HIP_H
#define LTP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ltp_planner ltp_planner;

typedef enum {
    LTP_OK = 0,
    LTP_ERR_INVALID_ARGUMENT = 1,
    LTP_ERR_NO_DEVICE = 2,      /* no HIP device / HIP runtime error: the product has no CPU fallback */
    LTP_ERR_OUT_OF_MEMORY = 3,
    LTP_ERR_HIP = 4
} ltp_error;

/* per-query status bits; LongTermPlanner::planTrajectory's bool is (status == 0) */
#define LTP_STATUS_INVALID_INPUT 1  /* checkInputs false            (src/long_term_planner.cc:14-15, 68-77) */
#define LTP_STATUS_OPT_FAILED    2  /* optSwitchTimes false         (cc:29)                               */
#define LTP_STATUS_NO_SLOWEST    4  /* slowest_joint == -1          (cc:39)                               */
#define LTP_STATUS_END_LIMIT     8  /* last q outside [q_min,q_max] (cc:59-61); trajectory IS filled      */
#define LTP_STATUS_NONFINITE    16  /* defined here: non-finite switching times or a length beyond int   */
                                    /* range; traj_len = 0, not sampled (reference: undefined behaviour)  */
#define LTP_STATUS_OVERFLOW     32  /* trajectory did not fit the output tile passed to ltp_sample_batch  */
#define LTP_STATUS_GOAL_OUTSIDE 64  /* only with ltp_set_goal_check(p, 1): q_goal outside [q_min,q_max]   */
#define LTP_STATUS_MATLAB_ERROR 128 /* only with LTP_SEMANTICS_MATLAB: LTPlanner.m would have raised an error */
                                    /* (checkInputs, index past / vector of filtered roots); traj_len = 0     */
#define LTP_STATUS_MATLAB_COMPLEX 256 /* only with LTP_SEMANTICS_MATLAB, informational: LTPlanner.m would have */
                                    /* carried a complex intermediate; real parts used, the plan IS delivered */
#define LTP_STATUS_BAD_LIMIT_SET 512 /* only with a bound limit-set index: the query's index lies outside [0, n_sets); */
                                    /* traj_len 0, slowest -1, nothing sampled, not retime-eligible               */

/* Which source the arithmetic follows where the two references diverge:
 * LTP_SEMANTICS_CPP     src/long_term_planner.cc — the parity reference, the default.
 * LTP_SEMANTICS_MATLAB  the MATLAB original LTPlanner.m: polynomial roots picked by POSITION in the output of roots()
 *                       (:346-416) or first-through-a-filter (:247-250, 272-275); optSwitchTimes returns zeros where the C++
 *                       returns false (:222-227, 288-303); fallback rule ~any(t_scaled) (:82); no position limits (no q_0
 *                       check, no end-limit verdict); the slowest joint's jerk-profile flag stays false (:64); sampler with
 *                       1-based correction indices, mod(), cumsum-then-overwrite integration and the acceleration tail zeroed
 *                       for the LAST joint only (:531-624). Rows still carry j as the fourth array. The order of MATLAB's
 *                       roots() is restated from LAPACK's DGEEV path and checked against numpy.roots; against MATLAB itself
 *                       this mode is pinned only by the MATLAB unit tables and grid tests the reference holds. */
#define LTP_SEMANTICS_CPP 0
#define LTP_SEMANTICS_MATLAB 1

/* How the reference's pow(x, 3 | 4 | 6) and pow(x, 1.0 / 2) calls (src/long_term_planner.cc:125-331, 378-621) are formed
 * (pow(x, 2) is x * x in every build: gcc folds it). Both rules are IEEE binary64; they differ in the last bit of about one
 * power in a thousand, which timeScaling's cancelling v_drive formulas (cc:378-446) turn into up to ~5e-11 s of a switching
 * time and the sampler's jerk corrections (cc:768-807) into |dt| * j_max / Ts of single jerk samples.
 * LTP_POW_LIBM   THE DEFAULT. glibc's pow (>= 2.28; the build glibc selects on x86-64 hosts with FMA) restated operation for
 *                operation (csrc/ltp_libm_pow.hpp, bit-identical to the installed libm on 1.7e10 inputs): every record has the
 *                bits a reference built with gcc + glibc computes on such a host and every sample is within 1e-9 of it, no plan
 *                excepted (tests/test_gpu_parity.py; 34.1 M dense trajectories in profiles/r05_parity_report.json). Costs ~45 fp64
 *                operations and 3 table reads per power: +1 % on a full-sampling batch, +10 % on switching times only (round 6: the
 *                powers of the limits are formed once per ltp_set_limits; +35 % before).
 * LTP_POW_EXACT  one rounding of the exact product, sqrt for the power 1/2: what a correctly rounded pow returns; within
 *                1 ulp of ANY libm (so within the differences between two libm builds of the reference); the faster rule. */
#define LTP_POW_EXACT 0
#define LTP_POW_LIBM 1

/* Queries: element (query p, joint j) of each array is ptr[p*query_stride + j*joint_stride].
 * Row-major [n][dof] (the reference's vector-per-query view): query_stride = dof, joint_stride = 1.
 * Joint-major SoA [dof][n]: query_stride = 1, joint_stride = n. */
typedef struct {
    const double* q_goal;
    const double* q_0;
    const double* v_0;
    const double* a_0;
    long long query_stride;
    long long joint_stride;
} ltp_queries;

/* Switching-time records, query-major (what planTrajectory holds in locals, cc:18-24, 31-32, 42). */
typedef struct {
    double* t_opt;        /* [n][dof][7] optimal switch times  (cc:18, 27-30)            */
    double* t_scaled;     /* [n][dof][7] synchronised times after the fallback (cc:20, 43-55) */
    double* dir;          /* [n][dof]    direction of motion   (cc:22)                    */
    double* v_drive;      /* [n][dof]    cruise velocity       (cc:42)                    */
    signed char* mod;     /* [n][dof]    modified-jerk-profile flag (cc:24)               */
    double* t_required;   /* [n]         slowest joint's end time (cc:31)                 */
    int* slowest;         /* [n]         slowest joint, -1 if none (cc:32)                */
    int* traj_len;        /* [n]         Trajectory::length (cc:716-719), 0 if not sampled */
    int* status;          /* [n]         LTP_STATUS_* bits                                 */
} ltp_records;

/* ---- lifetime / configuration -------------------------------------------------------------- */

/* LongTermPlanner::LongTermPlanner(dof, t_sample, q_min, q_max, v_max, a_max, j_max)
 * (long_term_planner.h:118-131). The five arrays hold `dof` doubles. device = HIP ordinal. */
int ltp_create(int dof, double t_sample, const double* q_min, const double* q_max, const double* v_max,
               const double* a_max, const double* j_max, int device, ltp_planner** out);
void ltp_destroy(ltp_planner* p);
/* LongTermPlanner::setLimits (long_term_planner.h:176-187); n_limits = entries per array */
int ltp_set_limits(ltp_planner* p, int n_limits, const double* q_min, const double* q_max, const double* v_max,
                   const double* a_max, const double* j_max);
/* NEW: limit sets — one batch of queries that do not share one set of limits (several arm models, randomised simulation
 * environments, a per-robot speed override).
 *
 * Contract. A query that uses set s gets exactly what the same query gets on a handle whose ltp_set_limits are set s, bit for bit,
 * all other settings equal (dof, t_sample, pow rule, goal check, max_samples, sample_stride): records and status, traj_len and its
 * share of the offsets, rows in every format and from every sampler, envelopes in both modes, run tables, restart states, the
 * end-limit verdict and retimes.
 *
 * ltp_set_limit_sets: host arrays, row-major [n_sets][dof] with the handle's current dof (set s, joint j at s * dof + j).
 *   n_sets = 0 removes the sets and unbinds. Synchronises the device before it replaces the sets, like ltp_set_limits, and cannot be
 *   captured into a graph. Every call increments the sets' generation. Graphs: a captured graph keeps the table's address, its
 *   capacity and n_sets in its kernel arguments. Replacing the VALUES of the same n_sets (same dof) is replay-safe: the buffer is
 *   reused in place and laid out by capacity, so a replay reads the new values. Any change of n_sets or of the dof invalidates
 *   graphs captured before (a replay would still accept the old index range), and so does growth beyond the buffer (a new
 *   allocation), as for the workspace. The powers of the limits are formed on the device by a grid over the n_sets * dof rows.
 *   Threads: like the other configuration calls, not concurrent with batch calls of the same handle; a *_host call and a
 *   device-pointer plan of the same handle must not run at the same time from two threads either (the host call restores the
 *   handle's planned batch geometry when it returns).
 * ltp_get_limit_sets: n_sets (-1 for a NULL handle).
 * ltp_bind_limit_sets: device int[n] or NULL. NULL = the handle's own limits, today's behaviour byte for byte. The binding applies
 *   to the device-pointer batch calls: query q of the batch uses set set_index[q], and a consumer call on plans
 *   [first, first + count) reads set_index[first + i]. Honoured by ltp_plan_switch_times_batch, ltp_retime_batch,
 *   ltp_end_limit_batch, ltp_sample_batch_ex, ltp_sample_batch, ltp_sample_batch_f32, ltp_envelope_batch,
 *   ltp_build_tables_batch, ltp_replan_states*_batch and ltp_state_at_batch. Never read by the *_host calls, the one-lane
 *   mirrors of the protected methods and ltp_generate_queries_batch. The caller keeps the index array alive and unchanged from
 *   planning to the batch's last consumer call (as for `in` and `rec`). The binding is host state: a captured graph replays
 *   with whatever the array holds at replay time.
 * A bad index (outside [0, n_sets)) sets LTP_STATUS_BAD_LIMIT_SET: the query gets traj_len 0 and slowest -1, nothing of it is
 *   sampled and it is not retime-eligible; its other record fields are unspecified. No kernel reads a set through such an index
 *   (reads clamp) and neighbouring queries are not affected.
 * Refusals (LTP_ERR_INVALID_ARGUMENT, message in ltp_last_error): ltp_bind_limit_sets with a non-NULL pointer while the handle
 *   has no sets; planning with a binding when the sets were given for a dof other than the handle's current one; a binding
 *   together with LTP_SEMANTICS_MATLAB; any ltp_*_multi* entry while one of its planners has a binding; a consumer call after
 *   the binding, n_sets or the sets' generation changed since planning (Batch geometry). */
int ltp_set_limit_sets(ltp_planner* p, int n_sets, const double* q_min, const double* q_max, const double* v_max,
                       const double* a_max, const double* j_max);
int ltp_get_limit_sets(const ltp_planner* p);
int ltp_bind_limit_sets(ltp_planner* p, const int* set_index);
/* LongTermPlanner::setSampleTime (long_term_planner.h:194-196) */
int ltp_set_sample_time(ltp_planner* p, double t_sample);
/* LongTermPlanner::setDoF (long_term_planner.h:203-205) */
int ltp_set_dof(ltp_planner* p, int dof);
int ltp_get_dof(const ltp_planner* p);
double ltp_get_sample_time(const ltp_planner* p);
const char* ltp_last_error(const ltp_planner* p);
/* name of the kernel that wrote the rows / envelopes of the latest ltp_sample_batch* / ltp_envelope_batch call of this
 * handle ("k_sample", "k_sample_walk_f64_nt", "k_sample_tab_f64_nt", ...: the fused sampler, the walk sampler or the table-pass
 * sampler, see ltp_set_table_pass) */
const char* ltp_last_sampler_kernel(const ltp_planner* p);
/* rows of the packed trajectory layout are padded to this many elements (a multiple of 32) */
int ltp_row_stride(int stored_samples);
/* elements of such a row that ltp_sample_batch* write: the stored samples rounded up to whole 64-byte lines of `element_bytes`
 * (8: 8 doubles, 4: 16 floats; anything else: 0), never more than ltp_row_stride(stored_samples). See ltp_sample_batch. */
int ltp_row_line(int stored_samples, int element_bytes);
/* SURVEY.md §8(f).2 "first N samples only": store min(traj_len, max_samples) samples per row (0 = all of them, which
 * is the reference's behaviour and the default). traj_len in the records stays Trajectory::length; offsets, row
 * strides and the sampler follow the stored length ltp_stored_samples(p, traj_len). The end-limit check (cc:59-61)
 * still refers to the last sample of the whole trajectory. */
int ltp_set_max_samples(ltp_planner* p, int max_samples);
int ltp_get_max_samples(const ltp_planner* p);
int ltp_stored_samples(const ltp_planner* p, int traj_len);
/* SURVEY.md §8(f).2 strided rows: store samples 0, stride, 2*stride, ... (default 1 = every sample); combined with
 * max_samples the cap counts STORED samples. ltp_replan_states_batch's sample index is a stored-sample index. */
int ltp_set_sample_stride(ltp_planner* p, int stride);
int ltp_get_sample_stride(const ltp_planner* p);
/* SURVEY.md §8(f).3 q_goal pre-check, off by default. The reference validates q_0, v_0, a_0 (cc:68-77) but not
 * q_goal: a goal beyond the joint range is planned, sampled and only then reported by the end-limit check (cc:59-61).
 * With enabled != 0 such a query (or a NaN goal) gets LTP_STATUS_GOAL_OUTSIDE, traj_len 0 and is not sampled; every
 * other query is planned exactly as before. */
int ltp_set_goal_check(ltp_planner* p, int enabled);
int ltp_get_goal_check(const ltp_planner* p);
/* LTP_SEMANTICS_CPP (default) or LTP_SEMANTICS_MATLAB, see above. Captured with the batch geometry: the
 * calls that consume a planned batch refuse a handle whose semantics changed in between. With MATLAB semantics rows are
 * written by k_sample_walk_matlab_* (or, on request, the table pass), envelopes take the table pass, single calls the staged
 * path; ltp_end_limit_batch does nothing. */
int ltp_set_semantics(ltp_planner* p, int semantics);
int ltp_get_semantics(const ltp_planner* p);
/* LTP_POW_LIBM (default) or LTP_POW_EXACT, see above. Applies to the calls that plan (switching times, single-joint entry
 * points, the one-launch single call); samplers and consumers form no powers and do not depend on it. */
int ltp_set_pow_rule(ltp_planner* p, int rule);
int ltp_get_pow_rule(const ltp_planner* p);
/* NEW (no counterpart in the reference): which pow rule reproduces the C library THIS process is linked against — the libm a
 * reference built on this host calls at src/long_term_planner.cc:125-331, 378-621. Runs on the host only (no handle, no GPU):
 * `probes` (<= 0: 2^18) planner-sized arguments through the installed pow(x, 3 | 4 | 6 | 1.0 / 2), compared bit for bit with
 * both rules. Returns LTP_POW_LIBM when every result has the restated glibc bits (then the default rule gives the reference's
 * records bit for bit), LTP_POW_EXACT when the installed pow is correctly rounded on all of them (then ltp_set_pow_rule(p,
 * LTP_POW_EXACT) does), or -1: neither — the installed libm is a third one, and about one power in a thousand differs in its
 * last bit from either rule: expect ~2 plans per million with a jerk sample beyond 1e-9 whichever rule is set.
 * The two mismatch counts are written where the pointers are non-null. */
int ltp_host_libm_pow_rule(long long probes, long long* mismatches_libm, long long* mismatches_exact);

/* Where the run tables come from. A sampler / envelope item needs the joint's run tables (<= 20 runs of constant jerk with 10
 * closed-form coefficients each). Three ways, all with bit-identical results:
 *   - built inside the sampler kernel by the item's whole block (k_sample, the envelope's fused form): no extra memory traffic,
 *     ~8 us of latency per item — right for whole float64 rows, which hide it;
 *   - built by one wave of the sampler's block beside its streaming waves (k_sample_walk_*, round 4): no extra memory traffic
 *     either and nothing to hide — right for every row format whose plans have few bytes (capped, float32, sparse rows);
 *   - the table pass: a kernel of their own before the consumer (lane = (plan, joint); 912 bytes per joint through the handle's
 *     workspace) — what ltp_envelope_batch and ltp_build_tables_batch use, and ltp_sample_batch on request (flags bit 2).
 * mode 0 = automatic (rows: k_sample_walk_* for a cap of <= 768 samples, float32 rows, every 3rd sample or sparser, MATLAB
 * semantics, else k_sample; envelopes: the table pass), 1 = never the block-wide fused build (rows: always k_sample_walk_*;
 * envelopes: the table pass), -1 = always the fused build (rows: k_sample; envelopes: built in the kernel). ltp_sample_batch's
 * flags bits 2 / 3 / 5 / 6 choose per call. */
int ltp_set_table_pass(ltp_planner* p, int mode);
int ltp_get_table_pass(const ltp_planner* p);
/* Upper bound (bytes) of the table workspace; default: the larger of 4 GiB and 1/16 of the device's memory (18 GiB on MI355X).
 * Ranges whose tables do not fit are processed in pieces; if the device cannot spare that much, the workspace is smaller. */
int ltp_set_table_workspace(ltp_planner* p, unsigned long long bytes);

/* ---- batched hot path (device pointers, asynchronous on `stream`) -------------------------- */

/* Allocates the handle's device workspace for batches of up to n queries now. The batched calls below grow it on
 * demand (hipMalloc / hipFree), which is not allowed while `stream` is being captured into a hipGraph: call this once
 * before hipStreamBeginCapture — and ltp_reserve_tables if the captured calls take the table pass — then
 * ltp_plan_switch_times_batch / ltp_sample_batch / ltp_envelope_batch / ltp_replan_states_batch only enqueue memset and
 * kernel nodes and the graph can be replayed on new inputs in place. Growing a workspace later (a larger n, a larger
 * ltp_reserve_tables) frees the old buffers: graphs instantiated before that must not be replayed any more. */
int ltp_reserve_batch(ltp_planner* p, long long n);
/* Allocates the table-pass workspace for ranges of up to n plans (at most ltp_set_table_workspace bytes; longer ranges
 * are processed in pieces). Needed before capturing a call that takes the table pass — ltp_envelope_batch by default,
 * ltp_build_tables_batch's callers with the library's workspace, ltp_sample_batch* when flag bit 2 is set, or when flag bit 5 forbids
 * the walk kernel for rows of at most 8 KB (float64) / 16 KB (float32) per joint under a cap (those then take the table pass), and
 * every ltp_sample_batch* call in MATLAB semantics with more than the walk kernel forbidden: while a stream is
 * being captured the library neither allocates nor frees; it cuts the range into pieces that fit the workspace it has
 * and returns LTP_ERR_INVALID_ARGUMENT if it has none. */
int ltp_reserve_tables(ltp_planner* p, long long n);

/* planTrajectory stages 1-3 for n queries (cc:14-55): checkInputs, optSwitchTimes per joint,
 * slowest-joint reduction, timeScaling per other joint, fallback copy; then traj_len (cc:716-719).
 * offsets (device, [n+1], may be NULL) receives the exclusive scan of the packed trajectory sizes
 * in elements (doubles, or floats for ltp_sample_batch_f32): plan p occupies [offsets[p], offsets[p+1]) of a packed
 * buffer, laid out [q,v,a,j][joint][ltp_row_stride(stored samples of p)]. */
int ltp_plan_switch_times_batch(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* out,
                                unsigned long long* offsets, void* stream);

/* NEW (no counterpart in the reference): retime a planned batch to requested durations and synchronised groups.
 * The reference's timeScaling (cc:358-645) takes the time a joint must take as an argument; planTrajectory (cc:41-48) only ever
 * passes the slowest joint's optimum. This call passes a time the caller chose, per query or per group of queries.
 *
 * Terms. A query is ELIGIBLE if (status & ~(LTP_STATUS_END_LIMIT | LTP_STATUS_OVERFLOW)) == 0 and slowest >= 0, i.e. it was
 * planned. T* is its optimum t_opt[slowest][6] (t_opt and slowest are never rewritten, so T* survives a retime). An eligible
 * query q gets the target
 *     T_q = max(T*_q, t_uniform, t_target[q], group_time[group[q]])
 * where a term that was not given does not count, and a per-query request that is not finite or negative never wins (like
 * NaN in the slowest-joint reduction cc:31-39). group_time[g] = max over the ELIGIBLE members of group g of
 * max(T*, t_uniform, t_target) (0 for a group without such members); group ids outside [0, n_groups) mean "no group".
 *
 *  - T_q <= T*_q, or the query is not eligible: nothing of that query is written, its records keep their bits (for a fresh
 *    batch: exactly planTrajectory's).
 *  - T_q > T*_q: every joint, the slowest one included, is handled the way cc:41-55 handles a non-slowest joint:
 *    timeScaling(j, ..., dir_j, T_q), and where that finds no profile the fallback of cc:50-55 (t_scaled = t_opt, mod = 0,
 *    v_drive = v_max). t_required = T_q; traj_len is recomputed (cc:716-719); LTP_STATUS_END_LIMIT and LTP_STATUS_OVERFLOW are
 *    cleared (sampling or ltp_end_limit_batch forms them again); LTP_STATUS_NONFINITE may be set. t_opt, dir, slowest stay.
 *  - A retime is a pure function of the queries, t_opt, dir, slowest and T_q: applying it twice gives the records of applying
 *    it once, and it only lengthens plans — to get the reference plan back, plan again.
 *
 * The whole batch of n queries planned by ltp_plan_switch_times_batch (offsets are a scan over all n); `offsets` (device
 * [n+1] or NULL) is rewritten. Asynchronous on `stream`; uses the handle's workspace like ltp_plan_switch_times_batch, and after
 * ltp_reserve_batch(p, n) enqueues only memset and kernel nodes (can be captured into a hipGraph).
 * LTP_ERR_INVALID_ARGUMENT: LTP_SEMANTICS_MATLAB (LTPlanner.m's timeScaling differs), a batch geometry changed since planning,
 * a non-finite or negative t_uniform, group without n_groups >= 1 and group_time, opts == NULL, and an opts->size that is
 * below the first version of the struct, not a multiple of 8, or covers non-zero bytes beyond the fields this library knows.
 * MATLAB semantics and the multi-device entries are out of scope. */
typedef struct {
    unsigned size;          /* sizeof(ltp_retime_opts) in the caller's build */
    const double* t_target; /* device [n] or NULL: requested duration per query, seconds */
    double t_uniform;       /* requested duration of every query, 0 = none */
    const int* group;       /* device [n] or NULL: group id per query */
    int n_groups;
    double* group_time;     /* device [n_groups], required with group: receives each group's common duration */
} ltp_retime_opts;
int ltp_retime_batch(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* rec, const ltp_retime_opts* opts,
                     unsigned long long* offsets, void* stream);

/* NEW (no counterpart in the reference's public interface): STOP PLANS — every joint of every query brakes to rest as hard as it
 * may, by optBraking (cc:650-701), in one batched call. A safety shield asks every control period: if each robot brakes now, where
 * does each joint come to rest, when, and along which samples? planTrajectory cannot answer: it needs the goal first, and it
 * stretches every faster joint to the slowest joint's time (timeScaling, cc:41-55), which is no time-optimal stop.
 *
 * A stop batch IS a planned batch: its records are what planTrajectory holds for a joint whose goal is its standstill position
 * (the early exit of optSwitchTimes cc:100-107, then the fallback copy cc:50-55). Every reader of a planned batch therefore works
 * on it unchanged: ltp_sample_batch*, ltp_sample_window_batch, ltp_sample_horizon_batch, ltp_sample_knots_batch,
 * ltp_envelope_batch, ltp_envelope_knots_batch, ltp_state_at_batch, ltp_replan_states*_batch, ltp_end_limit_batch,
 * ltp_build_tables_batch. in->q_goal is NOT read and may be NULL; no reader reads it either. The q_stop array may be handed to
 * readers as q_goal.
 *
 * Per accepted query (C++ semantics), for every joint j: optBraking(j, v_0, a_0) gives q, t_rel[0..2] and dir;
 *   t_opt[j] = t_scaled[j] = the running sum of t_rel with t_rel[3..6] = 0; dir[j] = optBraking's dir (0 for a joint at rest);
 *   mod[j] = 0; v_drive[j] = v_max[j] (what cc:42 and the fallback leave); q_stop = q_0 + q, one addition (the value cc:96
 *   compares the goal with). q_stop is optBraking's closed form; the last sampled position is getTrajectory's and differs from it
 *   by the discretisation (up to a few 1e-3 rad with panda limits at 1 ms).
 * Per query: t_required and slowest follow cc:31-39 on t_opt[j][6] (start -1 / -1, strict '>', the first joint wins, NaN never
 *   wins): a robot at rest gets slowest 0, t_required 0, traj_len 1. No joint with a time that is not NaN: LTP_STATUS_NO_SLOWEST
 *   (cc:39). traj_len follows cc:716-719; a non-finite time sets LTP_STATUS_NONFINITE and traj_len 0, as for any planned batch.
 *   offsets (device [n+1] or NULL): the exclusive scan ltp_plan_switch_times_batch writes, under max_samples / sample_stride.
 *   No end-limit verdict is formed: ltp_end_limit_batch and the samplers form it, and a standstill outside [q_min, q_max] is then
 *   LTP_STATUS_END_LIMIT.
 * Rejected queries: any joint fails the chosen check.
 *   LTP_STOP_CHECK_INPUTS   checkInputs (cc:68-77) as planTrajectory applies it (the default);
 *   LTP_STOP_CHECK_BRAKING  only its comparison |a_0| > a_max, the one optBraking's formulas rest on: with |a_0| > a_max the first
 *                           phase (a_max - a_0) / j_max is negative and the reference's sampler would index below zero (cc:759).
 *                           Sampled accelerations of the reference's own trajectories exceed a_max by rounding and by
 *                           discretisation (up to a few percent), so a caller that restarts from a sampled state clamps a_0 to
 *                           +-a_max first (the Python wrapper planStopFrom offers that by name); the library alters no state.
 *   A NaN passes every comparison, as in the reference, and ends as LTP_STATUS_NONFINITE. A rejected query gets
 *   LTP_STATUS_INVALID_INPUT, traj_len 0, and in every other record field exactly the bits ltp_plan_switch_times_batch leaves for
 *   the same query planned towards optBraking's standstill position: t_opt, dir, t_required and slowest as above, t_scaled zero,
 *   v_drive = v_max, mod 0. q_stop (if given) holds NaN for it.
 * Limit sets (ltp_bind_limit_sets) are honoured, and the contract sentence of ltp_set_limit_sets extends to this call; a bad index
 *   gives LTP_STATUS_BAD_LIMIT_SET, traj_len 0, slowest -1 (q_stop NaN). Both pow rules apply (only q_stop depends on the rule).
 * The call captures the batch geometry like ltp_plan_switch_times_batch, uses the handle's workspace for the scan alone, and after
 * ltp_reserve_batch(p, n) enqueues only memset and kernel nodes: it can be captured into a hipGraph and replayed on rewritten
 * states. n == 0 and dof == 0 behave as in ltp_plan_switch_times_batch.
 * ltp_retime_batch refuses a stop batch (timeScaling towards a goal that was never given has no meaning) until the handle plans
 * with ltp_plan_switch_times_batch again.
 * LTP_ERR_INVALID_ARGUMENT: LTP_SEMANTICS_MATLAB (LTPlanner.m's sampler differs: out of scope, as for retime); opts == NULL or a
 * bad size (versioned strictly, the rule of ltp_retime_opts); check outside {0, 1}; incomplete records; a null in, q_0, v_0 or a_0.
 * Out of scope: fusing ltp_state_at_batch into the call (ltp_stop_knots_batch is the fused reader for a whole knot grid: standstill
 * position and time only, no records), synchronised braking, stops to a non-zero velocity, the *_multi entries. */
#define LTP_STOP_CHECK_INPUTS  0
#define LTP_STOP_CHECK_BRAKING 1
typedef struct {
    unsigned size;     /* sizeof(ltp_stop_opts) in the caller's build */
    int check;         /* LTP_STOP_CHECK_* */
    double* q_stop;    /* device, or NULL: standstill position per (query, joint), laid out like the queries (same strides) */
} ltp_stop_opts;       /* 16 bytes */
int ltp_plan_stop_batch(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* out, const ltp_stop_opts* opts,
                        unsigned long long* offsets, void* stream);

/* The end-limit check of planTrajectory (cc:59-61) WITHOUT sampling: for plans [first, first+count) of a planned
 * batch, walks every joint's runs to the last trajectory sample (the value ltp_sample_batch would store at
 * traj_len-1, bit for bit) and sets LTP_STATUS_END_LIMIT where it lies outside [q_min, q_max]. After this call
 * status == 0 is exactly planTrajectory's return value. ltp_sample_batch* and ltp_envelope_batch apply the same
 * check themselves; ltp_plan_switch_times_batch alone does not (status then holds the pre-sampling verdict
 * cc:14-39 only). The _host calls that do not sample run it for the caller. */
int ltp_end_limit_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                        void* stream);

/* getTrajectory (cc:706-841) + the end-limit check (cc:59-61) for plans [first, first+count):
 * plan p is written at out + (offsets[p] - offsets[first]); plans that would end beyond
 * `capacity` ELEMENTS get LTP_STATUS_OVERFLOW and are skipped. offsets, row strides and capacity are in elements and identical
 * for both row formats (rows are padded to 32 elements). `out`: device, 16-byte aligned.
 *
 * What is written of a row. A row of slen stored samples occupies R = ltp_row_stride(slen) elements and starts on a 64-byte
 * line of the tile (given an `out` on one). With L = ltp_row_line(slen, sizeof element) — slen rounded up to 8 doubles / 16 floats:
 *   [0, slen)  the samples;
 *   [slen, L)  +0.0: the row's last line is finished, so that it reaches the memory as one whole 64-byte write (a partly written
 *              line costs the memory controller a read-modify-write; measured: DESIGN.md §4);
 *   [L, R)     NOT written, and neither is anything of a plan that stores no samples or anything between plans.
 * Every sampler choice below writes exactly this. (ltp_sample_window_batch / ltp_sample_horizon_batch have their own rule.)
 *
 * ltp_sample_batch_ex is the entry point; its policy is a struct of named fields. Zero-initialise it, set .size =
 * sizeof(ltp_sample_opts) and only the fields you mean (opts == NULL: all defaults). Every choice writes THE SAME ROWS; the
 * fields only pick which kernel does it (DESIGN.md §4 has the measurements behind the defaults). */
#define LTP_ROWS_F64 0               /* binary64 rows (the reference's) */
#define LTP_ROWS_F32 1               /* the same binary64 results, rounded once to float when stored */
#define LTP_STORES_NONTEMPORAL 0     /* default: rows bypass the caches (they are written once and read by someone else) */
#define LTP_STORES_PLAIN 1
#define LTP_SAMPLER_AUTO 0           /* default: the library picks by row format (below) */
#define LTP_SAMPLER_FUSED 1          /* k_sample_*: a block builds a plan's run tables in LDS and streams its rows (whole f64 rows take it) */
#define LTP_SAMPLER_WALK 2           /* k_sample_walk_*: builder wave + streaming waves, tables never leave the compute unit (capped rows of
                                      * <= 768 samples, float32 rows, rows of every 3rd sample or sparser, MATLAB semantics take it);
                                      * caps of <= 32 samples use its autonomous-wave form (every wave builds and writes its own batches) */
#define LTP_SAMPLER_WALK_STREAMING 3 /* ... and keep the builder / streaming-wave form for caps of <= 32 samples too (A/B runs) */
#define LTP_SAMPLER_TABLE 4          /* k_build_tables + k_sample_tab_*: through the packed run tables of include/ltp_run_tables.hpp in HBM */
#define LTP_VERDICT_KEEP 0           /* default: the call also forms planTrajectory's end-limit verdict (cc:59-61, LTP_STATUS_END_LIMIT) */
#define LTP_VERDICT_SKIP 1           /* capped rows: stop at the cap instead of walking every joint to its last sample; LTP_STATUS_END_LIMIT
                                      * is then left unspecified by this call (ltp_end_limit_batch / end_limit = 1 form it); same rows */
typedef struct {
    unsigned size;       /* sizeof(ltp_sample_opts) in the caller's build: fields beyond it keep their defaults */
    int format;          /* LTP_ROWS_* : the element type `out` points to */
    int stores;          /* LTP_STORES_* */
    int sampler;         /* LTP_SAMPLER_* */
    int verdict;         /* LTP_VERDICT_* */
    int interleave;      /* block interleave factor of the work queue: 0 = default (64), 1 = blocks in plan order, <= 65535. Large
                          * tiles (>= 64 GiB) written with the default reach the HBM fill ceiling */
    int dry_run;         /* DIAGNOSTIC, 0 | 1: the store pattern without the arithmetic (not results) */
} ltp_sample_opts;
int ltp_sample_batch_ex(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                        const unsigned long long* offsets, void* out, unsigned long long capacity, const ltp_sample_opts* opts,
                        void* stream);
/* The same call with the policy packed into an int (rounds 1-5; kept for its callers, a thin wrapper over the same launcher):
 * bit 0 = LTP_STORES_NONTEMPORAL (NOTE: 0 here means plain stores), bit 1 = dry_run, bit 2 = LTP_SAMPLER_TABLE, bit 3 =
 * LTP_SAMPLER_FUSED, bit 4 = LTP_VERDICT_SKIP, bit 5 = never the walk kernels, bit 6 = LTP_SAMPLER_WALK, bit 6 | bit 7 =
 * LTP_SAMPLER_WALK_STREAMING, bits 8..23 = interleave. New code: ltp_sample_batch_ex. */
int ltp_sample_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                     const unsigned long long* offsets, double* out, unsigned long long capacity, int flags, void* stream);
int ltp_sample_batch_f32(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                         const unsigned long long* offsets, float* out, unsigned long long capacity, int flags, void* stream);

/* SURVEY.md §8(f).2 on-device consumer: position envelopes instead of dense rows. For plans [first, first+count) of
 * a batch planned by ltp_plan_switch_times_batch, env[((i*dof + j)*n_windows + w)*2 + {0,1}] = {min, max} of the q
 * samples w*window .. (w+1)*window-1 of joint j of local plan i — exactly the values getTrajectory (cc:706-841) /
 * ltp_sample_batch would have stored, reduced on the fly, so the dense trajectories (32*dof*traj_len bytes per plan)
 * never exist. Windows that start at or after traj_len hold the last position twice; plans with traj_len 0 (failed or
 * rejected) hold NaN. The end-limit check (cc:59-61) sets LTP_STATUS_END_LIMIT as the sampler does. max_samples and
 * sample_stride do not apply. env: device, count*dof*n_windows*2 doubles, 16-byte aligned. */
int ltp_envelope_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                       int window, int n_windows, double* env, void* stream);
/* How the envelope calls (ltp_envelope_batch, ltp_envelope_multi, ltp_plan_envelope*_host) find a window's extreme samples.
 * LTP_ENVELOPE_ANALYTIC (default)    inside a run q is one cubic in the sample index, so only the samples at the ends of each (run,
 *                                    window) stretch and either side of the real roots of its derivative are evaluated (they ARE samples
 *                                    of the row): a few evaluations per run instead of `window`, by a lane-per-(plan, joint) walk without
 *                                    run tables or workspace (k_envelope_walk: 3x the plans/s). By construction within a few ulps of q
 *                                    (<= 1e-12) of the exhaustive result — it could differ only where a neighbouring sample undercuts by
 *                                    rounding alone; MEASURED identical in all 8.8e9 window values of profiles/r06_envelope_mode_soak.json
 *                                    (panda, the reference's limits, 30-DoF, 36 wide-fuzzed limit sets, six window geometries), which is
 *                                    why it is the default since round 6. With ltp_set_table_pass(p, 1 | -1) the block-cooperative
 *                                    kernel's analytic form runs instead (same values).
 * LTP_ENVELOPE_EXHAUSTIVE            every sample of the window is evaluated: min / max have the BITS of the same reduction of the rows,
 *                                    by construction. The opt-in for callers who need that guarantee rather than the measurement. */
#define LTP_ENVELOPE_EXHAUSTIVE 0
#define LTP_ENVELOPE_ANALYTIC 1
int ltp_set_envelope_mode(ltp_planner* p, int mode);
int ltp_get_envelope_mode(const ltp_planner* p);

/* SURVEY.md §8(f).2 consumer HOOK: the run tables of plans [first, first+count) of a planned batch in a CALLER buffer, for
 * consumers of the caller's own (include/ltp_run_tables.hpp: the format, run_coef / run_eval, for_each_run / for_each_sample, and
 * the block-cooperative LDS form — the same single-source device functions ltp_sample_batch and ltp_envelope_batch are built
 * from). Per (plan, joint) 912 bytes: the <= 20 runs into which getTrajectory's jerk array (cc:735-807) and snap rules
 * (cc:815-829) cut the trajectory, each with the state before it; every sample is a closed-form polynomial of its position in
 * its run, with exactly the bits ltp_sample_batch would have stored. Lane index of (plan, joint) = (plan - first) * dof + joint.
 * tables: device, 16-byte aligned, bytes >= ltp_run_tables_bytes(p, count) (whole tiles of 64 lanes; the lanes of the last tile
 * beyond count * dof are not written). Plans with traj_len 0 get runs == 0. Applies the end-limit check (cc:59-61,
 * LTP_STATUS_END_LIMIT) like the samplers do (C++ semantics). max_samples / sample_stride do not apply: tables always cover the
 * whole trajectory. tests/cpp/example_consumer.hip is a complete user-side consumer. */
unsigned long long ltp_run_tables_bytes(const ltp_planner* p, long long n_plans);
int ltp_build_tables_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                           unsigned long long* tables, unsigned long long bytes, void* stream);

/* SURVEY.md §8(f).1 receding horizon (reference README.md:10-13): start states of the next plans = sample k of the
 * trajectories sampled into `tile` by ltp_sample_batch(first, count, ...). sample_index: device int[count] or NULL
 * (then uniform_index for all); k is clamped to the stored samples; plans that were not sampled — traj_len 0,
 * LTP_STATUS_OVERFLOW, or rows that would end beyond `capacity` elements of `tile` (the capacity given to
 * ltp_sample_batch) — keep the start state they had in `in`; nothing outside the tile is read. Output element (local plan i, joint j) at
 * ptr[i*query_stride + j*joint_stride]. The float64 form IGNORES THE CONTENT of `tile` (only its capacity rule applies; the pointer
 * must still be non-NULL): a stored float64 sample has the bits of the closed-form run evaluation, so the state is recomputed from
 * the records (a quarter of the time of 8-byte gathers from the tile). It therefore returns what ltp_sample_batch WOULD have stored:
 * `rec` and `in` must be unchanged since the batch was planned, and a tile that was written by a dry run (flags bit 1), edited by the
 * caller or never sampled is not noticed. Callers that post-process the tile and want the edited values use the float32 form (which
 * reads the ROUNDED values the tile holds) or gather themselves. */
int ltp_replan_states_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                            const unsigned long long* offsets, const double* tile, unsigned long long capacity,
                            const int* sample_index, int uniform_index,
                            double* q_0, double* v_0, double* a_0, long long query_stride, long long joint_stride, void* stream);
int ltp_replan_states_f32_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                                const unsigned long long* offsets, const float* tile, unsigned long long capacity,
                                const int* sample_index, int uniform_index,
                                double* q_0, double* v_0, double* a_0, long long query_stride, long long joint_stride, void* stream);
/* The same without any sampled rows: the state at TRAJECTORY sample k (0 .. traj_len-1, clamped; not a stored-sample
 * index) of plans [first, first+count), computed from the switching-time records alone with the sampler's own run
 * tables, i.e. with the bits ltp_sample_batch would have stored at k. No tile, no offsets: the cheap way to close a
 * receding-horizon loop on the device when only the restart state is needed. */
int ltp_state_at_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                       const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                       long long query_stride, long long joint_stride, void* stream);

/* NEW (no counterpart in the reference): HORIZON WINDOWS — the n_samples samples [k, k + n_samples) of plans [first, first+count)
 * of a planned batch, k per plan, in a FIXED-SHAPE buffer. The reference's README (lines 10-13) names the use: a controller
 * consumes a dense trajectory while targets arrive sparsely, and without a new target the robot keeps following the plan it has.
 * Every control period then needs the next N samples of plans that already exist, from a different sample per robot — without
 * storing k + N samples per row (ltp_set_max_samples), without the whole trajectory, and without planning again.
 *
 * Layout. Local plan i occupies out + i * 4 * dof * R elements, R = ltp_row_stride(n_samples); inside a plan [q,v,a,j][joint][R]
 * — exactly the packed layout of a batch in which every plan stores n_samples samples, so no offsets scan is needed (a torch
 * tensor [count, 4, dof, R]). Rows are 256-byte (LTP_ROWS_F64) or 128-byte (LTP_ROWS_F32) aligned; `out`: device, 16-byte
 * aligned. ltp_window_elements returns count * 4 * dof * R; a `capacity` (elements) below that is LTP_ERR_INVALID_ARGUMENT,
 * checked on the host before anything is launched. Elements [n_samples, R) of a row are NOT written.
 * Indexing. k is a TRAJECTORY sample index, as in ltp_state_at_batch: first_sample[i] (device int[count]) or, when that is NULL,
 * uniform_first for every plan; max_samples and sample_stride do not apply; k < 0 counts as 0.
 * Real samples. Element s of a row with k + s < traj_len has the bits ltp_sample_batch stores at trajectory sample k + s of that
 * row; for LTP_ROWS_F32 that binary64 value rounded once to float, as in ltp_sample_batch_f32.
 * Past the end (k + s >= traj_len, traj_len > 0): the robot rests at the last sample (README:13) — q holds the position of sample
 * traj_len - 1, v, a and j hold +0.0. This includes k >= traj_len: every sample of such a window is past the end.
 * Plans with traj_len == 0 (failed or rejected): all n_samples samples of all four arrays are NaN (ltp_envelope_batch's convention).
 * valid[i] (device int[count], or NULL) receives the number of real samples of plan i: min(n_samples, max(0, traj_len - k)), 0
 * for traj_len == 0.
 * What the call leaves alone. It neither reads nor writes `status` or any offsets, forms no end-limit verdict (ltp_end_limit_batch
 * exists for that), does not use the handle's workspace and allocates nothing: one kernel is enqueued on `stream`, so the call
 * can be captured into a hipGraph (rewrite first_sample in place between replays).
 * Both semantics, bound limit sets (ltp_bind_limit_sets) and retimed batches (ltp_retime_batch: the call reads t_scaled) are supported.
 * LTP_ERR_INVALID_ARGUMENT: dof, t_sample, max_samples, sample_stride, the semantics or the limit sets changed since the batch was
 * planned (Batch geometry, as for ltp_state_at_batch); a null argument; n_samples < 1; an unknown format; opts == NULL or an
 * opts->size that is below the first version of the struct, not a multiple of 8, or covers non-zero bytes beyond the fields this
 * library knows (versioned strictly, the rule of ltp_retime_opts).
 * Out of scope: the *_multi entries, fusing the window into the planning call. A stride inside the window is the next call's. */
typedef struct {
    unsigned size;            /* sizeof(ltp_window_opts) in the caller's build */
    int format;               /* LTP_ROWS_F64 | LTP_ROWS_F32: the element type `out` points to */
    int n_samples;            /* N >= 1 */
    const int* first_sample;  /* device int[count] or NULL: k per plan (trajectory sample index) */
    int uniform_first;        /* k of every plan when first_sample == NULL */
    int* valid;               /* device int[count] or NULL: receives the number of real samples per plan */
} ltp_window_opts;
unsigned long long ltp_window_elements(const ltp_planner* p, long long count, int n_samples);
int ltp_sample_window_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                            const ltp_window_opts* opts, void* out, unsigned long long capacity, void* stream);

/* NEW (no counterpart in the reference): STRIDED HORIZON WINDOWS — ltp_sample_window_batch with a stride inside the window: element
 * w of a row is trajectory sample k + w * stride, k per plan, stride per call. A predictive controller's horizon is rarely on the
 * t_sample grid (20 to 64 knots, several t_sample apart); this call writes those knots and nothing in between, instead of a dense
 * window of n_samples * stride samples that the caller decimates. stride == 1 IS ltp_sample_window_batch (the same launch).
 *
 * Layout. [count][q,v,a,j][dof][R] with R = ltp_row_stride(n_samples), exactly as for ltp_sample_window_batch: the layout depends
 * on n_samples only, ltp_window_elements(p, count, n_samples) is the size rule, `out` is device memory, 16-byte aligned, and a
 * `capacity` (elements) below the size rule is LTP_ERR_INVALID_ARGUMENT. Elements [n_samples, R) of a row are NOT written.
 * Indexing. k is a TRAJECTORY sample index: first_sample[i] (device int[count]) or, when that is NULL, uniform_first for every
 * plan; max_samples and sample_stride of the handle do not apply; k < 0 counts as 0.
 * Real samples. Element w with k + w * stride < traj_len has the bits ltp_sample_batch stores at trajectory sample k + w * stride
 * of that row (all four arrays: j is the jerk sample at that index, as in the sampler's strided rows, not an aggregate over the
 * samples in between); for LTP_ROWS_F32 that binary64 value rounded once to float.
 * Past the end (k + w * stride >= traj_len, traj_len > 0): q holds the position of sample traj_len - 1, v, a and j hold +0.0;
 * k >= traj_len means every element is past the end. Plans with traj_len == 0: NaN in all four arrays.
 * valid[i] (device int[count], or NULL): min(n_samples, ceil(max(0, traj_len - k) / stride)), 0 for traj_len == 0.
 * What the call leaves alone. As ltp_sample_window_batch: no `status`, no offsets, no end-limit verdict, no workspace, no
 * allocation; ONE kernel on `stream`, so the call can be captured into a hipGraph (rewrite first_sample in place between replays).
 * Both semantics, bound limit sets and retimed batches are supported.
 * LTP_ERR_INVALID_ARGUMENT: everything ltp_sample_window_batch refuses (the batch geometry rule, a null argument, n_samples < 1,
 * an unknown format, the strict size rule of the options struct), and stride < 1 and a span n_samples * stride beyond 2^30 (the
 * kernel's indices are ints; inside that bound no admitted argument overflows one).
 * Non-uniform knot grids are ltp_sample_knots_batch's (below). Out of scope: per-plan strides, the *_multi entries, fusing the
 * horizon into the planning call. */
typedef struct {
    unsigned size;            /* sizeof(ltp_horizon_opts) in the caller's build */
    int format;               /* LTP_ROWS_F64 | LTP_ROWS_F32: the element type `out` points to */
    int n_samples;            /* N >= 1: elements per row */
    int stride;               /* s >= 1: element w is trajectory sample k + w * s */
    const int* first_sample;  /* device int[count] or NULL: k per plan (trajectory sample index) */
    int uniform_first;        /* k of every plan when first_sample == NULL */
    int* valid;               /* device int[count] or NULL: receives the number of real samples per plan */
} ltp_horizon_opts;
int ltp_sample_horizon_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                             const ltp_horizon_opts* opts, void* out, unsigned long long capacity, void* stream);

/* NEW (no counterpart in the reference): KNOT-GRID HORIZONS — ltp_sample_horizon_batch on any grid: element w of a row is trajectory
 * sample k + g[w], k per plan, g ONE list of n_knots offsets per call. A predictive controller's horizon is usually dense near the
 * present and sparse further out (16 knots one sample apart, then 12 four apart, then 12 sixteen apart: 40 knots over 240 samples);
 * this call writes those knots into the same fixed-shape buffer, instead of a dense window of g[N-1] + 1 samples that the caller
 * thins out, or one strided call per segment. g[w] = w * s IS ltp_sample_horizon_batch's result, g[w] = w ltp_sample_window_batch's.
 *
 * Everything not said here is what ltp_sample_horizon_batch documents, with N = n_knots: the layout [count][q,v,a,j][dof][R],
 * R = ltp_row_stride(n_knots), ltp_window_elements(p, count, n_knots) as the size rule, k < 0 counting as 0, NaN for plans without
 * a trajectory, elements [n_knots, R) NOT written; no status, no offsets, no workspace, no allocation, ONE kernel on `stream`
 * (capture it into a hipGraph and rewrite first_sample AND the content of knot_offsets in place between replays); both semantics,
 * bound limit sets, retimed batches, the batch geometry rule.
 * The grid. knot_offsets: DEVICE int[n_knots], non-decreasing, 0 <= g[w] <= 2^30. g[w] == g[w + 1] is allowed and repeats the
 * sample; g[0] need not be 0.
 * Real elements. Element w with k + g[w] < traj_len has the bits ltp_sample_batch stores at trajectory sample k + g[w] of that row;
 * for LTP_ROWS_F32 that binary64 value rounded once to float.
 * Past the end (k + g[w] >= traj_len, traj_len > 0): q holds the position of sample traj_len - 1, v, a and j hold +0.0.
 * valid[i] (device int[count], or NULL): the number of w with k + g[w] < traj_len, 0 for traj_len == 0.
 * A grid that breaks the contract. The grid is device memory, so this call cannot look at it without a synchronisation and does
 * not: a decreasing, negative or beyond-2^30 grid gives unspecified VALUES in elements [0, n_knots) of the call's rows and in
 * valid — and nothing else. The call still reads nothing outside the batch and the n_knots ints, writes nothing outside those
 * elements, and forms no signed overflow (the kernel clamps every offset to [0, 2^30] when it reads the grid, and every range of
 * elements it derives to [0, n_knots]). The entries that are given the grid in HOST memory (ltp_plan_knots_host, the Python and
 * C++ wrappers) check it and refuse such a grid.
 * LTP_ERR_INVALID_ARGUMENT: everything ltp_sample_horizon_batch refuses (the batch geometry rule, a null argument, an unknown
 * format, the strict size rule of the options struct), knot_offsets == NULL, n_knots < 1 and n_knots > LTP_MAX_KNOTS.
 * Out of scope: per-plan grids, a unit multiplier on the offsets, the *_multi entries, fusing the call into planning. */
#define LTP_MAX_KNOTS 512
typedef struct {
    unsigned size;            /* sizeof(ltp_knots_opts) in the caller's build */
    int format;               /* LTP_ROWS_F64 | LTP_ROWS_F32: the element type `out` points to */
    int n_knots;              /* N, 1 .. LTP_MAX_KNOTS: elements per row */
    int uniform_first;        /* k of every plan when first_sample == NULL */
    const int* knot_offsets;  /* DEVICE int[n_knots]: g[w], non-decreasing, 0 <= g[w] <= 2^30 */
    const int* first_sample;  /* device int[count] or NULL: k per plan (trajectory sample index) */
    int* valid;               /* device int[count] or NULL: receives the number of real elements per plan */
} ltp_knots_opts;             /* 40 bytes */
int ltp_sample_knots_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                           const ltp_knots_opts* opts, void* out, unsigned long long capacity, void* stream);

/* NEW (no counterpart in the reference): HORIZON ENVELOPES — ltp_envelope_batch on the intervals of a knot grid, counted from where
 * each robot is now: per plan and joint {min q, max q} over the trajectory samples between knot w and knot w + 1 of the horizon the
 * caller hands to ltp_sample_knots_batch, k per plan, g ONE list of n_intervals + 1 edges per call. A safety shield that runs every
 * control period asks "where can joint j be between knot w and knot w + 1 of my horizon" and gets n_intervals * 16 bytes per joint,
 * instead of a dense window of g[M] + 1 samples of all four arrays that it reduces, or ltp_envelope_batch's windows of one width
 * counted from sample 0 of every plan.
 *
 * Layout: env[((i * dof + j) * M + w) * 2 + {0, 1}] = {min, max}, M = n_intervals, i = plan - first: ltp_envelope_batch's layout
 * with n_windows = M. float64, device memory, 16-byte aligned; `capacity` (in doubles) below ltp_envelope_knots_elements(p, count,
 * M) = count * dof * M * 2 is refused on the host before anything is launched.
 * Indexing: k = first_sample[i] (or uniform_first) is a TRAJECTORY sample index exactly as in ltp_sample_knots_batch: k < 0 counts
 * as 0, k > traj_len as traj_len; max_samples / sample_stride of the handle do not apply.
 * Interval w covers the trajectory samples t with a_w <= t <= b_w, a_w = k + g[w], b_w = max(a_w, k + g[w + 1] - 1 + closed), every
 * t clamped to traj_len - 1 (the robot rests at its last sample). closed = 0: the intervals of a strictly increasing grid tile
 * [k + g[0], k + g[M]) like ltp_envelope_batch's windows. closed = 1: interval w also holds the knot sample k + g[w + 1], which
 * neighbouring intervals then share — what a shield that bounds the motion BETWEEN two knots needs. g[w] == g[w + 1] is allowed:
 * that interval is the single sample a_w in either mode. An interval that starts at or past traj_len holds the last position
 * twice; one the trajectory ends in holds the samples that exist; plans with traj_len == 0 hold NaN.
 * Values: those of the ANALYTIC envelope form, whatever ltp_set_envelope_mode says (it does not apply to this call): the
 * candidates of every (run, interval) stretch are its two end samples and the samples either side of a real root of q'(m), each
 * evaluated as the sampler evaluates it, so every stored value IS a sample of the row, bit for bit; against the exhaustive
 * minimum / maximum of the interval's samples the result lies inside them and within a few ulps (see ltp_set_envelope_mode). A
 * caller who wants the exhaustive guarantee reduces a window (ltp_sample_window_batch). With k = 0, g[w] = w * window and
 * closed = 0 the result is bit-identical to ltp_envelope_batch(window, M) in analytic mode without a table pass.
 * valid[i] (device int[count], or NULL): the number of w in [0, M) with k + g[w] < traj_len, 0 for traj_len == 0.
 * Left alone: status (NO end-limit verdict: the walk stops when the last interval is stored), the offsets, the workspace; no
 * allocation, ONE kernel on `stream` (capture it into a hipGraph and rewrite first_sample AND the content of edge_offsets in place
 * between replays); both semantics, bound limit sets, retimed batches; the batch geometry rule of ltp_state_at_batch.
 * A grid that breaks the contract: edge_offsets is device memory, so this call cannot look at it without a synchronisation and does
 * not (the knots rule): a decreasing, negative or beyond-2^30 grid gives unspecified VALUES in the M pairs of each of the call's
 * (plan, joint) and in valid — every pair is still written exactly once — and nothing else. The call reads nothing outside the
 * batch and the M + 1 ints and forms no signed overflow (every edge is clamped to [0, 2^30] when the kernel reads the grid). The
 * entries that are given the grid in HOST memory (ltp_plan_envelope_knots_host, the Python and C++ wrappers) check it and refuse.
 * LTP_ERR_INVALID_ARGUMENT: everything ltp_sample_knots_batch refuses (the batch geometry rule, a null argument, a misaligned or
 * too small buffer, the strict size rule of the options struct), n_intervals < 1 or > LTP_MAX_KNOTS - 1, closed outside {0, 1},
 * edge_offsets == NULL.
 * Out of scope: float32, per-plan grids, the *_multi entries, an exhaustive mode, fusing the call into planning. (Envelopes of
 * v, a and j: ltp_envelope_knots_arrays_batch, below.) */
typedef struct {
    unsigned size;            /* sizeof(ltp_envelope_knots_opts) in the caller's build */
    int n_intervals;          /* M, 1 .. LTP_MAX_KNOTS - 1: the grid has M + 1 edges */
    int closed;               /* 0 | 1, see above */
    int uniform_first;        /* k of every plan when first_sample == NULL */
    const int* edge_offsets;  /* DEVICE int[M + 1]: g[w], non-decreasing, 0 <= g[w] <= 2^30 */
    const int* first_sample;  /* device int[count] or NULL: k per plan (trajectory sample index) */
    int* valid;               /* device int[count] or NULL: receives the number of intervals that start inside the trajectory */
} ltp_envelope_knots_opts;    /* 40 bytes */
unsigned long long ltp_envelope_knots_elements(const ltp_planner* p, long long count, int n_intervals);   /* count * dof * M * 2 */
int ltp_envelope_knots_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                             const ltp_envelope_knots_opts* opts, double* env, unsigned long long capacity, void* stream);

/* NEW (no counterpart in the reference): HORIZON ENVELOPES OF q, v, a AND j — ltp_envelope_knots_batch for any of the four arrays of
 * a row in one call: how fast, how hard accelerated and how hard jerked can joint j be between knot w and knot w + 1 of the
 * horizon? Speed-and-separation monitoring wants the peak |v| per interval, torque and power feasibility the peak |a|, actuator
 * wear limits the peak |j|; knot samples (ltp_sample_knots_batch) miss a peak between two knots, and a dense window of g[M] + 1
 * samples of all four arrays that the caller reduces is what this call replaces. The peak of |x| is max(-min, max).
 *
 * Everything not said here is what ltp_envelope_knots_batch documents: the grid, k, the intervals [a_w, b_w] and `closed`, valid,
 * a grid that breaks the contract (unspecified values in the pairs of the call and in valid, every pair still written exactly
 * once, no address and no signed overflow affected), what is left alone (status, the offsets, the workspace; no allocation, ONE
 * kernel on `stream`: capture it into a hipGraph and rewrite first_sample AND the content of edge_offsets between replays), both
 * semantics, bound limit sets, retimed batches, stop batches, the batch geometry rule and the refusals.
 * arrays: a non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J. With A = popcount(arrays) and x the rank of an array
 * among the selected ones, in the order q, v, a, j:
 * Layout: env[((((i * A + x) * dof + j) * M + w) * 2 + {0, 1}] = {min, max}, i = plan - first: a tensor [count][A][dof][M][2].
 * float64, device memory, 16-byte aligned; `capacity` (in doubles) below ltp_envelope_knots_arrays_elements(p, count, M, arrays) =
 * count * A * dof * M * 2 is refused on the host before anything is launched. With arrays == LTP_ENV_Q the call gives the layout
 * AND the bits of ltp_envelope_knots_batch.
 * Values. For array X let S_X(t) be what ltp_sample_knots_batch (float64) stores for trajectory sample t of row (i, j): the
 * sampler's bits for t < traj_len; for t >= traj_len the last position for q and +0.0 for v, a and j. Pair (X, w) is the minimum
 * and maximum of S_X(t) over a_w <= t <= b_w. For q that is ltp_envelope_knots_batch's rule (clamping t to traj_len - 1 gives the
 * same set); for v, a and j an interval with b_w >= traj_len also holds the value 0, and one that starts at or past traj_len holds
 * {0, 0}. Plans with traj_len == 0 hold NaN in every pair.
 * Candidates per (run, interval) stretch m0 .. m1 of run-local positions (include/ltp_run_tables.hpp: run_eval), each evaluated as
 * the sampler evaluates it, so every stored value IS a sample of the row (or the +0.0 past the end):
 *   q  ltp_envelope_knots_batch's: the two end samples and the samples either side of a real root of q'(m);
 *   v  the two end samples and, for m1 - m0 > 1, the samples either side of the root -c[5] / (2 c[6]) of v'(m) where c[6] != 0 and
 *      the root lies in (m0 - 1, m1 + 1): like q inside the exhaustive minimum / maximum and within a few ulps of it;
 *   a  the two end samples: fma(c[8], m, c[7]) is monotone in m as computed, so this IS the exhaustive result;
 *   j  c[9]: exhaustive too.
 * Which sign of zero is stored where both -0.0 and +0.0 occur in an interval is unspecified.
 * LTP_ERR_INVALID_ARGUMENT: everything ltp_envelope_knots_batch refuses, arrays outside 1 .. 15, reserved != 0.
 * Out of scope: float32, per-plan grids, the *_multi entries, peaks of |x|, the whole-plan ltp_envelope_batch. */
#define LTP_ENV_Q 1
#define LTP_ENV_V 2
#define LTP_ENV_A 4
#define LTP_ENV_J 8
typedef struct {
    unsigned size;            /* sizeof(ltp_envelope_arrays_opts) in the caller's build; the strict size rule of ltp_retime_opts */
    int n_intervals;          /* M, 1 .. LTP_MAX_KNOTS - 1: the grid has M + 1 edges */
    int closed;               /* 0 | 1, as ltp_envelope_knots_opts */
    int uniform_first;        /* k of every plan when first_sample == NULL */
    int arrays;               /* non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J */
    int reserved;             /* 0 */
    const int* edge_offsets;  /* DEVICE int[M + 1]: g[w], non-decreasing, 0 <= g[w] <= 2^30 */
    const int* first_sample;  /* device int[count] or NULL: k per plan (trajectory sample index) */
    int* valid;               /* device int[count] or NULL: receives the number of intervals that start inside the trajectory */
} ltp_envelope_arrays_opts;   /* 48 bytes */
/* count * popcount(arrays) * dof * M * 2; 0 for arrays outside 1 .. 15 */
unsigned long long ltp_envelope_knots_arrays_elements(const ltp_planner* p, long long count, int n_intervals, int arrays);
int ltp_envelope_knots_arrays_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                                    const ltp_envelope_arrays_opts* opts, double* env, unsigned long long capacity, void* stream);

/* NEW (no counterpart in the reference): FIRST EXITS — the readers above answer "what is the state at sample t" and "how far does
 * the joint go between two knots"; this one answers WHEN: per plan, selected array X of q, v, a, j and joint j, the smallest
 * trajectory sample t in [k, k + horizon) with S_X(t) < lo || S_X(t) > hi, for a box [lo, hi] per (plan, joint, array). A safety
 * shield or a task scheduler that follows existing plans asks every control period at which sample joint j first leaves its
 * position range, first exceeds the collaborative speed limit or a torque-derived bound on |a|. Composed of merged calls that is a
 * dense window of `horizon` samples of all four arrays plus a reduction on the caller's side, a cost that grows with the horizon;
 * an envelope over a knot grid narrows the answer to an interval but cannot name the sample. Here the cost is that of a one-interval
 * envelope: a stretch of a run whose extreme candidates lie inside the box holds no exit; where one lies outside, the first exit is
 * found by bisection on a monotone piece of the run's polynomial (csrc/ltp_crossings.hpp, which the host tests run too).
 *
 * S_X(t) is ltp_envelope_knots_arrays_batch's: for t < traj_len the bits ltp_sample_knots_batch (float64) stores; for t >= traj_len
 * the last position for q and +0.0 for v, a and j. A NaN sample never exits, and a NaN bound bounds nothing (the comparison of the
 * end-limit verdict, cc:59-61).
 * Layout: exit_sample[(i * A + x) * dof + j], i = plan - first, A = popcount(arrays), x the rank of the array among the selected ones
 * in the order q, v, a, j: a tensor [count][A][dof] of ints, device memory. The value is the ABSOLUTE trajectory sample index t
 * (>= the clamped k), LTP_EXIT_NONE when no sample of [k, k + horizon) lies outside, LTP_EXIT_NO_PLAN for a plan with
 * traj_len == 0. `capacity` (in ints) below ltp_first_exit_elements(p, count, arrays) = count * A * dof is refused on the host
 * before anything is launched.
 * Indexing: k = first_sample[i] (or uniform_first) is clamped as in ltp_envelope_knots_batch: k < 0 counts as 0, k > traj_len as
 * traj_len; max_samples / sample_stride of the handle do not apply. horizon = 2^30 is "the whole plan and the rest after it". Past
 * the end nothing is looped over: only sample max(k, traj_len) can be a new exit there, for v, a and j when the box excludes 0
 * (for q that sample equals the last one, which is an exit of its own when k < traj_len).
 * Boxes: lo[x] / hi[x] (x = 0 .. 3 for q, v, a, j) are device arrays of doubles or NULL. Element (i, j) of a given array is read
 * at ptr[i * box_query_stride + j * box_joint_stride]; box_query_stride == 0 is one box per joint for the whole call. A NULL side
 * is the plan's own limit on that side: q_min / q_max, -v_max / v_max, -a_max / a_max, -j_max / j_max — under a bound limit set,
 * the plan's own set. NOTE on the default a box: the sampled accelerations of the reference's trajectories exceed a_max by rounding
 * in most plans (see ltp_plan_stop_batch), so with it "most plans exit" is the truthful answer; a caller who wants a margin
 * passes a [dof] array with box_query_stride = 0. With arrays = LTP_ENV_Q, horizon = 2^30, k = 0 and default boxes,
 * exit != LTP_EXIT_NONE is the PATH-limit verdict the reference does not form: planTrajectory checks the last position alone
 * (cc:59-61, LTP_STATUS_END_LIMIT), so a plan that starts fast towards a joint stop overshoots the range in the middle and is
 * reported as fine.
 * first_any (device int[count], or NULL): the minimum over the selected arrays and joints of the plan, LTP_EXIT_NONE where every
 * entry is, LTP_EXIT_NO_PLAN for traj_len == 0. When given, ONE fill kernel (LTP_EXIT_NONE in every plan) is enqueued before the
 * kernel and the lanes fold with an unsigned atomicMin (LTP_EXIT_NONE > LTP_EXIT_NO_PLAN > every index); with first_any == NULL the
 * call enqueues exactly one kernel. (A fill kernel and not a memset: the memset node of a captured graph did not keep its value
 * over repeated replays on the runtime this was measured with.) Which array or joint won is not reported: the caller reads the
 * [A][dof] table.
 * Guarantees: a and j are exhaustive by construction (fma(c[8], m, c[7]) is monotone in m as computed; j is the run's constant).
 * q and v equal the exhaustive scan of the row unless an earlier sample lies outside by rounding alone (<= 1e-12, the bound of the
 * analytic envelope form): the call never reports an exit the row does not have — the reported sample IS outside the box, bit for
 * bit — and may report a later one only past samples that are outside by <= 1e-12.
 * Left alone: status (NO end-limit verdict), the offsets, the workspace; no allocation; the call can be captured into a hipGraph
 * either way (rewrite first_sample and the box arrays in place between replays); both semantics, bound limit sets, retimed
 * batches, stop batches; the batch geometry rule of ltp_state_at_batch.
 * LTP_ERR_INVALID_ARGUMENT: what ltp_envelope_knots_arrays_batch refuses that applies (the batch geometry rule, null in, rec or
 * exit_sample, the strict size rule of the options struct, a too small buffer), arrays outside 1 .. 15, horizon outside 1 .. 2^30,
 * a box pointer given for an array that is not selected, box_joint_stride == 0 with dof > 1 while any box pointer is given.
 * Out of scope: the first ENTRY into a box, the LAST exit (settling), which array or joint won first_any, float32, per-array
 * horizons, the *_multi entries, fusing the call into planning. */
#define LTP_EXIT_NONE    (-1)   /* no sample of [k, k + horizon) lies outside */
#define LTP_EXIT_NO_PLAN (-2)   /* traj_len == 0 */
typedef struct {
    unsigned size;              /* sizeof(ltp_first_exit_opts) in the caller's build; the strict size rule of ltp_retime_opts */
    int arrays;                 /* non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J */
    int horizon;                /* H, 1 .. 2^30 samples; 2^30 = "the whole plan and the rest after it" */
    int uniform_first;          /* k of every plan when first_sample == NULL */
    const int* first_sample;    /* device int[count] or NULL: k per plan (trajectory sample index) */
    const double* lo[4];        /* per array (index 0 .. 3 = q, v, a, j): device, or NULL = the plan's own limit on that side */
    const double* hi[4];
    long long box_query_stride; /* element (local plan i, joint j) of a box array at ptr[i * box_query_stride + j * box_joint_stride]; */
    long long box_joint_stride; /* box_query_stride == 0: one box per joint for the whole call */
    int* first_any;             /* device int[count] or NULL: min over the selected arrays and joints, LTP_EXIT_NONE / _NO_PLAN */
} ltp_first_exit_opts;          /* 112 bytes */
unsigned long long ltp_first_exit_elements(const ltp_planner* p, long long count, int arrays);   /* count * popcount(arrays) * dof; 0 for arrays outside 1 .. 15 */
int ltp_first_exit_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                         const ltp_first_exit_opts* opts, int* exit_sample, unsigned long long capacity, void* stream);

/* NEW (no counterpart in the reference): SETTLING — the question a task scheduler asks about every plan it follows: FROM WHICH
 * SAMPLE ON is joint j inside its tolerance and stays there? "Robot i is within 1 mrad of its goal and slower than 0.01 rad/s from
 * sample s on", "from sample s on the joint is below the collaborative speed limit for the rest of the plan", "from sample s on |a|
 * stays under the torque-derived bound". It is ltp_first_exit_batch read from the other end, and uses that call's terms without
 * exception: S_X(t) (the sampler's bits for t < traj_len; past the end the last position for q and +0.0 for v, a, j), outside =
 * S_X(t) < lo || S_X(t) > hi (a NaN sample is never outside, a NaN bound bounds nothing), k = first_sample[i] (or uniform_first)
 * clamped to [0, traj_len], horizon 1 .. 2^30 with 2^30 = "the whole plan and the rest after it", the boxes lo[4] / hi[4] with
 * box_query_stride / box_joint_stride and a NULL side = the plan's own limit on that side (under a bound limit set the plan's own
 * set; the NOTE on the default a box applies). Composed of merged calls the answer costs a dense window of `horizon` samples, or the
 * full rows for "the rest of the plan", plus a reverse scan on the caller's side; a knot-grid envelope narrows it to an interval,
 * never to a sample. Here the cost is that of a one-interval envelope: the LAST candidate outside, then one bisection on the
 * monotone piece that FOLLOWS it (csrc/ltp_crossings.hpp, which the host tests run too).
 *
 * With reach = k + horizon and O = { t in [k, reach) : S_X(t) outside }, the entry per plan, selected array and joint is
 *   LTP_EXIT_NO_PLAN    for traj_len == 0;
 *   LTP_SETTLE_NOT_YET  when sample reach - 1 is in O: the joint has not settled by the end of the horizon. For reach > traj_len
 *                       that is decided by the resting state alone: the last position for q, +0.0 for v, a and j;
 *   max(O) + 1          otherwise, k when O is empty: an ABSOLUTE trajectory sample index in [k, min(reach - 1, traj_len)];
 *                       == k means "inside throughout".
 * Layout: settle_sample[(i * A + x) * dof + j], i = plan - first, A = popcount(arrays), x the rank of the array among the selected
 * ones in the order q, v, a, j: a tensor [count][A][dof] of ints in device memory, exactly ltp_first_exit_batch's layout. `capacity`
 * (in ints) below ltp_settle_elements(p, count, arrays) = count * A * dof is refused on the host before anything is launched.
 * settle_all (device int[count], or NULL): the sample from which EVERY selected array of every joint of the plan is inside — the
 * maximum of the plan's indices —, LTP_SETTLE_NOT_YET where any entry is, LTP_EXIT_NO_PLAN for traj_len == 0. When given, ONE fill
 * kernel (0 in every plan) is enqueued before the kernel and the lanes fold with an unsigned atomicMax (as unsigned,
 * LTP_EXIT_NO_PLAN > LTP_SETTLE_NOT_YET > every index); a fill kernel and not a memset, for the reason given above. With
 * settle_all == NULL the call enqueues exactly one kernel. Which array or joint decided settle_all is not reported: the caller reads
 * the [A][dof] table.
 * Guarantees: a and j are exhaustive by construction (fma(c[8], m, c[7]) is monotone in m as computed; j is the run's constant).
 * For q and v the sample before a reported index IS outside the box, bit for bit, or the index is k: the call never reports a later
 * settling sample than the row has. It may report an EARLIER one than the exhaustive scan only past samples that are outside by
 * rounding alone (<= 1e-12, the project's bound for the analytic envelope form).
 * Left alone: status (NO end-limit verdict), the offsets, the workspace; no allocation; the call can be captured into a hipGraph
 * either way (rewrite first_sample and the box arrays in place between replays); both semantics, bound limit sets, retimed
 * batches, stop batches; the batch geometry rule of ltp_state_at_batch.
 * LTP_ERR_INVALID_ARGUMENT: everything ltp_first_exit_batch refuses (the batch geometry rule, null in, rec or settle_sample, the
 * strict size rule of the options struct, a too small buffer, arrays outside 1 .. 15, horizon outside 1 .. 2^30, a box pointer given
 * for an array that is not selected, box_joint_stride == 0 with dof > 1 while any box pointer is given).
 * Out of scope: the first ENTRY into a box, every exit in between, which array or joint decided settle_all, float32, per-array
 * horizons, the *_multi entries, fusing the call into planning. */
#define LTP_SETTLE_NOT_YET (-3) /* sample k + horizon - 1 lies outside: not settled by the end of the horizon */
typedef struct {
    unsigned size;              /* sizeof(ltp_settle_opts) in the caller's build; the strict size rule of ltp_retime_opts */
    int arrays;                 /* non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J */
    int horizon;                /* H, 1 .. 2^30 samples; 2^30 = "the whole plan and the rest after it" */
    int uniform_first;          /* k of every plan when first_sample == NULL */
    const int* first_sample;    /* device int[count] or NULL: k per plan (trajectory sample index) */
    const double* lo[4];        /* per array (index 0 .. 3 = q, v, a, j): device, or NULL = the plan's own limit on that side */
    const double* hi[4];
    long long box_query_stride; /* element (local plan i, joint j) of a box array at ptr[i * box_query_stride + j * box_joint_stride]; */
    long long box_joint_stride; /* box_query_stride == 0: one box per joint for the whole call */
    int* settle_all;            /* device int[count] or NULL: max over the selected arrays and joints, LTP_SETTLE_NOT_YET / LTP_EXIT_NO_PLAN */
} ltp_settle_opts;              /* 112 bytes */
unsigned long long ltp_settle_elements(const ltp_planner* p, long long count, int arrays);   /* count * popcount(arrays) * dof; 0 for arrays outside 1 .. 15 */
int ltp_settle_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                     const ltp_settle_opts* opts, int* settle_sample, unsigned long long capacity, void* stream);

/* NEW (no counterpart in the reference): STOP HORIZONS — ltp_plan_stop_batch asked at every knot of a horizon: "if robot i keeps
 * following its plan and starts braking at knot w, where does joint j come to rest, and how long does that take?" A fail-safe
 * shield needs this every control period; the answers over the horizon decide the latest knot up to which the intended plan may
 * still be followed. Composed of merged calls it is ltp_sample_knots_batch (four arrays, j unused), a transpose to count * N
 * states, a clamp of the accelerations and ONE ltp_plan_stop_batch over count * N states that writes 137 bytes of records per
 * (state, joint) for the 16 that are wanted. This call is that composition fused: nothing but the two answers is written.
 *
 * Layout. out[((i * 2 + x) * dof + j) * R + w], i = plan - first, x = 0 for q_stop and 1 for t_stop, R = ltp_row_stride(n_knots):
 * [count][{q_stop, t_stop}][dof][R] (a torch tensor [count, 2, dof, R]). float64, device memory, 16-byte aligned; `capacity` (in
 * doubles) below ltp_stop_knots_elements(p, count, n_knots) = count * 2 * dof * R is refused on the host before anything is
 * launched. Elements [n_knots, R) of a row are NOT written.
 * Indexing, the grid and valid are exactly ltp_sample_knots_batch's: k = first_sample[i] (or uniform_first) is a TRAJECTORY sample
 * index, k < 0 counts as 0 and k > traj_len as traj_len; knot_offsets is DEVICE int[n_knots], non-decreasing, 0 <= g[w] <= 2^30;
 * valid[i] (device int[count], or NULL) receives the number of w with k + g[w] < traj_len, 0 for traj_len == 0. A grid that breaks
 * the contract changes VALUES in elements [0, n_knots) of the call's rows and in valid, never an address: every offset is clamped
 * to [0, 2^30] when the kernel reads the grid and every range of elements it derives to [0, n_knots]. The entries that are given the
 * grid in HOST memory (ltp_plan_stop_knots_host, the Python and C++ wrappers) check it and refuse such a grid.
 * Element (i, j, w). Let (q, v, a) be what ltp_sample_knots_batch stores at element w of row (i, j), bit for bit — past the end
 * that is (q_last, +0.0, +0.0): no special case, the resting state goes through the same formula (and stops where it is, in no
 * time). The braking acceleration a' is
 *   LTP_STOP_ACCEL_CLAMP   a > a_max ? a_max : (a < -a_max ? -a_max : a); a NaN passes. torch.clamp, i.e. what planStopFrom offers
 *                          by name: sampled accelerations of the reference's trajectories exceed a_max by rounding in most plans
 *                          (see ltp_plan_stop_batch);
 *   LTP_STOP_ACCEL_STRICT  a itself; where |a| > a_max — LTP_STOP_CHECK_BRAKING's comparison — both planes hold NaN. The rule
 *                          applies PER (plan, joint, knot), not per query as in ltp_plan_stop_batch: this reader answers per joint
 *                          and the caller combines (a knot at which any joint is NaN is one the robot cannot be stopped from by
 *                          this rule).
 * Then optBraking (cc:650-701) on (v, a') under the joint's a_max and j_max gives qb and the three phases r[0..2]:
 *   q_stop = q + qb (one addition, as ltp_plan_stop_batch forms it), t_stop = (r[0] + r[1]) + r[2] —
 * the bits ltp_plan_stop_batch leaves in q_stop and in t_opt[j][6] for the state (q, v, a'). Plans with traj_len == 0 hold NaN in
 * both planes. The limits are the plan's own under a bound limit set. Only q_stop depends on the pow rule.
 * What the call leaves alone: status, the offsets, the workspace; no allocation, ONE kernel on `stream` (capture it into a
 * hipGraph and rewrite first_sample AND the content of knot_offsets in place between replays). Retimed batches, bound limit sets
 * and both pow rules are supported; a stop batch (ltp_plan_stop_batch) is a planned batch and is accepted as input.
 * LTP_ERR_INVALID_ARGUMENT: everything ltp_sample_knots_batch refuses (the batch geometry rule, a null argument, a misaligned or
 * too small buffer, the strict size rule of the options struct, knot_offsets == NULL, n_knots < 1 or > LTP_MAX_KNOTS), accel outside
 * {0, 1}, and LTP_SEMANTICS_MATLAB (the call follows the C++ reference's sampler, as ltp_plan_stop_batch does).
 * Out of scope: the robot-level stop time (the caller takes the maximum of t_stop over dof), dir, float32, per-plan grids, the
 * *_multi entries, synchronised braking. */
#define LTP_STOP_ACCEL_CLAMP  0
#define LTP_STOP_ACCEL_STRICT 1
typedef struct {
    unsigned size;            /* sizeof(ltp_stop_knots_opts) in the caller's build; the strict size rule of ltp_retime_opts */
    int n_knots;              /* N, 1 .. LTP_MAX_KNOTS: elements per row */
    int accel;                /* LTP_STOP_ACCEL_* */
    int uniform_first;        /* k of every plan when first_sample == NULL */
    const int* knot_offsets;  /* DEVICE int[n_knots]: g[w], non-decreasing, 0 <= g[w] <= 2^30 */
    const int* first_sample;  /* device int[count] or NULL: k per plan (trajectory sample index) */
    int* valid;               /* device int[count] or NULL: receives the number of knots inside the trajectory per plan */
} ltp_stop_knots_opts;        /* 40 bytes */
unsigned long long ltp_stop_knots_elements(const ltp_planner* p, long long count, int n_knots);   /* count * 2 * dof * R */
int ltp_stop_knots_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                         const ltp_stop_knots_opts* opts, double* out, unsigned long long capacity, void* stream);

/* Synthetic queries of SURVEY.md §8(d) (distribution of tests/randomConfiguration.m:14-34 with per-joint
 * limits), counter-based: query index first_query+p, so shards of one batch can be generated anywhere. */
int ltp_generate_queries_batch(ltp_planner* p, long long n, unsigned long long seed, long long first_query,
                               double* q_goal, double* q_0, double* v_0, double* a_0,
                               long long query_stride, long long joint_stride, void* stream);

/* ---- host-pointer convenience (synchronous) ------------------------------------------------- */

/* Full planTrajectory (cc:7-63) for n row-major [n][dof] host queries. Any record pointer may be NULL.
 * If packed != NULL, *packed receives a malloc'ed buffer of offsets[n] doubles (free with ltp_free_host)
 * and offsets ([n+1], host) must be non-NULL. With packed == NULL nothing is sampled, but status still carries
 * LTP_STATUS_END_LIMIT (ltp_end_limit_batch runs instead of the sampler): status == 0 is planTrajectory's bool. */
int ltp_plan_batch_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                        const double* a_0, const ltp_records* host_records, unsigned long long* offsets,
                        double** packed);
/* NEW: ltp_plan_batch_host with a retime (ltp_retime_batch) between planning and sampling. t_target: host [n] or NULL, requested
 * duration per query; t_uniform: requested duration of every query, 0 = none. Always the staged path (plan, retime, sample). */
int ltp_plan_retimed_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                          const double* a_0, const double* t_target, double t_uniform, const ltp_records* host_records,
                          unsigned long long* offsets, double** packed);
/* NEW: ltp_plan_batch_host with per-query limit sets (ltp_set_limit_sets): query q uses set set_index[q] (host [n]), bound for
 * this call only. Always the staged path (plan, then sampler or end-limit check). LTP_ERR_INVALID_ARGUMENT without sets. */
int ltp_plan_batch_sets_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                             const double* a_0, const int* set_index, const ltp_records* host_records,
                             unsigned long long* offsets, double** packed);

/* NEW: ltp_plan_stop_batch for n row-major [n][dof] host states, always the staged path (stop plan, then the sampler or
 * ltp_end_limit_batch). check: LTP_STOP_CHECK_*. Records, offsets and packed follow ltp_plan_batch_host, so status carries
 * LTP_STATUS_END_LIMIT. q_stop: host [n][dof] or NULL. */
int ltp_plan_stop_host(ltp_planner* p, long long n, const double* q_0, const double* v_0, const double* a_0, int check,
                       const ltp_records* host_records, double* q_stop, unsigned long long* offsets, double** packed);

/* ---- one process, several devices: contiguous query ranges, no collective ---------------- */

/* Range of shard `rank` of `world` over n queries: [*first, *first + *count), remainder to the lowest ranks. The same
 * rule as longtermplanner_amd/parallel.py::shard_range, bench.py and planTrajectoryBatchSharded. */
void ltp_shard_range(long long n, int rank, int world, long long* first, long long* count);

/* ltp_plan_batch_host over k planners, normally one per device (ltp_create(..., device = g, ...)), all configured
 * identically (else LTP_ERR_INVALID_ARGUMENT): shard g plans queries ltp_shard_range(n, g, k) on its own device from
 * its own host thread, all shards concurrently; there is no exchange between devices (queries are independent; the
 * only cross-lane step of planTrajectory, the slowest-joint reduction cc:31-39, is inside a query). Results are
 * written as ONE batch: records at their global query index, offsets rebased to the concatenated `*packed` buffer —
 * bit-identical to a single ltp_plan_batch_host call over all n queries. Several planners may name the same device
 * ("virtual shards", how the tests check this on one GPU). On error the first failing shard's code is returned
 * and ltp_last_error(planners[0]) names the shard. */
int ltp_plan_batch_multi(ltp_planner* const* planners, int k, long long n, const double* q_goal, const double* q_0,
                         const double* v_0, const double* a_0, const ltp_records* host_records, unsigned long long* offsets,
                         double** packed);

/* The same sharding with DEVICE-RESIDENT shards: nothing passes through the host. Shard g = queries ltp_shard_range(n, g, k)
 * of one batch of n; its queries, records and offsets live on planners[g]'s device as SHARD-LOCAL arrays (element 0 is the
 * shard's first query). One host thread per shard enqueues the work on shards[g].stream; the calls return when everything
 * is enqueued (asynchronous like the _batch calls; ltp_synchronize_multi waits for all shards). Results are bit-identical
 * to the single-handle calls over the whole batch, shard by shard. Planners as for ltp_plan_batch_multi (distinct
 * handles, identically configured, devices may repeat). */
typedef struct {
    ltp_queries in;                /* device pointers, shard-local */
    ltp_records out;               /* device pointers, shard-local, all non-NULL */
    unsigned long long* offsets;   /* device [count + 1] or NULL */
    void* stream;                  /* hipStream_t on planners[g]'s device, NULL = its default stream */
} ltp_shard;
/* ltp_plan_switch_times_batch per shard; end_limit != 0 adds ltp_end_limit_batch (status == 0 is then planTrajectory's bool) */
int ltp_plan_switch_times_multi(ltp_planner* const* planners, int k, long long n, const ltp_shard* shards, int end_limit);
/* ltp_envelope_batch per shard of a batch planned by ltp_plan_switch_times_multi; env[g]: device, count_g*dof*n_windows*2 doubles */
int ltp_envelope_multi(ltp_planner* const* planners, int k, long long n, const ltp_shard* shards, int window, int n_windows,
                       double* const* env);
/* ltp_state_at_batch per shard (receding horizon without rows). sample_index: NULL or per-shard device int arrays (entries may
 * be NULL); q_0[g], v_0[g], a_0[g]: device arrays laid out like the shard's queries (same strides) */
int ltp_state_at_multi(ltp_planner* const* planners, int k, long long n, const ltp_shard* shards, const int* const* sample_index,
                       int uniform_index, double* const* q_0, double* const* v_0, double* const* a_0);
int ltp_synchronize_multi(ltp_planner* const* planners, int k, const ltp_shard* shards);
/* ltp_plan_envelope_host over k planners: host arrays in, host envelopes and records out at their global query index
 * (what LongTermPlanner::planEnvelopeBatchSharded calls) */
int ltp_plan_envelope_multi_host(ltp_planner* const* planners, int k, long long n, const double* q_goal, const double* q_0,
                                 const double* v_0, const double* a_0, int window, int n_windows, const ltp_records* host_records,
                                 double* env);

/* planTrajectory stages 1-3 + the on-device envelope consumer (ltp_envelope_batch) for host arrays: a host caller
 * cannot take in the dense trajectories of a large batch (32*dof*traj_len bytes per plan over PCIe), but it can take
 * their position envelopes. env: host, n*dof*n_windows*2 doubles, layout as in ltp_envelope_batch. host_records
 * (optional, members may be NULL) receives the records as ltp_plan_batch_host does; status includes END_LIMIT. */
int ltp_plan_envelope_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                           const double* a_0, int window, int n_windows, const ltp_records* host_records, double* env);

/* NEW: planTrajectory stages 1-3 + ltp_sample_window_batch for host arrays: the n_samples samples from first_sample[q] (host
 * int[n], or NULL: uniform_first for every query) on of every plan, float64. rows: host, caller-owned, ltp_window_elements(p, n,
 * n_samples) doubles, layout and content as ltp_sample_window_batch writes them (elements [n_samples, R) of a row are zero);
 * valid: host int[n] or NULL. host_records (optional, members may be NULL) receives the records as ltp_plan_batch_host does;
 * ltp_end_limit_batch runs too, so status == 0 is planTrajectory's bool. Always the staged path. */
int ltp_plan_window_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                         const double* a_0, const int* first_sample, int uniform_first, int n_samples,
                         const ltp_records* host_records, double* rows, int* valid);
/* NEW: ltp_plan_window_host with a stride (ltp_sample_horizon_batch): element w of a row is trajectory sample k + w * stride.
 * rows: host, ltp_window_elements(p, n, n_samples) doubles (elements [n_samples, R) of a row are zero); everything else as above. */
int ltp_plan_horizon_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                          const double* a_0, const int* first_sample, int uniform_first, int n_samples, int stride,
                          const ltp_records* host_records, double* rows, int* valid);
/* NEW: ltp_plan_window_host on a knot grid (ltp_sample_knots_batch): element w of a row is trajectory sample k + knot_offsets[w].
 * knot_offsets: HOST int[n_knots], and therefore checked: n_knots outside 1 .. LTP_MAX_KNOTS, a decreasing grid, a negative offset
 * or one beyond 2^30 is LTP_ERR_INVALID_ARGUMENT and nothing is launched. rows: host, ltp_window_elements(p, n, n_knots) doubles
 * (elements [n_knots, R) of a row are zero); everything else as above. */
int ltp_plan_knots_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                        const double* a_0, const int* first_sample, int uniform_first, int n_knots, const int* knot_offsets,
                        const ltp_records* host_records, double* rows, int* valid);
/* NEW: plan + the stop horizons (ltp_stop_knots_batch) for host arrays: ltp_plan_knots_host's arguments plus accel
 * (LTP_STOP_ACCEL_*). knot_offsets: HOST int[n_knots], and therefore checked like ltp_plan_knots_host's: nothing is launched for a
 * grid outside the contract. out: host, ltp_stop_knots_elements(p, n, n_knots) doubles, [n][{q_stop, t_stop}][dof][R] (elements
 * [n_knots, R) of a row are zero); valid: host int[n] or NULL. Like its siblings the entry runs ltp_end_limit_batch: status
 * carries LTP_STATUS_END_LIMIT as after ltp_plan_batch_host without rows. Not available with LTP_SEMANTICS_MATLAB. */
int ltp_plan_stop_knots_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                             const double* a_0, const int* first_sample, int uniform_first, int n_knots,
                             const int* knot_offsets /* HOST, checked */, int accel,
                             const ltp_records* host_records, double* out, int* valid);
/* NEW: plan + the horizon envelopes (ltp_envelope_knots_batch) for host arrays. edge_offsets: HOST int[n_intervals + 1], and
 * therefore checked: n_intervals outside 1 .. LTP_MAX_KNOTS - 1 (fewer than 2 edges), a decreasing grid, a negative edge or one
 * beyond 2^30 is LTP_ERR_INVALID_ARGUMENT and nothing is launched. first_sample: host int[n] or NULL (then uniform_first); env:
 * host, n * dof * n_intervals * 2 doubles; valid: host int[n] or NULL. Like its siblings the entry runs ltp_end_limit_batch:
 * status carries LTP_STATUS_END_LIMIT as after ltp_plan_batch_host without rows. */
int ltp_plan_envelope_knots_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                                 const double* a_0, const int* first_sample, int uniform_first, int n_intervals,
                                 const int* edge_offsets /* HOST, checked */, int closed,
                                 const ltp_records* host_records, double* env, int* valid);

/* NEW: ltp_plan_envelope_knots_host plus `arrays` (ltp_envelope_knots_arrays_batch): env: host, n * popcount(arrays) * dof *
 * n_intervals * 2 doubles, [n][A][dof][M][2]. arrays outside 1 .. 15 is LTP_ERR_INVALID_ARGUMENT and nothing is launched; everything
 * else as above. */
int ltp_plan_envelope_knots_arrays_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                                        const double* a_0, const int* first_sample, int uniform_first, int n_intervals,
                                        const int* edge_offsets /* HOST, checked */, int closed, int arrays,
                                        const ltp_records* host_records, double* env, int* valid);

/* NEW: plan + the first exits (ltp_first_exit_batch) for host arrays: n row-major host queries are planned, then the call from
 * k = first_sample[i] (host int[n], or NULL: uniform_first) over `horizon` samples. lo / hi: per array (index 0 .. 3 = q, v, a, j)
 * HOST arrays of doubles or NULL (the plan's own limit on that side), every given one [dof] (box_per_plan == 0: one box per joint
 * for the whole call) or [n][dof] (box_per_plan == 1); NULL for lo or hi itself is four NULLs. exit_sample: host, n *
 * popcount(arrays) * dof ints, [n][A][dof]; first_any: host int[n] or NULL. arrays outside 1 .. 15, horizon outside 1 .. 2^30,
 * box_per_plan outside {0, 1} or a box given for an array that is not selected is LTP_ERR_INVALID_ARGUMENT and nothing is launched.
 * Like its siblings the entry runs ltp_end_limit_batch: status carries LTP_STATUS_END_LIMIT as after ltp_plan_batch_host without
 * rows. */
int ltp_plan_first_exit_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                             const double* a_0, const int* first_sample, int uniform_first, int horizon, int arrays,
                             const double* const* lo /* HOST [4] or NULL */, const double* const* hi /* HOST [4] or NULL */,
                             int box_per_plan, const ltp_records* host_records, int* exit_sample, int* first_any);

/* NEW: plan + settling (ltp_settle_batch) for host arrays: ltp_plan_first_exit_host's arguments and rules, with settle_sample (host,
 * n * popcount(arrays) * dof ints, [n][A][dof]) and settle_all (host int[n] or NULL) in place of exit_sample and first_any. */
int ltp_plan_settle_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                         const double* a_0, const int* first_sample, int uniform_first, int horizon, int arrays,
                         const double* const* lo /* HOST [4] or NULL */, const double* const* hi /* HOST [4] or NULL */,
                         int box_per_plan, const ltp_records* host_records, int* settle_sample, int* settle_all);

/* LongTermPlanner::getTrajectory (cc:706-841) for n host records ([n][dof][7] times etc.). */
int ltp_get_trajectory_host(ltp_planner* p, long long n, const double* t, const double* dir, const signed char* mod,
                            const double* q_0, const double* v_0, const double* a_0, const double* v_drive,
                            int* traj_len, int* status, unsigned long long* offsets, double** packed);
void ltp_free_host(void* ptr);

/* LongTermPlanner::checkInputs (cc:68-77) */
int ltp_check_inputs_host(ltp_planner* p, const double* q_0, const double* v_0, const double* a_0, int* ok);
/* LongTermPlanner::optBraking (cc:650-701); t_rel[7] is in/out (only [0..2] are written) */
int ltp_opt_braking_host(ltp_planner* p, int joint, double v_0, double a_0, double* q, double* t_rel, double* dir);
/* LongTermPlanner::optSwitchTimes (cc:82-353); t[7] is in/out (written only where the reference writes it) */
int ltp_opt_switch_times_host(ltp_planner* p, int joint, double q_goal, double q_0, double v_0, double a_0, double v_drive,
                              double* t, double* dir, char* mod, int* ok);
/* LongTermPlanner::timeScaling (cc:358-645); accepted_case (may be NULL): 1..8, 0 = none */
int ltp_time_scaling_host(ltp_planner* p, int joint, double q_goal, double q_0, double v_0, double a_0, double dir,
                          double t_required, double* scaled_t, double* v_drive, char* mod, int* ok, int* accepted_case);

/* roots<T>() of the reference's long_term_planner/roots.h:22-34 (the one third-party computation of the hot path: Eigen 3.4's
 * EigenSolver on the monic companion matrix) for n polynomials of degree 1..8: ALL eigenvalues, in Eigen's output order and
 * conjugate-pair convention ((re, +im) first), real eigenvalues with an exactly zero imaginary part — what
 * getSmallestPositiveNonComplexRoot (roots.h:43-50) selects from. coef: [n][degree+1], highest coefficient first; re, im:
 * [n][degree]. A non-finite companion matrix or a non-converged iteration gives NaN (the reference: uninitialised).
 * The float form exists because the reference's own known-answer test is in float (tests/src/roots_tests.cc:9-32). */
int ltp_roots_f64_host(ltp_planner* p, long long n, int degree, const double* coef, double* re, double* im);
int ltp_roots_f32_host(ltp_planner* p, long long n, int degree, const float* coef, float* re, float* im);

/* ---- diagnostics used by the parity tests ---------------------------------------------------- */
/* MATLAB semantics: flags of the latest one-lane call (ltp_opt_*_host, ltp_time_scaling_host): 1 = complex intermediate, 2 = LTPlanner.m would have raised an error */
int ltp_debug_last_matlab_flags(const ltp_planner* p);
/* MATLAB's roots() as the MATLAB-semantics kernels compute it, n polynomials of degree 1..6: re, im [n][degree] in MATLAB's
 * output order, nroots [n] (degree minus stripped leading zeros), status [n] (0 ok, 1 no convergence, 2 NaN / Inf) */
int ltp_debug_roots_matlab_host(ltp_planner* p, long long n, int degree, const double* coef, double* re, double* im, int* nroots, int* status);
/* device_buffer (3 x count u64, or NULL to switch off): k_sample block start / run tables ready / end on the
 * 100 MHz wall clock; ltp_envelope_batch writes 16 u64 per (plan, joint group) item instead: loop top, item drawn,
 * traj_len read, after each of the seven table-build barriers, reduction done */
int ltp_debug_set_sample_stamps(ltp_planner* p, unsigned long long* device_buffer);
/* tuning aid: size of the persistent k_sample / k_envelope grid (0 = what the device holds at once, the default) */
int ltp_debug_set_sample_blocks(ltp_planner* p, int blocks);
/* resident blocks of the persistent grids: which = 0 k_sample float64, 1 k_sample float32, 2 k_envelope, 3 / 4 k_sample_tab float64 / float32 */
int ltp_debug_get_sample_blocks(ltp_planner* p, int which);
/* out[i*8 + {0..7}] = x/y, sqrt|x|, x^3, x^4, x^6, floor(x/y), ceil(x/y), x*y+x computed on the device */
int ltp_debug_math_probe_host(ltp_planner* p, long long n, const double* x, const double* y, double* out);
/* out[i] = pow(x[i], y[i]) by the restated glibc pow of LTP_POW_LIBM (csrc/ltp_libm_pow.hpp), any finite or non-finite x, y */
int ltp_debug_libm_pow_host(ltp_planner* p, long long n, const double* x, const double* y, double* out);
/* root[i] = smallest positive exactly-real root of the degree-`degree` polynomial coef[i*7 .. i*7+degree]
 * (roots.h:22-50 semantics) */
int ltp_debug_roots_probe_host(ltp_planner* p, long long n, int degree, const double* coef, double* root);

#ifdef __cplusplus
}
#endif
#endif /* LTP_HIP_H */
