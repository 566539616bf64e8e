// ltp_capi_batch.hip — C ABI (include/ltp_hip.h): the batched hot path on device pointers (asynchronous on the caller's stream).
#include "ltp_handle.hpp"

#include <cmath>

using namespace ltp_capi;

// each work-queue launch gets its own head from a ring of 64, zeroed on `s` in stream order just before the kernel
static int next_queue_head(ltp_planner* p, hipStream_t s, unsigned long long** head)
{
    *head = p->d_sample_next + (p->sample_next_slot++ & 63u);
    LTP_HIP_TRY(p, hipMemsetAsync(*head, 0, sizeof(unsigned long long), s));
    return LTP_OK;
}

static int blocks_or_override(const ltp_planner* p, int resident) { return p->sample_blocks_override > 0 ? p->sample_blocks_override : resident; }

// the table pass over the plans of `range`: per piece of the range that fits the table workspace,
// launch(piece, head) runs k_build_tables and the kernel that reads the tables, named `kernel`
template <class Launch>
static int table_pass_pieces(ltp_planner* p, hipStream_t s, const ltp::PlanRange& range, const char* kernel, Launch&& launch)
{
    bool capturing = false;
    int rc;
    if ((rc = workspace_acquire(p, s, capturing)) != LTP_OK) return rc;
    long long per_piece = 0;
    if ((rc = ensure_tables(p, range.count, capturing, &per_piece)) != LTP_OK) return rc;
    const long long end = range.first + range.count;
    for (ltp::PlanRange piece = range; piece.first < end; piece.first += per_piece) {
        piece.count = end - piece.first < per_piece ? end - piece.first : per_piece;
        unsigned long long* head = nullptr;
        if ((rc = next_queue_head(p, s, &head)) != LTP_OK) return rc;
        launch(piece, head);
    }
    LTP_HIP_TRY(p, hipGetLastError());
    p->last_kernel = kernel;
    return workspace_release(p, s, capturing);
}

// A size-versioned options struct, strictly: the first version is the struct as it is now; a later version only appends fields whose
// zero value means "not used", so a newer caller's bytes beyond ours must be zero. *o receives the fields this library knows;
// returns what is wrong with *opts, or "".
template <class T>
static std::string checked_opts(const T* opts, const char* name, T* o)
{
    const std::string n(name);
    if (!opts) return n + " is NULL";
    if (opts->size < sizeof(T)) return n + ".size is below the first version of the struct";
    if (opts->size % 8u != 0) return n + ".size is not a multiple of 8";
    const unsigned char* tail = (const unsigned char*)opts;
    for (size_t b = sizeof(T); b < opts->size; ++b)
        if (tail[b] != 0) return n + " has non-zero bytes beyond the fields this library knows";
    memcpy(o, opts, sizeof(T));
    return "";
}

// What every call on a planned batch does first and last (the shape host_begin gives the *_host calls). begin(): the common null
// checks (null_arg: the entry's own pointers), then `refuse` — what the entry itself has against its arguments, "" for nothing —
// then, under the handle's lock from here to the end of the entry, the configuration and the batch geometry, the device, and the
// range as the launchers take it. end(): the launches' verdict; `kernel` is what ltp_last_sampler_kernel reports from then on.
struct BatchCall {
    std::unique_lock<std::mutex> lock;
    ltp::PlanRange r;
    hipStream_t s;
    int begin(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec, void* stream, bool null_arg,
              const std::string& refuse = "")
    {
        if (!p || first < 0 || count < 0 || !in || !records_complete(rec) || null_arg) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
        if (!refuse.empty()) return fail(p, LTP_ERR_INVALID_ARGUMENT, refuse);
        lock = std::unique_lock<std::mutex>(p->mu);
        int rc = check_config(p);
        if (rc == LTP_OK) rc = check_geometry(p);
        if (rc != LTP_OK) return rc;
        LTP_HIP_TRY(p, hipSetDevice(p->device));
        r = plan_range(p, first, count, in, rec);
        s = (hipStream_t)stream;
        return LTP_OK;
    }
    int end(ltp_planner* p, const char* kernel = nullptr)
    {
        LTP_HIP_TRY(p, hipGetLastError());
        if (kernel) p->last_kernel = kernel;
        return LTP_OK;
    }
};

// What a batch without a query or without a joint gets in place of a launch: zero offsets and, per query, the record of a plan
// that fails with slowest_joint == -1 (cc:39). The synchronisation keeps the host vectors alive until they are copied.
static int unplanned_batch(ltp_planner* p, long long n, const ltp_records* out, unsigned long long* offsets, hipStream_t s)
{
    if (offsets) LTP_HIP_TRY(p, hipMemsetAsync(offsets, 0, sizeof(unsigned long long) * (size_t)(n + 1), s));
    if (n == 0) return LTP_OK;
    std::vector<int> st((size_t)n, LTP_STATUS_NO_SLOWEST), neg((size_t)n, -1);
    std::vector<double> tr((size_t)n, -1.0);
    LTP_HIP_TRY(p, hipMemcpyAsync(out->status, st.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    LTP_HIP_TRY(p, hipMemcpyAsync(out->slowest, neg.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    LTP_HIP_TRY(p, hipMemcpyAsync(out->t_required, tr.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    LTP_HIP_TRY(p, hipMemsetAsync(out->traj_len, 0, sizeof(int) * (size_t)n, s));
    LTP_HIP_TRY(p, hipStreamSynchronize(s));
    return LTP_OK;
}

// What every planner of a batch does first and last (BatchCall's counterpart: it makes the geometry the readers check). begin():
// the common null checks (null_arg: the entry's own pointers); then, under the handle's lock from here to the end of the entry, the
// configuration and the binding (sets for this dof, C++ semantics), `cpp_only` — the refusal of an entry that follows the C++
// reference alone, NULL for none —, the device, the workspace (the scan's block sums, the offsets scratch) unless the batch is unplanned, the geometry, and
// planned(): what the entry records about its batch. An unplanned batch is finished here, and `launch` stays false. end(): offsets
// (the caller's, or the scratch) and stored lengths from the records the entry's kernels wrote, keep_status as launch_offsets takes
// it. A planned batch costs no heap allocation here: the arena tier of the host calls comes through it.
struct PlanCall {
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    bool capturing = false, launch = false;
    template <class Planned>
    int begin(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* out, unsigned long long* offsets, void* stream,
              bool null_arg, const char* cpp_only, Planned planned)
    {
        if (!p || n < 0 || !in || !records_complete(out) || null_arg) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
        lock = std::unique_lock<std::mutex>(p->mu);
        int rc = check_config(p);
        if (rc == LTP_OK) rc = check_sets(p);
        if (rc != LTP_OK) return rc;
        if (cpp_only && p->semantics == LTP_SEMANTICS_MATLAB) return fail(p, LTP_ERR_INVALID_ARGUMENT, cpp_only);
        s = (hipStream_t)stream;
        LTP_HIP_TRY(p, hipSetDevice(p->device));
        launch = n != 0 && p->dof != 0;
        if (launch && (rc = reserve(p, n)) != LTP_OK) return rc;
        if (launch && (rc = workspace_acquire(p, s, capturing)) != LTP_OK) return rc;
        capture_geometry(p);
        planned();
        return launch ? LTP_OK : unplanned_batch(p, n, out, offsets, s);
    }
    int end(ltp_planner* p, long long n, const ltp::Records& r, unsigned long long* offsets, int keep_status)
    {
        ltp::launch_offsets(s, n, p->dof, p->t_sample, r, p->d_block_sums, offsets ? offsets : p->d_offsets_scratch, true,
                            ltp::RowSpec{p->max_samples, p->sample_stride}, keep_status);
        LTP_HIP_TRY(p, hipGetLastError());
        return workspace_release(p, s, capturing);
    }
};

// what a reader has against the caller's output buffer, called the `noun` buffer in the texts: it is there, and 16-byte aligned
static std::string buffer_refusal(const void* buf, const char* noun)
{
    if (!buf) return std::string("null ") + noun + " buffer";
    if (((uintptr_t)buf & 15u) != 0) return std::string(noun) + " buffer must be 16-byte aligned";
    return "";
}

// The readers whose output has a fixed layout per plan (windows, horizons and knot grids; stop horizons; horizon envelopes), after
// their own argument rules: the entry prologue with `refuse`; `cpp_only` — the refusal of an entry that follows the C++ reference
// alone, NULL for none —; the capacity against elements(p, count, per_plan), which the texts call `elements_call`; the empty range;
// the bound of one launch; launch(c), the entry's one kernel.
template <class Elements, class Launch>
static int fixed_layout_read(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec, void* stream,
                             const std::string& refuse, const char* cpp_only, const char* noun,
                             Elements elements /* (const ltp_planner*, long long, int) -> unsigned long long */, const char* elements_call, int per_plan,
                             unsigned long long capacity, Launch launch)
{
    BatchCall c;
    const int rc = c.begin(p, first, count, in, rec, stream, false, refuse);
    if (rc != LTP_OK) return rc;
    if (cpp_only && p->semantics == LTP_SEMANTICS_MATLAB) return fail(p, LTP_ERR_INVALID_ARGUMENT, cpp_only);
    if (capacity < elements(p, count, per_plan))
        return fail(p, LTP_ERR_INVALID_ARGUMENT, std::string(noun) + " buffer smaller than " + elements_call);
    if (count == 0 || p->dof == 0) return LTP_OK;
    if ((count * (long long)p->dof + 63) / 64 > 0x7fffffffll) return fail(p, LTP_ERR_INVALID_ARGUMENT, "count * dof is beyond one launch");
    launch(c);
    return c.end(p);
}

// The two readers that hold a horizon [k, k + H) of selected arrays against boxes (first exits, settling): their options structs
// are the same field for field up to the last pointer, so the argument rules are stated once, with the struct's name in the texts;
// then fixed_layout_read over the int table [count][A][dof] both calls fill, and launch(c, o), the entry's kernel(s).
template <class Opts, class Launch>
static int box_horizon_read(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec, const Opts* opts,
                            const char* opts_name, const char* noun, const char* elements_call, const int* table, unsigned long long capacity,
                            void* stream, Launch launch)
{
    Opts o{};
    std::string refuse = checked_opts(opts, opts_name, &o);
    if (refuse.empty()) {
        bool any_box = false, unselected_box = false;
        for (int x = 0; x < 4; ++x) {
            const bool given = o.lo[x] || o.hi[x];
            any_box = any_box || given;
            unselected_box = unselected_box || (given && !(o.arrays >> x & 1));
        }
        const std::string name(opts_name);
        refuse = o.arrays < 1 || o.arrays > 15 ? name + ".arrays is no non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J"
                 : o.horizon < 1 || o.horizon > (1 << 30) ? name + ".horizon must be in 1 .. 2^30"
                 : unselected_box ? name + ": a box is given for an array that is not selected"
                 : any_box && o.box_joint_stride == 0 && p && p->dof > 1 ? name + ".box_joint_stride is 0 although the batch has more than one joint"
                 : !table ? std::string("null ") + noun + " buffer" : std::string();
    }
    const int arrays = o.arrays;
    return fixed_layout_read(p, first, count, in, rec, stream, refuse, nullptr, noun,
                             [arrays](const ltp_planner* h, long long c, int) { return ltp_first_exit_elements(h, c, arrays); },
                             elements_call, 0, capacity, [&](const BatchCall& c) { launch(c, o); });
}

extern "C" {

int ltp_plan_switch_times_batch(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* out,
                                unsigned long long* offsets, void* stream)
{
    PlanCall c;
    const int rc = c.begin(p, n, in, out, offsets, stream, false, nullptr, [] {});
    if (rc != LTP_OK || !c.launch) return rc;
    const ltp::Records r = to_dev(out);
    LTP_HIP_TRY(p, hipMemsetAsync(p->d_queue_count, 0, 16 * sizeof(unsigned long long), c.s));
    ltp::launch_switch_times(c.s, n, p->dof, p->t_sample, p->goal_check, dev_limits(p), to_dev(in), r, p->d_lane_flags, p->d_queue,
                             p->d_queue_count, stage_variant(p));
    return c.end(p, n, r, offsets, ltp::kStatusMatlabComplex);
}

int ltp_retime_batch(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* rec, const ltp_retime_opts* opts,
                     unsigned long long* offsets, void* stream)
{
    ltp_retime_opts o{};
    std::string refuse = checked_opts(opts, "ltp_retime_opts", &o);
    if (refuse.empty())
        refuse = !std::isfinite(o.t_uniform) ? "ltp_retime_opts.t_uniform is not finite"
                 : o.t_uniform < 0.0 ? "ltp_retime_opts.t_uniform is negative"
                 : o.group && o.n_groups < 1 ? "ltp_retime_opts.group needs n_groups >= 1"
                 : o.group && !o.group_time ? "ltp_retime_opts.group needs group_time" : "";
    BatchCall c;
    int rc = c.begin(p, 0, n, in, rec, stream, false, refuse);
    if (rc != LTP_OK) return rc;
    if (p->semantics == LTP_SEMANTICS_MATLAB)
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_batch follows the C++ reference's timeScaling: not available with LTP_SEMANTICS_MATLAB");
    if (p->planned.valid && p->planned.stop)
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_batch: the batch is a stop plan (ltp_plan_stop_batch), which has no goal to scale towards");
    if (o.group) LTP_HIP_TRY(p, hipMemsetAsync(o.group_time, 0, sizeof(double) * (size_t)o.n_groups, c.s));
    if (n == 0 || p->dof == 0) return LTP_OK;   // dof == 0: no query was planned (cc:39), there is nothing to retime
    if ((rc = reserve(p, n)) != LTP_OK) return rc;
    bool capturing = false;
    if ((rc = workspace_acquire(p, c.s, capturing)) != LTP_OK) return rc;
    LTP_HIP_TRY(p, hipMemsetAsync(p->d_queue_count, 0, 16 * sizeof(unsigned long long), c.s));
    const ltp::RetimeRequest req{o.t_target, o.t_uniform, o.group, o.n_groups, o.group_time};
    ltp::launch_retime(c.s, n, p->dof, p->t_sample, c.r.lim, c.r.in, c.r.rec, req, p->d_queue, p->d_queue_count, p->d_block_sums,
                       offsets ? offsets : p->d_offsets_scratch, ltp::RowSpec{p->max_samples, p->sample_stride}, stage_variant(p));
    if ((rc = c.end(p)) != LTP_OK) return rc;
    return workspace_release(p, c.s, capturing);
}

int ltp_plan_stop_batch(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* out, const ltp_stop_opts* opts,
                        unsigned long long* offsets, void* stream)
{
    ltp_stop_opts o{};
    std::string refuse = checked_opts(opts, "ltp_stop_opts", &o);
    if (refuse.empty() && o.check != LTP_STOP_CHECK_INPUTS && o.check != LTP_STOP_CHECK_BRAKING)
        refuse = "ltp_stop_opts.check is neither LTP_STOP_CHECK_INPUTS nor LTP_STOP_CHECK_BRAKING";
    if (!refuse.empty()) return fail(p, LTP_ERR_INVALID_ARGUMENT, refuse);   // the opts first: before the null checks
    PlanCall c;
    const int rc = c.begin(p, n, in, out, offsets, stream, !in || !in->q_0 || !in->v_0 || !in->a_0,
                           "ltp_plan_stop_batch follows the C++ reference's sampler: not available with LTP_SEMANTICS_MATLAB",
                           [&] { p->planned.stop = true; });
    if (rc != LTP_OK || !c.launch) return rc;
    const ltp::Records r = to_dev(out);
    ltp::launch_stop(c.s, n, p->dof, p->t_sample, dev_limits(p), to_dev(in), r, o.q_stop, o.check, stage_variant(p));
    return c.end(p, n, r, offsets, 0);
}

int ltp_end_limit_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec, void* stream)
{
    BatchCall c;
    const int rc = c.begin(p, first, count, in, rec, stream, false);
    if (rc != LTP_OK) return rc;
    if (p->semantics == LTP_SEMANTICS_MATLAB) return LTP_OK;   // LTPlanner.m has no position limits: there is no end-limit verdict
    ltp::launch_end_limit(c.s, c.r);
    return c.end(p);
}

static int sample_batch_any(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                            const unsigned long long* offsets, void* out, bool f32, unsigned long long capacity,
                            const ltp::SamplePolicy& pol, void* stream)
{
    BatchCall c;
    int rc = c.begin(p, first, count, in, rec, stream, !offsets || (!out && capacity > 0),
                     ((uintptr_t)out & 15u) != 0 ? "trajectory buffer must be 16-byte aligned" : "");
    if (rc != LTP_OK) return rc;
    if (count == 0 || p->dof == 0) return LTP_OK;
    if ((rc = reserve(p, 0)) != LTP_OK) return rc;   // work-queue heads, resident block counts (no-op after the first call)
    const ltp::RowSpec rows{p->max_samples, p->sample_stride};
    const ltp::SampleChoice k = ltp::choose_sampler(pol, p->semantics, p->table_pass, p->dbg_stamps != nullptr, f32, rows, p->dof);
    if (k.path == ltp::SamplePath::Table)
        return table_pass_pieces(p, c.s, c.r, k.kernel, [&](const ltp::PlanRange& piece, unsigned long long* head) {
            ltp::launch_build_tables(c.s, piece, rows, false, offsets, first, p->d_tables);
            ltp::launch_sample_tab(c.s, piece, first, offsets, out, f32, capacity, pol.nontemporal, pol.interleave, rows, head,
                                   blocks_or_override(p, p->tab_blocks[f32]), p->d_tables, p->dbg_stamps);
        });
    unsigned long long* head = nullptr;
    if ((rc = next_queue_head(p, c.s, &head)) != LTP_OK) return rc;
    if (k.path == ltp::SamplePath::Fused) {
        ltp::launch_sample(c.s, c.r, offsets, out, f32, capacity, pol.nontemporal, pol.dry, pol.interleave, rows, head,
                           blocks_or_override(p, p->fused_blocks[f32]), p->dbg_stamps);
    } else {
        ltp::launch_sample_walk(c.s, c.r, offsets, out, capacity, k.walk_kernel, pol.interleave, rows, head,
                                blocks_or_override(p, p->walk_blocks[f32]), p->walk_auto_cus);
    }
    return c.end(p, k.kernel);
}

int ltp_sample_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                     const unsigned long long* offsets, double* out, unsigned long long capacity, int flags, void* stream)
{
    return sample_batch_any(p, first, count, in, rec, offsets, out, false, capacity, ltp::policy_from_flags(flags), stream);
}

int ltp_sample_batch_f32(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                         const unsigned long long* offsets, float* out, unsigned long long capacity, int flags, void* stream)
{
    return sample_batch_any(p, first, count, in, rec, offsets, out, true, capacity, ltp::policy_from_flags(flags), stream);
}

int ltp_sample_batch_ex(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                        const unsigned long long* offsets, void* out, unsigned long long capacity, const ltp_sample_opts* opts, void* stream)
{
    ltp_sample_opts o;
    memset(&o, 0, sizeof o);
    if (opts) {
        // size-versioned: a caller built against an older (shorter) struct leaves the newer fields at their defaults (0)
        if (opts->size < sizeof(unsigned) + sizeof(int)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_sample_opts.size is not set");
        memcpy(&o, opts, opts->size < sizeof o ? opts->size : sizeof o);
    }
    if ((o.format != LTP_ROWS_F64 && o.format != LTP_ROWS_F32) || (o.stores != LTP_STORES_NONTEMPORAL && o.stores != LTP_STORES_PLAIN) ||
        o.sampler < LTP_SAMPLER_AUTO || o.sampler > LTP_SAMPLER_TABLE || (o.verdict != LTP_VERDICT_KEEP && o.verdict != LTP_VERDICT_SKIP) ||
        o.interleave < 0 || o.interleave > 0xFFFF || (o.dry_run != 0 && o.dry_run != 1))
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_sample_opts: a field is out of range");
    return sample_batch_any(p, first, count, in, rec, offsets, out, o.format == LTP_ROWS_F32, capacity, ltp::policy_from_opts(o), stream);
}

int ltp_envelope_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                       int window, int n_windows, double* env, void* stream)
{
    BatchCall c;
    int rc = c.begin(p, first, count, in, rec, stream, !env,
                     window < 1 || n_windows < 1 ? "window and n_windows must be >= 1"
                     : ((uintptr_t)env & 15u) != 0 ? "envelope buffer must be 16-byte aligned" : "");
    if (rc != LTP_OK) return rc;
    if (count == 0 || p->dof == 0) return LTP_OK;
    if ((rc = reserve(p, 0)) != LTP_OK) return rc;
    const int blocks = blocks_or_override(p, p->envelope_blocks);
    const ltp::EnvelopeChoice k = ltp::choose_envelope(p->envelope_mode, p->semantics, p->table_pass, p->dbg_stamps != nullptr);
    if (k.path == ltp::EnvelopePath::Table)
        return table_pass_pieces(p, c.s, c.r, k.kernel, [&](const ltp::PlanRange& piece, unsigned long long* head) {
            ltp::launch_build_tables(c.s, piece, ltp::RowSpec{0, 1}, true, nullptr, piece.first, p->d_tables);
            ltp::launch_envelope(c.s, piece, first, window, n_windows, env, head, blocks, nullptr, p->d_tables, k.analytic);
        });
    if (k.path == ltp::EnvelopePath::Walk) {
        ltp::launch_envelope_walk(c.s, c.r, first, window, n_windows, env);
    } else {
        unsigned long long* head = nullptr;
        if ((rc = next_queue_head(p, c.s, &head)) != LTP_OK) return rc;
        ltp::launch_envelope(c.s, c.r, first, window, n_windows, env, head, blocks, p->dbg_stamps, nullptr, k.analytic);
    }
    return c.end(p, k.kernel);
}

unsigned long long ltp_run_tables_bytes(const ltp_planner* p, long long n_plans)
{
    if (!p || n_plans <= 0 || p->dof <= 0) return 0ull;
    return ltp::table_bytes(n_plans * (long long)p->dof);
}

int ltp_build_tables_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                           unsigned long long* tables, unsigned long long bytes, void* stream)
{
    BatchCall c;
    const int rc = c.begin(p, first, count, in, rec, stream, !tables && count > 0,
                           ((uintptr_t)tables & 15u) != 0 ? "run-table buffer must be 16-byte aligned" : "");
    if (rc != LTP_OK) return rc;
    if (count == 0 || p->dof == 0) return LTP_OK;
    if (bytes < ltp::table_bytes(count * (long long)p->dof))
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "run-table buffer smaller than ltp_run_tables_bytes(p, count)");
    // whole tables (every run of every joint), lane = (plan - first) * dof + joint; the caller's buffer, not the handle's workspace
    ltp::launch_build_tables(c.s, c.r, ltp::RowSpec{0, 1}, true, nullptr, first, tables);
    return c.end(p);
}

static int replan_states_any(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                             const unsigned long long* offsets, const void* tile, bool f32, unsigned long long capacity,
                             const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                             long long query_stride, long long joint_stride, void* stream)
{
    BatchCall c;
    const int rc = c.begin(p, first, count, in, rec, stream, !offsets || (!tile && capacity > 0) || !q_0 || !v_0 || !a_0);
    if (rc != LTP_OK) return rc;
    ltp::launch_replan_states(c.s, c.r, ltp::RowSpec{p->max_samples, p->sample_stride}, offsets, tile, f32, capacity, sample_index, uniform_index,
                              q_0, v_0, a_0, query_stride, joint_stride);
    return c.end(p);
}

int ltp_state_at_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                       const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                       long long query_stride, long long joint_stride, void* stream)
{
    BatchCall c;
    const int rc = c.begin(p, first, count, in, rec, stream, !q_0 || !v_0 || !a_0);
    if (rc != LTP_OK) return rc;
    ltp::launch_state_at(c.s, c.r, sample_index, uniform_index, q_0, v_0, a_0, query_stride, joint_stride);
    return c.end(p);
}

unsigned long long ltp_window_elements(const ltp_planner* p, long long count, int n_samples)
{
    if (!p || count <= 0 || n_samples < 1 || p->dof <= 0) return 0ull;
    return (unsigned long long)count * 4ull * (unsigned long long)p->dof * (unsigned long long)ltp_row_stride(n_samples);
}

// ltp_sample_window_batch (stride 1), ltp_sample_horizon_batch and ltp_sample_knots_batch (knots != NULL, stride 1: n_samples is the
// number of knots): what they have against their opts, and the one launch. `name` is the options struct the texts speak of;
// `refuse` is what the entry has against its own opts ("" for nothing).
static int sample_window_any(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                             const char* name, std::string refuse, int format, int n_samples, int stride, const int* knots,
                             const int* first_sample, int uniform_first, int* valid, void* out, unsigned long long capacity, void* stream)
{
    const std::string n(name);
    if (refuse.empty())
        refuse = format != LTP_ROWS_F64 && format != LTP_ROWS_F32 ? n + ".format is neither LTP_ROWS_F64 nor LTP_ROWS_F32"
                 : n_samples < 1 ? n + (knots ? ".n_knots must be >= 1" : ".n_samples must be >= 1")
                 : n_samples > (1 << 30) ? n + ".n_samples is beyond 2^30"   // the kernel's sample indices are ints
                 : stride < 1 ? n + ".stride must be >= 1"
                 : (long long)n_samples * stride > (1ll << 30) ? n + ": the span n_samples * stride is beyond 2^30"
                 : buffer_refusal(out, "window");
    return fixed_layout_read(p, first, count, in, rec, stream, refuse, nullptr, "window", ltp_window_elements,
                             "ltp_window_elements(p, count, n_samples)", n_samples, capacity, [&](const BatchCall& c) {
        ltp::launch_sample_window(c.s, c.r, n_samples, ltp_row_stride(n_samples), stride, knots, first_sample, uniform_first, valid, out,
                                  format == LTP_ROWS_F32);
    });
}

int ltp_sample_window_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                            const ltp_window_opts* opts, void* out, unsigned long long capacity, void* stream)
{
    ltp_window_opts o{};
    const std::string refuse = checked_opts(opts, "ltp_window_opts", &o);
    return sample_window_any(p, first, count, in, rec, "ltp_window_opts", refuse, o.format, o.n_samples, 1, nullptr, o.first_sample,
                             o.uniform_first, o.valid, out, capacity, stream);
}

int ltp_sample_horizon_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                             const ltp_horizon_opts* opts, void* out, unsigned long long capacity, void* stream)
{
    ltp_horizon_opts o{};
    const std::string refuse = checked_opts(opts, "ltp_horizon_opts", &o);
    return sample_window_any(p, first, count, in, rec, "ltp_horizon_opts", refuse, o.format, o.n_samples, o.stride, nullptr, o.first_sample,
                             o.uniform_first, o.valid, out, capacity, stream);
}

int ltp_sample_knots_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                           const ltp_knots_opts* opts, void* out, unsigned long long capacity, void* stream)
{
    ltp_knots_opts o{};
    std::string refuse = checked_opts(opts, "ltp_knots_opts", &o);
    // the grid is device memory: its CONTENT is the kernel's to clamp (ltp_knots.hpp), its length and presence are checked here
    if (refuse.empty())
        refuse = !o.knot_offsets ? "ltp_knots_opts.knot_offsets is NULL"
                 : o.n_knots > LTP_MAX_KNOTS ? "ltp_knots_opts.n_knots is beyond LTP_MAX_KNOTS" : "";
    return sample_window_any(p, first, count, in, rec, "ltp_knots_opts", refuse, o.format, o.n_knots, 1, o.knot_offsets, o.first_sample,
                             o.uniform_first, o.valid, out, capacity, stream);
}

unsigned long long ltp_stop_knots_elements(const ltp_planner* p, long long count, int n_knots)
{
    if (!p || count <= 0 || n_knots < 1 || p->dof <= 0) return 0ull;
    return (unsigned long long)count * 2ull * (unsigned long long)p->dof * (unsigned long long)ltp_row_stride(n_knots);
}

int ltp_stop_knots_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                         const ltp_stop_knots_opts* opts, double* out, unsigned long long capacity, void* stream)
{
    ltp_stop_knots_opts o{};
    std::string refuse = checked_opts(opts, "ltp_stop_knots_opts", &o);
    // the grid is device memory: its CONTENT is the kernel's to clamp (ltp_knots.hpp), its length and presence are checked here
    if (refuse.empty())
        refuse = o.n_knots < 1 ? "ltp_stop_knots_opts.n_knots must be >= 1"
                 : o.n_knots > LTP_MAX_KNOTS ? "ltp_stop_knots_opts.n_knots is beyond LTP_MAX_KNOTS"
                 : o.accel != LTP_STOP_ACCEL_CLAMP && o.accel != LTP_STOP_ACCEL_STRICT ? "ltp_stop_knots_opts.accel is neither LTP_STOP_ACCEL_CLAMP nor LTP_STOP_ACCEL_STRICT"
                 : !o.knot_offsets ? "ltp_stop_knots_opts.knot_offsets is NULL"
                 : buffer_refusal(out, "stop");
    return fixed_layout_read(p, first, count, in, rec, stream, refuse,
                             "ltp_stop_knots_batch follows the C++ reference's sampler: not available with LTP_SEMANTICS_MATLAB", "stop",
                             ltp_stop_knots_elements, "ltp_stop_knots_elements(p, count, n_knots)", o.n_knots, capacity, [&](const BatchCall& c) {
        ltp::launch_stop_knots(c.s, c.r, o.n_knots, ltp_row_stride(o.n_knots), o.knot_offsets, o.first_sample, o.uniform_first, o.valid, o.accel,
                               stage_variant(p), out);
    });
}

unsigned long long ltp_envelope_knots_elements(const ltp_planner* p, long long count, int n_intervals)
{
    if (!p || count <= 0 || n_intervals < 1 || p->dof <= 0) return 0ull;
    return (unsigned long long)count * (unsigned long long)p->dof * (unsigned long long)n_intervals * 2ull;
}

static int env_arrays_count(int arrays) { return __builtin_popcount((unsigned)arrays & 15u); }

unsigned long long ltp_envelope_knots_arrays_elements(const ltp_planner* p, long long count, int n_intervals, int arrays)
{
    if (arrays < 1 || arrays > 15) return 0ull;
    return ltp_envelope_knots_elements(p, count, n_intervals) * (unsigned long long)env_arrays_count(arrays);
}

// ltp_envelope_knots_batch (q_only: its opts with arrays = LTP_ENV_Q, its own kernel) and ltp_envelope_knots_arrays_batch: what they
// have against their opts, and the one launch. `name` is the options struct the texts speak of, `elements_call` the size function;
// `refuse` is what the entry has against its own opts ("" for nothing).
static int envelope_knots_any(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                              const char* name, std::string refuse, const char* elements_call, bool q_only,
                              const ltp_envelope_arrays_opts& o, double* env, unsigned long long capacity, void* stream)
{
    const std::string n(name);
    // the grid is device memory: its CONTENT is the kernel's to clamp (ltp_knots.hpp), its length and presence are checked here
    if (refuse.empty())
        refuse = o.n_intervals < 1 ? n + ".n_intervals must be >= 1"
                 : o.n_intervals > LTP_MAX_KNOTS - 1 ? n + ".n_intervals is beyond LTP_MAX_KNOTS - 1"
                 : o.closed != 0 && o.closed != 1 ? n + ".closed is neither 0 nor 1"
                 : o.arrays < 1 || o.arrays > 15 ? n + ".arrays is no non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J"
                 : o.reserved != 0 ? n + ".reserved must be 0"
                 : !o.edge_offsets ? n + ".edge_offsets is NULL"
                 : buffer_refusal(env, "envelope");
    return fixed_layout_read(p, first, count, in, rec, stream, refuse, nullptr, "envelope",
                             [&o](const ltp_planner* h, long long c, int m) { return ltp_envelope_knots_arrays_elements(h, c, m, o.arrays); },
                             elements_call, o.n_intervals, capacity, [&](const BatchCall& c) {
        if (q_only) ltp::launch_envelope_knots(c.s, c.r, o.n_intervals, o.closed, o.edge_offsets, o.first_sample, o.uniform_first, o.valid, env);
        else ltp::launch_envelope_knots_arrays(c.s, c.r, o.n_intervals, o.closed, o.arrays, o.edge_offsets, o.first_sample, o.uniform_first, o.valid, env);
    });
}

int ltp_envelope_knots_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                             const ltp_envelope_knots_opts* opts, double* env, unsigned long long capacity, void* stream)
{
    ltp_envelope_knots_opts o{};
    const std::string refuse = checked_opts(opts, "ltp_envelope_knots_opts", &o);
    // (A = 1 plane per plan is the q-only layout and size)
    const ltp_envelope_arrays_opts any{sizeof(ltp_envelope_arrays_opts), o.n_intervals, o.closed, o.uniform_first, LTP_ENV_Q, 0,
                                       o.edge_offsets, o.first_sample, o.valid};
    return envelope_knots_any(p, first, count, in, rec, "ltp_envelope_knots_opts", refuse, "ltp_envelope_knots_elements(p, count, n_intervals)",
                              true, any, env, capacity, stream);
}

int ltp_envelope_knots_arrays_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                                    const ltp_envelope_arrays_opts* opts, double* env, unsigned long long capacity, void* stream)
{
    ltp_envelope_arrays_opts o{};
    const std::string refuse = checked_opts(opts, "ltp_envelope_arrays_opts", &o);
    return envelope_knots_any(p, first, count, in, rec, "ltp_envelope_arrays_opts", refuse,
                              "ltp_envelope_knots_arrays_elements(p, count, n_intervals, arrays)", false, o, env, capacity, stream);
}

unsigned long long ltp_first_exit_elements(const ltp_planner* p, long long count, int arrays)
{
    if (!p || count <= 0 || p->dof <= 0 || arrays < 1 || arrays > 15) return 0ull;
    return (unsigned long long)count * (unsigned long long)env_arrays_count(arrays) * (unsigned long long)p->dof;
}

int ltp_first_exit_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                         const ltp_first_exit_opts* opts, int* exit_sample, unsigned long long capacity, void* stream)
{
    return box_horizon_read(p, first, count, in, rec, opts, "ltp_first_exit_opts", "exit", "ltp_first_exit_elements(p, count, arrays)", exit_sample,
                            capacity, stream, [&](const BatchCall& c, const ltp_first_exit_opts& o) {
        ltp::launch_first_exit(c.s, c.r, o.arrays, o.horizon, o.first_sample, o.uniform_first, o.lo, o.hi, o.box_query_stride, o.box_joint_stride,
                               exit_sample, o.first_any);
    });
}

unsigned long long ltp_settle_elements(const ltp_planner* p, long long count, int arrays)
{
    return ltp_first_exit_elements(p, count, arrays);           // the same layout: count * popcount(arrays) * dof
}

int ltp_settle_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                     const ltp_settle_opts* opts, int* settle_sample, unsigned long long capacity, void* stream)
{
    return box_horizon_read(p, first, count, in, rec, opts, "ltp_settle_opts", "settle", "ltp_settle_elements(p, count, arrays)", settle_sample,
                            capacity, stream, [&](const BatchCall& c, const ltp_settle_opts& o) {
        ltp::launch_settle(c.s, c.r, o.arrays, o.horizon, o.first_sample, o.uniform_first, o.lo, o.hi, o.box_query_stride, o.box_joint_stride,
                           settle_sample, o.settle_all);
    });
}

int ltp_replan_states_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                            const unsigned long long* offsets, const double* tile, unsigned long long capacity,
                            const int* sample_index, int uniform_index,
                            double* q_0, double* v_0, double* a_0, long long query_stride, long long joint_stride, void* stream)
{
    return replan_states_any(p, first, count, in, rec, offsets, tile, false, capacity, sample_index, uniform_index, q_0, v_0, a_0,
                             query_stride, joint_stride, stream);
}

int ltp_replan_states_f32_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                                const unsigned long long* offsets, const float* tile, unsigned long long capacity,
                                const int* sample_index, int uniform_index,
                                double* q_0, double* v_0, double* a_0, long long query_stride, long long joint_stride, void* stream)
{
    return replan_states_any(p, first, count, in, rec, offsets, tile, true, capacity, sample_index, uniform_index, q_0, v_0, a_0,
                             query_stride, joint_stride, stream);
}

int ltp_generate_queries_batch(ltp_planner* p, long long n, unsigned long long seed, long long first_query,
                               double* q_goal, double* q_0, double* v_0, double* a_0,
                               long long query_stride, long long joint_stride, void* stream)
{
    if (!p || n < 0 || !q_goal || !q_0 || !v_0 || !a_0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc != LTP_OK) return rc;
    if (p->dof > 64) return fail(p, LTP_ERR_INVALID_ARGUMENT, "generator supports dof <= 64");
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    ltp::launch_generate((hipStream_t)stream, n, p->dof, dev_limits(p), seed, first_query, q_goal, q_0, v_0, a_0, query_stride,
                         joint_stride);
    LTP_HIP_TRY(p, hipGetLastError());
    return LTP_OK;
}

int ltp_debug_set_sample_stamps(ltp_planner* p, unsigned long long* device_buffer)
{
    if (!p) return LTP_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> g(p->mu);
    p->dbg_stamps = device_buffer;
    return LTP_OK;
}

int ltp_debug_get_sample_blocks(ltp_planner* p, int which)
{
    if (!p || which < 0 || which > 4) return -1;
    std::lock_guard<std::mutex> g(p->mu);
    if (reserve(p, 0) != LTP_OK) return -1;
    const int blocks[5] = {p->fused_blocks[0], p->fused_blocks[1], p->envelope_blocks, p->tab_blocks[0], p->tab_blocks[1]};   // include/ltp_hip.h
    return blocks[which];
}

int ltp_debug_set_sample_blocks(ltp_planner* p, int blocks)
{
    if (!p || blocks < 0) return LTP_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> g(p->mu);
    p->sample_blocks_override = blocks;
    return LTP_OK;
}

}  // extern "C"
