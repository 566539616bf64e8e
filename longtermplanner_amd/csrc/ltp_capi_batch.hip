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

// the table pass over plans [first, first + count): per piece of the range that fits the table workspace,
// launch(f, c, head) runs k_build_tables and the kernel that reads the tables, named `kernel`
template <class Launch>
static int table_pass_pieces(ltp_planner* p, hipStream_t s, long long first, long long count, const char* kernel, Launch&& launch)
{
    bool capturing = false;
    int rc;
    if ((rc = workspace_acquire(p, s, capturing)) != LTP_OK) return rc;
    long long piece = 0;
    if ((rc = ensure_tables(p, count, capturing, &piece)) != LTP_OK) return rc;
    for (long long f = first; f < first + count; f += piece) {
        const long long c = first + count - f < piece ? first + count - f : piece;
        unsigned long long* head = nullptr;
        if ((rc = next_queue_head(p, s, &head)) != LTP_OK) return rc;
        launch(f, c, head);
    }
    LTP_HIP_TRY(p, hipGetLastError());
    p->last_kernel = kernel;
    return workspace_release(p, s, capturing);
}

extern "C" {

int ltp_plan_switch_times_batch(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* out,
                                unsigned long long* offsets, void* stream)
{
    if (!p || n < 0 || !in || !records_complete(out)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_sets(p);   // a binding: sets for this dof, C++ semantics
    if (rc != LTP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    if (n == 0 || p->dof == 0) {
        capture_geometry(p);
        // dof == 0: every query fails with slowest_joint == -1 (cc:39); nothing to launch per joint
        if (offsets) LTP_HIP_TRY(p, hipMemsetAsync(offsets, 0, sizeof(unsigned long long) * (size_t)(n + 1), s));
        if (n > 0) {
            std::vector<int> st((size_t)n, LTP_STATUS_NO_SLOWEST), neg((size_t)n, -1);
            std::vector<double> tr((size_t)n, -1.0);
            LTP_HIP_TRY(p, hipMemcpyAsync(out->status, st.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
            LTP_HIP_TRY(p, hipMemcpyAsync(out->slowest, neg.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
            LTP_HIP_TRY(p, hipMemcpyAsync(out->t_required, tr.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
            LTP_HIP_TRY(p, hipMemsetAsync(out->traj_len, 0, sizeof(int) * (size_t)n, s));
            LTP_HIP_TRY(p, hipStreamSynchronize(s));
        }
        return LTP_OK;
    }
    rc = reserve(p, n);
    if (rc != LTP_OK) return rc;
    bool capturing = false;
    if ((rc = workspace_acquire(p, s, capturing)) != LTP_OK) return rc;
    capture_geometry(p);
    const ltp::PlanLimits L = dev_limits(p);
    const ltp::Queries q = to_dev(in);
    const ltp::Records r = to_dev(out);
    LTP_HIP_TRY(p, hipMemsetAsync(p->d_queue_count, 0, 16 * sizeof(unsigned long long), s));
    ltp::launch_switch_times(s, n, p->dof, p->t_sample, p->goal_check, L, q, r, p->d_lane_flags, p->d_queue, p->d_queue_count, stage_variant(p));
    ltp::launch_offsets(s, n, p->dof, p->t_sample, r, p->d_block_sums, offsets ? offsets : p->d_offsets_scratch, true, ltp::RowSpec{p->max_samples, p->sample_stride});
    LTP_HIP_TRY(p, hipGetLastError());
    return workspace_release(p, s, capturing);
}

int ltp_retime_batch(ltp_planner* p, long long n, const ltp_queries* in, const ltp_records* rec, const ltp_retime_opts* opts,
                     unsigned long long* offsets, void* stream)
{
    if (!p || n < 0 || !in || !records_complete(rec)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    if (!opts) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_opts is NULL");
    // size-versioned, strictly: the first version is the struct as it is now; a later version only appends fields whose zero
    // value means "not used", so a newer caller's bytes beyond ours must be zero
    if (opts->size < sizeof(ltp_retime_opts)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_opts.size is below the first version of the struct");
    if (opts->size % 8u != 0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_opts.size is not a multiple of 8");
    const unsigned char* tail = (const unsigned char*)opts;
    for (size_t b = sizeof(ltp_retime_opts); b < opts->size; ++b)
        if (tail[b] != 0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_opts has non-zero bytes beyond the fields this library knows");
    ltp_retime_opts o;
    memcpy(&o, opts, sizeof o);
    if (!std::isfinite(o.t_uniform)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_opts.t_uniform is not finite");
    if (o.t_uniform < 0.0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_opts.t_uniform is negative");
    if (o.group && o.n_groups < 1) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_opts.group needs n_groups >= 1");
    if (o.group && !o.group_time) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_opts.group needs group_time");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_geometry(p);
    if (rc != LTP_OK) return rc;
    if (p->semantics == LTP_SEMANTICS_MATLAB)
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_retime_batch follows the C++ reference's timeScaling: not available with LTP_SEMANTICS_MATLAB");
    const hipStream_t s = (hipStream_t)stream;
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    if (o.group) LTP_HIP_TRY(p, hipMemsetAsync(o.group_time, 0, sizeof(double) * (size_t)o.n_groups, s));
    if (n == 0 || p->dof == 0) return LTP_OK;   // dof == 0: no query was planned (cc:39), there is nothing to retime
    if ((rc = reserve(p, n)) != LTP_OK) return rc;
    bool capturing = false;
    if ((rc = workspace_acquire(p, s, capturing)) != LTP_OK) return rc;
    LTP_HIP_TRY(p, hipMemsetAsync(p->d_queue_count, 0, 16 * sizeof(unsigned long long), s));
    const ltp::RetimeRequest req{o.t_target, o.t_uniform, o.group, o.n_groups, o.group_time};
    ltp::launch_retime(s, n, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), req, p->d_queue, p->d_queue_count, p->d_block_sums,
                       offsets ? offsets : p->d_offsets_scratch, ltp::RowSpec{p->max_samples, p->sample_stride}, stage_variant(p));
    LTP_HIP_TRY(p, hipGetLastError());
    return workspace_release(p, s, capturing);
}

int ltp_end_limit_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec, void* stream)
{
    if (!p || first < 0 || count < 0 || !in || !records_complete(rec)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_geometry(p);
    if (rc != LTP_OK) return rc;
    if (p->semantics == LTP_SEMANTICS_MATLAB) return LTP_OK;   // LTPlanner.m has no position limits: there is no end-limit verdict
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    ltp::launch_end_limit((hipStream_t)stream, first, count, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec));
    LTP_HIP_TRY(p, hipGetLastError());
    return LTP_OK;
}

static int sample_batch_any(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                            const unsigned long long* offsets, void* out, bool f32, unsigned long long capacity,
                            const ltp::SamplePolicy& pol, void* stream)
{
    if (!p || first < 0 || count < 0 || !in || !records_complete(rec) || !offsets || (!out && capacity > 0))
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    if (((uintptr_t)out & 15u) != 0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "trajectory buffer must be 16-byte aligned");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_geometry(p);
    if (rc != LTP_OK) return rc;
    if (count == 0 || p->dof == 0) return LTP_OK;
    if ((rc = reserve(p, 0)) != LTP_OK) return rc;   // work-queue heads, resident block counts (no-op after the first call)
    const hipStream_t s = (hipStream_t)stream;
    const ltp::RowSpec rows{p->max_samples, p->sample_stride};
    const ltp::SampleChoice c = ltp::choose_sampler(pol, p->semantics, p->table_pass, p->dbg_stamps != nullptr, f32, rows, p->dof);
    if (c.path == ltp::SamplePath::Table)
        return table_pass_pieces(p, s, first, count, c.kernel, [&](long long f, long long n, unsigned long long* head) {
            ltp::launch_build_tables(s, f, n, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), rows, false, offsets, first, p->d_tables, p->semantics);
            ltp::launch_sample_tab(s, f, n, first, p->dof, to_dev(rec), offsets, out, f32, capacity, pol.nontemporal, pol.interleave, rows, head,
                                   blocks_or_override(p, p->tab_blocks[f32]), p->d_tables, p->t_sample, p->dbg_stamps);
        });
    unsigned long long* head = nullptr;
    if ((rc = next_queue_head(p, s, &head)) != LTP_OK) return rc;
    if (c.path == ltp::SamplePath::Fused) {
        ltp::launch_sample(s, first, count, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), offsets, out, f32, capacity,
                           pol.nontemporal, pol.dry, pol.interleave, rows, head, blocks_or_override(p, p->fused_blocks[f32]), p->dbg_stamps);
    } else {
        ltp::launch_sample_walk(s, first, count, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), offsets, out, capacity, c.walk_kernel,
                                pol.interleave, rows, head, blocks_or_override(p, p->walk_blocks[f32]), p->walk_auto_cus);
    }
    LTP_HIP_TRY(p, hipGetLastError());
    p->last_kernel = c.kernel;
    return LTP_OK;
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
    if (!p || first < 0 || count < 0 || !in || !records_complete(rec) || !env) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    if (window < 1 || n_windows < 1) return fail(p, LTP_ERR_INVALID_ARGUMENT, "window and n_windows must be >= 1");
    if (((uintptr_t)env & 15u) != 0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "envelope buffer must be 16-byte aligned");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_geometry(p);
    if (rc != LTP_OK) return rc;
    if (count == 0 || p->dof == 0) return LTP_OK;
    if ((rc = reserve(p, 0)) != LTP_OK) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const int blocks = blocks_or_override(p, p->envelope_blocks);
    const ltp::EnvelopeChoice c = ltp::choose_envelope(p->envelope_mode, p->semantics, p->table_pass, p->dbg_stamps != nullptr);
    if (c.path == ltp::EnvelopePath::Table)
        return table_pass_pieces(p, s, first, count, c.kernel, [&](long long f, long long n, unsigned long long* head) {
            ltp::launch_build_tables(s, f, n, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), ltp::RowSpec{0, 1}, true, nullptr, f, p->d_tables, p->semantics);
            ltp::launch_envelope(s, f, n, first, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), window, n_windows, env, head,
                                 blocks, nullptr, p->d_tables, c.analytic);
        });
    if (c.path == ltp::EnvelopePath::Walk) {
        ltp::launch_envelope_walk(s, first, count, first, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), window, n_windows, env, p->semantics);
    } else {
        unsigned long long* head = nullptr;
        if ((rc = next_queue_head(p, s, &head)) != LTP_OK) return rc;
        ltp::launch_envelope(s, first, count, first, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), window,
                             n_windows, env, head, blocks, p->dbg_stamps, nullptr, c.analytic);
    }
    LTP_HIP_TRY(p, hipGetLastError());
    p->last_kernel = c.kernel;
    return LTP_OK;
}

unsigned long long ltp_run_tables_bytes(const ltp_planner* p, long long n_plans)
{
    if (!p || n_plans <= 0 || p->dof <= 0) return 0ull;
    return ltp::table_bytes(n_plans * (long long)p->dof);
}

int ltp_build_tables_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                           unsigned long long* tables, unsigned long long bytes, void* stream)
{
    if (!p || first < 0 || count < 0 || !in || !records_complete(rec) || (!tables && count > 0)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    if (((uintptr_t)tables & 15u) != 0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "run-table buffer must be 16-byte aligned");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_geometry(p);
    if (rc != LTP_OK) return rc;
    if (count == 0 || p->dof == 0) return LTP_OK;
    if (bytes < ltp::table_bytes(count * (long long)p->dof))
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "run-table buffer smaller than ltp_run_tables_bytes(p, count)");
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    // whole tables (every run of every joint), lane = (plan - first) * dof + joint; the caller's buffer, not the handle's workspace
    ltp::launch_build_tables((hipStream_t)stream, first, count, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), ltp::RowSpec{0, 1}, true,
                             nullptr, first, tables, p->semantics);
    LTP_HIP_TRY(p, hipGetLastError());
    return LTP_OK;
}

static int replan_states_any(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                             const unsigned long long* offsets, const void* tile, bool f32, unsigned long long capacity,
                             const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                             long long query_stride, long long joint_stride, void* stream)
{
    if (!p || first < 0 || count < 0 || !in || !records_complete(rec) || !offsets || (!tile && capacity > 0) || !q_0 || !v_0 || !a_0)
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_geometry(p);
    if (rc != LTP_OK) return rc;
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    ltp::launch_replan_states((hipStream_t)stream, first, count, p->dof, ltp::RowSpec{p->max_samples, p->sample_stride}, to_dev(in), to_dev(rec), offsets, tile, f32,
                              capacity, sample_index, uniform_index, q_0, v_0, a_0, query_stride, joint_stride, p->t_sample, dev_limits(p), p->semantics);
    LTP_HIP_TRY(p, hipGetLastError());
    return LTP_OK;
}

int ltp_state_at_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                       const int* sample_index, int uniform_index, double* q_0, double* v_0, double* a_0,
                       long long query_stride, long long joint_stride, void* stream)
{
    if (!p || first < 0 || count < 0 || !in || !records_complete(rec) || !q_0 || !v_0 || !a_0)
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_geometry(p);
    if (rc != LTP_OK) return rc;
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    ltp::launch_state_at((hipStream_t)stream, first, count, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), sample_index,
                         uniform_index, q_0, v_0, a_0, query_stride, joint_stride, p->semantics);
    LTP_HIP_TRY(p, hipGetLastError());
    return LTP_OK;
}

unsigned long long ltp_window_elements(const ltp_planner* p, long long count, int n_samples)
{
    if (!p || count <= 0 || n_samples < 1 || p->dof <= 0) return 0ull;
    return (unsigned long long)count * 4ull * (unsigned long long)p->dof * (unsigned long long)ltp_row_stride(n_samples);
}

int ltp_sample_window_batch(ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec,
                            const ltp_window_opts* opts, void* out, unsigned long long capacity, void* stream)
{
    if (!p || first < 0 || count < 0 || !in || !records_complete(rec)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    if (!opts) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_window_opts is NULL");
    // size-versioned, strictly (the rule of ltp_retime_opts): a later version only appends fields whose zero value means "not used"
    if (opts->size < sizeof(ltp_window_opts)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_window_opts.size is below the first version of the struct");
    if (opts->size % 8u != 0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_window_opts.size is not a multiple of 8");
    const unsigned char* tail = (const unsigned char*)opts;
    for (size_t b = sizeof(ltp_window_opts); b < opts->size; ++b)
        if (tail[b] != 0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_window_opts has non-zero bytes beyond the fields this library knows");
    ltp_window_opts o;
    memcpy(&o, opts, sizeof o);
    if (o.format != LTP_ROWS_F64 && o.format != LTP_ROWS_F32) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_window_opts.format is neither LTP_ROWS_F64 nor LTP_ROWS_F32");
    if (o.n_samples < 1) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_window_opts.n_samples must be >= 1");
    if (o.n_samples > (1 << 30)) return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_window_opts.n_samples is beyond 2^30");   // the kernel's sample indices are ints
    if (!out) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null window buffer");
    if (((uintptr_t)out & 15u) != 0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "window buffer must be 16-byte aligned");
    std::lock_guard<std::mutex> g(p->mu);
    int rc = check_config(p);
    if (rc == LTP_OK) rc = check_geometry(p);
    if (rc != LTP_OK) return rc;
    if (capacity < ltp_window_elements(p, count, o.n_samples))
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "window buffer smaller than ltp_window_elements(p, count, n_samples)");
    if (count == 0 || p->dof == 0) return LTP_OK;
    if ((count * (long long)p->dof + 63) / 64 > 0x7fffffffll) return fail(p, LTP_ERR_INVALID_ARGUMENT, "count * dof is beyond one launch");
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    ltp::launch_sample_window((hipStream_t)stream, first, count, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), o.n_samples,
                              ltp_row_stride(o.n_samples), o.first_sample, o.uniform_first, o.valid, out, o.format == LTP_ROWS_F32, p->semantics);
    LTP_HIP_TRY(p, hipGetLastError());
    return LTP_OK;
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
