// ltp_handle.hpp — the planner handle behind include/ltp_hip.h and the helpers the C-ABI translation units share
// (ltp_capi_handle.hip: lifetime / configuration / workspace; ltp_capi_batch.hip: device-pointer batch calls;
// ltp_capi_host.hip: host-pointer convenience calls; ltp_capi_multi.hip: one process, several shards). Host-side only; every
// computation is a kernel in the ltp_*.hip kernel files. There is deliberately no CPU implementation behind the entry points:
// without a HIP device they fail with LTP_ERR_NO_DEVICE.
//
// Locks: host_mu (the synchronous host-pointer calls and their arena) is taken BEFORE mu (configuration and the device
// workspace), everywhere.
#pragma once
#include "../../include/ltp_hip.h"
#include "ltp_kernels.hpp"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

struct ltp_planner {
    int dof = 0;
    double t_sample = 0.001;
    int device = 0;
    int max_samples = 0;                   // 0 = store whole trajectories (reference behaviour)
    int sample_stride = 1;                 // store every sample_stride-th sample
    int goal_check = 0;                    // 1 = reject q_goal outside [q_min,q_max] up front (reference: unchecked)
    // resident blocks of the work-queue kernels (their grids), [f32] where the row type matters; per device, filled by reserve()
    int fused_blocks[2] = {0, 0};          // k_sample
    int tab_blocks[2] = {0, 0};            // k_sample_tab_*
    int walk_blocks[2] = {0, 0};           // k_sample_walk_* (builder / streaming waves)
    int envelope_blocks = 0;               // k_envelope
    int walk_auto_cus = 0;                 // compute units of `device`, set with the autonomous-wave kernels' LDS limit
    int sample_blocks_override = 0;        // tuning aid (ltp_debug_set_sample_blocks)
    unsigned long long* d_sample_next = nullptr;   // ring of work-queue heads, one per in-flight sampler launch
    unsigned sample_next_slot = 0;
    std::vector<double> h_lim[5];          // q_min, q_max, v_max, a_max, j_max as given (any length)
    double* d_lim = nullptr;               // 5 * lim_cap doubles
    int lim_cap = 0;
    // limit sets (ltp_set_limit_sets): [5][n_sets * sets_dof] limit values, then the rows' LimPow under LTP_POW_EXACT and under
    // LTP_POW_LIBM ([n_sets * sets_dof][kLimPowN] each); reused in place while they fit sets_cap rows
    int n_sets = 0;
    int sets_dof = 0;                      // the handle's dof when the sets were given
    double* d_sets = nullptr;
    long long sets_cap = 0;                // rows (set, joint) d_sets holds
    unsigned long long sets_gen = 0;       // incremented by every ltp_set_limit_sets
    const int* bound_sets = nullptr;       // ltp_bind_limit_sets: device int[n] of the device-pointer batch calls, or null
    unsigned long long* d_queue = nullptr; // two compaction queues of (query*dof + joint), 8 shards each
    unsigned long long* d_queue_count = nullptr;   // [16]
    signed char* d_lane_flags = nullptr;   // per (query, joint) status bits of stage 1
    unsigned long long* d_block_sums = nullptr;
    unsigned long long* d_offsets_scratch = nullptr;
    long long ws_items = 0;                // capacity of d_lane_flags in (query, joint) items
    long long ws_queue_entries = 0;        // capacity of d_queue in u64 entries
    long long ws_queries = 0;
    int table_pass = 0;                    // 0 = automatic, 1 = always, -1 = never (ltp_set_table_pass)
    unsigned long long* d_tables = nullptr;   // run tables of the table pass (k_build_tables); part of the workspace
    unsigned long long tables_bytes = 0;      // allocated
    unsigned long long tables_cap = 4ull << 30;   // upper bound for d_tables (ltp_create: 1/16 of the device's memory if that
                                                  // is more — 18 GiB of 288); longer ranges are processed in pieces
    double* d_small = nullptr;             // 16 doubles for the one-lane entry points
    bool small_dirty = false;              // a fused small-batch call failed: k_plan_small's arrival word may be non-zero
    const char* last_kernel = "";          // row / envelope kernel of the latest ltp_sample_batch* / ltp_envelope_batch
    int semantics = 0;                     // LTP_SEMANTICS_CPP (the reference's C++, default) or LTP_SEMANTICS_MATLAB
    int envelope_mode = LTP_ENVELOPE_ANALYTIC;   // the default since round 6 (8.8e9 window values identical to the exhaustive form, profiles/r06_envelope_mode_soak.json); LTP_ENVELOPE_EXHAUSTIVE: bit-identical to the reduced rows by construction
    int pow_rule = LTP_POW_LIBM;           // LTP_POW_LIBM (default) or LTP_POW_EXACT: how pow(x, 3 | 4 | 6 | 1/2) is formed (ltp_math.hpp)
    int last_matlab_flags = 0;             // MATLAB semantics: flags of the latest one-lane call (1 = complex intermediate, 2 = error)
    unsigned long long* dbg_stamps = nullptr; // diagnostic: per-block start/end stamps of k_sample (caller-owned)
    // persistent buffers of the small synchronous host-pointer calls (no hipMalloc per call)
    std::mutex host_mu;
    unsigned char* d_arena = nullptr;
    unsigned char* h_arena = nullptr;      // pinned mirror of d_arena
    size_t arena_bytes = 0;
    double* d_traj = nullptr;
    double* h_traj = nullptr;              // pinned
    size_t traj_doubles = 0;
    // the workspace above has one user at a time: the stream of the latest ltp_plan_switch_times_batch and an event
    // recorded behind its work; a call on another stream waits for that event first (include/ltp_hip.h, "Streams")
    hipStream_t ws_stream = nullptr;
    hipEvent_t ws_event = nullptr;
    bool ws_used = false;
    // geometry of the batches planned by this handle (include/ltp_hip.h, "Batch geometry")
    struct Geometry {
        bool valid = false; int dof = 0; double t_sample = 0.0; int max_samples = 0; int stride = 1; int semantics = 0;
        const int* sets = nullptr; int n_sets = 0; unsigned long long sets_gen = 0;   // the binding and the sets it was planned with
        bool stop = false;   // planned by ltp_plan_stop_batch: no goal was given, so ltp_retime_batch refuses it
    } planned;
    std::mutex mu;
    std::string err;
};

namespace ltp_capi {

int fail(ltp_planner* p, int code, const std::string& msg);
int hip_fail(ltp_planner* p, hipError_t e, const char* what);
#define LTP_HIP_TRY(p, expr)                                              \
    do {                                                                  \
        hipError_t e_ = (expr);                                           \
        if (e_ != hipSuccess) return ltp_capi::hip_fail((p), e_, #expr);  \
    } while (0)

int upload_limits(ltp_planner* p);
// The binding a call honours: the handle's (ltp_bind_limit_sets) for the device-pointer batch calls; a *_host call replaces it for
// its own thread while it runs (NULL, or ltp_plan_batch_sets_host's device copy of the index), see SetsScope
const int* effective_sets(const ltp_planner* p);
// the limits of the kernels: the handle's own set, plus the set table and the effective binding (ltp::PlanLimits)
ltp::PlanLimits dev_limits(const ltp_planner* p);
// the template variant of the stage kernels: semantics (bit 0) | pow rule (bit 1) | bound sets (bit 2), see ltp::dispatch_stage_variant
inline int stage_variant(const ltp_planner* p)
{
    return p->semantics | (p->pow_rule == LTP_POW_LIBM ? 2 : 0) | (effective_sets(p) ? ltp::kStageSets : 0);
}
// a *_host call: for its duration, on this thread, the batch calls honour `sets` instead of the handle's binding; the handle's
// planned geometry is restored afterwards, so that a device-pointer batch planned before stays consumable
struct SetsScope {
    ltp_planner* p;
    ltp_planner::Geometry saved;
    SetsScope(ltp_planner* p, const int* sets);
    ~SetsScope();
    void bind(const int* sets);   // the index, once it is on the device (ltp_plan_batch_sets_host)
};
// planning with a binding: the sets must be for the handle's dof, and C++ semantics
int check_sets(ltp_planner* p);
int check_config(ltp_planner* p);                        // the reference indexes its limit vectors unchecked (UB when short); here it is an error
int reserve(ltp_planner* p, long long n);
ltp::Queries to_dev(const ltp_queries* in);
ltp::Records to_dev(const ltp_records* r);
bool records_complete(const ltp_records* r);
// plans [first, first + count) of the caller's batch as the reader launchers take them (with p->mu held: the limits are the handle's)
inline ltp::PlanRange plan_range(const ltp_planner* p, long long first, long long count, const ltp_queries* in, const ltp_records* rec)
{
    return ltp::PlanRange{first, count, p->dof, p->t_sample, dev_limits(p), to_dev(in), to_dev(rec), p->semantics};
}
int workspace_acquire(ltp_planner* p, hipStream_t s, bool& capturing);
int workspace_release(ltp_planner* p, hipStream_t s, bool capturing);
void capture_geometry(ltp_planner* p);
int check_geometry(ltp_planner* p);
int ensure_tables(ltp_planner* p, long long count, bool capturing, long long* plans_per_piece);

// The nine record arrays of ltp_records (include/ltp_hip.h), stated once: f(member, elements per query, index in this list) for
// each; the element type is the member's. Stops at the first non-zero result of f and returns it. Everything that allocates,
// copies, lays out, checks or offsets "all the records" goes through here.
constexpr int kRecordFields = 9;
template <class F> int for_each_record_field(int dof, F f)
{
    const size_t d = (size_t)dof;
    int rc = 0;
    (void)((rc = f(&ltp_records::t_opt, 7 * d, 0)) || (rc = f(&ltp_records::t_scaled, 7 * d, 1)) || (rc = f(&ltp_records::dir, d, 2)) ||
           (rc = f(&ltp_records::v_drive, d, 3)) || (rc = f(&ltp_records::mod, d, 4)) || (rc = f(&ltp_records::t_required, 1, 5)) ||
           (rc = f(&ltp_records::slowest, 1, 6)) || (rc = f(&ltp_records::traj_len, 1, 7)) || (rc = f(&ltp_records::status, 1, 8)));
    return rc;
}
template <class T> constexpr size_t elem_size(T* ltp_records::*) { return sizeof(T); }
// sets of fields, as bits of the index above: all of them, and the two the sampler writes (traj_len, status)
constexpr unsigned kAllRecords = (1u << kRecordFields) - 1, kSampledRecords = 1u << 7 | 1u << 8;

// device memory owned for the duration of a *_host call: the record arrays (alloc_all) and whatever else the call stages
struct DevRecords {
    ltp_records r{};
    std::vector<void*> owned;
    ~DevRecords() { for (void* q : owned) (void)hipFree(q); }
    template <class T> hipError_t alloc(T** out, size_t count)
    {
        void* ptr = nullptr;
        hipError_t e = hipMalloc(&ptr, sizeof(T) * (count ? count : 1));
        if (e == hipSuccess) { owned.push_back(ptr); *out = (T*)ptr; }
        return e;
    }
    // alloc + copy of `count` elements from the host (none copied when count is 0)
    template <class T> hipError_t up(T** out, const T* host, size_t count)
    {
        hipError_t e = alloc(out, count);
        if (e == hipSuccess && count) e = hipMemcpy(*out, host, sizeof(T) * count, hipMemcpyHostToDevice);
        return e;
    }
    template <class T> static hipError_t down(T* host, const T* dev, size_t count)
    {
        return hipMemcpy(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost);
    }
    hipError_t alloc_all(long long n, int dof)
    {
        return (hipError_t)for_each_record_field(dof, [&](auto m, size_t per, int) { return (int)alloc(&(r.*m), per * (size_t)n); });
    }
};

}  // namespace ltp_capi
