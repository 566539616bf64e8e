// ltp_capi_host.hip — C ABI (include/ltp_hip.h): host-pointer convenience calls (synchronous): whole batches, the reference's
// protected methods as one-lane calls, roots().
//
// A batch call (ltp_plan_batch_host, ltp_get_trajectory_host) takes one of three tiers, chosen by size alone:
//   fused   n * dof <= small_batch_pairs() (128) and C++ semantics: ONE launch of k_plan_small, which reads the queries from and
//           writes records, offsets and rows to pinned host memory; the host waits on a completion word. No copy, no second
//           launch: this is the single planTrajectory call (tens of microseconds). Falls through to the arena tier when the
//           rows exceed the pinned result buffer (kFusedRowsBytes) or no pinned memory is to be had.
//   arena   arena_layout(n, dof).end <= kSmallHostBytes (8 MiB; 7-DoF: n up to ~7 260): the handle's persistent device arena and
//           its pinned mirror — inputs first, everything the device writes behind them — so a call is one upload, the batch
//           kernels, one download, and no hipMalloc. Rows come back through the cached d_traj / pinned h_traj.
//   staged  everything larger, and every call that only exists here (limit sets, retiming, envelopes): per-call device
//           allocations and one copy per array (struct Staged). At these sizes the kernels and the row download dominate.
// All three produce the same bits (tests/test_gpu_edge.py).
#include "ltp_handle.hpp"
#include "ltp_intervals.hpp"

#include <optional>

using namespace ltp_capi;

// ---- pinned result buffers: what ltp_plan_batch_host / ltp_get_trajectory_host hand out as *packed for small batches.
// The fused small-batch kernel writes the rows straight into such a buffer (host memory the device can address), so the
// caller gets them without any copy; ltp_free_host returns the buffer here instead of to the heap. ----
namespace {

struct PinnedPool {
    struct Buf { void* ptr; size_t bytes; bool used; };
    std::mutex mu;
    std::vector<Buf> bufs;
    static constexpr size_t kKeep = 16;           // buffers kept for reuse

    void* acquire(size_t bytes)
    {
        std::lock_guard<std::mutex> g(mu);
        for (auto& b : bufs)
            if (!b.used && b.bytes >= bytes) { b.used = true; return b.ptr; }
        void* ptr = nullptr;
        // the pool is process-wide and its buffers are handed to kernels on any device (ltp_plan_batch_multi): portable, and
        // explicitly coherent — Portable alone makes the memory non-coherent, and the completion word the host spins on
        // (wait_done) as well as the rows themselves rely on coherence
        if (hipHostMalloc(&ptr, bytes, hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        bufs.push_back(Buf{ptr, bytes, true});
        return ptr;
    }
    // true if ptr is one of ours
    bool release(void* ptr)
    {
        std::lock_guard<std::mutex> g(mu);
        size_t idle = 0;
        for (auto& b : bufs) idle += !b.used;
        for (size_t i = 0; i < bufs.size(); ++i)
            if (bufs[i].ptr == ptr) {
                if (idle >= kKeep) { (void)hipHostFree(ptr); bufs.erase(bufs.begin() + (long)i); }
                else bufs[i].used = false;
                return true;
            }
        return false;
    }
};
PinnedPool g_pinned;

// waits for the kernel's completion word in pinned memory (a few microseconds sooner than a stream synchronisation)
int wait_done(ltp_planner* p, volatile int* done)
{
    for (long spins = 0; *done == 0; ++spins) {
        if (spins > 2000000) {                      // ~ a second without news: ask the runtime (reports a faulted kernel)
            LTP_HIP_TRY(p, hipStreamSynchronize(nullptr));
            if (*done == 0) return fail(p, LTP_ERR_HIP, "small-batch kernel finished without reporting");
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    std::atomic_thread_fence(std::memory_order_acquire);   // the result buffers are read after the flag
    return LTP_OK;
}

constexpr size_t kFusedRowsBytes = 8u << 20;      // rows of a fused call: up to 1 Mi doubles (7-DoF, 1 ms: 48 k)
constexpr size_t kSmallHostBytes = 8u << 20;      // batches whose arena fits in 8 MiB take the arena tier
constexpr size_t kPinnedTrajDoubles = (32u << 20) / sizeof(double);   // pinned staging only for small results

// The arena: the four inputs first, then one contiguous block of everything the device writes (the record arrays in the order of
// for_each_record_field, then offsets), each part 16-byte aligned: upload [0, rec_begin), download [rec_begin, end).
struct ArenaLayout {
    size_t in[4], rec[kRecordFields], offsets, end, rec_begin;
};

ArenaLayout arena_layout(long long n, int dof)
{
    ArenaLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
    for (int k = 0; k < 4; ++k) L.in[k] = take(sizeof(double) * (size_t)n * dof);
    L.rec_begin = o;
    for_each_record_field(dof, [&](auto m, size_t per, int k) { L.rec[k] = take(elem_size(m) * per * (size_t)n); return 0; });
    L.offsets = take(sizeof(unsigned long long) * ((size_t)n + 1));
    L.end = o;
    return L;
}

// the records inside the arena at `base` (device arena or pinned mirror)
ltp_records arena_records(unsigned char* base, const ArenaLayout& L)
{
    ltp_records r;
    for_each_record_field(0, [&](auto m, size_t, int k) { r.*m = (std::remove_reference_t<decltype(r.*m)>)(base + L.rec[k]); return 0; });
    return r;
}

// host copy of the arrays both `dst` and `src` have, among the fields in `mask`
void copy_records(long long n, int dof, const ltp_records& dst, const ltp_records& src, unsigned mask)
{
    for_each_record_field(dof, [&](auto m, size_t per, int k) {
        if ((mask >> k & 1u) && dst.*m && src.*m) memcpy(dst.*m, src.*m, elem_size(m) * per * (size_t)n);
        return 0;
    });
}

// device-to-host copy of the arrays `h` asks for
int download_records(ltp_planner* p, long long n, int dof, const ltp_records& d, const ltp_records* h)
{
    if (!h) return LTP_OK;
    return for_each_record_field(dof, [&](auto m, size_t per, int) -> int {
        if (h->*m) LTP_HIP_TRY(p, hipMemcpy(h->*m, d.*m, elem_size(m) * per * (size_t)n, hipMemcpyDeviceToHost));
        return LTP_OK;
    });
}

int ensure_arena(ltp_planner* p, size_t bytes)
{
    if (bytes <= p->arena_bytes) return LTP_OK;
    if (p->d_arena) LTP_HIP_TRY(p, hipFree(p->d_arena));
    if (p->h_arena) LTP_HIP_TRY(p, hipHostFree(p->h_arena));
    p->d_arena = nullptr; p->h_arena = nullptr; p->arena_bytes = 0;
    const size_t cap = bytes < 65536 ? 65536 : bytes;
    LTP_HIP_TRY(p, hipMalloc((void**)&p->d_arena, cap));
    LTP_HIP_TRY(p, hipHostMalloc((void**)&p->h_arena, cap, hipHostMallocDefault));
    p->arena_bytes = cap;
    return LTP_OK;
}

int ensure_traj(ltp_planner* p, size_t doubles)
{
    if (doubles <= p->traj_doubles) return LTP_OK;
    if (p->d_traj) LTP_HIP_TRY(p, hipFree(p->d_traj));
    if (p->h_traj) LTP_HIP_TRY(p, hipHostFree(p->h_traj));
    p->d_traj = nullptr; p->h_traj = nullptr; p->traj_doubles = 0;
    LTP_HIP_TRY(p, hipMalloc((void**)&p->d_traj, sizeof(double) * doubles));
    if (doubles <= kPinnedTrajDoubles) LTP_HIP_TRY(p, hipHostMalloc((void**)&p->h_traj, sizeof(double) * doubles, hipHostMallocDefault));
    p->traj_doubles = doubles;
    return LTP_OK;
}

// Sample all n plans into a device buffer and hand back a malloc'ed host copy of the `total` doubles. The arena tier
// (h_status: the arena's host copy of `status`, refreshed here because the sampler may set LTP_STATUS_END_LIMIT) uses the handle's
// cached d_traj, asynchronous calls and the pinned h_traj as landing zone; the staged tier (h_status NULL) a buffer of its own and
// synchronous copies.
int sample_to_host(ltp_planner* p, long long n, const ltp_queries& dq, const ltp_records& dr, unsigned long long* d_off,
                   unsigned long long total, int* h_status, double** packed)
{
    const size_t bytes = sizeof(double) * (size_t)(total ? total : 2);
    DevRecords own;
    double* d_out = nullptr;
    if (h_status) {
        const int rc = ensure_traj(p, bytes / sizeof(double));
        if (rc != LTP_OK) return rc;
        d_out = p->d_traj;
    } else LTP_HIP_TRY(p, own.alloc(&d_out, bytes / sizeof(double)));
    // row padding beyond a row's last 16-byte slot is never written by the sampler (the tail of that slot is
    // zero-filled): make the host copy deterministic
    LTP_HIP_TRY(p, h_status ? hipMemsetAsync(d_out, 0, bytes, nullptr) : hipMemset(d_out, 0, bytes));
    const int rc = ltp_sample_batch(p, 0, n, &dq, &dr, d_off, d_out, total, 0, nullptr);
    if (rc != LTP_OK) return rc;
    if (!h_status) LTP_HIP_TRY(p, hipStreamSynchronize(nullptr));
    double* h = (double*)malloc(sizeof(double) * (size_t)(total ? total : 1));
    if (!h) return fail(p, LTP_ERR_OUT_OF_MEMORY, "malloc");
    hipError_t e = hipSuccess;
    if (h_status) {
        double* landing = p->h_traj ? p->h_traj : h;   // pinned staging when the result is small
        if (total) e = hipMemcpyAsync(landing, d_out, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, nullptr);
        if (e == hipSuccess) e = hipMemcpyAsync(h_status, dr.status, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess && total && landing != h) memcpy(h, landing, sizeof(double) * (size_t)total);
    } else e = hipMemcpy(h, d_out, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(h); return hip_fail(p, e, "trajectory download"); }
    *packed = h;
    return LTP_OK;
}

// The fused tier of ltp_plan_batch_host / ltp_get_trajectory_host: one launch of one block that reads the queries from and writes
// records and rows to pinned host memory (k_plan_small), one wait. `given` (getTrajectory): t_scaled, dir, mod, v_drive are
// inputs, and only what the sampler writes is copied out. Caller holds host_mu. Returns LTP_OK with *handled = false when the
// rows do not fit the pinned result buffer (caller takes the arena tier).
int plan_batch_host_fused(ltp_planner* p, long long n, const double* const (&h_in)[4], const ltp_records* host_records,
                          const ltp_records* given, unsigned long long* offsets, double** packed, bool* handled)
{
    *handled = false;
    const int dof = p->dof;
    const size_t nd = (size_t)n * dof;
    const ArenaLayout L = arena_layout(n, dof);
    const size_t flag_at = (L.end + 63) & ~(size_t)63;
    const int blocks = ltp::small_batch_blocks(dof, packed != nullptr);
    const size_t ends_at = flag_at + 64;                         // [blocks][n] end-limit bits
    int rc = ensure_arena(p, ends_at + sizeof(int) * (size_t)blocks * (size_t)n);
    if (rc != LTP_OK) return rc;
    for (int k = 0; k < 4; ++k)
        if (h_in[k]) memcpy(p->h_arena + L.in[k], h_in[k], sizeof(double) * nd);
    const ltp_records hr = arena_records(p->h_arena, L);
    if (given) copy_records(n, dof, hr, *given, kAllRecords);
    double* rows = nullptr;
    if (packed) {
        rows = (double*)g_pinned.acquire(kFusedRowsBytes);
        if (!rows) return LTP_OK;                                // no pinned memory to be had: arena tier
    }
    if (p->small_dirty) {
        // an earlier fused call failed or was abandoned: whatever it left running must be over and k_plan_small's arrival
        // word zero again before the next launch counts on it
        LTP_HIP_TRY(p, hipStreamSynchronize(nullptr));
        LTP_HIP_TRY(p, hipMemset(p->d_small, 0, sizeof(unsigned int)));
        p->small_dirty = false;
    }
    volatile int* done = (volatile int*)(p->h_arena + flag_at);
    *done = 0;
    const double* in[4] = {(const double*)(p->h_arena + L.in[0]), (const double*)(p->h_arena + L.in[1]),
                           (const double*)(p->h_arena + L.in[2]), (const double*)(p->h_arena + L.in[3])};
    {
        std::lock_guard<std::mutex> g(p->mu);
        capture_geometry(p);
        ltp::launch_plan_small(nullptr, (int)n, dof, p->t_sample, p->goal_check, ltp::RowSpec{p->max_samples, p->sample_stride}, dev_limits(p), in,
                               to_dev(&hr), (unsigned long long*)(p->h_arena + L.offsets), rows, kFusedRowsBytes / sizeof(double),
                               (int*)(p->h_arena + ends_at), (unsigned int*)p->d_small, done, given != nullptr, p->pow_rule == LTP_POW_LIBM, true);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { if (rows) g_pinned.release(rows); return hip_fail(p, e, "k_plan_small"); }   // nothing was launched
    }
    rc = wait_done(p, done);
    if (rc != LTP_OK) {
        // the kernel may still be running (or have died half way): its arrival word is suspect, and `rows` goes back to the
        // pool only once the stream is known to be idle — otherwise it stays allocated (leaked) rather than be written behind a later owner's back
        p->small_dirty = true;
        if (rows && hipStreamSynchronize(nullptr) == hipSuccess) g_pinned.release(rows);
        (void)hipGetLastError();
        return rc;
    }
    if (*done == 2) {                                            // rows larger than the pinned buffer
        g_pinned.release(rows);
        return LTP_OK;
    }
    if (packed) {                                                // end-limit bits of the blocks that sampled (cc:59-61)
        const int* ends = (const int*)(p->h_arena + ends_at);
        for (int b = 0; b < blocks; ++b)
            for (long long i = 0; i < n; ++i) hr.status[i] |= ends[(size_t)b * n + i];
    }
    if (offsets) memcpy(offsets, p->h_arena + L.offsets, sizeof(unsigned long long) * ((size_t)n + 1));
    if (host_records) copy_records(n, dof, *host_records, hr, given ? kSampledRecords : kAllRecords);
    if (packed) *packed = rows;
    *handled = true;
    return LTP_OK;
}

// The arena tier. The inputs are in the pinned mirror (caller); upload its first `up_bytes`, run `work` on the arena's device
// views, then the shared tail: one download of everything the device wrote, rows if asked for, copy-out. Caller holds host_mu.
template <class Work>
int run_in_arena(ltp_planner* p, long long n, const ArenaLayout& L, size_t up_bytes, int q_goal_in, const ltp_records* host_records,
                 unsigned long long* offsets, double** packed, Work work)
{
    const int dof = p->dof;
    if (up_bytes) LTP_HIP_TRY(p, hipMemcpyAsync(p->d_arena, p->h_arena, up_bytes, hipMemcpyHostToDevice, nullptr));
    const ltp_queries dq{(double*)(p->d_arena + L.in[q_goal_in]), (double*)(p->d_arena + L.in[1]), (double*)(p->d_arena + L.in[2]),
                         (double*)(p->d_arena + L.in[3]), dof, 1};
    const ltp_records dr = arena_records(p->d_arena, L);
    unsigned long long* d_off = (unsigned long long*)(p->d_arena + L.offsets);
    int rc = work(dq, dr, d_off);
    if (rc != LTP_OK) return rc;
    LTP_HIP_TRY(p, hipMemcpyAsync(p->h_arena + L.rec_begin, p->d_arena + L.rec_begin, L.end - L.rec_begin, hipMemcpyDeviceToHost, nullptr));
    LTP_HIP_TRY(p, hipStreamSynchronize(nullptr));
    const ltp_records hr = arena_records(p->h_arena, L);
    const unsigned long long* h_off = (const unsigned long long*)(p->h_arena + L.offsets);
    if (packed && (rc = sample_to_host(p, n, dq, dr, d_off, h_off[n], hr.status, packed)) != LTP_OK) return rc;
    if (offsets) memcpy(offsets, h_off, sizeof(unsigned long long) * ((size_t)n + 1));
    if (host_records) copy_records(n, dof, *host_records, hr, kAllRecords);
    return LTP_OK;
}

// The staged tier: device copies of a call's arrays for its duration. begin() allocates the records and the offsets array and
// uploads the inputs; the entry then runs its batch calls on dq / dr.r / d_off and ends with finish().
struct Staged {
    ltp_planner* p;
    long long n;
    int dof;
    DevRecords dr;
    ltp_queries dq{};
    unsigned long long* d_off = nullptr;

    // h_in[first..3] are uploaded; q_goal aliases h_in[first] (getTrajectory has none: first = 1, the sampler does not read it)
    int begin(const double* const (&h_in)[4], int first = 0)
    {
        LTP_HIP_TRY(p, dr.alloc_all(n, dof));
        double* d_in[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = first; k < 4; ++k) LTP_HIP_TRY(p, dr.up(&d_in[k], h_in[k], (size_t)n * dof));
        LTP_HIP_TRY(p, dr.alloc(&d_off, (size_t)n + 1));
        dq = ltp_queries{d_in[first], d_in[1], d_in[2], d_in[3], dof, 1};
        return LTP_OK;
    }
    // synchronise; offsets, and rows through the sampler if asked for; the records last, because the sampler and the consumers
    // add LTP_STATUS_END_LIMIT to status
    int finish(const ltp_records* host_records, unsigned long long* offsets, double** packed)
    {
        LTP_HIP_TRY(p, hipStreamSynchronize(nullptr));
        if (offsets) LTP_HIP_TRY(p, hipMemcpy(offsets, d_off, sizeof(unsigned long long) * ((size_t)n + 1), hipMemcpyDeviceToHost));
        if (packed) {
            const int rc = sample_to_host(p, n, dq, dr.r, d_off, offsets[n], nullptr, packed);
            if (rc != LTP_OK) return rc;
        }
        return download_records(p, n, dof, dr.r, host_records);
    }
    // planner(): the entry's planning call(s) on the staged batch; end-limit check if no rows are asked for (cc:59-61 without the
    // sampler); fetch(): what the entry downloads besides records, offsets and rows; finish
    template <class Planner, class Fetch>
    int plan_by(const ltp_records* host_records, unsigned long long* offsets, double** packed, Planner planner, Fetch fetch)
    {
        int rc = planner();
        if (rc == LTP_OK && !packed) rc = ltp_end_limit_batch(p, 0, n, &dq, &dr.r, nullptr);
        if (rc == LTP_OK) rc = fetch();
        if (rc != LTP_OK) return rc;
        return finish(host_records, offsets, packed);
    }
    // plan_by the switching times and `middle` (retiming, or nothing)
    template <class Middle>
    int plan(const ltp_records* host_records, unsigned long long* offsets, double** packed, Middle middle)
    {
        return plan_by(host_records, offsets, packed, [&] {
            const int rc = ltp_plan_switch_times_batch(p, n, &dq, &dr.r, d_off, nullptr);
            return rc == LTP_OK ? middle() : rc;
        }, [] { return LTP_OK; });
    }
    // The reader entries (windows, horizons, knot grids, horizon envelopes): begin, the starts up, `valid` and `doubles` of output
    // allocated — zeroed first if `zero`: the padding of rows is never written, and the result is to be deterministic; envelopes
    // are written whole —, plan, read(d_first, d_valid, d_out): the entry's own device call on the staged batch, the end-limit
    // verdict, output and valid down, finish.
    template <class Read>
    int plan_reader(const double* const (&h_in)[4], const int* first_sample, unsigned long long doubles, bool zero,
                    const ltp_records* host_records, double* out, int* valid, Read read)
    {
        int rc;
        if ((rc = begin(h_in)) != LTP_OK) return rc;
        int *d_first = nullptr, *d_valid = nullptr;
        if (first_sample) LTP_HIP_TRY(p, dr.up(&d_first, first_sample, (size_t)n));
        if (valid) LTP_HIP_TRY(p, dr.alloc(&d_valid, (size_t)n));
        double* d_out = nullptr;
        LTP_HIP_TRY(p, dr.alloc(&d_out, (size_t)doubles));
        if (zero && doubles) LTP_HIP_TRY(p, hipMemsetAsync(d_out, 0, sizeof(double) * (size_t)doubles, nullptr));
        rc = ltp_plan_switch_times_batch(p, n, &dq, &dr.r, nullptr, nullptr);
        if (rc == LTP_OK) rc = read(d_first, d_valid, d_out);
        if (rc == LTP_OK) rc = ltp_end_limit_batch(p, 0, n, &dq, &dr.r, nullptr);   // cc:59-61: the readers form no verdict
        if (rc != LTP_OK) return rc;
        if (doubles) LTP_HIP_TRY(p, DevRecords::down(out, d_out, (size_t)doubles));   // synchronises
        if (valid && n) LTP_HIP_TRY(p, DevRecords::down(valid, d_valid, (size_t)n));
        return finish(host_records, nullptr, nullptr);   // after the end-limit check: status carries END_LIMIT
    }
};

// a size-versioned options struct as a caller of this version hands it over: every byte zero, `size` set
template <class Opts>
Opts sized_opts()
{
    Opts opts;
    memset(&opts, 0, sizeof opts);
    opts.size = sizeof opts;
    return opts;
}

// What the opts structs of the three row readers share in a staged call: float64 rows, the staged starts and valid.
template <class Opts>
Opts staged_row_opts(const int* d_first, int uniform_first, int* d_valid)
{
    Opts opts = sized_opts<Opts>();
    opts.format = LTP_ROWS_F64;
    opts.first_sample = d_first;
    opts.uniform_first = uniform_first;
    opts.valid = d_valid;
    return opts;
}

// one-lane entry points: the kernel reads its 16 doubles from, and writes them back to, the pinned arena (host memory the
// device addresses directly): one launch, one synchronisation, no copy engine
template <class Launch>
int run_one_lane(ltp_planner* p, int joint, double (&buf)[16], Launch launch)
{
    std::lock_guard<std::mutex> hg(p->host_mu);        // host_mu before mu (see ltp_set_limits)
    double t_sample;
    int semantics;
    ltp::Limits lim;
    {
        std::lock_guard<std::mutex> g(p->mu);
        if (joint < 0 || joint >= p->lim_cap) return fail(p, LTP_ERR_INVALID_ARGUMENT, "joint out of range");
        t_sample = p->t_sample;
        semantics = stage_variant(p) & 3;              // semantics | pow rule << 1 (the one-lane mirrors never read a binding)
        lim = dev_limits(p);                           // stays valid: ltp_set_limits needs host_mu, which this call holds
    }
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    int rc = ensure_arena(p, sizeof(buf));
    if (rc != LTP_OK) return rc;
    memcpy(p->h_arena, buf, sizeof(buf));
    launch((double*)p->h_arena, t_sample, lim, semantics);
    LTP_HIP_TRY(p, hipGetLastError());
    LTP_HIP_TRY(p, hipStreamSynchronize(nullptr));
    memcpy(buf, p->h_arena, sizeof(buf));
    p->last_matlab_flags = (int)buf[11];
    return LTP_OK;
}

// The prologue of every batch *_host call, in the order that decides which error a bad call reports: `null_arg` (the entry's own
// required pointers; packed needs offsets), `refuse` (the entry's own argument rule, or NULL), the query arrays, then the
// configuration under mu (need_sets: limit sets must exist; reserve_n >= 0: the workspace), the device, and the call's one
// SetsScope: a _host call never reads the handle's binding, and the geometry of an earlier device batch is restored at its end.
int host_begin(ltp_planner* p, long long n, const double* const (&h_in)[4], bool null_arg, const char* refuse, double** packed,
               std::optional<SetsScope>& scope, bool need_sets = false, long long reserve_n = -1)
{
    if (!p || n < 0 || null_arg) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    if (refuse) return fail(p, LTP_ERR_INVALID_ARGUMENT, refuse);
    if (n > 0 && p->dof > 0 && (!h_in[0] || !h_in[1] || !h_in[2] || !h_in[3])) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null query array");
    if (packed) *packed = nullptr;
    int rc;
    {
        std::lock_guard<std::mutex> g(p->mu);
        rc = check_config(p);
        if (rc == LTP_OK && need_sets && p->n_sets < 1) rc = fail(p, LTP_ERR_INVALID_ARGUMENT, "the handle has no limit sets (ltp_set_limit_sets)");
        if (rc == LTP_OK && reserve_n >= 0) rc = reserve(p, reserve_n);
    }
    if (rc != LTP_OK) return rc;
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    scope.emplace(p, nullptr);
    return LTP_OK;
}

}  // namespace

// ltp_plan_first_exit_host and ltp_plan_settle_host: stages 1-3, then the reader of a horizon against boxes for host arrays. The two
// options structs are the same field for field up to the last pointer (`fold`: first_any / settle_all, which rides in the reader
// frame's `valid` and starts from `fold_fill` in every byte where nothing is launched); `read` is the device entry.
template <class Opts, class Read>
static int plan_box_horizon_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                                 const int* first_sample, int uniform_first, int horizon, int arrays, const double* const* lo,
                                 const double* const* hi, int box_per_plan, const ltp_records* host_records, int* table, int* fold_out,
                                 int* Opts::*fold, int fold_fill, Read read)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    const double* h_box[2][4];
    bool unselected_box = false;
    for (int x = 0; x < 4; ++x) {
        h_box[0][x] = lo ? lo[x] : nullptr;
        h_box[1][x] = hi ? hi[x] : nullptr;
        unselected_box = unselected_box || ((h_box[0][x] || h_box[1][x]) && !(arrays >> x & 1));
    }
    const char* bad = arrays < 1 || arrays > 15 ? "arrays is no non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J"
                      : horizon < 1 || horizon > (1 << 30) ? "horizon must be in 1 .. 2^30"
                      : box_per_plan != 0 && box_per_plan != 1 ? "box_per_plan must be 0 or 1"
                      : unselected_box ? "a box is given for an array that is not selected" : "";
    const int rc = host_begin(p, n, h_in, !table, *bad ? bad : nullptr, nullptr, scope);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    const unsigned long long elements = ltp_first_exit_elements(p, n, arrays);
    // (the reader frame's own output is not used: the table holds ints. The fold rides in its `valid`.)
    return st.plan_reader(h_in, first_sample, 0, false, host_records, nullptr, fold_out, [&](const int* d_first, int* d_fold, double*) -> int {
        Opts opts = sized_opts<Opts>();
        opts.arrays = arrays;
        opts.horizon = horizon;
        opts.uniform_first = uniform_first;
        opts.first_sample = d_first;
        opts.*fold = d_fold;
        opts.box_query_stride = box_per_plan ? p->dof : 0;
        opts.box_joint_stride = 1;
        const size_t box_doubles = (size_t)(box_per_plan ? n : 1) * (size_t)p->dof;
        for (int x = 0; x < 4; ++x) {
            double* d = nullptr;
            if (h_box[0][x]) { LTP_HIP_TRY(p, st.dr.up(&d, h_box[0][x], box_doubles)); opts.lo[x] = d; }
            if (h_box[1][x]) { LTP_HIP_TRY(p, st.dr.up(&d, h_box[1][x], box_doubles)); opts.hi[x] = d; }
        }
        int* d_table = nullptr;
        LTP_HIP_TRY(p, st.dr.alloc(&d_table, (size_t)elements));
        if (d_fold && n) LTP_HIP_TRY(p, hipMemsetAsync(d_fold, fold_fill, sizeof(int) * (size_t)n, nullptr));   // dof == 0: nothing is launched
        const int rc2 = read(p, 0, n, &st.dq, &st.dr.r, &opts, d_table, elements, nullptr);
        if (rc2 != LTP_OK) return rc2;
        if (elements) LTP_HIP_TRY(p, DevRecords::down(table, d_table, (size_t)elements));   // synchronises
        return LTP_OK;
    });
}

extern "C" {

int ltp_plan_batch_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                        const double* a_0, const ltp_records* host_records, unsigned long long* offsets, double** packed)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    int rc = host_begin(p, n, h_in, packed && !offsets, nullptr, packed, scope);
    if (rc != LTP_OK) return rc;
    const int dof = p->dof;
    const size_t nd = (size_t)n * dof;
    const ArenaLayout L = arena_layout(n, dof);
    if (n > 0 && dof > 0 && L.end <= kSmallHostBytes) {
        std::lock_guard<std::mutex> hg(p->host_mu);
        if (nd <= (size_t)ltp::small_batch_pairs() && p->semantics == LTP_SEMANTICS_CPP) {   // k_plan_small exists for the C++ semantics only
            bool handled = false;
            rc = plan_batch_host_fused(p, n, h_in, host_records, nullptr, offsets, packed, &handled);
            if (rc != LTP_OK || handled) return rc;
        }
        if ((rc = ensure_arena(p, L.end)) != LTP_OK) return rc;
        for (int k = 0; k < 4; ++k) memcpy(p->h_arena + L.in[k], h_in[k], sizeof(double) * nd);
        return run_in_arena(p, n, L, L.rec_begin, 0, host_records, offsets, packed,
                            [&](const ltp_queries& dq, const ltp_records& dr, unsigned long long* d_off) {
            int r = ltp_plan_switch_times_batch(p, n, &dq, &dr, d_off, nullptr);
            if (r == LTP_OK && !packed) r = ltp_end_limit_batch(p, 0, n, &dq, &dr, nullptr);   // cc:59-61 without the sampler
            return r;
        });
    }
    Staged st{p, n, dof};
    if ((rc = st.begin(h_in)) != LTP_OK) return rc;
    return st.plan(host_records, offsets, packed, [] { return LTP_OK; });
}

int ltp_plan_batch_sets_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                             const double* a_0, const int* set_index, const ltp_records* host_records, unsigned long long* offsets,
                             double** packed)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    int rc = host_begin(p, n, h_in, packed && !offsets, n > 0 && !set_index ? "null set_index" : nullptr, packed, scope, true);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    if ((rc = st.begin(h_in)) != LTP_OK) return rc;
    if (set_index) {
        int* d_sets = nullptr;
        LTP_HIP_TRY(p, st.dr.up(&d_sets, set_index, (size_t)n));
        scope->bind(d_sets);   // bound for this call only
    }
    return st.plan(host_records, offsets, packed, [] { return LTP_OK; });
}

int ltp_plan_retimed_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                          const double* a_0, const double* t_target, double t_uniform, const ltp_records* host_records,
                          unsigned long long* offsets, double** packed)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    int rc = host_begin(p, n, h_in, packed && !offsets, nullptr, packed, scope);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    if ((rc = st.begin(h_in)) != LTP_OK) return rc;
    ltp_retime_opts opts = sized_opts<ltp_retime_opts>();
    opts.t_uniform = t_uniform;
    if (t_target) {
        double* d_target = nullptr;
        LTP_HIP_TRY(p, st.dr.up(&d_target, t_target, (size_t)n));
        opts.t_target = d_target;
    }
    return st.plan(host_records, offsets, packed, [&] { return ltp_retime_batch(p, n, &st.dq, &st.dr.r, &opts, st.d_off, nullptr); });
}

int ltp_plan_stop_host(ltp_planner* p, long long n, const double* q_0, const double* v_0, const double* a_0, int check,
                       const ltp_records* host_records, double* q_stop, unsigned long long* offsets, double** packed)
{
    const double* const h_in[4] = {q_0, q_0, v_0, a_0};   // no goal: the staged queries carry q_0 in its place, which nothing reads
    std::optional<SetsScope> scope;
    int rc = host_begin(p, n, h_in, packed && !offsets,
                        check != LTP_STOP_CHECK_INPUTS && check != LTP_STOP_CHECK_BRAKING ? "check is neither LTP_STOP_CHECK_INPUTS nor LTP_STOP_CHECK_BRAKING" : nullptr,
                        packed, scope);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    if ((rc = st.begin(h_in, 1)) != LTP_OK) return rc;
    const size_t nd = (size_t)n * p->dof;
    ltp_stop_opts opts = sized_opts<ltp_stop_opts>();
    opts.check = check;
    if (q_stop) LTP_HIP_TRY(p, st.dr.alloc(&opts.q_stop, nd));
    return st.plan_by(host_records, offsets, packed, [&] { return ltp_plan_stop_batch(p, n, &st.dq, &st.dr.r, &opts, st.d_off, nullptr); }, [&]() -> int {
        if (q_stop && nd) LTP_HIP_TRY(p, DevRecords::down(q_stop, opts.q_stop, nd));   // synchronises
        return LTP_OK;
    });
}

int ltp_plan_envelope_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                           const double* a_0, int window, int n_windows, const ltp_records* host_records, double* env)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    int rc = host_begin(p, n, h_in, !env, window < 1 || n_windows < 1 ? "window and n_windows must be >= 1" : nullptr, nullptr, scope);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    if ((rc = st.begin(h_in)) != LTP_OK) return rc;
    double* d_env = nullptr;
    const size_t env_doubles = (size_t)n * p->dof * (size_t)n_windows * 2;
    LTP_HIP_TRY(p, st.dr.alloc(&d_env, env_doubles));
    rc = ltp_plan_switch_times_batch(p, n, &st.dq, &st.dr.r, nullptr, nullptr);
    if (rc == LTP_OK) rc = ltp_envelope_batch(p, 0, n, &st.dq, &st.dr.r, window, n_windows, d_env, nullptr);
    if (rc != LTP_OK) return rc;
    if (env_doubles) LTP_HIP_TRY(p, DevRecords::down(env, d_env, env_doubles));   // synchronises
    return st.finish(host_records, nullptr, nullptr);   // after the consumer: status carries END_LIMIT
}

int ltp_plan_window_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                         const double* a_0, const int* first_sample, int uniform_first, int n_samples,
                         const ltp_records* host_records, double* rows, int* valid)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    const int rc = host_begin(p, n, h_in, !rows, n_samples < 1 ? "n_samples must be >= 1" : nullptr, nullptr, scope);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    const unsigned long long elements = ltp_window_elements(p, n, n_samples);
    return st.plan_reader(h_in, first_sample, elements, true, host_records, rows, valid, [&](const int* d_first, int* d_valid, double* d_rows) {
        ltp_window_opts opts = staged_row_opts<ltp_window_opts>(d_first, uniform_first, d_valid);
        opts.n_samples = n_samples;
        return ltp_sample_window_batch(p, 0, n, &st.dq, &st.dr.r, &opts, d_rows, elements, nullptr);
    });
}

int ltp_plan_horizon_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                          const double* a_0, const int* first_sample, int uniform_first, int n_samples, int stride,
                          const ltp_records* host_records, double* rows, int* valid)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    const int rc = host_begin(p, n, h_in, !rows, n_samples < 1 ? "n_samples must be >= 1" : stride < 1 ? "stride must be >= 1" : nullptr, nullptr, scope);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    const unsigned long long elements = ltp_window_elements(p, n, n_samples);
    return st.plan_reader(h_in, first_sample, elements, true, host_records, rows, valid, [&](const int* d_first, int* d_valid, double* d_rows) {
        ltp_horizon_opts opts = staged_row_opts<ltp_horizon_opts>(d_first, uniform_first, d_valid);
        opts.n_samples = n_samples;
        opts.stride = stride;
        return ltp_sample_horizon_batch(p, 0, n, &st.dq, &st.dr.r, &opts, d_rows, elements, nullptr);
    });
}

int ltp_plan_knots_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                        const double* a_0, const int* first_sample, int uniform_first, int n_knots, const int* knot_offsets,
                        const ltp_records* host_records, double* rows, int* valid)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    // this entry sees the grid, so it checks it: nothing is launched for a grid outside the contract
    const char* bad_grid = knot_offsets ? ltp::knots_refusal(n_knots, knot_offsets) : "";
    const int rc = host_begin(p, n, h_in, !rows || !knot_offsets, *bad_grid ? bad_grid : nullptr, nullptr, scope);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    const unsigned long long elements = ltp_window_elements(p, n, n_knots);
    return st.plan_reader(h_in, first_sample, elements, true, host_records, rows, valid, [&](const int* d_first, int* d_valid, double* d_rows) {
        int* d_knots = nullptr;
        LTP_HIP_TRY(p, st.dr.up(&d_knots, knot_offsets, (size_t)n_knots));
        ltp_knots_opts opts = staged_row_opts<ltp_knots_opts>(d_first, uniform_first, d_valid);
        opts.n_knots = n_knots;
        opts.knot_offsets = d_knots;
        return ltp_sample_knots_batch(p, 0, n, &st.dq, &st.dr.r, &opts, d_rows, elements, nullptr);
    });
}

int ltp_plan_stop_knots_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                             const double* a_0, const int* first_sample, int uniform_first, int n_knots, const int* knot_offsets,
                             int accel, const ltp_records* host_records, double* out, int* valid)
{
    const double* const h_in[4] = {q_goal, q_0, v_0, a_0};
    std::optional<SetsScope> scope;
    // this entry sees the grid, so it checks it: nothing is launched for a grid outside the contract
    const char* bad = !knot_offsets ? ""
                      : accel != LTP_STOP_ACCEL_CLAMP && accel != LTP_STOP_ACCEL_STRICT ? "accel is neither LTP_STOP_ACCEL_CLAMP nor LTP_STOP_ACCEL_STRICT"
                                                                                        : ltp::knots_refusal(n_knots, knot_offsets);
    const int rc = host_begin(p, n, h_in, !out || !knot_offsets, *bad ? bad : nullptr, nullptr, scope);
    if (rc != LTP_OK) return rc;
    if (p->semantics == LTP_SEMANTICS_MATLAB)   // before anything is staged or planned
        return fail(p, LTP_ERR_INVALID_ARGUMENT, "ltp_plan_stop_knots_host follows the C++ reference's sampler: not available with LTP_SEMANTICS_MATLAB");
    Staged st{p, n, p->dof};
    const unsigned long long elements = ltp_stop_knots_elements(p, n, n_knots);
    return st.plan_reader(h_in, first_sample, elements, true, host_records, out, valid, [&](const int* d_first, int* d_valid, double* d_out) {
        int* d_knots = nullptr;
        LTP_HIP_TRY(p, st.dr.up(&d_knots, knot_offsets, (size_t)n_knots));
        ltp_stop_knots_opts opts = sized_opts<ltp_stop_knots_opts>();
        opts.n_knots = n_knots;
        opts.accel = accel;
        opts.uniform_first = uniform_first;
        opts.knot_offsets = d_knots;
        opts.first_sample = d_first;
        opts.valid = d_valid;
        return ltp_stop_knots_batch(p, 0, n, &st.dq, &st.dr.r, &opts, d_out, elements, nullptr);
    });
}

// ltp_plan_envelope_knots_host (arrays == NULL: the q-only batch entry and its options struct) and ltp_plan_envelope_knots_arrays_host
static int plan_envelope_knots_any(ltp_planner* p, long long n, const double* const (&h_in)[4], const int* first_sample, int uniform_first,
                                   int n_intervals, const int* edge_offsets, int closed, const int* arrays, const ltp_records* host_records,
                                   double* env, int* valid)
{
    std::optional<SetsScope> scope;
    // this entry sees the grid, so it checks it: nothing is launched for a grid outside the contract
    const char* bad = !edge_offsets ? ""
                      : closed != 0 && closed != 1 ? "closed must be 0 or 1"
                      : arrays && (*arrays < 1 || *arrays > 15) ? "arrays is no non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J"
                                                                : ltp::intervals_refusal(n_intervals, edge_offsets);
    const int rc = host_begin(p, n, h_in, !env || !edge_offsets, *bad ? bad : nullptr, nullptr, scope);
    if (rc != LTP_OK) return rc;
    Staged st{p, n, p->dof};
    const unsigned long long elements = ltp_envelope_knots_arrays_elements(p, n, n_intervals, arrays ? *arrays : LTP_ENV_Q);
    return st.plan_reader(h_in, first_sample, elements, false, host_records, env, valid, [&](const int* d_first, int* d_valid, double* d_env) {
        int* d_edges = nullptr;
        LTP_HIP_TRY(p, st.dr.up(&d_edges, edge_offsets, (size_t)n_intervals + 1));
        if (!arrays) {
            const ltp_envelope_knots_opts opts{sizeof(opts), n_intervals, closed, uniform_first, d_edges, d_first, d_valid};
            return ltp_envelope_knots_batch(p, 0, n, &st.dq, &st.dr.r, &opts, d_env, elements, nullptr);
        }
        const ltp_envelope_arrays_opts opts{sizeof(opts), n_intervals, closed, uniform_first, *arrays, 0, d_edges, d_first, d_valid};
        return ltp_envelope_knots_arrays_batch(p, 0, n, &st.dq, &st.dr.r, &opts, d_env, elements, nullptr);
    });
}

int ltp_plan_envelope_knots_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                                 const double* a_0, const int* first_sample, int uniform_first, int n_intervals,
                                 const int* edge_offsets, int closed, const ltp_records* host_records, double* env, int* valid)
{
    return plan_envelope_knots_any(p, n, {q_goal, q_0, v_0, a_0}, first_sample, uniform_first, n_intervals, edge_offsets, closed, nullptr,
                                   host_records, env, valid);
}

int ltp_plan_envelope_knots_arrays_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                                        const double* a_0, const int* first_sample, int uniform_first, int n_intervals,
                                        const int* edge_offsets, int closed, int arrays, const ltp_records* host_records, double* env, int* valid)
{
    return plan_envelope_knots_any(p, n, {q_goal, q_0, v_0, a_0}, first_sample, uniform_first, n_intervals, edge_offsets, closed, &arrays,
                                   host_records, env, valid);
}

int ltp_plan_first_exit_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                             const double* a_0, const int* first_sample, int uniform_first, int horizon, int arrays,
                             const double* const* lo, const double* const* hi, int box_per_plan, const ltp_records* host_records,
                             int* exit_sample, int* first_any)
{
    return plan_box_horizon_host(p, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, horizon, arrays, lo, hi, box_per_plan, host_records,
                                 exit_sample, first_any, &ltp_first_exit_opts::first_any, 0xFF, ltp_first_exit_batch);
}

int ltp_plan_settle_host(ltp_planner* p, long long n, const double* q_goal, const double* q_0, const double* v_0,
                         const double* a_0, const int* first_sample, int uniform_first, int horizon, int arrays,
                         const double* const* lo, const double* const* hi, int box_per_plan, const ltp_records* host_records,
                         int* settle_sample, int* settle_all)
{
    return plan_box_horizon_host(p, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, horizon, arrays, lo, hi, box_per_plan, host_records,
                                 settle_sample, settle_all, &ltp_settle_opts::settle_all, 0, ltp_settle_batch);
}

int ltp_get_trajectory_host(ltp_planner* p, long long n, const double* t, const double* dir, const signed char* mod,
                            const double* q_0, const double* v_0, const double* a_0, const double* v_drive,
                            int* traj_len, int* status, unsigned long long* offsets, double** packed)
{
    const double* const h_in[4] = {nullptr, q_0, v_0, a_0};
    const double* const h_checked[4] = {q_0, q_0, v_0, a_0};   // there is no q_goal, and this entry's own null check covers the rest
    std::optional<SetsScope> scope;
    int rc = host_begin(p, n, h_checked, !offsets || !packed || (n > 0 && (!t || !dir || !mod || !q_0 || !v_0 || !a_0 || !v_drive)), nullptr,
                        packed, scope, false, n > 0 ? n : 1);
    if (rc != LTP_OK) return rc;
    // the switching times are given: of the records, t_scaled, dir, v_drive and mod are inputs, and the sampler writes the last two
    const ltp_records given{nullptr, const_cast<double*>(t), const_cast<double*>(dir), const_cast<double*>(v_drive),
                            const_cast<signed char*>(mod), nullptr, nullptr, nullptr, nullptr};
    const ltp_records outr{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, traj_len, status};
    const int dof = p->dof;
    const size_t nd = (size_t)n * dof;
    const ArenaLayout L = arena_layout(n, dof);
    // the device records hold the given arrays; traj_len and offsets for them (status starts from zero), then the sampler
    auto offsets_for = [&](const ltp_records& dr, unsigned long long* d_off) -> int {
        std::lock_guard<std::mutex> g(p->mu);
        capture_geometry(p);
        ltp::launch_offsets(nullptr, n, dof, p->t_sample, to_dev(&dr), p->d_block_sums, d_off, false, ltp::RowSpec{p->max_samples, p->sample_stride});
        LTP_HIP_TRY(p, hipGetLastError());
        return LTP_OK;
    };
    if (n > 0 && dof > 0 && L.end <= kSmallHostBytes) {
        std::lock_guard<std::mutex> hg(p->host_mu);
        if (nd <= (size_t)ltp::small_batch_pairs() && p->semantics == LTP_SEMANTICS_CPP) {
            bool handled = false;
            rc = plan_batch_host_fused(p, n, h_in, &outr, &given, offsets, packed, &handled);
            if (rc != LTP_OK || handled) return rc;
        }
        if ((rc = ensure_arena(p, L.end)) != LTP_OK) return rc;
        memset(p->h_arena, 0, L.end);
        for (int k = 1; k < 4; ++k) memcpy(p->h_arena + L.in[k], h_in[k], sizeof(double) * nd);
        copy_records(n, dof, arena_records(p->h_arena, L), given, kAllRecords);
        return run_in_arena(p, n, L, L.end, 1, &outr, offsets, packed,
                            [&](const ltp_queries&, const ltp_records& dr, unsigned long long* d_off) { return offsets_for(dr, d_off); });
    }
    Staged st{p, n, dof};
    if ((rc = st.begin(h_in, 1)) != LTP_OK) return rc;
    rc = for_each_record_field(dof, [&](auto m, size_t per, int) -> int {
        if (given.*m && nd) LTP_HIP_TRY(p, hipMemcpy(st.dr.r.*m, given.*m, elem_size(m) * per * (size_t)n, hipMemcpyHostToDevice));
        return LTP_OK;
    });
    if (rc != LTP_OK) return rc;
    if (n) LTP_HIP_TRY(p, hipMemset(st.dr.r.status, 0, sizeof(int) * (size_t)n));
    LTP_HIP_TRY(p, hipMemset(st.d_off, 0, sizeof(unsigned long long) * ((size_t)n + 1)));
    if (n > 0 && dof > 0 && (rc = offsets_for(st.dr.r, st.d_off)) != LTP_OK) return rc;
    return st.finish(&outr, offsets, packed);
}

void ltp_free_host(void* ptr)
{
    if (ptr && !g_pinned.release(ptr)) free(ptr);
}

int ltp_check_inputs_host(ltp_planner* p, const double* q_0, const double* v_0, const double* a_0, int* ok)
{
    if (!p || !ok) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    { std::lock_guard<std::mutex> g(p->mu); rc = check_config(p); }
    if (rc != LTP_OK) return rc;
    const int dof = p->dof;
    if (dof == 0) { *ok = 1; return LTP_OK; }   // the reference's loop over zero joints (cc:72-76)
    if (!q_0 || !v_0 || !a_0) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> hg(p->host_mu);
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    const size_t row = ((sizeof(double) * dof) + 15) & ~(size_t)15;
    rc = ensure_arena(p, 3 * row + 16);
    if (rc != LTP_OK) return rc;
    memcpy(p->h_arena, q_0, sizeof(double) * dof);
    memcpy(p->h_arena + row, v_0, sizeof(double) * dof);
    memcpy(p->h_arena + 2 * row, a_0, sizeof(double) * dof);
    ltp::launch_check_inputs(nullptr, dof, dev_limits(p), (const double*)p->h_arena, (const double*)(p->h_arena + row),
                             (const double*)(p->h_arena + 2 * row), (int*)(p->h_arena + 3 * row), p->semantics);   // pinned: no copies (checkInputs forms no powers)
    LTP_HIP_TRY(p, hipGetLastError());
    LTP_HIP_TRY(p, hipStreamSynchronize(nullptr));
    *ok = *(const int*)(p->h_arena + 3 * row);
    return LTP_OK;
}

int ltp_opt_braking_host(ltp_planner* p, int joint, double v_0, double a_0, double* q, double* t_rel, double* dir)
{
    if (!p || !q || !t_rel || !dir) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    double buf[16] = {0};
    memcpy(buf, t_rel, sizeof(double) * 7);
    const int rc = run_one_lane(p, joint, buf, [&](double* io, double ts, const ltp::Limits& lim, int sem) { ltp::launch_single_opt_braking(nullptr, joint, ts, lim, v_0, a_0, io, sem); });
    if (rc != LTP_OK) return rc;
    memcpy(t_rel, buf, sizeof(double) * 7);
    *q = buf[7];
    *dir = buf[8];
    return LTP_OK;
}

int ltp_opt_switch_times_host(ltp_planner* p, int joint, double q_goal, double q_0, double v_0, double a_0, double v_drive,
                              double* t, double* dir, char* mod, int* ok)
{
    if (!p || !t || !dir || !mod || !ok) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    double buf[16] = {0};
    memcpy(buf, t, sizeof(double) * 7);
    const int rc = run_one_lane(p, joint, buf, [&](double* io, double ts, const ltp::Limits& lim, int sem) { ltp::launch_single_opt_switch(nullptr, joint, ts, lim, q_goal, q_0, v_0, a_0, v_drive, io, sem); });
    if (rc != LTP_OK) return rc;
    memcpy(t, buf, sizeof(double) * 7);
    *dir = buf[7];
    *mod = (char)(int)buf[8];
    *ok = (int)buf[9];
    return LTP_OK;
}

int ltp_time_scaling_host(ltp_planner* p, int joint, double q_goal, double q_0, double v_0, double a_0, double dir,
                          double t_required, double* scaled_t, double* v_drive, char* mod, int* ok, int* accepted_case)
{
    if (!p || !scaled_t || !v_drive || !mod || !ok) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    double buf[16] = {0};
    memcpy(buf, scaled_t, sizeof(double) * 7);
    const int rc = run_one_lane(p, joint, buf, [&](double* io, double ts, const ltp::Limits& lim, int sem) { ltp::launch_single_time_scaling(nullptr, joint, ts, lim, q_goal, q_0, v_0, a_0, dir, t_required, io, sem); });
    if (rc != LTP_OK) return rc;
    memcpy(scaled_t, buf, sizeof(double) * 7);
    *v_drive = buf[7];
    *mod = (char)(int)buf[8];
    *ok = (int)buf[9];
    if (accepted_case) *accepted_case = (int)buf[10];
    return LTP_OK;
}

static int roots_host_any(ltp_planner* p, long long n, int degree, bool f32, const void* coef, void* re, void* im)
{
    if (!p || n < 0 || degree < 1 || degree > 8 || !coef || !re || !im) return fail(p, LTP_ERR_INVALID_ARGUMENT, "bad argument (degree 1..8)");
    // long_term_planner/roots.h routes every roots() call of a process through one handle: serialise them, and stage through
    // the handle's pinned arena (host memory the kernel reads and writes directly) instead of three allocations and copies per call
    std::lock_guard<std::mutex> hg(p->host_mu);
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    if (n == 0) return LTP_OK;
    const size_t es = f32 ? sizeof(float) : sizeof(double);
    const size_t cb = ((size_t)n * (degree + 1) * es + 15) & ~(size_t)15, rb = ((size_t)n * degree * es + 15) & ~(size_t)15;
    if (cb + 2 * rb <= kSmallHostBytes) {
        int rc = ensure_arena(p, cb + 2 * rb);
        if (rc != LTP_OK) return rc;
        memcpy(p->h_arena, coef, (size_t)n * (degree + 1) * es);
        ltp::launch_roots_all(nullptr, n, degree, f32, p->h_arena, p->h_arena + cb, p->h_arena + cb + rb);
        LTP_HIP_TRY(p, hipGetLastError());
        LTP_HIP_TRY(p, hipStreamSynchronize(nullptr));
        memcpy(re, p->h_arena + cb, (size_t)n * degree * es);
        memcpy(im, p->h_arena + cb + rb, (size_t)n * degree * es);
        return LTP_OK;
    }
    char *dc = nullptr, *dr = nullptr, *di = nullptr;   // bytes: the element is float or double
    DevRecords dev;
    LTP_HIP_TRY(p, dev.up(&dc, (const char*)coef, (size_t)n * (degree + 1) * es));
    LTP_HIP_TRY(p, dev.alloc(&dr, (size_t)n * degree * es));
    LTP_HIP_TRY(p, dev.alloc(&di, (size_t)n * degree * es));
    ltp::launch_roots_all(nullptr, n, degree, f32, dc, dr, di);
    LTP_HIP_TRY(p, hipGetLastError());
    LTP_HIP_TRY(p, dev.down((char*)re, dr, (size_t)n * degree * es));
    LTP_HIP_TRY(p, dev.down((char*)im, di, (size_t)n * degree * es));
    return LTP_OK;
}

int ltp_roots_f64_host(ltp_planner* p, long long n, int degree, const double* coef, double* re, double* im)
{
    return roots_host_any(p, n, degree, false, coef, re, im);
}

int ltp_roots_f32_host(ltp_planner* p, long long n, int degree, const float* coef, float* re, float* im)
{
    return roots_host_any(p, n, degree, true, coef, re, im);
}

int ltp_debug_last_matlab_flags(const ltp_planner* p) { return p ? p->last_matlab_flags : -1; }

int ltp_debug_roots_matlab_host(ltp_planner* p, long long n, int degree, const double* coef, double* re, double* im, int* nroots, int* status)
{
    if (!p || n < 0 || degree < 1 || degree > 6 || !coef || !re || !im || !nroots || !status) return fail(p, LTP_ERR_INVALID_ARGUMENT, "bad argument (degree 1..6)");
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    double *dc = nullptr, *dr = nullptr, *di = nullptr;
    int *dn = nullptr, *ds = nullptr;
    DevRecords dev;
    LTP_HIP_TRY(p, dev.up(&dc, coef, (size_t)n * (degree + 1)));
    LTP_HIP_TRY(p, dev.alloc(&dr, (size_t)n * degree));
    LTP_HIP_TRY(p, dev.alloc(&di, (size_t)n * degree));
    LTP_HIP_TRY(p, dev.alloc(&dn, (size_t)n));
    LTP_HIP_TRY(p, dev.alloc(&ds, (size_t)n));
    ltp::launch_roots_matlab(nullptr, n, degree, dc, dr, di, dn, ds);
    LTP_HIP_TRY(p, hipGetLastError());
    LTP_HIP_TRY(p, dev.down(re, dr, (size_t)n * degree));
    LTP_HIP_TRY(p, dev.down(im, di, (size_t)n * degree));
    LTP_HIP_TRY(p, dev.down(nroots, dn, (size_t)n));
    LTP_HIP_TRY(p, dev.down(status, ds, (size_t)n));
    return LTP_OK;
}

int ltp_debug_math_probe_host(ltp_planner* p, long long n, const double* x, const double* y, double* out)
{
    if (!p || n < 0 || !x || !y || !out) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    DevRecords dev;
    LTP_HIP_TRY(p, dev.up(&dx, x, (size_t)n));
    LTP_HIP_TRY(p, dev.up(&dy, y, (size_t)n));
    LTP_HIP_TRY(p, dev.alloc(&dout, (size_t)n * 8));
    ltp::launch_math_probe(nullptr, n, dx, dy, dout);
    LTP_HIP_TRY(p, hipGetLastError());
    LTP_HIP_TRY(p, dev.down(out, dout, (size_t)n * 8));
    return LTP_OK;
}

int ltp_debug_libm_pow_host(ltp_planner* p, long long n, const double* x, const double* y, double* out)
{
    if (!p || n < 0 || !x || !y || !out) return fail(p, LTP_ERR_INVALID_ARGUMENT, "null argument");
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    DevRecords dev;
    LTP_HIP_TRY(p, dev.up(&dx, x, (size_t)n));
    LTP_HIP_TRY(p, dev.up(&dy, y, (size_t)n));
    LTP_HIP_TRY(p, dev.alloc(&dout, (size_t)n));
    ltp::launch_libm_pow_probe(nullptr, n, dx, dy, dout);
    LTP_HIP_TRY(p, hipGetLastError());
    LTP_HIP_TRY(p, dev.down(out, dout, (size_t)n));
    return LTP_OK;
}

int ltp_debug_roots_probe_host(ltp_planner* p, long long n, int degree, const double* coef, double* root)
{
    if (!p || n < 0 || !coef || !root || degree < 4 || degree > 6) return fail(p, LTP_ERR_INVALID_ARGUMENT, "bad argument");
    LTP_HIP_TRY(p, hipSetDevice(p->device));
    double *dc = nullptr, *dr = nullptr;
    DevRecords dev;
    LTP_HIP_TRY(p, dev.up(&dc, coef, (size_t)n * 7));
    LTP_HIP_TRY(p, dev.alloc(&dr, (size_t)n));
    ltp::launch_roots_probe(nullptr, n, degree, dc, dr);
    LTP_HIP_TRY(p, hipGetLastError());
    LTP_HIP_TRY(p, dev.down(root, dr, (size_t)n));
    return LTP_OK;
}

}  // extern "C"
