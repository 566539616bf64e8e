// ltp_sampler_policy.hpp — which row / envelope kernel a call launches (and the name ltp_last_sampler_kernel reports), decided in
// one place from the caller's policy, decoded at the C ABI; with it the row geometry every sampler shares and the walk kernels' queue
// arithmetic. Host logic without HIP headers: tests/cpp/sampler_policy_test.cc and tests/cpp/walk_queue_test.cc pin it.
#pragma once
#include "../../include/ltp_hip.h"

#if defined(__HIPCC__)
#define LTP_POLICY_HD __host__ __device__
#else
#define LTP_POLICY_HD
#endif

namespace ltp {

constexpr int kRowAlign = 32;          // trajectory rows padded to 32 elements (256 B of doubles, 128 B of floats)
// padded length of a row of n stored samples, in n's own type (walk_stream, ltp_sampler_walk.hip, forms byte offsets in 32 bits)
template <typename N> LTP_POLICY_HD constexpr N row_stride(N n) { return (n + (N)(kRowAlign - 1)) / (N)kRowAlign * (N)kRowAlign; }
// THE extent a dense sampler writes of a row of n stored samples: up to the end of the row's last memory line, elements [n, row_line)
// as +0.0, so that no line of a row reaches the memory as a partial write (the controller turns one into a read-modify-write);
// [row_line, row_stride) stays unwritten. Rows start on a line (kRowAlign elements are whole lines of either type) and
// row_line(n) <= row_stride(n): the padding never leaves the row.
constexpr int kLineBytes = 64;
template <typename T, typename N> LTP_POLICY_HD constexpr N row_line(N n)
{
    constexpr N per = (N)(kLineBytes / (int)sizeof(T));
    return (n + per - 1) / per * per;
}
static_assert(kRowAlign * 4 % kLineBytes == 0 && kRowAlign * 8 % kLineBytes == 0, "a row stride is whole lines of float and of double");
// elements of a plan's four arrays (q, v, a, j: dof rows each) at `len` stored samples per row
LTP_POLICY_HD inline unsigned long long plan_size(int len, int dof)
{
    return len <= 0 ? 0ull : 4ull * (unsigned long long)dof * row_stride((unsigned long long)len);
}
// THE fit rule of every sampler, and of every reader that must skip what a sampler skipped: a plan whose arrays start `rel` elements
// into a tile of `capacity` elements ends beyond the tile (the sampler then stores nothing and sets kStatusOverflow)
LTP_POLICY_HD inline bool plan_beyond_tile(unsigned long long rel, int slen, int dof, unsigned long long capacity)
{
    // rel + plan_size(slen, dof) for a stored_len (never negative), without plan_size's own test for it: k_sample's code is the
    // same to the instruction with the product written out, and differs in half its lines with the select
    return rel + 4ull * dof * row_stride((unsigned long long)slen) > capacity;
}

// which samples of a trajectory are stored in its rows
struct RowSpec {
    int max_samples;   // at most this many stored samples per row; 0 = no cap
    int stride;        // every stride-th sample (0, stride, 2*stride, ...); <= 1 = every sample
};

// a compact walk slot's run starts have 28 bits (ltp_sampler_walk.hip); rows whose cap times stride reaches this are built wide
constexpr long long kWalkCompactEnd = 0x0fffffffll;

// caps the autonomous-wave walk kernels take (ltp_sampler_walk.hip; make EXTRA=-DLTP_WALK_AUTO_CAP=n for A/B runs)
#ifndef LTP_WALK_AUTO_CAP
#define LTP_WALK_AUTO_CAP 32
#endif
constexpr int kWalkAutoCap = LTP_WALK_AUTO_CAP;
LTP_POLICY_HD inline bool walk_auto_rows(RowSpec rows)
{
    return rows.max_samples > 0 && rows.max_samples <= kWalkAutoCap && (long long)rows.max_samples * (rows.stride > 1 ? rows.stride : 1) < kWalkCompactEnd;
}

// ---- the walk kernels' batches and work queue (ltp_sampler_walk.hip): plain integer arithmetic, pinned on the host by
// tests/cpp/walk_queue_test.cc ----
constexpr int kWalkLanes = 63;                                // (plan, joint) lanes of a compact batch: 9 plans of 7 joints
constexpr int kWalkMaxPlans = 9;
constexpr int kWideLanes = 21;                                // lanes of a WIDE batch (all kMaxSegments runs per lane): 3 plans of 7 joints
// LONG rows — no cap, or a cap beyond kWalkBatchCap samples: wide batches only, one row per wave pass (walk_stream_rows). Short rows: compact
// batches, several rows per pass, one descriptor with 32-bit offsets over the batch (walk_stream).
constexpr int kWalkBatchCap = 1024;
LTP_POLICY_HD inline bool walk_long_rows(RowSpec rows) { return rows.max_samples <= 0 || rows.max_samples > kWalkBatchCap; }

// plans per batch: a compact batch; for long rows two wide batches
LTP_POLICY_HD inline int walk_plans_per_batch(int dof, RowSpec rows)
{
    if (dof > kWalkLanes) return 1;                                                // one plan, kWalkLanes joints at a time
    const int compact = (kWalkLanes / dof) < kWalkMaxPlans ? (kWalkLanes / dof) : kWalkMaxPlans;
    if (!walk_long_rows(rows)) return compact;
    const int two_wide = 2 * (kWideLanes / dof) > 1 ? 2 * (kWideLanes / dof) : 1;
    return two_wide < compact ? two_wide : compact;
}
// a WIDE batch: its plans, and the joints it holds of each (beyond kWideLanes joints: a part of one plan)
LTP_POLICY_HD inline int walk_wide_plans(int dof) { return kWideLanes / dof > 1 ? kWideLanes / dof : 1; }
LTP_POLICY_HD inline int walk_wide_joints(int dof) { return dof < kWideLanes ? dof : kWideLanes; }
// plans per QUEUE ITEM. Rows of at most kWalkGatherCap samples — where the builder's walks are what a block waits for — take
// kWalkGather batches' worth of consecutive plans per item, and a batch is made of the item's LIVE plans — the ones that store
// samples — walk_plans_per_batch at a time: plans that were rejected (traj_len 0) have no rows and take no lane of a walk. (In
// the later cycles of a receding-horizon loop a third of the random plans are dead; a batch of nine consecutive plans then walked
// six. Rows of the live plans of an item are neighbours in the tile whatever lies between them. Longer rows are bound by their
// stores: an item stays one batch there — gathered items cost first-256 1.3 % on one box, profiles/EXPERIMENTS.md E7.7.)
constexpr int kWalkGather = 3;
constexpr int kWalkGatherCap = 64;
LTP_POLICY_HD inline int walk_plans_per_item(int dof, RowSpec rows)
{
    const int ppb = walk_plans_per_batch(dof, rows);
    if (rows.max_samples <= 0 || rows.max_samples > kWalkGatherCap) return ppb;
    const int g = 64 / ppb < kWalkGather ? (64 / ppb > 1 ? 64 / ppb : 1) : kWalkGather;     // (one traj_len load per lane)
    return g * ppb;
}
// The work queue of a launch: items of walk_plans_per_item consecutive plans, interleaved over `spread` stripes of the call's plans
// (item -> stripe item % spread, place item / spread; holes included).
struct WalkQueue {
    int ipp, ppb, spread;
    long long count, items, per;
    unsigned long long total;
};
LTP_POLICY_HD inline WalkQueue walk_queue(long long count, int dof, RowSpec rows, int spread)
{
    WalkQueue q;
    q.ppb = walk_plans_per_batch(dof, rows);
    q.ipp = walk_plans_per_item(dof, rows);
    q.spread = spread > 0 ? spread : 1;
    q.count = count;
    q.items = (count + q.ipp - 1) / q.ipp;
    q.per = (q.items + q.spread - 1) / q.spread;
    q.total = (unsigned long long)q.per * (unsigned long long)q.spread;
    return q;
}
// first plan (local number) and plan count of a queue item; 0 plans: a hole of the interleave, or the end of the queue
LTP_POLICY_HD inline void walk_queue_item(const WalkQueue& q, unsigned long long item, long long& pb, int& np)
{
    pb = 0;
    np = 0;
    if (item >= q.total) return;
    const long long bi = (long long)(item % (unsigned long long)q.spread) * q.per + (long long)(item / (unsigned long long)q.spread);
    if (bi < q.items) {
        pb = bi * q.ipp;
        np = (int)(q.count - pb < q.ipp ? q.count - pb : q.ipp);
    }
}
// the interleave a launch runs with: the requested one, at most one stripe per queue item (items: walk_queue(.., 1).items)
LTP_POLICY_HD inline int walk_launch_spread(int spread, long long items) { return (long long)spread > items ? (int)items : spread; }
// lanes per row (as a power of two) of a capped row format, a lane taking a pair of samples at a time: the cap bounds every row of
// the call (down to one lane per row — at a cap of 16 samples a floor of 16 lanes per row left half of every pass idle)
LTP_POLICY_HD inline int walk_row_lanes_log2(RowSpec rows)
{
    const int max_slots = (rows.max_samples + 1) / 2;
    return max_slots > 32 ? 6 : (max_slots > 16 ? 5 : (max_slots > 8 ? 4 : (max_slots > 4 ? 3 : (max_slots > 2 ? 2 : (max_slots > 1 ? 1 : 0)))));
}

// rows the walk kernels take: every format, any number of joints
inline bool sample_walk_applies(int dof, RowSpec rows)
{
    if (dof < 1 || rows.max_samples < 0) return false;
    // capped rows up to kWalkBatchCap samples go through walk_stream (ltp_sampler_walk.hip), whose offsets inside a batch
    // are 32-bit BYTE offsets behind one buffer descriptor: the four arrays of a plan (4 * dof * row stride elements of at most 8
    // bytes) must stay below 2 GiB (round-4 advisor). That holds up to dof ~ 65 000 at a 1024-sample cap; beyond, the fused sampler / the table pass take the rows.
    if (rows.max_samples > 0 && rows.max_samples <= kWalkBatchCap && plan_size(rows.max_samples, dof) * 8ull >= (1ull << 31)) return false;
    return true;
}

// Table pass or fused build? (DESIGN.md "Table pass".) The pass writes and re-reads up to 912 bytes per joint and runs
// the sampler with streaming waves that never wait; the fused build costs every item ~8 us of latency, three barriers and
// a drain of its own stores: the pass pays when a joint's rows are short (measured crossover: a cap between 256 and 512
// float64 samples, and beyond 1024 float32 samples, whose fused kernel only holds 16 waves per CU). `row_bytes` = bytes of one
// joint's four rows under the cap (0 = no cap). table_pass: the handle's ltp_set_table_pass (0 automatic, 1 always, -1 never).
inline bool want_table_pass(int table_pass, unsigned long long row_bytes, bool f32)
{
    if (table_pass != 0) return table_pass > 0;
    return row_bytes > 0 && row_bytes <= (f32 ? 16384ull : 8192ull);
}

// k_sample_walk_* (tables built inside the sampler's block) or the fused build of k_sample? Measured, 1 M panda plans
// unless noted (profiles/r04_whole_rows_walk_ab.txt, walk vs fused in TB/s): what decides is how many bytes a plan's rows have —
// below ~150 KB the fused sampler's per-plan build shows. First-512 float64 7.16 vs 6.16, every 3rd sample 6.71 vs 5.85, every 4th
// 6.29 vs 4.75, float32 every 4th sample 4.64 vs 2.40, whole float32 rows 6.83 vs 6.59 (S-ref: 6.80 vs 6.88); level or just behind
// from ~190 KB per plan: first-1024 float64 7.02 vs 7.09, every 2nd sample 6.85 vs 6.91, whole float64 rows 7.03 vs 7.08, S-ref every
// 4th sample 6.93 vs 6.97. The lengths are not known on the host, so the rule goes by what is: the cap, the stride, the element type.
inline bool want_walk(int table_pass, int max_samples, int stride, bool f32)
{
    if (table_pass != 0) return table_pass > 0;
    return f32 || stride >= 3 || (max_samples > 0 && max_samples <= 768);
}

constexpr bool kEnvelopeTablePassByDefault = true;   // measured: see DESIGN.md "Table pass"

// the caller's sampler policy (include/ltp_hip.h, ltp_sample_opts)
struct SamplePolicy {
    enum class Walk { Auto, Force, Forbid };      // the walk kernels (where they apply)
    enum class Build { Auto, Table, Fused };      // otherwise: the table pass or the fused build of k_sample
    bool nontemporal = false, dry = false, skip_verdict = false;
    int interleave = 0;                           // work-queue block interleave, 0 = default
    Walk walk = Walk::Auto;
    Build build = Build::Auto;
    bool walk_streaming = false;                  // the builder / streaming-wave walk also where the autonomous waves would run
};

// ltp_sample_batch's flag word; bit 5 wins over bit 6, bit 2 over bit 3
inline SamplePolicy policy_from_flags(int flags)
{
    SamplePolicy o;
    o.nontemporal = flags & 1;
    o.dry = flags & 2;
    o.build = (flags & 4) ? SamplePolicy::Build::Table : (flags & 8) ? SamplePolicy::Build::Fused : SamplePolicy::Build::Auto;
    o.skip_verdict = flags & 16;
    o.walk = (flags & 32) ? SamplePolicy::Walk::Forbid : (flags & 64) ? SamplePolicy::Walk::Force : SamplePolicy::Walk::Auto;
    o.walk_streaming = flags & 128;
    o.interleave = (flags >> 8) & 0xFFFF;
    return o;
}

// ltp_sample_opts, validated by the caller
inline SamplePolicy policy_from_opts(const ltp_sample_opts& o)
{
    SamplePolicy p;
    p.nontemporal = o.stores == LTP_STORES_NONTEMPORAL;
    p.dry = o.dry_run != 0;
    p.skip_verdict = o.verdict == LTP_VERDICT_SKIP;
    p.interleave = o.interleave;
    switch (o.sampler) {
    case LTP_SAMPLER_FUSED: p.build = SamplePolicy::Build::Fused; p.walk = SamplePolicy::Walk::Forbid; break;
    case LTP_SAMPLER_WALK: p.walk = SamplePolicy::Walk::Force; break;
    case LTP_SAMPLER_WALK_STREAMING: p.walk = SamplePolicy::Walk::Force; p.walk_streaming = true; break;
    case LTP_SAMPLER_TABLE: p.build = SamplePolicy::Build::Table; p.walk = SamplePolicy::Walk::Forbid; break;
    default: break;
    }
    return p;
}

// The walk kernels (ltp_sampler_walk.hip defines and launches them from this list): symbol, then autonomous waves, MATLAB semantics,
// no end-limit verdict, float32 rows, non-temporal stores — in the order of walk_kernel_index
#define LTP_WALK_KERNELS(X)                          \
    X(k_sample_walk_f64, 0, 0, 0, 0, 0)              \
    X(k_sample_walk_f64_nt, 0, 0, 0, 0, 1)           \
    X(k_sample_walk_f32, 0, 0, 0, 1, 0)              \
    X(k_sample_walk_f32_nt, 0, 0, 0, 1, 1)           \
    X(k_sample_walk_matlab_f64, 0, 1, 0, 0, 0)       \
    X(k_sample_walk_matlab_f64_nt, 0, 1, 0, 0, 1)    \
    X(k_sample_walk_matlab_f32, 0, 1, 0, 1, 0)       \
    X(k_sample_walk_matlab_f32_nt, 0, 1, 0, 1, 1)    \
    X(k_sample_walk_f64_nv, 0, 0, 1, 0, 0)           \
    X(k_sample_walk_f64_nt_nv, 0, 0, 1, 0, 1)        \
    X(k_sample_walk_f32_nv, 0, 0, 1, 1, 0)           \
    X(k_sample_walk_f32_nt_nv, 0, 0, 1, 1, 1)        \
    X(k_sample_walk_auto_f64, 1, 0, 0, 0, 0)         \
    X(k_sample_walk_auto_f64_nt, 1, 0, 0, 0, 1)      \
    X(k_sample_walk_auto_f32, 1, 0, 0, 1, 0)         \
    X(k_sample_walk_auto_f32_nt, 1, 0, 0, 1, 1)      \
    X(k_sample_walk_matlab_auto_f64, 1, 1, 0, 0, 0)    \
    X(k_sample_walk_matlab_auto_f64_nt, 1, 1, 0, 0, 1) \
    X(k_sample_walk_matlab_auto_f32, 1, 1, 0, 1, 0)    \
    X(k_sample_walk_matlab_auto_f32_nt, 1, 1, 0, 1, 1) \
    X(k_sample_walk_auto_f64_nv, 1, 0, 1, 0, 0)      \
    X(k_sample_walk_auto_f64_nt_nv, 1, 0, 1, 0, 1)   \
    X(k_sample_walk_auto_f32_nv, 1, 0, 1, 1, 0)      \
    X(k_sample_walk_auto_f32_nt_nv, 1, 0, 1, 1, 1)
#define LTP_WALK_NAME(K, AU, ML, NV, F32, NT) #K,
constexpr const char* kWalkKernelNames[] = {LTP_WALK_KERNELS(LTP_WALK_NAME)};
#undef LTP_WALK_NAME
constexpr int kWalkKernelCount = (int)(sizeof(kWalkKernelNames) / sizeof(kWalkKernelNames[0]));
#define LTP_WALK_BUILDER_FORM(K, AU, ML, NV, F32, NT) +((AU) ? 0 : 1)
constexpr int kWalkAutoFirst = 0 LTP_WALK_KERNELS(LTP_WALK_BUILDER_FORM);   // the autonomous-wave kernels: [kWalkAutoFirst, kWalkKernelCount)
#undef LTP_WALK_BUILDER_FORM
constexpr int walk_kernel_index(bool autonomous, bool matlab, bool no_verdict, bool f32, bool nontemporal)
{
    return (autonomous ? kWalkAutoFirst : 0) + (nontemporal ? 1 : 0) + (f32 ? 2 : 0) + (matlab ? 4 : no_verdict ? 8 : 0);
}
constexpr bool walk_kernels_in_index_order()
{
    int i = 0;
    bool ok = true;
#define LTP_WALK_AT(K, AU, ML, NV, F32, NT) ok = ok && walk_kernel_index(AU, ML, NV, F32, NT) == i++;
    LTP_WALK_KERNELS(LTP_WALK_AT)
#undef LTP_WALK_AT
    return ok && walk_kernel_index(true, false, true, true, true) == i - 1;   // (and no index lies beyond the list)
}
static_assert(walk_kernels_in_index_order(), "row i of LTP_WALK_KERNELS is the kernel walk_kernel_index gives for the row's properties");

enum class SamplePath { Fused, Table, Walk, WalkAuto };   // WalkAuto: the walk kernels' autonomous-wave form
struct SampleChoice {
    SamplePath path;
    const char* kernel;   // what ltp_last_sampler_kernel reports
    int walk_kernel;      // Walk / WalkAuto: walk_kernel_index; else -1
};

// the row kernel of ltp_sample_batch*; semantics, table_pass (ltp_set_table_pass) and stamps are the handle's
inline SampleChoice choose_sampler(const SamplePolicy& o, int semantics, int table_pass, bool stamps, bool f32, RowSpec rows, int dof)
{
    using Walk = SamplePolicy::Walk;
    using Build = SamplePolicy::Build;
    // MATLAB semantics: the fused build of k_sample exists for the C++ semantics only; the walk kernel and the table pass (whose
    // builders are for_each_run<SEM>) serve both, and the kernels that read tables do not depend on the semantics
    const bool matlab = semantics == LTP_SEMANTICS_MATLAB;
    // k_sample_walk_* — the tables stay in the compute unit, no table pass at all. Taken by itself for the rows want_walk() names
    // (capped, float32, sparse) and for every row format in MATLAB semantics; a table-pass or fused-build request keeps its meaning.
    // (Diagnostic runs — dry stores, stamps — stay with the kernels that implement them.)
    if (!stamps && !o.dry && o.walk != Walk::Forbid && sample_walk_applies(dof, rows) &&
        (o.walk == Walk::Force || (o.build == Build::Auto && (matlab || want_walk(table_pass, rows.max_samples, rows.stride, f32))))) {
        const bool autonomous = walk_auto_rows(rows) && !o.walk_streaming;
        const bool no_verdict = !matlab && o.skip_verdict && rows.max_samples > 0;   // uncapped rows reach the last sample anyway
        const int k = walk_kernel_index(autonomous, matlab, no_verdict, f32, o.nontemporal);
        return {autonomous ? SamplePath::WalkAuto : SamplePath::Walk, kWalkKernelNames[k], k};
    }
    // bytes of one joint's four rows when the cap applies (a cap is the only way rows are known to be short up front)
    const unsigned long long row_bytes = rows.max_samples > 0 ? 4ull * (f32 ? 4 : 8) * (unsigned long long)rows.max_samples : 0ull;
    // (in MATLAB semantics a dry request, too, is served by the table pass, whose kernels have no dry form)
    if (matlab || (!o.dry && (!stamps || o.build == Build::Table) &&
                   (o.build == Build::Table || (o.build == Build::Auto && want_table_pass(table_pass, row_bytes, f32)))))
        return {SamplePath::Table, f32 ? (o.nontemporal ? "k_sample_tab_f32_nt" : "k_sample_tab_f32") : (o.nontemporal ? "k_sample_tab_f64_nt" : "k_sample_tab_f64"), -1};
    return {SamplePath::Fused, "k_sample", -1};   // one name for its store / dry / element variants
}

enum class EnvelopePath { Walk, Table, InKernel };
struct EnvelopeChoice {
    EnvelopePath path;
    bool analytic;        // Table / InKernel: k_envelope's analytic form
    const char* kernel;
};

// The envelope kernel of ltp_envelope_batch. Analytic envelopes: the register walk (no tables, no workspace); ltp_set_table_pass(p,
// 1 | -1) asks for k_envelope's analytic form instead (through the table pass / with the build inside the kernel): A/B runs.
inline EnvelopeChoice choose_envelope(int envelope_mode, int semantics, int table_pass, bool stamps)
{
    const bool matlab = semantics == LTP_SEMANTICS_MATLAB;
    const bool analytic = envelope_mode == LTP_ENVELOPE_ANALYTIC;
    if (analytic && table_pass == 0 && !stamps)
        return {EnvelopePath::Walk, true, matlab ? "k_envelope_walk_matlab analytic" : "k_envelope_walk analytic"};
    if (matlab || (!stamps && (table_pass > 0 || (table_pass == 0 && kEnvelopeTablePassByDefault))))
        return {EnvelopePath::Table, analytic, analytic ? "k_envelope analytic (run tables from k_build_tables)" : "k_envelope (run tables from k_build_tables)"};
    return {EnvelopePath::InKernel, analytic, analytic && !stamps ? "k_envelope analytic" : "k_envelope"};
}

}  // namespace ltp
