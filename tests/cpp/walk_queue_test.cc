// walk_queue_test — the arithmetic of the walk kernels' batches and work queue (longtermplanner_amd/csrc/ltp_sampler_policy.hpp:
// walk_plans_per_batch, walk_plans_per_item, walk_queue, walk_queue_item, walk_row_lanes_log2) over the product of plan counts,
// joint counts, caps, strides and interleaves on each side of every threshold, on the host (plain g++, no GPU, no ROCm headers).
//   walk_queue_test      exit status 0 = every property holds
#include "../../longtermplanner_amd/csrc/ltp_sampler_policy.hpp"

#include <cstdio>
#include <vector>

using namespace ltp;

static const long long kCounts[] = {1, 2, 8, 9, 10, 26, 27, 28, 63, 64, 65, 577, 4099};
static const int kDofs[] = {1, 2, 3, 7, 9, 10, 21, 22, 30, 63, 64, 100};
static const int kCaps[] = {0, 4, 32, 33, 64, 65, 1024, 1025};
static const int kStrides[] = {1, 3};
constexpr int kDefaultSpread = 64;   // kSampleSpread (ltp_kernels.hpp): what a call without an interleave of its own asks for

static int g_failures = 0;
#define CHECK(COND, ...)                                                          \
    do {                                                                          \
        if (!(COND) && ++g_failures <= 20) {                                      \
            std::printf("FAILED %s: ", #COND);                                    \
            std::printf(__VA_ARGS__);                                             \
            std::printf("\n");                                                    \
        }                                                                         \
    } while (0)

int main()
{
    long combos = 0;
    std::vector<int> seen;
    for (long long count : kCounts)
        for (int dof : kDofs)
            for (int cap : kCaps)
                for (int stride : kStrides) {
                    const RowSpec rows{cap, stride};
                    const long long items = walk_queue(count, dof, rows, 1).items;
                    const int spreads[] = {1, 3, 64, walk_launch_spread(kDefaultSpread, items), (int)items + 1};
                    for (int spread : spreads) {
                        ++combos;
                        char in[128];
                        std::snprintf(in, sizeof in, "count %lld dof %d cap %d stride %d spread %d", count, dof, cap, stride, spread);
                        const WalkQueue q = walk_queue(count, dof, rows, spread);
                        // batch and item shapes
                        CHECK(q.ppb == walk_plans_per_batch(dof, rows) && q.ipp == walk_plans_per_item(dof, rows), "%s", in);
                        CHECK(q.ppb >= 1 && q.ppb * (dof < kWalkLanes ? dof : kWalkLanes) <= kWalkLanes, "%s: ppb %d", in, q.ppb);
                        CHECK(q.ppb <= kWalkMaxPlans, "%s: ppb %d", in, q.ppb);
                        CHECK(q.ipp <= 64 && q.ipp % q.ppb == 0, "%s: ipp %d ppb %d (one traj_len load per lane)", in, q.ipp, q.ppb);
                        CHECK(walk_wide_plans(dof) * walk_wide_joints(dof) <= kWideLanes, "%s: wide %d x %d", in, walk_wide_plans(dof), walk_wide_joints(dof));
                        CHECK(q.items == items && q.total >= (unsigned long long)items, "%s: items %lld total %llu", in, q.items, q.total);
                        // every plan of the call lies in exactly one queue item
                        seen.assign((size_t)count, 0);
                        long long pieces = 0;
                        for (unsigned long long item = 0; item < q.total; ++item) {
                            long long pb = -1;
                            int np = -1;
                            walk_queue_item(q, item, pb, np);
                            CHECK(np >= 0 && np <= q.ipp, "%s: item %llu np %d ipp %d", in, item, np, q.ipp);
                            if (np <= 0) continue;                                  // a hole of the interleave
                            ++pieces;
                            CHECK(pb >= 0 && pb + np <= count, "%s: item %llu [%lld, %lld)", in, item, pb, pb + np);
                            for (long long p = pb; p < pb + np && p < count; ++p)
                                if (p >= 0) ++seen[(size_t)p];
                        }
                        long long once = 0;
                        for (int s : seen) once += s == 1;
                        CHECK(once == count, "%s: %lld of %lld plans lie in exactly one item", in, once, count);
                        CHECK(pieces == items, "%s: %lld items with plans, %lld expected", in, pieces, items);
                        // items at or beyond the end of the queue have no plans
                        for (unsigned long long item : {q.total, q.total + 1, q.total + (unsigned long long)spread, ~0ull}) {
                            long long pb = -1;
                            int np = -1;
                            walk_queue_item(q, item, pb, np);
                            CHECK(np == 0, "%s: item %llu beyond total %llu has np %d", in, item, q.total, np);
                        }
                    }
                }
    // lanes per row: the smallest power of two of lanes that holds the cap's slots (a slot: a pair of samples), at most a wave
    for (int cap = 1; cap <= 1024; ++cap) {
        const int slots = (cap + 1) / 2;
        int lg = 0;
        while (lg < 6 && (1 << lg) < slots) ++lg;
        CHECK(walk_row_lanes_log2(RowSpec{cap, 1}) == lg, "cap %d: %d, expected %d", cap, walk_row_lanes_log2(RowSpec{cap, 1}), lg);
    }
    // long rows: no cap, or a cap beyond kWalkBatchCap
    CHECK(walk_long_rows(RowSpec{0, 1}) && !walk_long_rows(RowSpec{1, 1}) && !walk_long_rows(RowSpec{kWalkBatchCap, 1}) && walk_long_rows(RowSpec{kWalkBatchCap + 1, 1}), "walk_long_rows");
    std::printf("%ld combinations, %d failures\n", combos, g_failures);
    return g_failures ? 1 : 0;
}
