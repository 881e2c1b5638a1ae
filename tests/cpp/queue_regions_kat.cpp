// Known-answer checks of the queue wavefront's region size (csrc/drt_tuning.h: queue_region_shift, queue_regions), the choice
// shard_plan makes for every batch of the queue route: unchanged without DRT_HIP_REGION_SIZE (256 slots, halved down to 64 while the
// batch makes fewer than 32 regions per CU), and a set size taken as given -- what tests/test_gpu_queue_geometry.py relies on to render
// frames of 315 and 1771 paths in regions of several chunks.
#define DRT_FAST_PARAMS 8        // (csrc/drt_device.h; the table's clamp of DRT_HIP_GEN_ABOVE)
#include "../../differentiable-renderer_amd/csrc/drt_tuning.h"

#include <cstdio>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// what shard_plan computed before the choice became a function of its own (no setting)
static unsigned plan_as_it_was(unsigned long long N, int n_cu)
{
    unsigned shift = 8;
    while (shift > 6 && (N >> shift) < (unsigned long long)n_cu * 32)
        --shift;
    return shift;
}

int main()
{
    // no setting, 256 CUs
    CHECK(queue_region_shift(315, 256, 0) == 6);
    CHECK(queue_region_shift(1771, 256, 0) == 6);
    CHECK(queue_region_shift(2097151, 256, 0) == 7);
    CHECK(queue_region_shift(2097152, 256, 0) == 8);
    CHECK(queue_region_shift(1048575, 256, 0) == 6);         // (2^20 - 1: one short of 32 regions of 128 per CU)
    CHECK(queue_region_shift(1048576, 256, 0) == 7);
    CHECK(queue_region_shift(1ull << 31, 256, 0) == 8);
    CHECK(queue_region_shift(0, 256, 0) == 6);
    CHECK(queue_region_shift(1771, 256, -1) == 6);           // (a negative setting is no setting)
    // ... and on every device size and batch the rule of before
    const int cus[] = {1, 8, 64, 104, 228, 256, 304};
    for (int n_cu : cus)
        for (unsigned long long N = 1; N < (1ull << 33); N = N * 3 / 2 + 1) {
            CHECK(queue_region_shift(N, n_cu, 0) == plan_as_it_was(N, n_cu));
            CHECK(queue_region_shift(N - 1, n_cu, 0) == plan_as_it_was(N - 1, n_cu));
        }
    for (int n_cu : cus)
        for (unsigned s = 6; s <= 8; ++s) {                  // the thresholds themselves
            const unsigned long long N = ((unsigned long long)n_cu * 32) << s;
            CHECK(queue_region_shift(N, n_cu, 0) == plan_as_it_was(N, n_cu));
            CHECK(queue_region_shift(N - 1, n_cu, 0) == plan_as_it_was(N - 1, n_cu));
            CHECK(queue_region_shift(N, n_cu, 0) == s && (s == 6 || queue_region_shift(N - 1, n_cu, 0) == s - 1));
        }
    // a setting is taken as given: the smallest power of two in [64, 2^20] that holds it, whatever the batch
    const unsigned long long batches[] = {0, 1, 45, 315, 1771, 2097151, 2097152, 1ull << 31};
    for (unsigned long long N : batches)
        for (int n_cu : cus) {
            CHECK(queue_region_shift(N, n_cu, 128) == 7);
            CHECK(queue_region_shift(N, n_cu, 100) == 7);
            CHECK(queue_region_shift(N, n_cu, 1) == 6);
            CHECK(queue_region_shift(N, n_cu, 64) == 6);
            CHECK(queue_region_shift(N, n_cu, 65) == 7);
            CHECK(queue_region_shift(N, n_cu, 1 << 30) == 20);
            CHECK(queue_region_shift(N, n_cu, (1 << 20) + 1) == 20);
            CHECK(queue_region_shift(N, n_cu, 1ll << 40) == 20);
        }
    CHECK(queue_region_shift(315, 256, 256) == 8);
    CHECK(queue_region_shift(1771, 256, 1024) == 10);
    // the regions of a batch: ceil(N / size)
    CHECK(queue_regions(315, queue_region_shift(315, 256, 256)) == 2);
    CHECK(queue_regions(1771, queue_region_shift(1771, 256, 1024)) == 2);
    CHECK(queue_regions(1771, queue_region_shift(1771, 256, 256)) == 7);
    CHECK(queue_regions(1771, queue_region_shift(1771, 256, 128)) == 14);
    CHECK(queue_regions(595, queue_region_shift(595, 256, 256)) == 3);
    CHECK(queue_regions(1771, queue_region_shift(1771, 256, 0)) == 28);
    CHECK(queue_regions(256, 8) == 1 && queue_regions(257, 8) == 2 && queue_regions(1, 20) == 1 && queue_regions(0, 8) == 0);
    CHECK(queue_regions(0x7FFFFFFFull, 6) == 33554432u);     // (the largest batch the plan makes, in the smallest regions)
    // every slot a region's wave may touch lies inside ceil(N / size) * size, and every path has a slot
    for (unsigned long long N : batches)
        for (unsigned s = 6; s <= 20; ++s) {
            const unsigned long long r = queue_regions(N, s);
            CHECK((r << s) >= N && (r == 0 || ((r - 1) << s) < N));
        }
    if (failures)
        std::printf("%d failures\n", failures);
    else
        std::printf("ok\n");
    return failures ? 1 : 0;
}
