// The packing behind drt_hip_render_pixels (csrc/drt_pixels.h), as a stand-alone program: validation and the per-view grid records.
// Prints "ok" and exits 0, or reports the first failure.
#include <cstdio>
#include <cstring>
#include <vector>

#include "drt_pixels.h"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static int grid_checks(uint32_t n_ranges)
{
    const int32_t counts[7] = {0, 1, 63, 64, 65, 257, 0};
    const uint32_t groups[7] = {0, 1, 1, 1, 2, 5, 0};
    PixelsGrid g;
    pixels_pack(counts, 7, n_ranges, g);
    uint32_t block = 0, entry = 0;
    uint64_t fp = 0, cw = 0, waves = 0;
    for (int v = 0; v < 7; ++v) {
        const PixelsViewGrid& r = g.view[v];
        const uint32_t blocks = (groups[v] * n_ranges + 3) / 4;
        CHECK(r.first_block == block && r.n_blocks == blocks);
        CHECK(r.first_entry == entry && r.n_entries == (uint32_t)counts[v]);
        CHECK(r.n_groups == groups[v]);
        CHECK(r.fpart_at == fp && r.counts_at == cw);
        block += blocks;
        entry += (uint32_t)counts[v];
        fp += (uint64_t)n_ranges * 3 * (uint64_t)counts[v];
        cw += 2ull * groups[v] * n_ranges;
        waves += (uint64_t)groups[v] * n_ranges;
    }
    CHECK(g.n_views == 7 && g.n_blocks == block && g.n_entries == entry && g.n_entries == 450);
    CHECK(g.fpart_doubles == fp && g.count_words == cw && g.n_waves == waves);
    // (the numbers themselves: ten groups; one range -> 1, 1, 1, 1, 2 blocks; five -> 2, 2, 2, 3, 7)
    if (n_ranges == 1)
        CHECK(g.n_blocks == 6 && g.view[5].first_block == 4 && g.view[6].first_block == 6);
    if (n_ranges == 5)
        CHECK(g.n_blocks == 16 && g.view[5].first_block == 9 && g.view[6].first_block == 16 && g.view[0].first_block == 0 && g.view[1].first_block == 0);
    return 0;
}

int main()
{
    if (grid_checks(1) || grid_checks(5))
        return 1;
    const uint64_t WH = 480;
    std::vector<uint32_t> pix(450);
    for (size_t i = 0; i < pix.size(); ++i)
        pix[i] = (uint32_t)((i * 131u) % WH);
    const int32_t counts[7] = {0, 1, 63, 64, 65, 257, 0};
    uint64_t n = 0;
    CHECK(pixels_check(counts, 7, pix.data(), WH, 5, &n) == DRT_PIXELS_OK && n == 450);
    CHECK(pixels_check(counts, 7, pix.data(), WH, 5, nullptr) == DRT_PIXELS_OK);
    // a pixel equal to W H (the last entry; the first), a negative count, an all-zero batch, 65 views, no views, NULL lists
    pix[449] = (uint32_t)WH;
    CHECK(pixels_check(counts, 7, pix.data(), WH, 5, &n) == DRT_PIXELS_OUTSIDE);
    pix[449] = (uint32_t)WH - 1;
    CHECK(pixels_check(counts, 7, pix.data(), WH, 5, &n) == DRT_PIXELS_OK);
    pix[0] = 0xFFFFFFFFu;
    CHECK(pixels_check(counts, 7, pix.data(), WH, 5, &n) == DRT_PIXELS_OUTSIDE);
    pix[0] = 0;
    {
        int32_t neg[7];
        memcpy(neg, counts, sizeof neg);
        neg[3] = -1;
        CHECK(pixels_check(neg, 7, pix.data(), WH, 5, &n) == DRT_PIXELS_NEGATIVE);
        const int32_t zero[3] = {0, 0, 0};
        CHECK(pixels_check(zero, 3, pix.data(), WH, 5, &n) == DRT_PIXELS_EMPTY);
        std::vector<int32_t> many(65, 1);
        CHECK(pixels_check(many.data(), 65, pix.data(), WH, 5, &n) == DRT_PIXELS_N_VIEWS);
        CHECK(pixels_check(many.data(), 64, pix.data(), WH, 5, &n) == DRT_PIXELS_OK && n == 64);
        CHECK(pixels_check(many.data(), 0, pix.data(), WH, 5, &n) == DRT_PIXELS_N_VIEWS);
        CHECK(pixels_check(nullptr, 7, pix.data(), WH, 5, &n) == DRT_PIXELS_NULL);
        CHECK(pixels_check(counts, 7, nullptr, WH, 5, &n) == DRT_PIXELS_NULL);
    }
    for (int why = DRT_PIXELS_N_VIEWS; why <= DRT_PIXELS_TOO_MANY; ++why)
        CHECK(strlen(pixels_refusal_text(why)) > 0);
    CHECK(strstr(pixels_refusal_text(DRT_PIXELS_OUTSIDE), "outside the frame") && strstr(pixels_refusal_text(DRT_PIXELS_NEGATIVE), "negative count"));
    // totals at and just above 2^31 samples: 2^20 entries of pixel 0 at 2047 spp (2^31 - 2^20: passes), at 2048 (2^31: refused -- the limit is
    // 2^31 - 1 samples, as for a frame), and 2^20 + 1 entries at 2047 spp (passes), 2^20 - 1 at 2048 (passes: 2^31 - 2048)
    {
        std::vector<uint32_t> zeros(((size_t)1 << 20) + 1, 0u);
        int32_t c2[2] = {1 << 19, 1 << 19};
        CHECK(pixels_check(c2, 2, zeros.data(), WH, 2047, &n) == DRT_PIXELS_OK && n == (1u << 20));
        CHECK(pixels_check(c2, 2, zeros.data(), WH, 2048, &n) == DRT_PIXELS_TOO_MANY);
        c2[1] += 1;
        CHECK(pixels_check(c2, 2, zeros.data(), WH, 2047, &n) == DRT_PIXELS_OK);
        c2[1] -= 2;
        CHECK(pixels_check(c2, 2, zeros.data(), WH, 2048, &n) == DRT_PIXELS_OK);
        // exactly 2^31 - 1 samples: one entry at 2^31 - 1 spp passes, two are refused; counts near INT32_MAX do not overflow the total
        const int32_t one[1] = {1}, two[1] = {2};
        CHECK(pixels_check(one, 1, zeros.data(), WH, 0x7FFFFFFFull, &n) == DRT_PIXELS_OK);
        CHECK(pixels_check(two, 1, zeros.data(), WH, 0x7FFFFFFFull, &n) == DRT_PIXELS_TOO_MANY);
        std::vector<int32_t> huge(64, 0x7FFFFFFF);
        CHECK(pixels_check(huge.data(), 64, zeros.data(), WH, 0x7FFFFFFFull, &n) == DRT_PIXELS_TOO_MANY);
    }
    std::printf("ok\n");
    return 0;
}
