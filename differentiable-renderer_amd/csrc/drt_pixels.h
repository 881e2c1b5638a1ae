// drt_pixels.h -- the packing behind drt_hip_render_pixels: the caller's per-view pixel lists -> validation, and the launch grid's per-view
// records.  Plain host C++ without a HIP include: a stand-alone program tests it (tests/cpp/pixels_packing.cpp).
//
// View v's list is a "frame" of counts[v] pixels: ceil(counts[v] / 64) pixel groups (a wave each) times n_ranges sample ranges, in blocks
// of four waves, every view starting on a block boundary; a view without entries has no blocks.  The partial sums follow the views one
// behind the other: fpart per view [range][row][entry], counts per view [row][wave].
#pragma once
#include <cstddef>
#include <cstdint>

#define DRT_PIXELS_MAX_VIEWS 64      // == DRT_HIP_MAX_VIEWS (drt_hip.h)
#define DRT_PIXELS_WAVE 64           // == DRT_WAVE
#define DRT_PIXELS_BLOCK_WAVES 4     // == DRT_BLOCK / DRT_WAVE

// why a batch is refused (pixels_check), 0: it is not
enum PixelsRefusal {
    DRT_PIXELS_OK = 0,
    DRT_PIXELS_N_VIEWS,              // n_views outside 1 ... 64
    DRT_PIXELS_NULL,                 // no counts or no pixels
    DRT_PIXELS_NEGATIVE,             // a negative count
    DRT_PIXELS_EMPTY,                // sum(counts) == 0
    DRT_PIXELS_OUTSIDE,              // a pixel >= W H
    DRT_PIXELS_TOO_MANY,             // more than 2^31 camera samples over all entries (DRT_ERR_UNSUPPORTED; the others DRT_ERR_INVALID)
};
inline const char* pixels_refusal_text(int why)
{
    switch (why) {
    case DRT_PIXELS_N_VIEWS: return "n_views outside 1 ... DRT_HIP_MAX_VIEWS = 64";
    case DRT_PIXELS_NULL: return "counts or pixels is NULL";
    case DRT_PIXELS_NEGATIVE: return "a negative count";
    case DRT_PIXELS_EMPTY: return "an empty batch (sum(counts) == 0)";
    case DRT_PIXELS_OUTSIDE: return "a pixel outside the frame (>= W * H)";
    case DRT_PIXELS_TOO_MANY: return "more than 2^31 camera samples over all entries (they render in one launch)";
    default: return "";
    }
}

// The batch as the entry point takes it: -> DRT_PIXELS_OK and the number of entries, or the first reason to refuse it (in the order of the
// enum; the sample total is checked before the pixels are read, so a refused total costs no pass over the list)
inline int pixels_check(const int32_t* counts, int n_views, const uint32_t* pixels, uint64_t frame_pixels, uint64_t spp, uint64_t* n_entries)
{
    if (n_views < 1 || n_views > DRT_PIXELS_MAX_VIEWS)
        return DRT_PIXELS_N_VIEWS;
    if (!counts || !pixels)
        return DRT_PIXELS_NULL;
    uint64_t n = 0;
    for (int v = 0; v < n_views; ++v) {
        if (counts[v] < 0)
            return DRT_PIXELS_NEGATIVE;
        n += (uint64_t)counts[v];
    }
    if (n == 0)
        return DRT_PIXELS_EMPTY;
    if (n > 0x7FFFFFFFull / (spp > 0 ? spp : 1))       // (n spp > 2^31 - 1, without the product: it can pass 64 bits)
        return DRT_PIXELS_TOO_MANY;
    for (uint64_t e = 0; e < n; ++e)
        if ((uint64_t)pixels[e] >= frame_pixels)
            return DRT_PIXELS_OUTSIDE;
    if (n_entries)
        *n_entries = n;
    return DRT_PIXELS_OK;
}

// a view's place in the launch and in the partial sums
struct PixelsViewGrid {
    uint32_t first_block, n_blocks;  // of the path launch's grid
    uint32_t first_entry, n_entries; // of the caller's list
    uint32_t n_groups;               // waves a sample range: ceil(n_entries / 64)
    uint32_t pad;
    uint64_t fpart_at;               // doubles in front of the view's [n_ranges][3][n_entries] radiance sums
    uint64_t counts_at;              // words in front of the view's [2][n_groups n_ranges] counters
};
struct PixelsGrid {
    PixelsViewGrid view[DRT_PIXELS_MAX_VIEWS];
    uint32_t n_views, n_blocks;      // blocks of the whole grid
    uint64_t n_entries, n_waves;     // over all views (n_waves without the blocks' padding)
    uint64_t fpart_doubles, count_words;
};
// counts that pixels_check has passed, for `n_ranges` sample ranges a view -> the grid
inline void pixels_pack(const int32_t* counts, int n_views, uint32_t n_ranges, PixelsGrid& g)
{
    g = PixelsGrid();
    g.n_views = (uint32_t)n_views;
    for (int v = 0; v < n_views; ++v) {
        PixelsViewGrid& r = g.view[v];
        r.first_block = g.n_blocks;
        r.first_entry = (uint32_t)g.n_entries;
        r.n_entries = (uint32_t)counts[v];
        r.n_groups = (r.n_entries + DRT_PIXELS_WAVE - 1) / DRT_PIXELS_WAVE;
        const uint64_t waves = (uint64_t)r.n_groups * n_ranges;
        r.n_blocks = (uint32_t)((waves + DRT_PIXELS_BLOCK_WAVES - 1) / DRT_PIXELS_BLOCK_WAVES);
        r.fpart_at = g.fpart_doubles;
        r.counts_at = g.count_words;
        g.n_blocks += r.n_blocks;
        g.n_entries += r.n_entries;
        g.n_waves += waves;
        g.fpart_doubles += (uint64_t)n_ranges * 3 * r.n_entries;
        g.count_words += 2 * waves;
    }
}
