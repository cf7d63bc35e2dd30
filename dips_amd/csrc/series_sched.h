// series_sched.h -- the schedules of the series and the regional products as
// functions of plain numbers: how many waves a launch runs and how its frames
// are cut into parts.  No HIP here (tests/test_sched_cpu.py compiles this
// header alone with g++): what needs the runtime -- the wave slots a kernel
// has resident (series_host.h resident_waves) and the parsed
// DIPS_PIXEL_PART_FRAMES pin -- comes in as a value or a callable.
#pragma once

#include <algorithm>
#include <cstdint>

#include "series_slots.h"

namespace dips_sched {

// The schedule of one fast launch.  ok false: the generic kernel runs.
struct Geom {
    bool ok = false;
    bool small_tile = false;      // background / Sigma-Delta: tiles of 64 vecs
    uint32_t tiles_per_cell = 0;  // grid
    uint32_t part_frames = 0;     // frames per part (series: 0 = contiguous ranges)
    uint32_t parts = 0;
    uint64_t n_tiles = 0, n_waves = 0, blocks = 0;
};

// The series adds its item count and the split between the vectorised and
// the generic kernel.
struct FastGeom : Geom {
    uint64_t items = 0;
    uint64_t vec_bytes = 0;  // whole vecs of a frame (the vectorised kernel's range)
    uint64_t tail_px0 = 0;   // first pixel of the ragged tail (npx: none)
};

struct PartCut {
    uint32_t part_frames = 0;  // 0: the batch is left alone
    uint64_t n_waves = 0;
};

// The part-major schedule of the series kernels (series_v2.hip,
// series_gray.hip): the batch's frames cut into P parts of L, items (part,
// tile) dealt to the waves with stride n_waves, so that concurrent waves read
// adjacent tiles of the same frames.  Measured 0.3-1.1 points above one
// contiguous (tile, frame) range per wave on each of four frame buffers,
// 0.7-1.2 % less energy per frame (tools/alloc_policy_ab.hip,
// profiles/r03/alloc/); per-frame 77.3 % against 75.4 % of 8 TB/s, 'overall'
// 74.1 against 72.05 % (profiles/r03/parts/, profiles/r04/l/).  Parts of at
// least 128 frames (each item re-reads its reference tile: +1/L of the
// traffic), P from the one that gives every resident wave slot an item up to
// 4x that: the smallest whose items fill >= 98 % of the slots (k items per
// slot), else the best-filling one (98 rather than 95 %: 8K's 3 parts fill
// 99.9 % against 2 parts' 97.4 %, +0.5 points in alternated runs,
// profiles/r05/ab_fill/; every other config keeps its part count); the
// waves then get ceil(items / n_waves) or one fewer items each (4K RGB8, 5000
// frames, U = 5: L = 1000, 4,050 waves).
// Batches of fewer than 256 frames keep the contiguous ranges.
inline PartCut part_geometry(uint64_t n_tiles, uint64_t n_frames, uint64_t resident) {
    PartCut c;
    if (n_frames < 256 || n_tiles == 0 || resident == 0) return c;
    const uint64_t p_min = std::max<uint64_t>((resident + n_tiles - 1) / n_tiles, (n_frames + 1249) / 1250);
    const uint64_t p_max = std::min<uint64_t>(4 * p_min, n_frames / 128);
    if (p_max < p_min) return c;
    uint64_t best_p = 0;
    double best_fill = -1.0;
    for (uint64_t p = p_min; p <= p_max; ++p) {
        const uint64_t L = (n_frames + p - 1) / p;
        const uint64_t parts = (n_frames + L - 1) / L;
        const uint64_t items = parts * n_tiles;
        const uint64_t k = (items + resident - 1) / resident;
        const double fill = (double)items / (double)(k * resident);
        if (fill > best_fill + 1e-9) {
            best_fill = fill;
            best_p = p;
        }
        if (fill >= 0.98) break;
    }
    const uint64_t L = (n_frames + best_p - 1) / best_p;
    const uint64_t items = ((n_frames + L - 1) / L) * n_tiles;
    const uint64_t k = (items + resident - 1) / resident;
    c.part_frames = (uint32_t)L;
    c.n_waves = (items + k - 1) / k;
    return c;
}

// The RGB8 / RGBA8 series kernel (and the f32 GRAY8 one): `ppv` pixels per
// vec, `unroll` vecs per lane, `resident` wave slots (0: no such kernel).
inline FastGeom fast_geometry(uint32_t width, uint32_t height, uint32_t n_frames, int C, int ppv, int unroll,
                              uint64_t resident) {
    FastGeom g;
    const uint64_t npx = (uint64_t)width * height;
    const uint64_t fb = npx * (uint64_t)C;
    // any alignment and pixel count: the vectorised kernel takes the whole
    // vecs of every frame (unaligned frames through unaligned buffer loads,
    // exact on gfx950: tests/test_gpu_series.py::test_unaligned_device_batches), the generic kernel the
    // < ppv trailing pixels
    const uint64_t nvec = npx / (uint64_t)ppv;
    if (nvec == 0 || fb >= (1ull << 31) || n_frames == 0) return g;
    const uint64_t U = (uint64_t)unroll;
    g.vec_bytes = nvec * (uint64_t)ppv * (uint64_t)C;
    g.tail_px0 = nvec * (uint64_t)ppv;
    g.n_tiles = (nvec + 64 * U - 1) / (64 * U);
    g.items = g.n_tiles * n_frames;
    if (resident == 0) return g;
    g.n_waves = g.items < resident ? g.items : resident;
    if (C == 3 || C == 4) {
        const PartCut c = part_geometry(g.n_tiles, n_frames, resident);
        if (c.part_frames != 0) {
            g.part_frames = c.part_frames;
            g.n_waves = c.n_waves;
        }
    }
    g.blocks = (g.n_waves + 3) / 4;
    g.ok = g.n_tiles < (1ull << 32) && g.blocks < (1ull << 31);
    return g;
}

// The GRAY8 table kernel (series_gray.hip): 16 pixels per vec, workgroups of
// `group_waves` waves, one per CU (the tables fill its LDS).
inline FastGeom gray_lut_geometry(uint32_t width, uint32_t height, uint32_t n_frames, int unroll,
                                  uint32_t group_waves, bool per_frame, uint64_t resident) {
    FastGeom g;
    const uint64_t npx = (uint64_t)width * height;
    const uint64_t nvec = npx / 16u;
    if (nvec == 0 || npx >= (1ull << 31) || n_frames == 0) return g;
    const uint64_t U = (uint64_t)unroll;
    g.vec_bytes = nvec * 16u;
    g.tail_px0 = nvec * 16u;
    g.n_tiles = (nvec + 64 * U - 1) / (64 * U);
    g.items = g.n_tiles * n_frames;
    g.n_waves = g.items < resident ? g.items : resident;
    // 'per-frame' batches: the part-major schedule, as for RGB8 (part_geometry)
    if (per_frame) {
        const PartCut c = part_geometry(g.n_tiles, n_frames, resident);
        if (c.part_frames != 0) {
            g.part_frames = c.part_frames;
            g.n_waves = c.n_waves;
        }
    }
    g.blocks = (g.n_waves + group_waves - 1) / group_waves;
    g.ok = g.n_tiles < (1ull << 32) && g.blocks < (1ull << 31);
    return g;
}

// Part rule of the grid and the mask: as part_geometry cuts the frames, or
// for the batches it leaves alone as many parts of >= 16 frames as give every
// wave slot an item.
inline void cut_parts_to_fill(Geom& q, uint64_t n_tiles, uint32_t n_frames, uint64_t resident) {
    const PartCut c = part_geometry(n_tiles, n_frames, resident);
    if (c.part_frames != 0) {
        q.part_frames = c.part_frames;
        q.parts = (uint32_t)((n_frames + q.part_frames - 1) / q.part_frames);
        q.n_waves = c.n_waves;
    } else {
        const uint64_t want = (resident + n_tiles - 1) / n_tiles;
        const uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>(want, n_frames / 16u));
        q.part_frames = (uint32_t)((n_frames + parts - 1) / parts);
        q.parts = (uint32_t)((n_frames + q.part_frames - 1) / q.part_frames);
        q.n_waves = std::min((uint64_t)q.parts * n_tiles, resident);
    }
}

// Part rule of the pixel sums and the change times: one part -- every wave
// owns all frames of its pixels -- unless the tiles fill less than 98 % of the
// wave slots (part_geometry's fill rule: a second part would buy 2 % and cost
// the memset and atomics, or the combine), then enough parts of >= 16 frames
// to give every slot an item; at most `max_parts` parts, at most
// `max_part_frames` frames in one (0: no cap).  `pin` (DIPS_PIXEL_PART_FRAMES,
// 0: none) pins the part length where those two limits admit it (the tests
// run the accumulators at their limit on a small frame with it).
inline void cut_parts_unless_full(Geom& q, uint64_t n_tiles, uint32_t n_frames, uint64_t resident,
                                  uint64_t max_parts, uint64_t max_part_frames, uint64_t pin) {
    const uint64_t want = n_tiles * 100u >= resident * 98u ? 1u : (resident + n_tiles - 1) / n_tiles;
    uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>(std::min(want, max_parts), n_frames / 16u));
    if (max_part_frames != 0)
        parts = std::max<uint64_t>(parts, ((uint64_t)n_frames + max_part_frames - 1) / max_part_frames);
    q.part_frames = (uint32_t)((n_frames + parts - 1) / parts);
    if (pin >= 1 && (max_part_frames == 0 || pin <= max_part_frames) &&
        ((uint64_t)n_frames + pin - 1) / pin <= max_parts)
        q.part_frames = (uint32_t)std::min<uint64_t>(pin, n_frames);
    q.parts = (uint32_t)((n_frames + q.part_frames - 1) / q.part_frames);
}

// What every regional product's fast kernel refuses: frames of 2^31 bytes or
// more, no frames, 2^28 frames.
inline bool region_batch_ok(uint64_t frame_bytes, uint32_t n_frames) {
    return frame_bytes < (1ull << 31) && n_frames != 0 && n_frames < (1u << 28);
}

// vecs of the region rows padded to whole mask words (8 vecs of 4 pixels each)
inline uint64_t mask_words_per_row(uint32_t roi_w) { return ((uint64_t)roi_w + 31u) / 32u; }

// Geometry of the fast grid kernel: every cell owns the tile count of the
// largest cell; a persistent grid of occupancy x CUs waves (fast_geometry's
// sizing), frames cut by cut_parts_to_fill.  Refused (the generic kernel
// runs): region_batch_ok's cases and grids whose records would outweigh the
// batch -- cells of a few pixels, where a 16-byte record per (tile, frame) is
// most of the traffic.
inline Geom grid_geometry(uint64_t frame_bytes, uint32_t n_frames, int unroll, uint32_t roi_w, uint32_t roi_h,
                          uint32_t rows, uint32_t cols, uint64_t resident) {
    Geom q;
    if (!region_batch_ok(frame_bytes, n_frames)) return q;
    const uint64_t vpt = 64u * (uint64_t)unroll;  // vecs per tile
    const uint64_t max_w = ((uint64_t)roi_w + cols - 1) / cols, max_h = ((uint64_t)roi_h + rows - 1) / rows;
    const uint64_t tpc = (((max_w + 3) / 4) * max_h + vpt - 1) / vpt;
    const uint64_t n_cells = (uint64_t)rows * cols;
    const uint64_t n_tiles = n_cells * tpc;
    if (n_tiles >= (1ull << 31)) return q;
    const uint64_t rec_bytes = n_tiles * n_frames * 16u;
    if (rec_bytes > (64ull << 20) && rec_bytes > frame_bytes * n_frames) return q;
    if (resident == 0) return q;
    cut_parts_to_fill(q, n_tiles, n_frames, resident);
    q.blocks = (q.n_waves + 3) / 4;
    q.tiles_per_cell = (uint32_t)tpc;
    q.n_tiles = n_tiles;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Geometry of the fast per-pixel kernel: a persistent grid of occupancy x CUs
// waves over items (frame part, tile), parts by cut_parts_unless_full with at
// most `max_part` frames in one (what the in-register accumulators hold);
// several parts add their shares with atomics.  Refused: region_batch_ok's
// cases.
inline Geom pix_geometry(uint64_t frame_bytes, uint32_t n_frames, int unroll, uint32_t roi_w, uint32_t roi_h,
                         uint64_t resident, uint32_t max_part, uint64_t pin) {
    Geom q;
    if (!region_batch_ok(frame_bytes, n_frames)) return q;
    const uint64_t vpt = 64u * (uint64_t)unroll;  // vecs per tile
    const uint64_t n_tiles = ((((uint64_t)roi_w + 3) / 4) * roi_h + vpt - 1) / vpt;
    if (resident == 0 || n_tiles == 0 || n_tiles >= (1ull << 31)) return q;
    cut_parts_unless_full(q, n_tiles, n_frames, resident, UINT64_MAX, max_part, pin);
    q.n_tiles = n_tiles;
    q.n_waves = std::min((uint64_t)q.parts * n_tiles, resident);
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Geometry of the fast mask kernel: a persistent grid of occupancy x CUs
// waves over items (frame part, tile), a tile = 64 * unroll vecs of the
// region rows padded to whole mask words.  Parts by cut_parts_to_fill; no
// upper cap on a part (nothing is accumulated), and every word has one writer
// whatever the part count.  Refused: region_batch_ok's cases, regions whose
// padded rows hold 2^31 vecs or more.
inline Geom mask_geometry(uint64_t frame_bytes, uint32_t n_frames, int unroll, uint32_t roi_w, uint32_t roi_h,
                          uint64_t resident) {
    Geom q;
    if (!region_batch_ok(frame_bytes, n_frames)) return q;
    const uint64_t vpt = 64u * (uint64_t)unroll;  // vecs per tile
    const uint64_t nvec8 = 8u * mask_words_per_row(roi_w) * roi_h;
    if (nvec8 >= (1ull << 31)) return q;
    const uint64_t n_tiles = (nvec8 + vpt - 1) / vpt;
    if (resident == 0 || n_tiles == 0) return q;
    cut_parts_to_fill(q, n_tiles, n_frames, resident);
    q.n_tiles = n_tiles;
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// The shortest part of the temporal vote at window k (mask_vote.hip): a part
// reads the k - 1 frames before it to prime its counters, so parts of at
// least 8 (k - 1) frames, and of at least cut_parts_to_fill's 16, keep those
// reads at or below 1 / 8 of the frames read as input.
inline uint32_t vote_min_part_frames(uint32_t window) { return std::max(16u, 8u * (window - 1u)); }

// Geometry of the temporal vote on a mask (mask_vote.hip): a persistent grid
// of occupancy x CUs waves over items (frame part, tile), a tile = 64 *
// `words` mask words of the frame.  Parts by cut_parts_to_fill, as for the
// mask itself (every word has one writer whatever the part count), then made
// no shorter than vote_min_part_frames: every part but the last has at least
// that many frames, so a part other than the first starts at or after frame
// k - 1 and primes from input frames alone.  `frame_words` > 0, `window` >= 1.
// Refused: no frames, 2^31 frames or more.
inline Geom vote_geometry(uint64_t frame_words, uint32_t n_frames, uint32_t window, int words, uint64_t resident) {
    Geom q;
    const uint64_t wpt = 64u * (uint64_t)words;  // words per tile
    const uint64_t n_tiles = (frame_words + wpt - 1) / wpt;
    if (n_frames == 0 || n_frames >= (1u << 31) || resident == 0 || n_tiles == 0 || n_tiles >= (1ull << 31)) return q;
    cut_parts_to_fill(q, n_tiles, n_frames, resident);
    const uint32_t lmin = vote_min_part_frames(window);
    if (q.part_frames < lmin) {
        const uint32_t parts = std::max(1u, n_frames / lmin);
        q.part_frames = (uint32_t)(((uint64_t)n_frames + parts - 1) / parts);
        q.parts = (uint32_t)(((uint64_t)n_frames + q.part_frames - 1) / q.part_frames);
        q.n_waves = std::min((uint64_t)q.parts * n_tiles, resident);
    }
    q.n_tiles = n_tiles;
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Geometry of the change times and per-pixel sums of a mask (mask_stats.hip
// mask_times_kernel): a persistent grid of occupancy x CUs waves over items
// (frame part, tile), a tile = 64 lane slots of `frame_slots` (a slot is the
// few pixels of one mask byte that a lane owns).  Parts by
// cut_parts_unless_full, as for the change times of the frames: one part
// unless the tiles leave wave slots empty, then parts of >= 16 frames, at most
// what keeps the summaries (`summary_bytes` per part) within `parts_bytes`.
// The parts [p L, min(n, (p + 1) L)) tile the frames and the combine folds
// them in order, so the result does not depend on the cut.  Refused: no
// frames, no slots, 2^31 tiles or more.
inline Geom mask_times_geometry(uint64_t frame_slots, uint32_t n_frames, uint64_t summary_bytes, uint64_t parts_bytes,
                                uint64_t resident) {
    Geom q;
    const uint64_t n_tiles = (frame_slots + 63u) / 64u;
    if (n_frames == 0 || resident == 0 || n_tiles == 0 || n_tiles >= (1ull << 31) || summary_bytes == 0) return q;
    const uint64_t max_parts = std::max<uint64_t>(1, parts_bytes / summary_bytes);
    cut_parts_unless_full(q, n_tiles, n_frames, resident, max_parts, 0, 0);
    q.n_tiles = n_tiles;
    q.n_waves = std::min((uint64_t)q.parts * n_tiles, resident);
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Geometry of the grid counts of a mask (mask_stats.hip mask_counts_kernel).
// An item is (frame, grid row, chunk of at most `chunk_cells` grid columns,
// band of at most band_rows mask rows of that grid row): a block sums its
// item per cell in registers and LDS and adds each cell once.  The bands cut
// the tallest grid row, ceil(roi_h / rows) mask rows; a band that starts
// below a shorter grid row's end is empty.  Enough bands to give every
// resident block two items, none thinner than `min_band_words` mask words of
// its chunk.  bands == 1: a cell has one writer and is stored; else the
// blocks add with integer atomics onto cleared counts.  Refused: no frames,
// an empty region or grid, a grid finer than the region.
struct CountsGeom {
    bool ok = false;
    uint32_t col_chunks = 0;  // chunks of grid columns
    uint32_t bands = 0;       // bands per grid row
    uint32_t band_rows = 0;   // mask rows per band
    uint64_t items = 0, blocks = 0;
};

inline CountsGeom mask_counts_geometry(uint32_t roi_w, uint32_t roi_h, uint32_t rows, uint32_t cols, uint32_t n_frames,
                                       uint32_t chunk_cells, uint32_t min_band_words, uint64_t resident_blocks) {
    CountsGeom q;
    if (roi_w == 0 || roi_h == 0 || rows == 0 || cols == 0 || rows > roi_h || cols > roi_w || n_frames == 0 ||
        chunk_cells == 0 || min_band_words == 0 || resident_blocks == 0)
        return q;
    q.col_chunks = (uint32_t)(((uint64_t)cols + chunk_cells - 1) / chunk_cells);
    const uint64_t base = (uint64_t)n_frames * rows * q.col_chunks;
    const uint64_t max_h = ((uint64_t)roi_h + rows - 1) / rows;
    const uint64_t chunk_words = (mask_words_per_row(roi_w) + q.col_chunks - 1) / q.col_chunks;
    const uint64_t min_rows = std::max<uint64_t>(1, ((uint64_t)min_band_words + chunk_words - 1) / chunk_words);
    const uint64_t want = (2 * resident_blocks + base - 1) / base;
    const uint64_t bands = std::max<uint64_t>(1, std::min(want, (max_h + min_rows - 1) / min_rows));
    q.band_rows = (uint32_t)((max_h + bands - 1) / bands);
    q.bands = (uint32_t)((max_h + q.band_rows - 1) / q.band_rows);
    q.items = base * q.bands;
    q.blocks = std::min(q.items, 2 * resident_blocks);
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Geometry of the fast change-times kernel: pix_geometry's without a cap on
// the frames of a part (the state is u32 indices and run lengths, nothing
// overflows), and with the parts limited to what keeps their summaries (20
// bytes per pixel and part) within `parts_bytes`.  resident_of(multi): the
// wave slots of the kernel's several-parts or its one-part form (0: no such
// kernel).  Refused: region_batch_ok's cases.
template <typename ResidentOf>
Geom times_geometry(uint64_t frame_bytes, uint32_t n_frames, int unroll, uint32_t roi_w, uint32_t roi_h,
                    uint64_t parts_bytes, uint64_t pin, ResidentOf&& resident_of) {
    Geom q;
    if (!region_batch_ok(frame_bytes, n_frames)) return q;
    const uint64_t vpt = 64u * (uint64_t)unroll;  // vecs per tile
    const uint64_t n_tiles = ((((uint64_t)roi_w + 3) / 4) * roi_h + vpt - 1) / vpt;
    if (n_tiles == 0 || n_tiles >= (1ull << 31)) return q;
    const uint64_t sum_bytes = 20u * (uint64_t)roi_w * roi_h;  // one part's summaries
    const uint64_t max_parts = std::max<uint64_t>(1, parts_bytes / sum_bytes);
    // the slots of the several-parts form (its fifth register per pixel may
    // cost it occupancy): that is the form the parts would run
    const uint64_t res_p = resident_of(true);
    if (res_p == 0) return q;
    cut_parts_unless_full(q, n_tiles, n_frames, res_p, max_parts, 0, pin);
    const uint64_t resident = resident_of(q.parts > 1);
    if (resident == 0) return q;
    q.n_tiles = n_tiles;
    q.n_waves = std::min((uint64_t)q.parts * n_tiles, resident);
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Geometry of the fast background and Sigma-Delta kernels: a persistent grid
// of occupancy x CUs waves over the tiles of the region rows padded to whole
// mask words.  One part always (the recurrence is sequential in t), so tiles
// are the only parallelism: a region whose tiles of 64 * unroll vecs would
// fill under half of the wave slots takes tiles of 64 vecs instead.
// (Choosing the tile by how full the rounds of resident waves are -- 4K RGB8:
// 16,200 small tiles fill two rounds to 98.9 %, 8,100 large ones to 56.5 % --
// measured 3-5 % slower at 4K than this rule, DESIGN.md.)
// resident_of(small_tile): the wave slots of that kernel form (0: no such
// kernel).  Refused: region_batch_ok's cases, regions whose padded rows hold
// 2^31 vecs or more.
template <typename ResidentOf>
Geom background_geometry(uint64_t frame_bytes, uint32_t n_frames, int unroll, uint32_t roi_w, uint32_t roi_h,
                         ResidentOf&& resident_of) {
    Geom q;
    if (!region_batch_ok(frame_bytes, n_frames)) return q;
    const uint64_t nvec8 = 8u * mask_words_per_row(roi_w) * roi_h;
    if (nvec8 == 0 || nvec8 >= (1ull << 31)) return q;
    uint64_t vpt = 64u * (uint64_t)unroll;  // vecs per tile
    uint64_t resident = resident_of(false);
    if (resident == 0) return q;
    if (unroll > 1 && 2u * ((nvec8 + vpt - 1) / vpt) < resident) {
        q.small_tile = true;
        vpt = 64u;
        resident = resident_of(true);
        if (resident == 0) return q;
    }
    q.n_tiles = (nvec8 + vpt - 1) / vpt;
    q.n_waves = std::min(q.n_tiles, resident);
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// The vecs (4 pixels) a fast regional kernel leaves out: those that
// vec_crosses_frame_end (series_slots.h, the kernels' own test) finds to read
// past the frame's end, i.e. that start within 3 pixels of it.  Vecs of
// a row are 4 pixels apart and a full vec ends inside its row, so that is at
// most the partial last vec of each of the region's last rows: one row for
// frames 3 or more pixels wide, up to 4 for narrower ones.  row(r, i0) is
// called for each such region row r, the last first, with the vec's first
// column i0 within the region; a status other than T{} ends the walk and is
// returned.
template <typename Row>
auto for_frame_end_tail_rows(uint32_t width, uint32_t height, uint32_t roi_x, uint32_t roi_y, uint32_t roi_w,
                             uint32_t roi_h, Row&& row) -> decltype(row(0u, 0u)) {
    using T = decltype(row(0u, 0u));
    if (roi_w % 4u == 0u) return T{};
    const uint32_t i0 = (roi_w - 1u) & ~3u;  // the last vec of a region row
    const uint64_t npx = (uint64_t)width * height;
    for (uint32_t r = roi_h; r-- > 0 && roi_h - r <= 4u;) {
        // in pixels: it and every earlier row fit
        if (!vec_crosses_frame_end<uint64_t>((uint64_t)(roi_y + r) * width + roi_x + i0, 4u, npx)) break;
        const T st = row(r, i0);
        if (st != T{}) return st;
    }
    return T{};
}

// The same for a rows x cols grid of cells over the region {x, y, w, h}
// (series_grid.hip: every cell is a region of its own): the partial last vec
// of a cell row that crosses the frame's end.  These lie in the frame's last
// row, and in frames narrower than 3 pixels in up to three rows before it;
// cell edges grow with the column, so at most three cells of a row qualify.
// cell_rect(row, col) gives a cell's rectangle {x, y, w, h}; tail(row, col,
// x0, y, n) is called for the n <= 3 pixels from frame column x0 of frame row
// y that cell (row, col) leaves out; a status other than T{} ends the walk.
template <typename CellRect, typename Tail>
auto for_grid_frame_end_tails(uint32_t width, uint32_t height, uint32_t y0, uint32_t h, uint32_t rows, uint32_t cols,
                              CellRect&& cell_rect, Tail&& tail) -> decltype(tail(0u, 0u, 0u, 0u, 0u)) {
    using T = decltype(tail(0u, 0u, 0u, 0u, 0u));
    const uint64_t npx = (uint64_t)width * height;
    // crosses(y, x): a vec that started at frame pixel (x, y) would cross the
    // frame's end.  Asked of the last pixel of a row or of a cell it is a
    // bound, not a real vec: no vec of that row / cell starts later
    auto crosses = [&](uint64_t y, uint64_t x) { return vec_crosses_frame_end<uint64_t>(y * width + x, 4u, npx); };
    uint32_t crow = rows - 1u;  // the grid row of frame row y
    for (uint32_t y = y0 + h; y-- > y0;) {
        if (!crosses(y, (uint64_t)width - 1u)) break;  // every vec of this and the earlier rows fits
        while (cell_rect(crow, 0u).y > y) --crow;
        for (uint32_t c = cols; c-- > 0;) {
            const auto rc = cell_rect(crow, c);
            if (!crosses(y, (uint64_t)rc.x + rc.w - 1u)) break;  // so does every vec of the earlier columns
            const uint32_t x0 = rc.x + ((rc.w - 1u) & ~3u);      // the cell row's last vec
            if (rc.w % 4u == 0u || !crosses(y, x0)) continue;
            const T st = tail(crow, c, x0, y, rc.x + rc.w - x0);
            if (st != T{}) return st;
        }
    }
    return T{};
}

}  // namespace dips_sched
