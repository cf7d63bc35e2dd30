// dips_kernels.h -- kernel argument blocks and host launchers (internal).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dips_hip.h"

namespace dips {

// Unroll (vecs per lane) of the fast series kernel; a tile = 64 * U vecs.
// A dispatch holds fewer than 2^32 work-items (the grid size is a 32-bit
// count of work-items, not of workgroups): one-dimensional launches of
// 256-thread workgroups over n items must check n against this, or the grid
// wraps and the launch silently runs only the remainder.
constexpr bool fits_grid256(uint64_t n) { return n <= (1ull << 32) - 256u; }

constexpr int kUnrollRGB = 4;   // 1024 px / wave / frame for RGB8 and RGBA8
constexpr int kUnrollGray = 2;  // 2048 px / wave / frame for GRAY8
constexpr int kUnrollV2 = 4;    // series_v2_kernel RGBA8: 1024 px / wave / frame
constexpr int kUnrollV2Rgb = 5; // series_v2_kernel RGB8: 1280 px / wave / frame (12-B vecs: 5 x 64 x 12 < 4096)
template <int C>
constexpr int v2_unroll() { return C == 3 ? kUnrollV2Rgb : kUnrollV2; }
// series_gray_lut_kernel: 64 * 16 * U px / wave / frame (U = 4: 4K gray8
// 61.9-62.1 % of 8 TB/s vs 60.4-60.6 % at U = 2, profiles/r02_gray_lut_unroll.jsonl;
// confirmed in one process with the final kernel: U = 4 65.5-65.9 %, U = 3
// 64.9-65.7 %, U = 2 63.6-63.9 %, profiles/r02_gray_variant_ab.jsonl)
#ifndef DIPS_UNROLL_GRAY_LUT
#define DIPS_UNROLL_GRAY_LUT 4
#endif
constexpr int kUnrollGrayLut = DIPS_UNROLL_GRAY_LUT;
constexpr uint32_t kGrayLutWaves = 16;  // its waves per workgroup (one 1024-thread group per CU)
constexpr size_t kGrayLutBytes = 131072;  // its T_d / T_c tables
constexpr size_t kGrayLutAllocBytes = kGrayLutBytes + 256;  // + layout 5's band word (series_gray.hip)
// layout 4 (auto) keeps layout 5's table + band word and layout 2's after it
// Prefetch depth: frames of loads each wave keeps in flight.
#ifndef DIPS_DEPTH_RGB
#define DIPS_DEPTH_RGB 2
#endif
#ifndef DIPS_DEPTH_GRAY
#define DIPS_DEPTH_GRAY 2
#endif
constexpr int kDepthRGB = DIPS_DEPTH_RGB;
constexpr int kDepthGray = DIPS_DEPTH_GRAY;

struct SeriesArgs {
    const uint8_t* frames;   // n_frames * frame_bytes, contiguous
    const uint8_t* ref0;     // overall: reference; per-frame: predecessor of frame 0
    uint8_t* dmap;           // optional |F - R| map (same layout as frames)
    uint64_t* partials;      // [n_tiles][n_frames] x 16-byte records
    uint64_t items;          // n_tiles * n_frames
    uint32_t frame_bytes;    // frame stride in bytes (W * H * C; any alignment)
    uint32_t vec_bytes;      // bytes of whole vecs per frame (the descriptor range; the
                             // < pixels_per_vec trailing pixels go to the generic kernel)
    uint32_t n_frames;
    uint32_t n_tiles;
    uint32_t n_waves;
    float thr;               // threshold in kernel units: series_threshold()
    uint32_t screen;         // screened series_v2 (series_v2_screen.h): series_screen_level(tau), >= 0 there
    const void* lut;         // GRAY8 table kernel: T_d / T_c bytes (series_gray.hip), 128 KiB
    uint32_t part_frames;    // frames per part of the part-major schedule (series_v2 SCHED = 1)
    // GRAY8 table kernel, layout 4: each workgroup samples its waves' first
    // items and takes layout 5 when band >= probe_min / 1024 of the sampled
    // pixels and (band >= probe_hi / 1024 of them or the waves' byte spreads
    // average >= probe_spread), else layout 2 (probe_min 0: always 5, > 1024:
    // always 2 -- the pinned layouts)
    uint32_t probe_min;
    uint32_t probe_hi;
    uint32_t probe_spread;
    uint64_t* zero;          // when set: the kernel zeroes zero[0 .. zero_n) (the series, before its
    uint32_t zero_n;         // reduce's atomics; replaces a separate fill launch)
};

struct GenericArgs {
    const uint8_t* frames;
    const uint8_t* ref0;
    uint8_t* dmap;
    dips_series_entry* series;
    uint64_t frame_bytes;
    uint64_t n_px;
    uint64_t px0;            // first pixel of each frame to process (the fast kernel's ragged tail)
    uint32_t n_frames;
    uint32_t blocks_per_frame;
    uint32_t mode;
    uint32_t chroma;
    float tau;
};

// A rows x cols grid over the region of interest {x, y, w, h} of a frame
// (dips_diff_series_grid).  Column c covers [x + c*w/cols, x + (c+1)*w/cols),
// rows likewise -- the split dips_shard_range makes of a frame count; host
// and kernels take every cell rectangle from grid_cell_rect.
struct GridSpec {
    uint32_t x, y, w, h;
    uint32_t rows, cols;
};

struct GridRect {
    uint32_t x, y, w, h;
};

__host__ __device__ inline uint32_t grid_edge(uint32_t x0, uint32_t extent, uint32_t n, uint32_t i) {
    return x0 + (uint32_t)((uint64_t)i * extent / n);
}

__host__ __device__ inline GridRect grid_cell_rect(const GridSpec& g, uint32_t row, uint32_t col) {
    GridRect r;
    r.x = grid_edge(g.x, g.w, g.cols, col);
    r.y = grid_edge(g.y, g.h, g.rows, row);
    r.w = grid_edge(g.x, g.w, g.cols, col + 1) - r.x;
    r.h = grid_edge(g.y, g.h, g.rows, row + 1) - r.y;
    return r;
}

// series_grid_kernel (series_grid.hip): a tile = 64 * U vecs of ONE cell, a
// vec = 4 horizontally consecutive pixels of one cell row (the last vec of a
// row may hold fewer), (row, vec-in-row) flattened over the cell.  Every cell
// owns tiles_per_cell tile ids (the count of the largest cell; the ids past a
// smaller cell's last tile do nothing and have no records).
struct GridArgs {
    const uint8_t* frames;   // n_frames * frame_bytes, contiguous
    const uint8_t* ref0;     // overall: reference; per-frame: predecessor of frame 0
    uint64_t* partials;      // [n_cells * tiles_per_cell][n_frames] x 16-byte records
    uint64_t* zero;          // the cells array, zeroed by the kernel before the reduce's atomics
    uint32_t zero_n;         // its u64 count (4 * n_frames * n_cells)
    uint32_t frame_bytes;
    uint32_t width;          // frame width in pixels (the row pitch)
    uint32_t n_frames;
    uint32_t tiles_per_cell;
    uint32_t n_tiles;        // n_cells * tiles_per_cell
    uint32_t n_waves;
    uint32_t part_frames;    // frames per part of the part-major schedule (>= 1)
    float thr;               // series_threshold()
    GridSpec g;
};

// grid_generic_kernel: one thread per pixel of a cell, the reference's own
// intensity form, u64 atomics into cells[t * out_stride + out_base + cell].
struct GridGenericArgs {
    const uint8_t* frames;
    const uint8_t* ref0;
    dips_series_entry* cells;
    uint64_t frame_bytes;
    uint32_t width;
    uint32_t n_frames;
    uint32_t segs_per_cell;  // 256-pixel segments of the largest cell
    uint32_t out_stride;     // entries per frame of the cells array
    uint32_t out_base;       // first entry of this launch's cells within a frame's entries
    uint32_t mode;
    uint32_t chroma;
    float tau;
    GridSpec g;
};

// series_pixels_kernel (series_pixels.hip): the series summed over time per
// pixel of a region.  A tile = 64 * kUnrollPix vecs of the region in the grid
// kernel's addressing (one cell = the region); a wave keeps its tile and
// walks a part of the frames with per-pixel accumulators in registers.
#ifndef DIPS_UNROLL_PIX
#define DIPS_UNROLL_PIX 2
#endif
constexpr int kUnrollPix = DIPS_UNROLL_PIX;  // vecs per lane: 512 px / wave / frame
constexpr uint32_t kPixMaxPart = 2048;       // frames per part the packed SJ | count << 20 word holds
struct PixArgs {
    const uint8_t* frames;   // n_frames * frame_bytes, contiguous
    const uint8_t* ref0;     // overall: reference; per-frame: predecessor of frame 0
    dips_series_entry* sums; // roi.w * roi.h entries
    uint32_t frame_bytes;
    uint32_t width;          // frame width in pixels (the row pitch)
    uint32_t n_frames;
    uint32_t n_tiles;
    uint32_t n_waves;
    uint32_t part_frames;    // frames per part (1 .. kPixMaxPart)
    uint32_t out_mode;       // 0 store (one part), 1 load-add-store (one part, accumulate), 2 u64 atomic adds
    float thr;               // series_threshold()
    GridRect roi;
};

// pixels_generic_kernel: one thread per pixel of rect (inside the region)
// walks the frames; sums[(py - roi_y) * roi_w + px - roi_x] written or added to.
struct PixGenericArgs {
    const uint8_t* frames;
    const uint8_t* ref0;
    dips_series_entry* sums;
    uint64_t frame_bytes;
    uint32_t width;
    uint32_t n_frames;
    uint32_t mode;
    uint32_t chroma;
    float tau;
    uint32_t accumulate;
    uint32_t roi_x, roi_y, roi_w;
    GridRect rect;
};

// series_mask_kernel (series_mask.hip): the per-frame change mask, one bit
// per pixel of a region.  The vecs of a region row are padded to a multiple
// of 8 (one mask word = 8 vecs = 32 pixels), (row, vec) flattened over the
// padded rows: flat vec i belongs to flat mask word i >> 3 of the frame.
#ifndef DIPS_UNROLL_MASK
#define DIPS_UNROLL_MASK 4
#endif
constexpr int kUnrollMask = DIPS_UNROLL_MASK;  // vecs per lane: 1024 px / wave / frame
struct MaskArgs {
    const uint8_t* frames;   // n_frames * frame_bytes, contiguous
    const uint8_t* ref0;     // overall: reference; per-frame: predecessor of frame 0
    uint8_t* mask;           // n_frames * mask_frame_bytes, 4-byte aligned
    uint32_t frame_bytes;
    uint32_t mask_frame_bytes;  // roi.h * 4 * ceil(roi.w / 32)
    uint32_t width;          // frame width in pixels (the row pitch)
    uint32_t n_frames;
    uint32_t n_tiles;
    uint32_t n_waves;
    uint32_t part_frames;    // frames per part (>= 1)
    float thr;               // series_threshold(C, tau, 0)
    GridRect roi;
};

// mask_generic_kernel: one thread per (frame, mask word) of rows [row0, row0
// + n_rows) x words [word0, word0 + n_words) of the region's mask, frames
// [t0, t0 + n_frames) of the batch.
struct MaskGenericArgs {
    const uint8_t* frames;
    const uint8_t* ref0;
    uint8_t* mask;
    uint64_t frame_bytes;
    uint64_t mask_frame_bytes;
    uint32_t width;
    uint32_t t0, n_frames;
    uint32_t mode;
    uint32_t chroma;
    float tau;
    uint32_t row0, n_rows, word0, n_words;
    GridRect roi;
};

// series_times_kernel (series_times.hip): the change times per pixel of a
// region -- first, last, longest run, current run, four u32 planes of roi.w *
// roi.h.  Tiles as series_pixels_kernel's; a wave keeps its tile and walks a
// part of the frames with the state of its pixels in registers.
#ifndef DIPS_UNROLL_TIMES
#define DIPS_UNROLL_TIMES 2
#endif
constexpr int kUnrollTimes = DIPS_UNROLL_TIMES;  // vecs per lane: 512 px / wave / frame
struct TimesArgs {
    const uint8_t* frames;   // n_frames * frame_bytes, contiguous
    const uint8_t* ref0;     // overall: reference; per-frame: predecessor of frame 0
    uint32_t* out;           // one part: the four planes; several: parts x five summary planes (scratch)
    uint32_t frame_bytes;
    uint32_t width;          // frame width in pixels (the row pitch)
    uint32_t n_frames;
    uint32_t n_tiles;
    uint32_t n_waves;
    uint32_t part_frames;    // frames per part (>= 1; one part: >= n_frames)
    uint32_t t0;             // global index of frames[0]; t0 + n_frames <= 0xFFFFFFFF
    uint32_t accumulate;     // one part only: fold onto the state `out` holds
    float thr;               // series_threshold(C, tau, 0)
    GridRect roi;
};

// times_combine_kernel: one thread per pixel folds the parts' summaries
// (parts[(part * 5 + k) * npx + pixel]; k: first, last, run_max, leading,
// trailing) in order onto the initial or accumulated state in `times`.
struct TimesCombineArgs {
    const uint32_t* parts;
    uint32_t* times;
    uint32_t frame_bytes;
    uint32_t width;
    uint32_t channels;       // 3 or 4: with frame_bytes and width the test for the vecs the fast kernel leaves out
    uint32_t n_frames;
    uint32_t part_frames;
    uint32_t accumulate;
    GridRect roi;
};

// times_generic_kernel: one thread per pixel of rect (inside the region)
// walks the frames; the pixel's four values in `times` written or updated.
struct TimesGenericArgs {
    const uint8_t* frames;
    const uint8_t* ref0;
    uint32_t* times;
    uint64_t frame_bytes;
    uint32_t width;
    uint32_t n_frames;
    uint32_t mode;
    uint32_t chroma;
    float tau;
    uint32_t t0;
    uint32_t accumulate;
    GridRect roi;
    GridRect rect;
};

// series_background_kernel (series_background.hip): the running-average
// background of a region and the change mask against it.  The mask kernel's
// geometry (rows padded to 8 vecs per mask word), one part always: a wave
// owns every frame of its tile, with the state of its pixels -- a u16 per
// channel -- in registers.
#ifndef DIPS_UNROLL_BACKGROUND
#define DIPS_UNROLL_BACKGROUND 2
#endif
constexpr int kUnrollBackground = DIPS_UNROLL_BACKGROUND;  // vecs per lane: 512 px / wave / frame
struct BgArgs {
    const uint8_t* frames;   // n_frames * frame_bytes, contiguous
    const uint8_t* ref0;     // accumulate == 0: the initial state is 256 * its bytes
    uint16_t* background;    // C planes of roi.w * roi.h u16, 2-byte aligned
    uint8_t* mask;           // n_frames * mask_frame_bytes, 4-byte aligned, or NULL
    uint32_t frame_bytes;
    uint32_t mask_frame_bytes;  // roi.h * 4 * ceil(roi.w / 32)
    uint32_t width;          // frame width in pixels (the row pitch)
    uint32_t n_frames;       // >= 1
    uint32_t n_tiles;
    uint32_t n_waves;
    uint32_t rate_shift;     // 0 .. 8
    uint32_t selective;      // DIPS_BG_SELECTIVE set
    uint32_t accumulate;     // continue the state `background` holds
    float thr;               // series_threshold(C, tau, 0)
    GridRect roi;
};

// background_generic_kernel: one thread per mask word of rows [row0, row0 +
// n_rows) x words [word0, word0 + n_words) of the region walks the word's
// pixels and, per pixel, the frames; it stores the state of the pixels from
// region column state_x0 on.  n_frames may be 0 (the initial state alone).
struct BgGenericArgs {
    const uint8_t* frames;
    const uint8_t* ref0;
    uint16_t* background;
    uint8_t* mask;           // or NULL
    uint64_t frame_bytes;
    uint64_t mask_frame_bytes;
    uint32_t width;
    uint32_t n_frames;
    uint32_t chroma;
    float tau;
    uint32_t rate_shift;
    uint32_t selective;
    uint32_t accumulate;
    uint32_t row0, n_rows, word0, n_words;
    uint32_t state_x0;
    GridRect roi;
};

// The connected components of a chunk of change-mask frames
// (mask_components.hip).  Scratch per frame: parent, one u32 per pixel, and
// the statistics of the word-local runs, one slot per two pixels of a row.
struct ComponentsArgs {
    const uint32_t* mask;   // the chunk's frames, h * wpr words each
    uint32_t* parent;       // n_frames * npx
    uint64_t* sum_i;        // n_frames * nslots each, from here on
    uint64_t* sum_j;
    uint32_t* area;         // after cc_select_kernel: the label
    uint32_t* min_x;
    uint32_t* max_x;
    uint32_t* max_y;
    uint32_t* block_count;  // n_frames * bpf: kept roots per block, then their exclusive scan
    uint32_t* counts;       // the chunk's part of the outputs
    uint32_t* boxes;        // NULL with max_boxes = 0; cleared by the host
    uint32_t* labels;       // NULL: not produced
    uint32_t w, h;
    uint32_t npx;           // w * h < 2^30
    uint32_t wpr;           // mask words per row
    uint32_t hw;            // slots per row, ceil(w / 2)
    uint32_t nslots;        // hw * h
    uint32_t wpf;           // mask words per frame
    uint32_t bpf;           // blocks of 256 words per frame
    uint32_t n_frames;      // of the chunk
    uint32_t connectivity;  // 4 or 8
    uint32_t min_area;
    uint32_t max_boxes;
};

// The selection of components of a chunk of labelled mask frames
// (mask_select.hip), behind launch_mask_labelling on the same stream with the
// same ComponentsArgs `cc` (its min_area is the predicate's).
struct SelectArgs {
    ComponentsArgs cc;
    const uint32_t* marker;  // NULL: no marker; else frames in the mask's layout
    uint32_t* out;           // the chunk's frames; every word is written, pad bits 0
    uint32_t* counts;        // NULL: not produced; else the chunk's part, cleared by the host
    uint32_t marker_stride;  // words from marker frame f to f + 1: wpf, or 0 (one frame for all)
    uint32_t max_area;       // 0: no upper bound
    uint32_t select;         // DIPS_SELECT_* bits
};

// The shape records of a chunk of labelled mask frames (mask_shapes.hip),
// behind launch_mask_components on the same stream with the same
// ComponentsArgs `cc` (max_boxes > 0).
struct ShapesArgs {
    ComponentsArgs cc;
    const uint8_t* weights;  // NULL: none; else the chunk's planes, npx bytes each, any alignment
    uint32_t* shapes;        // the chunk's part, n_frames * max_boxes records; 8-byte aligned, cleared by the host
};

// Word-wise logic on mask frames (mask_select.hip): one launch, grid stride.
struct LogicArgs {
    const uint32_t* a;   // n_frames frames of wpf words
    const uint32_t* b;   // b_frames frames (NULL for DIPS_LOGIC_NOT)
    uint32_t* out;       // n_frames frames; every word is written, pad bits 0
    uint64_t words;      // n_frames * wpf
    uint32_t w;
    uint32_t wpr;        // mask words per row
    uint32_t wpf;        // mask words per frame
    uint32_t op;         // DIPS_LOGIC_*
    uint32_t b_bcast;    // 1: frame 0 of b serves every frame
};

// The links of a chunk of labelled mask frames to their predecessors
// (mask_tracks.hip).  `parent` and `label` are the planes
// launch_mask_components left, with one more plane in front: plane f + 1 is
// the chunk's frame f and plane f its predecessor, so plane 0 is the frame
// before the chunk.
struct TracksArgs {
    const uint32_t* mask;      // the chunk's frames, h * wpr words each
    const uint32_t* prev0;     // the frame before the chunk in the same layout; NULL: frame 0 has no predecessor
    uint32_t* parent;          // (n_frames + 1) * npx: every node's root
    uint32_t* label;           // (n_frames + 1) * nslots: ComponentsArgs::area after cc_select_kernel
    const uint32_t* counts;    // the chunk's part of the output, already written
    uint32_t* ov;              // n_frames * K * K, zero on entry: ov[f][a][b]
    uint32_t* cprev;           // n_frames * K: the record continued, DIPS_LINK_NONE for a head or no record
    uint32_t* hrank;           // n_frames * K: a head's rank among the heads of its frame
    uint32_t* heads;           // n_frames: heads per frame
    uint32_t* base;            // n_frames: the id of the frame's first head
    uint32_t* next_id;         // one word: the next unused id, read and advanced
    const uint32_t* carry_in;  // 2 * K: TRACK, then AGE, of the records of the frame before the chunk
    uint32_t* carry_out;       // 2 * K: the same of the chunk's last frame (not carry_in)
    uint32_t* links;           // the chunk's part of the output
    uint32_t w, h;
    uint32_t npx;              // w * h < 2^30
    uint32_t wpr;              // mask words per row
    uint32_t hw;               // slots per row, ceil(w / 2)
    uint32_t nslots;           // hw * h
    uint32_t wpf;              // mask words per frame
    uint32_t bpf;              // blocks of 256 words per frame
    uint32_t n_frames;         // of the chunk
    uint32_t K;                // max_boxes, 1 .. DIPS_TRACK_MAX_BOXES
};

// The binary morphology of a batch of change-mask frames (mask_morph.hip):
// one launch, tiles of the frames as a flattened 64-bit index.
struct MorphArgs {
    const uint32_t* in;   // n_frames frames of h * wpr words
    uint32_t* out;        // the same layout; every word is written, pad bits 0
    uint64_t items;       // n_frames * tiles_x * tiles_y
    uint32_t w, h;
    uint32_t wpr;         // mask words per row
    uint32_t n_frames;
    uint32_t op;          // DIPS_MORPH_ERODE .. DIPS_MORPH_CLOSE
    uint32_t shape;       // DIPS_MORPH_BOX or DIPS_MORPH_DIAMOND (then ry == rx)
    uint32_t rx, ry;      // <= DIPS_MORPH_MAX_RADIUS
    uint32_t tiles_x;     // from mask_morph_tiling
    uint32_t tiles_y;
};

// The temporal m-of-k vote on a batch of change-mask frames (mask_vote.hip):
// one launch over items (frame part, tile of 64 * kVoteWords words), and one
// over the window - 1 frames of the next history.
// Mask words a lane owns.  Measured at 4K, 500 frames: 1 word fills
// the wave slots at every window and is as fast as 2 at k = 3 and 1.4x faster
// at k = 31, where 2 words leave half the slots empty; 4 words spill.
#ifndef DIPS_VOTE_WORDS
#define DIPS_VOTE_WORDS 1
#endif
constexpr int kVoteWords = DIPS_VOTE_WORDS;
struct VoteArgs {
    const uint32_t* in;       // n_frames frames of wpf words (may be NULL when n_frames == 0)
    const uint32_t* hist_in;  // window - 1 frames before the clip, oldest first; NULL: all clear
    uint32_t* out;            // n_frames frames; every word is written, pad bits 0
    uint32_t* hist_out;       // window - 1 frames (launch_mask_vote_history only)
    uint32_t w;
    uint32_t wpr;             // mask words per row
    uint32_t wpf;             // mask words per frame, < 2^30
    uint32_t n_frames;
    uint32_t window;          // k, 1 .. DIPS_VOTE_MAX_WINDOW
    uint32_t votes;           // m, 1 .. k
    uint32_t part_frames;     // from vote_geometry
    uint32_t parts;
    uint32_t n_tiles;
    uint32_t n_waves;
};

// The statistics of a batch of change-mask frames (mask_stats.hip).
// Grid counts: one launch over items (frame, grid row, chunk of kCountsChunkCells
// grid columns, band of mask rows) from mask_counts_geometry.
constexpr uint32_t kCountsChunkCells = 1024;   // cells a block sums in LDS
constexpr uint32_t kCountsMinBandWords = 4096;  // mask words below which a band is not cut further
struct MaskCountsArgs {
    const uint32_t* mask;  // n_frames frames of h * wpr words
    uint32_t* counts;      // [n_frames][rows][cols]
    uint64_t items;
    uint32_t w, h;
    uint32_t wpr;          // mask words per row
    uint32_t n_frames;
    uint32_t rows, cols;
    uint32_t col_chunks, bands, band_rows;  // from mask_counts_geometry
};

// Change times and per-pixel sums: one launch over items (frame part, tile of
// 64 lane slots), a slot = kMaskTimesPx pixels of one mask byte; with several
// parts a second launch folds the parts' summaries in order.
// Pixels a lane owns (4 or 8).  Measured at 4K, 500 frames: 8
// are 12 % faster than 4 for the times and 30 % for the sums.
#ifndef DIPS_MASK_TIMES_PX
#define DIPS_MASK_TIMES_PX 8
#endif
constexpr int kMaskTimesPx = DIPS_MASK_TIMES_PX;
struct MaskTimesArgs {
    const uint8_t* mask;    // n_frames frames of frame_bytes bytes
    uint32_t* times;        // four planes of w * h, or NULL
    uint32_t* sums;         // one plane of w * h, or NULL
    uint32_t* parts;        // several parts: per part 5 planes (times given) and 1 plane (sums given)
    uint32_t w, h;
    uint32_t row_bytes;     // 4 * mask words per row
    uint32_t frame_bytes;   // row_bytes * h, < 2^32
    uint32_t n_frames;
    uint32_t t0;            // global index of frame 0
    uint32_t accumulate;    // fold onto what times / sums hold
    uint32_t part_frames;   // from mask_times_geometry
    uint32_t n_parts;
    uint32_t n_tiles;
    uint32_t n_waves;
};

struct SynthArgs {
    uint8_t* dst;
    uint64_t total_bytes;
    uint64_t frame_bytes;
    uint64_t seed;
    uint64_t t0;
    uint32_t channels;
    uint32_t width;
    uint32_t height;
    uint32_t radius;
};

struct CompatArgs {
    const uint8_t* raw;      // filter source (RGBA8) for the newest slot
    uint8_t* slots[4];       // temporal ring (RGBA8)
    const uint8_t* start;    // start texture (RGBA8 gray)
    uint8_t* out;            // visualisation (RGBA8)
    uint32_t width, height;
    uint32_t newest;         // starting_index uniform
    int32_t window;
    uint32_t chroma;
    uint32_t filter;
    float sensitivity;
    uint32_t colorize;
    uint32_t y0, y1;         // compat_main: rows [y0, y1) only (y1 = 0: all rows)
    uint32_t out_key;        // compat_main_host: 0 RGBA8 texels; 1 one byte (gray: R = G = B, A = 255);
                             // 2 two bytes R | G << 8 (colorized: B = min(R, G), A = 255) -- the host
                             // expands them (host_stream.h expand_keys)
    uint32_t in_key;         // compat_main_host: raw holds RGBA8 texels (0), or per pixel the chroma
                             // channel (1) / (max, min) of R, G, B (2) (copy_pool.h pack_frame);
                             // compat_main_host_packed_kernel, out_key 1 / 2 only
};

// dips ComputeState over a batch in steady state (compat_batch.hip).
struct CompatBatchArgs {
    const uint8_t* frames;   // n_frames x frame_bytes (RGBA8)
    uint8_t* out;            // n_frames x frame_bytes (RGBA8)
    const uint8_t* start;    // start texture (RGBA8 gray, R = S)
    const uint8_t* pre[3];   // ring slots of the frames before frames[0] (gray texels): t-1, t-2, t-3
    uint8_t* post[4];        // ring slots that receive frames n-1 .. n-4 as gray texels (null: none)
    uint32_t frame_bytes;
    uint32_t n_vec;          // 4-pixel vecs per frame
    uint32_t n_frames, chunk, n_chunks, n_tiles;
    float k;                 // sensitivity (SIGMOID_HORIZONTAL_SCALAR)
    float kneg_half;         // -k / 2
    const uint16_t* lut;     // epilogue table (compat_batch_lut_kernel): 65536 x (R | G << 8)
};
constexpr int kUnrollCompatBatch = 2;
// U vecs per lane and D frames of loads in flight per wave of the table
// kernel.  In one process over one batch (round 2,
// profiles/r02_compat_variant_ab.jsonl) U = 4, D = 3 ran 76.2 % of 8 TB/s
// read + write, against 72.4 % for U = 2, D = 2 (an earlier cross-process
// A/B had called U = 4 equal).  126 VGPRs: the 1024-thread workgroup's
// budget is 128, and D = 4 spills.
constexpr int kUnrollCompatLut = 4;
constexpr int kDepthCompatLut = 3;
constexpr uint32_t kCompatLutWaves = 16;  // waves per workgroup of compat_batch_lut_kernel (one per CU)
// the epilogue table of the current properties: lut[S * 256 + m]
hipError_t launch_compat_lut(uint16_t* lut, uint32_t filter, float k, bool colorize, hipStream_t s);
const void* compat_batch_lut_kernel_ptr(int chroma);
hipError_t launch_compat_batch_lut(const CompatBatchArgs& a, int chroma, uint32_t blocks, hipStream_t s);
const void* compat_batch_kernel_ptr(int chroma, int filter, bool colorize, bool fast);
hipError_t launch_compat_batch(const CompatBatchArgs& a, int chroma, int filter, bool colorize, bool fast,
                               uint32_t blocks, hipStream_t s);

// dips_alt DiPsCompute (alt_kernels.hip).
constexpr int kAltMaxTextures = 16;  // MAX_TEMPORAL_ARRAY_SIZE (dips_alt pre_compute_shader.wgsl:12)
constexpr int kUnrollAlt = 2;        // vecs (4 px) per lane of alt_batch_kernel
// vecs per lane / frames of loads in flight of its epilogue-table form.  In one process
// over one batch (round 2, profiles/r02_alt_variant_ab.jsonl):
// U = 4, D = 2 72.8 % of 8 TB/s read + write, U = 2, D = 2 72.1 %, the others
// 71.2-72.3 % (8 groups of 256 threads per CU already keep enough in flight).
constexpr int kUnrollAltLut = 4;
constexpr int kDepthAltLut = 2;

struct AltArgs {                     // one send_frame dispatch
    const uint8_t* slots[kAltMaxTextures];  // RGBA8 contents of the N texture slots
    uint8_t* snap;                   // snapshot texture, one byte (.r) per pixel
    uint8_t* out;                    // RGBA8 output texture
    uint32_t width, height;
    uint32_t n_tex;
    int32_t window;
    uint32_t chroma, filter;
    float scalar;
    uint32_t colorize;
    uint32_t snapshot;
    uint32_t y0, y1;                 // rows [y0, y1) only (y1 = 0: all rows)
};

struct AltBatchArgs {                // a run of frames, N = 2, W = 1
    const uint8_t* frames;           // n_frames x frame_bytes (RGBA8)
    const uint8_t* prev0;            // slot holding the frame before frames[0]
    const uint8_t* snap_in;          // snapshot bytes before the batch
    uint8_t* snap_out;               // snapshot bytes after the batch's last snapshot
    uint8_t* out;                    // n_frames x frame_bytes (RGBA8)
    const uint8_t* flags;            // device: n_frames snapshot flags
    const int32_t* chunk_snap;       // device: per chunk, last snapshot frame before it or -1
    uint32_t frame_bytes;
    uint32_t n_vec;                  // 4-pixel vecs per frame
    uint32_t n_frames, chunk, n_chunks, n_tiles;
    int32_t last_snap;               // last snapshot frame of the batch or -1
    float scalar;                    // SIGMOID_HORIZONTAL_SCALAR k
    float kneg_half;                 // -k / 2 (fast epilogue)
    const uint32_t* lut_l1;          // epilogue table (alt_lut.h): level-1 {x, sh} per cluster
    const uint16_t* lut_l2;          //   and the u16 texel entries (LUT kernel only)
};

hipError_t launch_alt_frame(const AltArgs& a, hipStream_t s);
// send_frame (W = 1) reading the new frame from pinned host memory `in`,
// storing it into `newest_slot` (= a.slots[newest]) and writing a.out (pinned
// host memory): the per-frame call's zero-copy form
hipError_t launch_alt_frame_host(const AltArgs& a, const uint8_t* in, uint8_t* newest_slot, uint32_t newest,
                                 hipStream_t s);

struct CopyFramesArgs {
    const uint8_t* src[2];
    uint8_t* dst[2];
    uint64_t n16;  // 16-byte words per frame (16-byte aligned frames)
};
hipError_t launch_copy_frames(const CopyFramesArgs& a, uint32_t count, hipStream_t s);
// fast: the branch-free epilogue (alt_fast_epilogue_ok)
// chroma -1: frames are prefiltered f32 I2s intensities (launch_alt_filter_frames)
const void* alt_batch_kernel_ptr(int chroma, int filter, bool colorize, bool fast);
// W > 1: the filtered intensity (I * 2^23, f32) of each pixel of n RGBA8
// frames, one f32 per pixel (the layout the batch kernel reads with chroma -1)
hipError_t launch_alt_filter_frames(const uint8_t* frames, float* dst, uint32_t width, uint32_t height, uint32_t n,
                                   int32_t window, uint32_t chroma, hipStream_t s);
hipError_t launch_alt_batch(const AltBatchArgs& a, int chroma, int filter, bool colorize, bool fast, uint32_t blocks,
                            hipStream_t s);
// the epilogue-table form (alt_lut.h): any filter / k / colour, same outputs
const void* alt_batch_lut_kernel_ptr(int chroma);
hipError_t launch_alt_batch_lut(const AltBatchArgs& a, int chroma, uint32_t blocks, hipStream_t s);
// lut_l2[slots[i]] = R | G << 8 of visual_epilogue(diffs[i], filter, k, colorize)
// exhaustive table check over every (S, max, min): mismatches added to *bad
hipError_t launch_alt_lut_check(const uint32_t* l1, const uint16_t* l2, uint32_t filter, float k, bool colorize,
                                unsigned long long* bad, hipStream_t s);
hipError_t launch_alt_lut_fill(uint16_t* lut_l2, const float* diffs, const uint16_t* slots, uint32_t n,
                               uint32_t filter, float k, bool colorize, hipStream_t s);
// the fast epilogue's preconditions (epilogue_fast.h): sigmoid with a scalar
// k of |k| <= 160 (0 or |k| >= 2^-60 so -k/2 is exact), or no filter
inline bool alt_fast_epilogue_ok(uint32_t filter, float k) {
    if (filter == 1u) return false;
    if (filter != 0u) return true;
    const float a = k < 0.0f ? -k : k;
    return a <= 160.0f && (a == 0.0f || a >= 0x1p-60f);
}

int pixels_per_vec(int channels);
int fast_unroll(int channels);
// isi (series_v2, RGB8 / RGBA8): 0 the exact f64 intensity sum, 1 the
// integer sum with a threshold select (ISI; needs tau >= 2^-5) -- for plain
// aligned RGB8 its screened form (series_v2_screen.h; SeriesArgs::screen) --,
// 3 the integer sum without the screen (as 1 where there is no screened form)
const void* series_fast_kernel_ptr(int channels, int chroma, bool per_frame, bool map, bool align = false,
                                   int isi = 0);
const void* series_v2_kernel_ptr(int channels, int chroma, bool per_frame, bool map, bool align = false,
                                 int isi = 0);
// whether tau admits the integer intensity sum of series_v2 (tau >= 2^-5)
bool series_v2_isi(float tau);
// threshold argument (SeriesArgs::thr) of the kernel series_fast_kernel_ptr picks
float series_threshold(int channels, float tau, int isi = 0);
hipError_t launch_series_fast(const SeriesArgs& a, int channels, int chroma, bool per_frame, bool map,
                              uint32_t blocks, hipStream_t s, bool align = false, int isi = 0);
// record layout: 0 RGB(A), 1 gray (series_fast_kernel), 2 gray table kernel (series_gray_lut_kernel)
hipError_t launch_series_reduce(const uint64_t* partials, uint32_t n_frames, uint32_t n_tiles, int layout,
                                dips_series_entry* series, hipStream_t s);
// GRAY8 table kernel: table layout 4, i.e. layout 5 (the u16 table keyed by
// (a ^ b, a) with the band clamp) or 2 (the u16 table keyed by (a, b),
// swizzled) per workgroup from a sample of its items
const void* series_gray_lut_kernel_ptr(bool per_frame, bool map);
// the tables of layout 4 (5, then 2 kGrayLutAllocBytes after it), or of one layout
hipError_t launch_gray_lut(uint8_t* tab, float tau, int layout, hipStream_t s);
hipError_t launch_series_gray_lut(const SeriesArgs& a, bool per_frame, bool map, uint32_t blocks, hipStream_t s);
hipError_t launch_series_generic(const GenericArgs& a, int channels, hipStream_t s);
// the grid form of the series (series_grid.hip): RGB8 / RGBA8 fast kernel
// (isi as series_v2), its per-(cell, frame) reduce and the any-format generic
// kernel
const void* series_grid_kernel_ptr(int channels, int chroma, bool per_frame, int isi);
hipError_t launch_series_grid(const GridArgs& a, int channels, int chroma, bool per_frame, int isi, uint32_t blocks,
                              hipStream_t s);
hipError_t launch_grid_reduce(const GridArgs& a, int channels, dips_series_entry* cells, hipStream_t s);
hipError_t launch_grid_generic(const GridGenericArgs& a, int channels, hipStream_t s);
// the per-pixel sums over time (series_pixels.hip): RGB8 / RGBA8 fast kernel
// (isi as series_v2) and the any-format generic kernel
const void* series_pixels_kernel_ptr(int channels, int chroma, bool per_frame, int isi);
hipError_t launch_series_pixels(const PixArgs& a, int channels, int chroma, bool per_frame, int isi, uint32_t blocks,
                                hipStream_t s);
hipError_t launch_pixels_generic(const PixGenericArgs& a, int channels, hipStream_t s);
// the per-frame change mask (series_mask.hip): RGB8 / RGBA8 fast kernel (one
// intensity form for every tau) and the any-format generic kernel
const void* series_mask_kernel_ptr(int channels, int chroma, bool per_frame);
hipError_t launch_series_mask(const MaskArgs& a, int channels, int chroma, bool per_frame, uint32_t blocks,
                              hipStream_t s);
hipError_t launch_mask_generic(const MaskGenericArgs& a, int channels, hipStream_t s);
// the change times per pixel (series_times.hip): RGB8 / RGBA8 fast kernel in
// its one-part and its several-parts form, the fold of the parts' summaries
// and the any-format generic kernel
const void* series_times_kernel_ptr(int channels, int chroma, bool per_frame, bool parts);
hipError_t launch_series_times(const TimesArgs& a, int channels, int chroma, bool per_frame, bool parts,
                               uint32_t blocks, hipStream_t s);
hipError_t launch_times_combine(const TimesCombineArgs& a, hipStream_t s);
hipError_t launch_times_generic(const TimesGenericArgs& a, int channels, hipStream_t s);
// the running-average background and its change mask (series_background.hip):
// RGB8 / RGBA8 fast kernel (tiles of kUnrollBackground vecs per lane, or of
// one for small regions) and the any-format generic kernel
const void* series_background_kernel_ptr(int channels, int chroma, bool small_tile);
hipError_t launch_series_background(const BgArgs& a, int channels, int chroma, bool small_tile, uint32_t blocks,
                                    hipStream_t s);
hipError_t launch_background_generic(const BgGenericArgs& a, int channels, hipStream_t s);
// the connected components of a chunk of mask frames (mask_components.hip):
// every launch of the chunk, in order, on `s`
hipError_t launch_mask_components(const ComponentsArgs& a, hipStream_t s);
// its launches 1-3 alone: every parent a root, the statistics in the roots' slots
hipError_t launch_mask_labelling(const ComponentsArgs& a, hipStream_t s);
// the selection of components of a chunk labelled by launch_mask_labelling on
// the same stream, and the word-wise logic of two masks (mask_select.hip)
hipError_t launch_mask_select(const SelectArgs& a, hipStream_t s);
hipError_t launch_mask_logic(const LogicArgs& a, hipStream_t s);
// the shape records of a chunk labelled by launch_mask_components on the same
// stream (mask_shapes.hip): one launch
hipError_t launch_mask_shapes(const ShapesArgs& a, hipStream_t s);
// the links of a chunk of frames labelled by launch_mask_components on the
// same stream (mask_tracks.hip): the clear of the overlap table and the four
// launches, in order, on `s`
hipError_t launch_mask_tracks(const TracksArgs& a, hipStream_t s);
// plane `plane` of parent and label, the labelling of the frame at `frame`,
// becomes plane 0, the predecessor of the next chunk: one launch over the
// frame's words that copies what its runs own and nothing else
hipError_t launch_mask_tracks_keep(const TracksArgs& a, const uint32_t* frame, uint32_t plane, hipStream_t s);
// the binary morphology of mask frames (mask_morph.hip): the one launch of a
// call on `s`, and the tiles it cuts a w x h frame into
hipError_t launch_mask_morph(const MorphArgs& a, hipStream_t s);
void mask_morph_tiling(uint32_t w, uint32_t h, uint32_t* tiles_x, uint32_t* tiles_y);
// the temporal vote on mask frames (mask_vote.hip): the launch over the
// frames of a call on `s` (`blocks` of 4 waves), and the one that writes the
// next history (any n_frames, 0 included)
const void* mask_vote_kernel_ptr();
hipError_t launch_mask_vote(const VoteArgs& a, uint32_t blocks, hipStream_t s);
hipError_t launch_mask_vote_history(const VoteArgs& a, hipStream_t s);
// the statistics of mask frames (mask_stats.hip): the grid counts (`blocks`
// of 256 threads; with a.bands > 1 the blocks add onto counts, which the
// caller has cleared on `s`), the change times and / or sums (`blocks` of 4
// waves; with a.n_parts > 1 into a.parts) and the fold of those parts
const void* mask_counts_kernel_ptr();
hipError_t launch_mask_counts(const MaskCountsArgs& a, uint32_t blocks, hipStream_t s);
const void* mask_times_kernel_ptr(bool times, bool sums, bool parts);
hipError_t launch_mask_times(const MaskTimesArgs& a, uint32_t blocks, hipStream_t s);
hipError_t launch_mask_times_combine(const MaskTimesArgs& a, hipStream_t s);
hipError_t launch_synth(const SynthArgs& a, hipStream_t s);
hipError_t launch_read_ceiling(const uint8_t* p, uint64_t bytes, uint32_t* out, hipStream_t s);
// read-only walk in the RGB8 / RGBA8 series kernel's shape (vec_bytes 12 / 16, U = kUnrollV2Rgb / kUnrollV2)
hipError_t launch_read_walk(const SeriesArgs& a, int vec_bytes, uint32_t blocks, uint32_t* out, hipStream_t s);
hipError_t launch_compat_precompute(const CompatArgs& a, hipStream_t s);
hipError_t launch_compat_main(const CompatArgs& a, hipStream_t s);
// compat_main with raw / out in pinned host memory (zero-copy per-frame call)
// slot_mode 0: store the quantised gray texel into the newest slot
// (compute_main); 1: store the raw frame texel, 2: store nothing (the
// speculative dispatch of a deferred add_texture, W = 1 / W > 1)
hipError_t launch_compat_main_host(const CompatArgs& a, hipStream_t s, int slot_mode = 0);
// a raw ring slot into its gray texel q(get_intensity) in place
hipError_t launch_compat_quantise_slot(uint8_t* slot, uint64_t n_px, uint32_t chroma, hipStream_t s);
// bytes (a multiple of 4, 4-B aligned) between pinned host memory (its
// device-visible pointer) and HBM, by a kernel instead of a DMA engine
hipError_t launch_copy_from_host(const uint8_t* src, uint8_t* dst, uint64_t bytes, hipStream_t s);
hipError_t launch_copy_to_host(const uint8_t* src, uint8_t* dst, uint64_t bytes, hipStream_t s);
hipError_t launch_compat_gray(const uint8_t* src, uint8_t* dst, uint64_t n_px, uint32_t chroma, hipStream_t s);
// W > 1 steady state: the ring texel compute_main stores for each of n frames
// (gray q(spatial_median_filter(frame)), dips_shader.wgsl:120-170, 187), so
// that the batch kernel can run on the filtered frames.  frames, dst: n x
// width x height RGBA8.
hipError_t launch_compat_filter_frames(const uint8_t* frames, uint8_t* dst, uint32_t width, uint32_t height,
                                       uint32_t n, int32_t window, uint32_t chroma, hipStream_t s);

}  // namespace dips
