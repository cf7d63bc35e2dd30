// region_abi.hip -- host side of include/dips_hip.h, part 4: the regional
// products of the difference series over a region of interest -- the grid of
// cells, the per-pixel sums, the per-frame change mask, the change times per
// pixel, the running-average background and the Sigma-Delta model with their
// masks.  Their schedules are in series_sched.h, what they share with the
// series in series_host.h.  Every extern "C" body runs inside
// dips_abi::guard (abi_guard.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "series_host.h"
#include "series_sigma_delta.h"

using dips_abi::guard;
using namespace dips_internal;

namespace {

// ---------------------------------------------------------------------------
// The grid form (dips_diff_series_grid; kernels in series_grid.hip)
// ---------------------------------------------------------------------------

// The grid of a call, validated: nullptr, or why it is refused.
const char* grid_spec(uint32_t width, uint32_t height, const uint32_t* roi, uint32_t rows, uint32_t cols,
                      dips::GridSpec* g) {
    if (width == 0 || height == 0) return "empty frame";
    g->x = roi ? roi[0] : 0u;
    g->y = roi ? roi[1] : 0u;
    g->w = roi ? roi[2] : width;
    g->h = roi ? roi[3] : height;
    g->rows = rows;
    g->cols = cols;
    if (g->w == 0 || g->h == 0) return "the region of interest has zero extent";
    if ((uint64_t)g->x + g->w > width || (uint64_t)g->y + g->h > height)
        return "the region of interest leaves the frame";
    if (rows == 0 || cols == 0) return "rows and cols must be at least 1";
    if (rows > g->h || cols > g->w) return "more rows or cols than the region has pixels (a cell would be empty)";
    return nullptr;
}

// The schedule of the fast grid kernel (series_sched.h grid_geometry).
dips_sched::Geom grid_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf,
                               int isi, const dips::GridSpec& g) {
    return dips_sched::grid_geometry(frame_bytes(h, width, height), n_frames, dips::fast_unroll(C), g.w, g.h, g.rows,
                                     g.cols,
                                     resident_waves(h, dips::series_grid_kernel_ptr(C, (int)h->p.chroma_filter, pf, isi)));
}

// Run the grid series on device pointers, asynchronously on `s`.
dips_status run_grid_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                            const uint8_t* ref0, const dips::GridSpec& g, dips_series_entry* cells, hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t fb = frame_bytes(h, width, height);
    const uint32_t n_cells = g.rows * g.cols;
    const int isi = series_isi_form(h);
    dips_sched::Geom q;
    if (regional_fast_path(h)) q = grid_geometry(h, width, height, n_frames, C, pf, isi, g);
    // the cells start at zero: the fast kernel clears them itself (GridArgs::zero)
    if (!q.ok) DIPS_HIP(h, hipMemsetAsync(cells, 0, sizeof(dips_series_entry) * (size_t)n_frames * n_cells, s));
    auto launch_generic = [&](const dips::GridSpec& gs, uint32_t out_base) -> dips_status {
        const uint64_t max_w = ((uint64_t)gs.w + gs.cols - 1) / gs.cols, max_h = ((uint64_t)gs.h + gs.rows - 1) / gs.rows;
        const uint64_t spc = (max_w * max_h + 255u) / 256u;
        if (spc >= (1ull << 32)) return fail(h, DIPS_ERR_INVALID, "diff_series_grid: cell too large for the generic kernel");
        dips::GridGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.cells = cells;
        a.frame_bytes = fb;
        a.width = width;
        a.n_frames = n_frames;
        a.segs_per_cell = (uint32_t)spc;
        a.out_stride = n_cells;
        a.out_base = out_base;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.g = gs;
        DIPS_HIP(h, dips::launch_grid_generic(a, C, s));
        return DIPS_OK;
    };

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    dips::GridArgs a{};
    if (q.ok) {
        DIPS_HIP(h, h->partials.ensure((size_t)q.n_tiles * n_frames * 16u));
        a.frames = frames;
        a.ref0 = ref0;
        a.partials = h->partials.as<uint64_t>();
        a.zero = reinterpret_cast<uint64_t*>(cells);
        a.zero_n = 4u * n_frames * n_cells;
        a.frame_bytes = (uint32_t)fb;
        a.width = width;
        a.n_frames = n_frames;
        a.tiles_per_cell = q.tiles_per_cell;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.part_frames = q.part_frames;
        a.thr = dips::series_threshold(C, h->p.tau, isi);
        a.g = g;
        DIPS_HIP(h, dips::launch_series_grid(a, C, (int)h->p.chroma_filter, pf, isi, (uint32_t)q.blocks, s));
        // the vecs the fast kernel leaves out (series_grid.hip; the walk is
        // series_sched.h for_grid_frame_end_tails): their <= 3 pixels go into
        // their cells by atomics (after the kernel's zeroing)
        DIPS_TRY(dips_sched::for_grid_frame_end_tails(
            width, height, g.y, g.h, g.rows, g.cols, [&](uint32_t r, uint32_t c) { return dips::grid_cell_rect(g, r, c); },
            [&](uint32_t crow, uint32_t c, uint32_t x0, uint32_t y, uint32_t n) {
                return launch_generic(dips::GridSpec{x0, y, n, 1u, 1u, 1u}, crow * g.cols + c);
            }));
    } else {
        DIPS_TRY(launch_generic(g, 0u));
    }
    DIPS_TRY(span.end(s));
    if (q.ok) DIPS_HIP(h, dips::launch_grid_reduce(a, C, cells, s));
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The per-pixel sums over time (dips_diff_pixel_sums; kernels in
// series_pixels.hip)
// ---------------------------------------------------------------------------

// The schedule of the fast per-pixel kernel (series_sched.h pix_geometry).
dips_sched::Geom pix_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf,
                              int isi, const dips::GridSpec& g) {
    return dips_sched::pix_geometry(frame_bytes(h, width, height), n_frames, dips::kUnrollPix, g.w, g.h,
                                    resident_waves(h, dips::series_pixels_kernel_ptr(C, (int)h->p.chroma_filter, pf, isi)),
                                    dips::kPixMaxPart, pixel_part_pin());
}

// Run the per-pixel sums on device pointers, asynchronously on `s`.
dips_status run_pixels_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                              const uint8_t* ref0, const dips::GridSpec& g, bool accumulate, dips_series_entry* sums,
                              hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t fb = frame_bytes(h, width, height);
    const int isi = series_isi_form(h);
    dips_sched::Geom q;
    if (regional_fast_path(h)) q = pix_geometry(h, width, height, n_frames, C, pf, isi, g);
    auto launch_generic = [&](const dips::GridRect& rect) -> dips_status {
        dips::PixGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.sums = sums;
        a.frame_bytes = fb;
        a.width = width;
        a.n_frames = n_frames;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.accumulate = accumulate ? 1u : 0u;
        a.roi_x = g.x;
        a.roi_y = g.y;
        a.roi_w = g.w;
        a.rect = rect;
        DIPS_HIP(h, dips::launch_pixels_generic(a, C, s));
        return DIPS_OK;
    };

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    if (q.ok) {
        // several parts add with atomics: the map is zeroed in this earlier
        // launch (waves of one launch are not ordered against each other)
        if (q.parts > 1 && !accumulate)
            DIPS_HIP(h, hipMemsetAsync(sums, 0, sizeof(dips_series_entry) * (size_t)g.w * g.h, s));
        dips::PixArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.sums = sums;
        a.frame_bytes = (uint32_t)fb;
        a.width = width;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.part_frames = q.part_frames;
        a.out_mode = q.parts > 1 ? 2u : (accumulate ? 1u : 0u);
        a.thr = dips::series_threshold(C, h->p.tau, isi);
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_series_pixels(a, C, (int)h->p.chroma_filter, pf, isi, (uint32_t)q.blocks, s));
        // the vecs the fast kernel leaves out (series_pixels.hip): their <= 3
        // pixels each are nobody else's
        DIPS_TRY(for_frame_end_tail_rows(width, height, g, [&](uint32_t r, uint32_t i0) {
            return launch_generic(dips::GridRect{g.x + i0, g.y + r, g.w - i0, 1u});
        }));
    } else {
        DIPS_TRY(launch_generic(dips::GridRect{g.x, g.y, g.w, g.h}));
    }
    return span.end(s);
}

// ---------------------------------------------------------------------------
// The per-frame change mask (dips_diff_change_mask; kernels in
// series_mask.hip)
// ---------------------------------------------------------------------------

// The schedule of the fast mask kernel (series_sched.h mask_geometry).
dips_sched::Geom mask_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf,
                               const dips::GridSpec& g) {
    return dips_sched::mask_geometry(frame_bytes(h, width, height), n_frames, dips::kUnrollMask, g.w, g.h,
                                     resident_waves(h, dips::series_mask_kernel_ptr(C, (int)h->p.chroma_filter, pf)));
}

// Run the change mask on device pointers, asynchronously on `s`.
dips_status run_mask_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                            const uint8_t* ref0, const dips::GridSpec& g, uint8_t* mask, hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t fb = frame_bytes(h, width, height);
    const uint64_t wpr = mask_words_per_row(g.w);
    const uint64_t mfb = wpr * g.h * 4u;
    dips_sched::Geom q;
    if (regional_fast_path(h)) q = mask_geometry(h, width, height, n_frames, C, pf, g);
    auto launch_generic = [&](uint32_t row0, uint32_t n_rows, uint32_t word0, uint32_t n_words) -> dips_status {
        dips::MaskGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.mask = mask;
        a.frame_bytes = fb;
        a.mask_frame_bytes = mfb;
        a.width = width;
        a.t0 = 0u;
        a.n_frames = n_frames;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.row0 = row0;
        a.n_rows = n_rows;
        a.word0 = word0;
        a.n_words = n_words;
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_mask_generic(a, C, s));
        return DIPS_OK;
    };

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    if (q.ok) {
        dips::MaskArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.mask = mask;
        a.frame_bytes = (uint32_t)fb;
        a.mask_frame_bytes = (uint32_t)mfb;
        a.width = width;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.part_frames = q.part_frames;
        a.thr = dips::series_threshold(C, h->p.tau, 0);
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_series_mask(a, C, (int)h->p.chroma_filter, pf, (uint32_t)q.blocks, s));
        // the vecs the fast kernel leaves out (series_mask.hip).  The fast
        // kernel stored the word that holds such a vec with zeros in its
        // place; this later launch recomputes and stores the whole word, so no
        // two launches race for it and nothing is ORed into memory
        DIPS_TRY(for_frame_end_tail_rows(width, height, g, [&](uint32_t r, uint32_t) {
            return launch_generic(r, 1u, (g.w - 1u) >> 5, 1u);
        }));
    } else {
        if ((uint64_t)g.h * wpr >= (1ull << 31))
            return fail(h, DIPS_ERR_INVALID, "diff_change_mask: region too large for the generic kernel");
        DIPS_TRY(launch_generic(0u, g.h, 0u, (uint32_t)wpr));
    }
    return span.end(s);
}

// ---------------------------------------------------------------------------
// The running-average background and its change mask
// (dips_diff_background_mask; kernels in series_background.hip)
// ---------------------------------------------------------------------------

// The schedule the two background models share, asynchronously on `s`:
// background_geometry (series_sched.h) for the kernel family `kernel_ptr`
// with `unroll` vecs per lane, then
//  * the generic kernel for the vecs the fast kernel leaves out (those that
//    would read past the frame's end).  It computes the whole mask word that
//    holds such a vec and the state of the vec's pixels BEFORE the fast kernel
//    runs: it starts every pixel of the word from its initial state, which an
//    accumulating call keeps in the buffer the fast kernel overwrites.  The
//    fast kernel stores neither that word nor those pixels' state, so each
//    word and each state value has one writer;
//  * the fast kernel -- or else the whole region through the generic kernel.
// launch_generic(row0, n_rows, word0, n_words, state_x0) and
// launch_fast(geometry) fill and launch the model's own argument structs;
// `name`: the exported function's, for its messages.
template <typename Generic, typename Fast>
dips_status run_model_device(dips_handle* h, const char* name, uint32_t width, uint32_t height, uint32_t n_frames,
                             const dips::GridSpec& g, const void* (*kernel_ptr)(int, int, bool), int unroll,
                             Generic&& launch_generic, Fast&& launch_fast, hipStream_t s) {
    const int C = (int)h->p.format;
    dips_sched::Geom q;
    if (regional_fast_path(h))
        q = dips_sched::background_geometry(frame_bytes(h, width, height), n_frames, unroll, g.w, g.h, [&](bool small_tile) {
            return resident_waves(h, kernel_ptr(C, (int)h->p.chroma_filter, small_tile));
        });
    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    if (q.ok) {
        DIPS_TRY(for_frame_end_tail_rows(width, height, g, [&](uint32_t r, uint32_t i0) {
            return launch_generic(r, 1u, (g.w - 1u) >> 5, 1u, i0);
        }));
        DIPS_TRY(launch_fast(q));
    } else {
        const uint64_t wpr = mask_words_per_row(g.w);
        if ((uint64_t)g.h * wpr >= (1ull << 31))
            return fail(h, DIPS_ERR_INVALID, std::string(name) + ": region too large for the generic kernel");
        DIPS_TRY(launch_generic(0u, g.h, 0u, (uint32_t)wpr, 0u));
    }
    return span.end(s);
}

// What the two models' argument structs, fast and generic, have in common.
template <typename Args>
Args model_args(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                const uint8_t* ref0, const dips::GridSpec& g, bool accumulate, uint8_t* mask) {
    Args a{};
    a.frames = frames;
    a.ref0 = ref0;
    a.mask = mask;
    a.frame_bytes = (decltype(a.frame_bytes))frame_bytes(h, width, height);
    a.mask_frame_bytes = (decltype(a.mask_frame_bytes))(mask_words_per_row(g.w) * g.h * 4u);
    a.width = width;
    a.n_frames = n_frames;
    a.accumulate = accumulate ? 1u : 0u;
    a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
    return a;
}

// The words and the state columns a launch of a model's generic kernel covers.
template <typename Args>
void model_generic_span(Args& a, const dips_handle* h, uint32_t row0, uint32_t n_rows, uint32_t word0, uint32_t n_words,
                        uint32_t state_x0) {
    a.chroma = h->p.format == DIPS_FMT_GRAY8 ? 0u : h->p.chroma_filter;
    a.row0 = row0;
    a.n_rows = n_rows;
    a.word0 = word0;
    a.n_words = n_words;
    a.state_x0 = state_x0;
}

// Run the background model on device pointers, asynchronously on `s`.  ref0:
// the initial state's bytes (accumulate false), else unused.  n_frames may be
// 0 (accumulate false: the initial state is written).
dips_status run_background_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                  uint32_t n_frames, const uint8_t* ref0, const dips::GridSpec& g, uint32_t rate_shift,
                                  bool selective, bool accumulate, uint16_t* background, uint8_t* mask, hipStream_t s) {
    const int C = (int)h->p.format;
    auto launch_generic = [&](uint32_t row0, uint32_t n_rows, uint32_t word0, uint32_t n_words,
                              uint32_t state_x0) -> dips_status {
        auto a = model_args<dips::BgGenericArgs>(h, width, height, frames, n_frames, ref0, g, accumulate, mask);
        model_generic_span(a, h, row0, n_rows, word0, n_words, state_x0);
        a.background = background;
        a.tau = h->p.tau;
        a.rate_shift = rate_shift;
        a.selective = selective ? 1u : 0u;
        DIPS_HIP(h, dips::launch_background_generic(a, C, s));
        return DIPS_OK;
    };
    auto launch_fast = [&](const dips_sched::Geom& q) -> dips_status {
        auto a = model_args<dips::BgArgs>(h, width, height, frames, n_frames, ref0, g, accumulate, mask);
        a.background = background;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.rate_shift = rate_shift;
        a.selective = selective ? 1u : 0u;
        a.thr = dips::series_threshold(C, h->p.tau, 0);
        DIPS_HIP(h, dips::launch_series_background(a, C, (int)h->p.chroma_filter, q.small_tile, (uint32_t)q.blocks, s));
        return DIPS_OK;
    };
    return run_model_device(h, "diff_background_mask", width, height, n_frames, g, dips::series_background_kernel_ptr,
                            dips::kUnrollBackground, launch_generic, launch_fast, s);
}

// ---------------------------------------------------------------------------
// The Sigma-Delta background and its per-pixel adaptive threshold mask
// (dips_diff_sigma_delta_mask; kernels in series_sigma_delta.hip)
// ---------------------------------------------------------------------------

// Run the Sigma-Delta model on device pointers, asynchronously on `s`.  ref0:
// the frame the initial M is taken from (accumulate false), else unused.
// n_frames may be 0 (accumulate false: the initial state is written).
dips_status run_sigma_delta_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                   uint32_t n_frames, const uint8_t* ref0, const dips::GridSpec& g, uint32_t n_amp,
                                   uint32_t v_min, uint32_t v_max, bool accumulate, uint16_t* state, uint8_t* mask,
                                   hipStream_t s) {
    const int C = (int)h->p.format;
    auto model = [&](auto& a) {
        a.state = state;
        a.n_amp = n_amp;
        a.v_min = v_min;
        a.v_max = v_max;
    };
    auto launch_generic = [&](uint32_t row0, uint32_t n_rows, uint32_t word0, uint32_t n_words,
                              uint32_t state_x0) -> dips_status {
        auto a = model_args<dips::SdGenericArgs>(h, width, height, frames, n_frames, ref0, g, accumulate, mask);
        model_generic_span(a, h, row0, n_rows, word0, n_words, state_x0);
        model(a);
        DIPS_HIP(h, dips::launch_sigma_delta_generic(a, C, s));
        return DIPS_OK;
    };
    auto launch_fast = [&](const dips_sched::Geom& q) -> dips_status {
        auto a = model_args<dips::SdArgs>(h, width, height, frames, n_frames, ref0, g, accumulate, mask);
        model(a);
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        DIPS_HIP(h, dips::launch_series_sigma_delta(a, C, (int)h->p.chroma_filter, q.small_tile, (uint32_t)q.blocks, s));
        return DIPS_OK;
    };
    return run_model_device(h, "diff_sigma_delta_mask", width, height, n_frames, g, dips::series_sigma_delta_kernel_ptr,
                            dips::kUnrollSigmaDelta, launch_generic, launch_fast, s);
}

// ---------------------------------------------------------------------------
// The change times per pixel (dips_diff_pixel_times; kernels in
// series_times.hip)
// ---------------------------------------------------------------------------

// the parts' summaries (20 bytes per pixel and part) stay within this
constexpr uint64_t kTimesPartsBytes = 1ull << 30;

// The schedule of the fast change-times kernel (series_sched.h times_geometry).
dips_sched::Geom times_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf,
                                const dips::GridSpec& g) {
    return dips_sched::times_geometry(frame_bytes(h, width, height), n_frames, dips::kUnrollTimes, g.w, g.h,
                                      kTimesPartsBytes, pixel_part_pin(), [&](bool multi_part) {
        return resident_waves(h, dips::series_times_kernel_ptr(C, (int)h->p.chroma_filter, pf, multi_part));
    });
}

// Run the change times on device pointers, asynchronously on `s`.
dips_status run_times_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                             const uint8_t* ref0, const dips::GridSpec& g, uint32_t t0, bool accumulate,
                             uint32_t* times, hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t fb = frame_bytes(h, width, height);
    const dips::GridRect roi{g.x, g.y, g.w, g.h};
    dips_sched::Geom q;
    if (regional_fast_path(h)) q = times_geometry(h, width, height, n_frames, C, pf, g);
    auto launch_generic = [&](const dips::GridRect& rect) -> dips_status {
        dips::TimesGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.times = times;
        a.frame_bytes = fb;
        a.width = width;
        a.n_frames = n_frames;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.t0 = t0;
        a.accumulate = accumulate ? 1u : 0u;
        a.roi = roi;
        a.rect = rect;
        DIPS_HIP(h, dips::launch_times_generic(a, C, s));
        return DIPS_OK;
    };
    // the summaries' buffer before the timed span (growing it synchronises)
    if (q.ok && q.parts > 1) DIPS_HIP(h, h->times_parts.ensure((size_t)q.parts * 20u * (size_t)g.w * g.h));

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    if (q.ok) {
        const bool mp = q.parts > 1;
        dips::TimesArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.out = mp ? h->times_parts.as<uint32_t>() : times;
        a.frame_bytes = (uint32_t)fb;
        a.width = width;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.part_frames = q.part_frames;
        a.t0 = t0;
        a.accumulate = !mp && accumulate ? 1u : 0u;
        a.thr = dips::series_threshold(C, h->p.tau, 0);
        a.roi = roi;
        DIPS_HIP(h, dips::launch_series_times(a, C, (int)h->p.chroma_filter, pf, mp, (uint32_t)q.blocks, s));
        if (mp) {
            // the parts in order onto the initial or accumulated state: a
            // later launch, so every summary is written before it is read
            dips::TimesCombineArgs c{};
            c.parts = h->times_parts.as<uint32_t>();
            c.times = times;
            c.frame_bytes = (uint32_t)fb;
            c.width = width;
            c.channels = (uint32_t)C;
            c.n_frames = n_frames;
            c.part_frames = q.part_frames;
            c.accumulate = accumulate ? 1u : 0u;
            c.roi = roi;
            DIPS_HIP(h, dips::launch_times_combine(c, s));
        }
        // the vecs the fast kernel leaves out (series_times.hip): neither it
        // nor the combine touches their <= 3 pixels each
        DIPS_TRY(for_frame_end_tail_rows(width, height, g, [&](uint32_t r, uint32_t i0) {
            return launch_generic(dips::GridRect{g.x + i0, g.y + r, g.w - i0, 1u});
        }));
    } else {
        DIPS_TRY(launch_generic(roi));
    }
    return span.end(s);
}

// What dips_diff_background_mask and dips_diff_sigma_delta_mask do once their
// own parameters are checked: the validation the two models share (messages
// under the exported function's `name`; `state_name` is what its header calls
// the state array of `state_planes` u16 planes), then run(frames, ref0,
// region, state, mask) on the caller's device pointers or on staged copies
// of its host arrays.
template <typename Run>
dips_status model_mask_call(dips_handle* h, const char* name, const char* state_name, uint32_t width, uint32_t height,
                            const uint8_t* frames, uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, bool acc,
                            uint16_t* state, size_t state_planes, uint8_t* mask, Run&& run) {
    const std::string pre = std::string(name) + ": ";
    if (!state || (!frames && n_frames > 0)) return fail(h, DIPS_ERR_INVALID, pre + "null argument");
    if (acc && ref) return fail(h, DIPS_ERR_INVALID, pre + "ref must be NULL when accumulating");
    if (!acc && !ref && n_frames == 0) return fail(h, DIPS_ERR_INVALID, pre + "the initial state needs ref or a frame");
    dips::GridSpec g{};
    if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g)) return fail(h, DIPS_ERR_INVALID, pre + why);
    const uint64_t n_px = (uint64_t)g.w * g.h;
    if (n_px >= (1ull << 30)) return fail(h, DIPS_ERR_INVALID, pre + "the region must stay below 2^30 pixels");
    const bool dev = (h->p.flags & DIPS_FLAG_DEVICE_PTRS) != 0;
    if (dev && ((uintptr_t)state & 1u) != 0)
        return fail(h, DIPS_ERR_INVALID, pre + "the device " + state_name + " must be 2-byte aligned");
    if (dev && ((uintptr_t)mask & 3u) != 0)
        return fail(h, DIPS_ERR_INVALID, pre + "the device mask must be 4-byte aligned");
    if (n_frames == 0 && acc) return DIPS_OK;  // nothing to fold
    if (dev) return run(frames, acc ? nullptr : (ref ? ref : frames), g, state, mask);
    // host pointers: stage through HBM (synchronous call)
    const uint64_t fb = frame_bytes(h, width, height);
    const size_t total = (size_t)fb * n_frames;
    const size_t state_bytes = sizeof(uint16_t) * state_planes * (size_t)n_px;
    const size_t mask_bytes = mask ? (size_t)(4u * mask_words_per_row(g.w) * g.h) * n_frames : 0u;
    DIPS_HIP(h, h->stage_map.ensure(mask_bytes));
    const uint8_t *frames_dev, *ref_dev;
    DIPS_TRY(stage_host_frames(h, frames, total, ref, fb, h->stage_series, state_bytes, &frames_dev, &ref_dev));
    if (acc) DIPS_HIP(h, hipMemcpyAsync(h->stage_series.p, state, state_bytes, hipMemcpyHostToDevice, h->stream));
    DIPS_TRY(run(frames_dev, acc ? nullptr : ref_dev, g, h->stage_series.as<uint16_t>(),
                 mask_bytes ? h->stage_map.as<uint8_t>() : nullptr));
    DIPS_HIP(h, hipMemcpyAsync(state, h->stage_series.p, state_bytes, hipMemcpyDeviceToHost, h->stream));
    if (mask_bytes) DIPS_HIP(h, hipMemcpyAsync(mask, h->stage_map.p, mask_bytes, hipMemcpyDeviceToHost, h->stream));
    DIPS_HIP(h, hipStreamSynchronize(h->stream));
    return DIPS_OK;
}

}  // namespace

extern "C" {

dips_status dips_grid_cell(uint32_t width, uint32_t height, const uint32_t* roi, uint32_t rows, uint32_t cols,
                           uint32_t row, uint32_t col, uint32_t* rect) {
    return guard(nullptr, [&]() -> dips_status {
        dips::GridSpec g{};
        if (!rect || grid_spec(width, height, roi, rows, cols, &g) != nullptr || row >= rows || col >= cols)
            return DIPS_ERR_INVALID;
        const dips::GridRect r = dips::grid_cell_rect(g, row, col);
        rect[0] = r.x;
        rect[1] = r.y;
        rect[2] = r.w;
        rect[3] = r.h;
        return DIPS_OK;
    });
}

dips_status dips_diff_series_grid(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                  uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t rows,
                                  uint32_t cols, dips_series_entry* cells) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!frames || !cells) return fail(h, DIPS_ERR_INVALID, "diff_series_grid: null argument");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, rows, cols, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_series_grid: ") + why);
        const uint64_t n_cells = (uint64_t)rows * cols;
        if (n_cells >= (1ull << 30) || n_cells * n_frames >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_series_grid: n_frames * rows * cols must stay below 2^30 entries");
        const uint64_t fb = frame_bytes(h, width, height);
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS)
            return run_grid_device(h, width, height, frames, n_frames, ref ? ref : frames, g, cells, h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        const size_t out_bytes = sizeof(dips_series_entry) * (size_t)(n_cells * n_frames);
        const uint8_t *frames_dev, *ref_dev;
        DIPS_TRY(stage_host_frames(h, frames, total, ref, fb, h->stage_series, out_bytes, &frames_dev, &ref_dev));
        st = run_grid_device(h, width, height, frames_dev, n_frames, ref_dev, g,
                             h->stage_series.as<dips_series_entry>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(cells, h->stage_series.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_diff_pixel_sums(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                 uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t accumulate,
                                 dips_series_entry* sums) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (!sums || (!frames && n_frames > 0)) return fail(h, DIPS_ERR_INVALID, "diff_pixel_sums: null argument");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_pixel_sums: ") + why);
        const uint64_t n_px = (uint64_t)g.w * g.h;
        if (n_px >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_pixel_sums: the region must stay below 2^30 pixels");
        const size_t out_bytes = sizeof(dips_series_entry) * (size_t)n_px;
        const bool dev = (h->p.flags & DIPS_FLAG_DEVICE_PTRS) != 0;
        if (n_frames == 0) {
            // nothing to add: an overwriting call leaves zeros
            if (accumulate != 0u) return DIPS_OK;
            if (dev)
                DIPS_HIP(h, hipMemsetAsync(sums, 0, out_bytes, h->stream));
            else
                std::memset(sums, 0, out_bytes);
            return DIPS_OK;
        }
        const uint64_t fb = frame_bytes(h, width, height);
        if (dev)
            return run_pixels_device(h, width, height, frames, n_frames, ref ? ref : frames, g, accumulate != 0u, sums,
                                     h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        const uint8_t *frames_dev, *ref_dev;
        DIPS_TRY(stage_host_frames(h, frames, total, ref, fb, h->stage_series, out_bytes, &frames_dev, &ref_dev));
        if (accumulate != 0u)
            DIPS_HIP(h, hipMemcpyAsync(h->stage_series.p, sums, out_bytes, hipMemcpyHostToDevice, h->stream));
        st = run_pixels_device(h, width, height, frames_dev, n_frames, ref_dev, g, accumulate != 0u,
                               h->stage_series.as<dips_series_entry>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(sums, h->stage_series.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

uint32_t dips_mask_row_bytes(uint32_t roi_w) {
    return guard(nullptr, [&]() -> uint32_t { return (uint32_t)(4u * mask_words_per_row(roi_w)); });
}

dips_status dips_diff_change_mask(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                  uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint8_t* mask) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!frames || !mask) return fail(h, DIPS_ERR_INVALID, "diff_change_mask: null argument");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_change_mask: ") + why);
        if ((uint64_t)g.w * g.h >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_change_mask: the region must stay below 2^30 pixels");
        const uint64_t fb = frame_bytes(h, width, height);
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            if (((uintptr_t)mask & 3u) != 0)
                return fail(h, DIPS_ERR_INVALID, "diff_change_mask: the device mask must be 4-byte aligned");
            return run_mask_device(h, width, height, frames, n_frames, ref ? ref : frames, g, mask, h->stream);
        }
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        const size_t out_bytes = (size_t)(4u * mask_words_per_row(g.w) * g.h) * n_frames;
        const uint8_t *frames_dev, *ref_dev;
        DIPS_TRY(stage_host_frames(h, frames, total, ref, fb, h->stage_map, out_bytes, &frames_dev, &ref_dev));
        st = run_mask_device(h, width, height, frames_dev, n_frames, ref_dev, g,
                             h->stage_map.as<uint8_t>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(mask, h->stage_map.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_diff_pixel_times(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                  uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t t0,
                                  uint32_t accumulate, uint32_t* times) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (!times || (!frames && n_frames > 0)) return fail(h, DIPS_ERR_INVALID, "diff_pixel_times: null argument");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_pixel_times: ") + why);
        const uint64_t n_px = (uint64_t)g.w * g.h;
        if (n_px >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_pixel_times: the region must stay below 2^30 pixels");
        if ((uint64_t)t0 + n_frames > 0xFFFFFFFFull)
            return fail(h, DIPS_ERR_INVALID,
                        "diff_pixel_times: t0 + n_frames must stay below 2^32 (index 0xFFFFFFFF is DIPS_TIME_NONE)");
        const bool dev = (h->p.flags & DIPS_FLAG_DEVICE_PTRS) != 0;
        if (dev && ((uintptr_t)times & 3u) != 0)
            return fail(h, DIPS_ERR_INVALID, "diff_pixel_times: the device times must be 4-byte aligned");
        const size_t plane_bytes = sizeof(uint32_t) * (size_t)n_px;
        const size_t out_bytes = DIPS_TIMES_PLANES * plane_bytes;
        if (n_frames == 0) {
            // nothing to fold: an overwriting call leaves the initial state
            if (accumulate != 0u) return DIPS_OK;
            uint8_t* b = reinterpret_cast<uint8_t*>(times);
            if (dev) {
                DIPS_HIP(h, hipMemsetAsync(b, 0xFF, 2u * plane_bytes, h->stream));
                DIPS_HIP(h, hipMemsetAsync(b + 2u * plane_bytes, 0, 2u * plane_bytes, h->stream));
            } else {
                std::memset(b, 0xFF, 2u * plane_bytes);
                std::memset(b + 2u * plane_bytes, 0, 2u * plane_bytes);
            }
            return DIPS_OK;
        }
        const uint64_t fb = frame_bytes(h, width, height);
        if (dev)
            return run_times_device(h, width, height, frames, n_frames, ref ? ref : frames, g, t0, accumulate != 0u,
                                    times, h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        const uint8_t *frames_dev, *ref_dev;
        DIPS_TRY(stage_host_frames(h, frames, total, ref, fb, h->stage_series, out_bytes, &frames_dev, &ref_dev));
        if (accumulate != 0u)
            DIPS_HIP(h, hipMemcpyAsync(h->stage_series.p, times, out_bytes, hipMemcpyHostToDevice, h->stream));
        st = run_times_device(h, width, height, frames_dev, n_frames, ref_dev, g, t0,
                              accumulate != 0u, h->stage_series.as<uint32_t>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(times, h->stage_series.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_diff_background_mask(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                      uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t rate_shift,
                                      uint32_t bg_flags, uint32_t accumulate, uint16_t* background, uint8_t* mask) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (rate_shift > DIPS_BG_MAX_RATE_SHIFT)
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: rate_shift must be 0 .. 8");
        if ((bg_flags & ~DIPS_BG_SELECTIVE) != 0u)
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: unknown bg_flags bits");
        const bool selective = (bg_flags & DIPS_BG_SELECTIVE) != 0u;
        return model_mask_call(h, "diff_background_mask", "background", width, height, frames, n_frames, ref, roi,
                               accumulate != 0u, background, (size_t)h->p.format, mask,
                               [&](const uint8_t* frames_dev, const uint8_t* ref0, const dips::GridSpec& g,
                                   uint16_t* state_dev, uint8_t* mask_dev) {
                                   return run_background_device(h, width, height, frames_dev, n_frames, ref0, g, rate_shift,
                                                                selective, accumulate != 0u, state_dev, mask_dev, h->stream);
                               });
    });
}

dips_status dips_diff_sigma_delta_mask(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                       uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t n_amp,
                                       uint32_t v_min, uint32_t v_max, uint32_t accumulate, uint16_t* state,
                                       uint8_t* mask) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_amp == 0u || n_amp > DIPS_SD_MAX_AMP)
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: n_amp must be 1 .. 15");
        if (v_min > v_max || v_max > DIPS_SD_MAX_V)
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: 0 <= v_min <= v_max <= 510 is required");
        return model_mask_call(h, "diff_sigma_delta_mask", "state", width, height, frames, n_frames, ref, roi,
                               accumulate != 0u, state, (size_t)DIPS_SD_PLANES, mask,
                               [&](const uint8_t* frames_dev, const uint8_t* ref0, const dips::GridSpec& g,
                                   uint16_t* state_dev, uint8_t* mask_dev) {
                                   return run_sigma_delta_device(h, width, height, frames_dev, n_frames, ref0, g, n_amp, v_min,
                                                                 v_max, accumulate != 0u, state_dev, mask_dev, h->stream);
                               });
    });
}

}  // extern "C"
