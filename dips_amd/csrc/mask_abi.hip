// mask_abi.hip -- host side of include/dips_hip.h, part 5: the products of a
// packed change mask -- its connected components and their shape records,
// the components linked across frames (tracks), the binary morphology, the
// temporal vote, the selection of components with the word-wise logic, and
// the statistics (grid counts, change times and per-pixel sums).  What they
// share with the series and the regional products is in series_host.h.
// The labelling family (components, shapes, select, tracks) takes its rounds
// and its scratch from one plan (mask_scratch.h label_scratch, applied by
// plan_labelling); every entry point is argument checks, its pointers added
// to a HostStaging (mask_host.h, with the checks they share), one call of a
// run_*_device function and finish().
// Every extern "C" body runs inside dips_abi::guard (abi_guard.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "mask_host.h"
#include "mask_scratch.h"

using dips_abi::guard;
using namespace dips_internal;

namespace {

// ---------------------------------------------------------------------------
// The connected components of a mask and their shape records
// (dips_mask_components, dips_mask_shapes; kernels in mask_components.hip and
// mask_shapes.hip)
// ---------------------------------------------------------------------------

// The labelling's view of a w x hgt mask (components and tracks)
dips::ComponentsArgs components_args(uint32_t w, uint32_t hgt, uint32_t connectivity, uint32_t min_area) {
    dips::ComponentsArgs a{};
    a.w = w;
    a.h = hgt;
    a.npx = w * hgt;
    a.wpr = (uint32_t)mask_words_per_row(w);
    a.hw = (w + 1u) / 2u;
    a.nslots = a.hw * hgt;
    a.wpf = a.wpr * hgt;
    a.bpf = (a.wpf + 255u) / 256u;
    a.connectivity = connectivity;
    a.min_area = min_area;
    return a;
}

// What dips_mask_components and dips_mask_tracks check of the region and the
// box count alike, under the exported function's `name`
dips_status check_labelling(dips_handle* h, const char* name, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                            uint32_t connectivity, uint32_t max_boxes) {
    const std::string pre = std::string(name) + ": ";
    if (connectivity != 4u && connectivity != 8u) return fail(h, DIPS_ERR_INVALID, pre + "connectivity must be 4 or 8");
    if (roi_w == 0 || roi_h == 0 || roi_w >= (1u << 24) || roi_h >= (1u << 24))
        return fail(h, DIPS_ERR_INVALID, pre + "roi_w and roi_h must be 1 .. 2^24 - 1");
    if ((uint64_t)roi_w * roi_h >= (1ull << 30))
        return fail(h, DIPS_ERR_INVALID, pre + "the region must stay below 2^30 pixels");
    if ((uint64_t)n_frames * max_boxes * DIPS_BOX_WORDS >= (1ull << 32))
        return fail(h, DIPS_ERR_INVALID, pre + "n_frames * max_boxes * 8 must stay below 2^32");
    return DIPS_OK;
}

// The rounds of a labelling call over n_frames frames, `chunk` per round (0:
// automatic), and its scratch (mask_scratch.h; K: 0, or the tracks'
// max_boxes): the handle's cc_scratch grown to the plan -- before the timed
// span, growing synchronises -- and a's planes pointed into it.
dips_status plan_labelling(dips_handle* h, dips::ComponentsArgs& a, uint32_t n_frames, uint32_t chunk, uint32_t K,
                           dips_sched::LabelScratch* plan) {
    const dips_sched::LabelScratch p = dips_sched::label_scratch(a.npx, a.nslots, a.bpf, n_frames, chunk, K);
    DIPS_HIP(h, h->cc_scratch.ensure((size_t)p.bytes));
    uint8_t* b = h->cc_scratch.as<uint8_t>();
    a.sum_i = reinterpret_cast<uint64_t*>(b + p.sum_i);
    a.sum_j = reinterpret_cast<uint64_t*>(b + p.sum_j);
    a.area = reinterpret_cast<uint32_t*>(b + p.area);
    a.min_x = reinterpret_cast<uint32_t*>(b + p.min_x);
    a.max_x = reinterpret_cast<uint32_t*>(b + p.max_x);
    a.max_y = reinterpret_cast<uint32_t*>(b + p.max_y);
    a.parent = reinterpret_cast<uint32_t*>(b + p.parent);
    a.block_count = reinterpret_cast<uint32_t*>(b + p.block_count);
    *plan = p;
    return DIPS_OK;
}

// Label the frames of a device mask, asynchronously on `s`, `chunk` frames
// per round (0: automatic) in the handle's scratch.  With `shapes`
// (dips_mask_shapes; max_boxes > 0) every round also adds its shape records,
// under `weights` if given (kernel in mask_shapes.hip).
dips_status run_components_device(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t w, uint32_t hgt,
                                  uint32_t connectivity, uint32_t min_area, uint32_t max_boxes, uint32_t chunk,
                                  uint32_t* counts, uint32_t* boxes, uint32_t* labels, hipStream_t s,
                                  const uint8_t* weights = nullptr, uint32_t* shapes = nullptr) {
    dips::ComponentsArgs a = components_args(w, hgt, connectivity, min_area);
    a.max_boxes = max_boxes;
    dips_sched::LabelScratch plan;
    DIPS_TRY(plan_labelling(h, a, n_frames, chunk, 0u, &plan));
    const uint32_t F = plan.F;

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    // the records no component fills are zeros
    if (max_boxes != 0u)
        DIPS_HIP(h, hipMemsetAsync(boxes, 0, sizeof(uint32_t) * DIPS_BOX_WORDS * (size_t)n_frames * max_boxes, s));
    // and the waves of shapes_kernel add onto the shape records
    if (shapes)
        DIPS_HIP(h, hipMemsetAsync(shapes, 0, sizeof(uint32_t) * DIPS_SHAPE_WORDS * (size_t)n_frames * max_boxes, s));
    const size_t frame_words = (size_t)a.wpf;
    for (uint32_t t = 0; t < n_frames; t += F) {
        a.n_frames = std::min(F, n_frames - t);
        a.mask = reinterpret_cast<const uint32_t*>(mask) + (size_t)t * frame_words;
        a.counts = counts + t;
        a.boxes = max_boxes != 0u ? boxes + (size_t)t * max_boxes * DIPS_BOX_WORDS : nullptr;
        a.labels = labels ? labels + (size_t)t * a.npx : nullptr;
        DIPS_HIP(h, dips::launch_mask_components(a, s));
        if (shapes) {
            dips::ShapesArgs g{};
            g.cc = a;
            g.weights = weights ? weights + (size_t)t * a.npx : nullptr;
            g.shapes = shapes + (size_t)t * max_boxes * DIPS_SHAPE_WORDS;
            DIPS_HIP(h, dips::launch_mask_shapes(g, s));
        }
    }
    return span.end(s);
}

// ---------------------------------------------------------------------------
// The components of a mask linked across frames (dips_mask_tracks; kernels in
// mask_components.hip and mask_tracks.hip)
// ---------------------------------------------------------------------------

// the geometry the tracks' kernels share with the labelling's
dips::TracksArgs tracks_args(const dips::ComponentsArgs& a, uint32_t K) {
    dips::TracksArgs tr{};
    tr.w = a.w;
    tr.h = a.h;
    tr.npx = a.npx;
    tr.wpr = a.wpr;
    tr.hw = a.hw;
    tr.nslots = a.nslots;
    tr.wpf = a.wpf;
    tr.bpf = a.bpf;
    tr.K = K;
    return tr;
}

// Label and link the frames of a device mask, asynchronously on `s`, `chunk`
// frames per round (0: automatic) in the handle's scratch.  The parent and
// label planes have one more frame in front, the predecessor of the chunk's
// first frame: prev_mask is labelled into it, and what the runs of a chunk's
// last frame own is copied there for the next chunk.  The next id and the last frame's tracks
// and ages stay in the scratch from chunk to chunk (two buffers, swapped) and
// move from and to `state` by copies in the stream.
dips_status run_tracks_device(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t w, uint32_t hgt,
                              uint32_t connectivity, uint32_t min_area, uint32_t K, uint32_t chunk,
                              const uint8_t* prev_mask, uint32_t* state, uint32_t* counts, uint32_t* boxes,
                              uint32_t* links, hipStream_t s) {
    dips::ComponentsArgs a = components_args(w, hgt, connectivity, min_area);
    dips_sched::LabelScratch plan;
    DIPS_TRY(plan_labelling(h, a, n_frames, chunk, K, &plan));
    const uint32_t F = plan.F;
    uint8_t* scratch = h->cc_scratch.as<uint8_t>();
    const auto at = [scratch](uint64_t off) { return reinterpret_cast<uint32_t*>(scratch + off); };

    dips::TracksArgs tr = tracks_args(a, K);
    tr.parent = at(plan.parent0);  // F + 1 planes
    tr.label = at(plan.label0);    // F + 1 planes
    tr.ov = at(plan.ov);
    tr.cprev = at(plan.cprev);
    tr.hrank = at(plan.hrank);
    tr.heads = at(plan.heads);
    tr.base = at(plan.base);
    tr.next_id = at(plan.next_id);
    uint32_t* prev_count = at(plan.prev_count);
    uint32_t* carry[2] = {at(plan.carry[0]), at(plan.carry[1])};

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    const size_t frame_words = (size_t)a.wpf;
    if (state)
        DIPS_HIP(h, hipMemcpyAsync(tr.next_id, state, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    else
        DIPS_HIP(h, hipMemsetAsync(tr.next_id, 0, sizeof(uint32_t), s));
    if (prev_mask) {
        DIPS_HIP(h, hipMemcpyAsync(carry[0], state + 1, sizeof(uint32_t) * 2u * K, hipMemcpyDeviceToDevice, s));
        // the same labels as the call that held this frame gave it: they do not depend on max_boxes
        a.n_frames = 1;
        a.mask = reinterpret_cast<const uint32_t*>(prev_mask);
        a.counts = prev_count;
        a.boxes = nullptr;
        a.max_boxes = 0;
        DIPS_HIP(h, dips::launch_mask_components(a, s));
        DIPS_HIP(h, dips::launch_mask_tracks_keep(tr, a.mask, 1u, s));
    }
    a.max_boxes = K;
    // the records no component fills are zeros
    DIPS_HIP(h, hipMemsetAsync(boxes, 0, sizeof(uint32_t) * DIPS_BOX_WORDS * (size_t)n_frames * K, s));
    tr.prev0 = reinterpret_cast<const uint32_t*>(prev_mask);
    uint32_t cin = 0;
    for (uint32_t t = 0; t < n_frames; t += F) {
        const uint32_t n = std::min(F, n_frames - t);
        a.n_frames = n;
        a.mask = reinterpret_cast<const uint32_t*>(mask) + (size_t)t * frame_words;
        a.counts = counts + t;
        a.boxes = boxes + (size_t)t * K * DIPS_BOX_WORDS;
        DIPS_HIP(h, dips::launch_mask_components(a, s));
        tr.n_frames = n;
        tr.mask = a.mask;
        tr.counts = a.counts;
        tr.links = links + (size_t)t * K * DIPS_LINK_WORDS;
        tr.carry_in = carry[cin];
        tr.carry_out = carry[cin ^ 1u];
        DIPS_HIP(h, dips::launch_mask_tracks(tr, s));
        cin ^= 1u;
        if (t + n < n_frames) {
            tr.prev0 = a.mask + (size_t)(n - 1u) * frame_words;
            DIPS_HIP(h, dips::launch_mask_tracks_keep(tr, tr.prev0, n, s));
        }
    }
    if (state) {
        DIPS_HIP(h, hipMemcpyAsync(state, tr.next_id, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        DIPS_HIP(h, hipMemcpyAsync(state + 1, carry[cin], sizeof(uint32_t) * 2u * K, hipMemcpyDeviceToDevice, s));
    }
    return span.end(s);
}

// ---------------------------------------------------------------------------
// The binary morphology of a mask (dips_mask_morph; kernel in mask_morph.hip)
// ---------------------------------------------------------------------------

// One launch over the frames of a device mask, asynchronously on `s`.
dips_status run_morph_device(dips_handle* h, const uint8_t* mask_in, uint32_t n_frames, uint32_t w, uint32_t hgt,
                             uint32_t op, uint32_t shape, uint32_t rx, uint32_t ry, uint8_t* mask_out,
                             hipStream_t s) {
    dips::MorphArgs a{};
    a.in = reinterpret_cast<const uint32_t*>(mask_in);
    a.out = reinterpret_cast<uint32_t*>(mask_out);
    a.w = w;
    a.h = hgt;
    a.wpr = (uint32_t)mask_words_per_row(w);
    a.n_frames = n_frames;
    a.op = op;
    a.shape = shape;
    a.rx = rx;
    a.ry = ry;
    dips::mask_morph_tiling(w, hgt, &a.tiles_x, &a.tiles_y);
    a.items = (uint64_t)n_frames * a.tiles_x * a.tiles_y;

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    DIPS_HIP(h, dips::launch_mask_morph(a, s));
    return span.end(s);
}

// ---------------------------------------------------------------------------
// The temporal m-of-k vote on a mask (dips_mask_vote; kernels in
// mask_vote.hip)
// ---------------------------------------------------------------------------

// The vote over the frames of a device mask and the next history, each one
// launch, asynchronously on `s`.  hist_in NULL: clear frames before the clip;
// hist_out NULL: no next history.  n_frames may be 0 (then only the history).
dips_status run_vote_device(dips_handle* h, const uint8_t* mask_in, uint32_t n_frames, uint32_t w, uint32_t hgt,
                            uint32_t window, uint32_t votes, const uint8_t* hist_in, uint8_t* hist_out,
                            uint8_t* mask_out, hipStream_t s) {
    dips::VoteArgs a{};
    a.in = reinterpret_cast<const uint32_t*>(mask_in);
    a.hist_in = reinterpret_cast<const uint32_t*>(hist_in);
    a.out = reinterpret_cast<uint32_t*>(mask_out);
    a.hist_out = reinterpret_cast<uint32_t*>(hist_out);
    a.w = w;
    a.wpr = (uint32_t)mask_words_per_row(w);
    a.wpf = a.wpr * hgt;
    a.n_frames = n_frames;
    a.window = window;
    a.votes = votes;
    dips_sched::Geom q;
    if (n_frames != 0) {
        q = dips_sched::vote_geometry(a.wpf, n_frames, window, dips::kVoteWords,
                                      resident_waves(h, dips::mask_vote_kernel_ptr()));
        if (!q.ok) return fail(h, DIPS_ERR_HIP, "mask_vote: no schedule for this mask");
        a.part_frames = q.part_frames;
        a.parts = q.parts;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
    }
    if (n_frames == 0 && !hist_out) return DIPS_OK;

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    if (n_frames != 0) DIPS_HIP(h, dips::launch_mask_vote(a, (uint32_t)q.blocks, s));
    if (hist_out) DIPS_HIP(h, dips::launch_mask_vote_history(a, s));
    return span.end(s);
}

// ---------------------------------------------------------------------------
// The selection of components of a mask and the logic of two masks
// (dips_mask_select, dips_mask_logic; kernels in mask_components.hip and
// mask_select.hip)
// ---------------------------------------------------------------------------

// Label the frames of a device mask and write the components selected,
// asynchronously on `s`, `chunk` frames per round (0: automatic) in the
// handle's scratch, planned as for run_components_device.  marker
// NULL: none; else marker_frames (1 or n_frames) frames.  counts NULL: none.
dips_status run_select_device(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t w, uint32_t hgt,
                              uint32_t connectivity, uint32_t min_area, uint32_t max_area, uint32_t select,
                              const uint8_t* marker, uint32_t marker_frames, uint32_t chunk, uint8_t* mask_out,
                              uint32_t* counts, hipStream_t s) {
    dips::SelectArgs g{};
    dips::ComponentsArgs& a = g.cc;
    a = components_args(w, hgt, connectivity, min_area);
    g.max_area = max_area;
    g.select = select;
    g.marker_stride = marker && marker_frames != 1u ? a.wpf : 0u;
    dips_sched::LabelScratch plan;
    DIPS_TRY(plan_labelling(h, a, n_frames, chunk, 0u, &plan));
    const uint32_t F = plan.F;

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    // the blocks of sel_write_kernel add onto the counts
    if (counts) DIPS_HIP(h, hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)n_frames, s));
    const size_t frame_words = (size_t)a.wpf;
    for (uint32_t t = 0; t < n_frames; t += F) {
        a.n_frames = std::min(F, n_frames - t);
        a.mask = reinterpret_cast<const uint32_t*>(mask) + (size_t)t * frame_words;
        g.marker = marker ? reinterpret_cast<const uint32_t*>(marker) + (size_t)t * g.marker_stride : nullptr;
        g.out = reinterpret_cast<uint32_t*>(mask_out) + (size_t)t * frame_words;
        g.counts = counts ? counts + t : nullptr;
        DIPS_HIP(h, dips::launch_mask_labelling(a, s));
        DIPS_HIP(h, dips::launch_mask_select(g, s));
    }
    return span.end(s);
}

// The logic of two device masks, asynchronously on `s`: one launch.
dips_status run_logic_device(dips_handle* h, const uint8_t* a_in, uint32_t n_frames, uint32_t w, uint32_t hgt,
                             uint32_t op, const uint8_t* b_in, uint32_t b_frames, uint8_t* mask_out, hipStream_t s) {
    dips::LogicArgs g{};
    g.a = reinterpret_cast<const uint32_t*>(a_in);
    g.b = reinterpret_cast<const uint32_t*>(b_in);
    g.out = reinterpret_cast<uint32_t*>(mask_out);
    g.w = w;
    g.wpr = (uint32_t)mask_words_per_row(w);
    g.wpf = g.wpr * hgt;
    g.words = (uint64_t)g.wpf * n_frames;
    g.op = op;
    g.b_bcast = b_in && b_frames == 1u && n_frames != 1u ? 1u : 0u;

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    DIPS_HIP(h, dips::launch_mask_logic(g, s));
    return span.end(s);
}

// ---------------------------------------------------------------------------
// The statistics of a mask (dips_mask_counts, dips_mask_pixel_times; kernels
// in mask_stats.hip)
// ---------------------------------------------------------------------------

// the parts' summaries of dips_mask_pixel_times stay within this (the handle's times_parts)
constexpr uint64_t kMaskTimesPartsBytes = 1ull << 30;

// The grid counts of a device mask, asynchronously on `s`: the clear of
// counts where several blocks add to a cell, and one launch.
dips_status run_counts_device(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t w, uint32_t hgt,
                              uint32_t rows, uint32_t cols, uint32_t* counts, hipStream_t s) {
    const uint64_t resident = (uint64_t)std::max(0, occupancy_blocks(h, dips::mask_counts_kernel_ptr())) * h->cu_count;
    const dips_sched::CountsGeom q = dips_sched::mask_counts_geometry(
        w, hgt, rows, cols, n_frames, dips::kCountsChunkCells, dips::kCountsMinBandWords, resident);
    if (!q.ok) return fail(h, DIPS_ERR_HIP, "mask_counts: no schedule for this mask");
    dips::MaskCountsArgs a{};
    a.mask = reinterpret_cast<const uint32_t*>(mask);
    a.counts = counts;
    a.items = q.items;
    a.w = w;
    a.h = hgt;
    a.wpr = (uint32_t)mask_words_per_row(w);
    a.n_frames = n_frames;
    a.rows = rows;
    a.cols = cols;
    a.col_chunks = q.col_chunks;
    a.bands = q.bands;
    a.band_rows = q.band_rows;

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    if (q.bands > 1u) DIPS_HIP(h, hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)n_frames * rows * cols, s));
    DIPS_HIP(h, dips::launch_mask_counts(a, (uint32_t)q.blocks, s));
    return span.end(s);
}

// The change times and / or sums of a device mask, asynchronously on `s`:
// one launch, and the fold of the parts where the frames are cut; with no
// frames the initial state.  times or sums may be NULL, not both.
dips_status run_mask_times_device(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t w, uint32_t hgt,
                                  uint32_t t0, bool accumulate, uint32_t* times, uint32_t* sums, hipStream_t s) {
    const size_t npx = (size_t)w * hgt;
    if (n_frames == 0) {
        if (accumulate) return DIPS_OK;
        KernelSpan span(h);
        DIPS_TRY(span.begin(s));
        if (times) {
            DIPS_HIP(h, hipMemsetAsync(times, 0xFF, sizeof(uint32_t) * 2u * npx, s));  // first, last = DIPS_TIME_NONE
            DIPS_HIP(h, hipMemsetAsync(times + 2u * npx, 0, sizeof(uint32_t) * 2u * npx, s));
        }
        if (sums) DIPS_HIP(h, hipMemsetAsync(sums, 0, sizeof(uint32_t) * npx, s));
        return span.end(s);
    }
    dips::MaskTimesArgs a{};
    a.mask = mask;
    a.times = times;
    a.sums = sums;
    a.w = w;
    a.h = hgt;
    a.row_bytes = (uint32_t)(4u * mask_words_per_row(w));
    a.frame_bytes = a.row_bytes * hgt;
    a.n_frames = n_frames;
    a.t0 = t0;
    a.accumulate = accumulate ? 1u : 0u;
    const uint64_t summary = sizeof(uint32_t) * ((times ? 5u : 0u) + (sums ? 1u : 0u)) * (uint64_t)npx;
    // the slots of the several-parts form: that is the form the parts would run
    dips_sched::Geom q = dips_sched::mask_times_geometry(
        (uint64_t)a.frame_bytes * (8 / dips::kMaskTimesPx), n_frames, summary, kMaskTimesPartsBytes,
        resident_waves(h, dips::mask_times_kernel_ptr(times != nullptr, sums != nullptr, true)));
    if (q.ok && q.parts == 1u)
        q = dips_sched::mask_times_geometry(
            (uint64_t)a.frame_bytes * (8 / dips::kMaskTimesPx), n_frames, summary, 0u,
            resident_waves(h, dips::mask_times_kernel_ptr(times != nullptr, sums != nullptr, false)));
    if (!q.ok) return fail(h, DIPS_ERR_HIP, "mask_pixel_times: no schedule for this mask");
    a.part_frames = q.part_frames;
    a.n_parts = q.parts;
    a.n_tiles = (uint32_t)q.n_tiles;
    a.n_waves = (uint32_t)q.n_waves;
    // the scratch before the timed span (growing it synchronises)
    if (q.parts > 1u) {
        DIPS_HIP(h, h->times_parts.ensure((size_t)(summary * q.parts)));
        a.parts = h->times_parts.as<uint32_t>();
    }

    KernelSpan span(h);
    DIPS_TRY(span.begin(s));
    DIPS_HIP(h, dips::launch_mask_times(a, (uint32_t)q.blocks, s));
    if (q.parts > 1u) DIPS_HIP(h, dips::launch_mask_times_combine(a, s));
    return span.end(s);
}

}  // namespace

extern "C" {

dips_status dips_mask_counts(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                             uint32_t rows, uint32_t cols, uint32_t* counts) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        DIPS_TRY(check_mask_region(h, "mask_counts", roi_w, roi_h));
        if (rows == 0 || cols == 0) return fail(h, DIPS_ERR_INVALID, "mask_counts: rows and cols must be at least 1");
        if (rows > roi_h || cols > roi_w)
            return fail(h, DIPS_ERR_INVALID,
                        "mask_counts: more rows or cols than the region has pixels (a cell would be empty)");
        if ((uint64_t)n_frames * rows * cols >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_counts: n_frames * rows * cols must stay below 2^30");
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts) return fail(h, DIPS_ERR_INVALID, "mask_counts: null argument");
        const size_t mask_bytes = mask_frame_bytes(roi_w, roi_h) * n_frames;
        const size_t counts_bytes = sizeof(uint32_t) * (size_t)n_frames * rows * cols;
        if (outputs_overlap({{counts, counts_bytes}}, {{mask, mask_bytes}}))
            return fail(h, DIPS_ERR_INVALID, "mask_counts: counts must not overlap mask");
        HostStaging sg(h, "mask_counts");
        sg.add(h->stage_frames, mask, mask_bytes, sg.kIn);
        sg.add(h->stage_series, counts, counts_bytes, sg.kOut);
        DIPS_TRY(sg.begin());
        DIPS_TRY(run_counts_device(h, mask, n_frames, roi_w, roi_h, rows, cols, counts, h->stream));
        return sg.finish();
    });
}

dips_status dips_mask_pixel_times(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w,
                                  uint32_t roi_h, uint32_t t0, uint32_t accumulate, uint32_t* times, uint32_t* sums) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        if (!times && !sums) return fail(h, DIPS_ERR_INVALID, "mask_pixel_times: times and sums are both null");
        if (!mask && n_frames > 0) return fail(h, DIPS_ERR_INVALID, "mask_pixel_times: null argument");
        DIPS_TRY(check_mask_region(h, "mask_pixel_times", roi_w, roi_h));
        if (times && (uint64_t)t0 + n_frames > 0xFFFFFFFFull)
            return fail(h, DIPS_ERR_INVALID,
                        "mask_pixel_times: t0 + n_frames must stay below 2^32 (index 0xFFFFFFFF is DIPS_TIME_NONE)");
        const size_t npx = (size_t)roi_w * roi_h;
        const size_t mask_bytes = mask_frame_bytes(roi_w, roi_h) * n_frames;
        const size_t times_bytes = times ? sizeof(uint32_t) * DIPS_TIMES_PLANES * npx : 0u;
        const size_t sums_bytes = sums ? sizeof(uint32_t) * npx : 0u;
        if (outputs_overlap({{times, times_bytes}, {sums, sums_bytes}}, {{mask, mask_bytes}}))
            return fail(h, DIPS_ERR_INVALID, "mask_pixel_times: an output must not overlap the mask or the other output");
        if (n_frames == 0) mask = nullptr;
        // the sums behind the times, the state uploaded first when accumulating
        HostStaging sg(h, "mask_pixel_times");
        const unsigned state = accumulate != 0u ? sg.kInOut : sg.kOut;
        sg.add(h->stage_frames, mask, mask_bytes, sg.kIn);
        sg.add(h->stage_series, times, times_bytes, state);
        sg.add(h->stage_series, sums, sums_bytes, state);
        DIPS_TRY(sg.check_aligned4());
        if (n_frames == 0 && accumulate != 0u) return DIPS_OK;  // nothing to add: nothing is staged
        DIPS_TRY(sg.upload());
        DIPS_TRY(run_mask_times_device(h, mask, n_frames, roi_w, roi_h, t0, accumulate != 0u, times, sums, h->stream));
        return sg.finish();
    });
}

dips_status dips_mask_components(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w,
                                 uint32_t roi_h, uint32_t connectivity, uint32_t min_area, uint32_t max_boxes,
                                 uint32_t chunk_frames, uint32_t* counts, uint32_t* boxes, uint32_t* labels) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts || (!boxes && max_boxes != 0u))
            return fail(h, DIPS_ERR_INVALID, "mask_components: null argument");
        DIPS_TRY(check_labelling(h, "mask_components", n_frames, roi_w, roi_h, connectivity, max_boxes));
        if (max_boxes == 0u) boxes = nullptr;
        const size_t counts_bytes = sizeof(uint32_t) * (size_t)n_frames;
        // counts and boxes share one buffer
        HostStaging sg(h, "mask_components");
        sg.add(h->stage_frames, mask, mask_frame_bytes(roi_w, roi_h) * n_frames, sg.kIn);
        sg.add(h->stage_series, counts, counts_bytes, sg.kOut);
        sg.add(h->stage_series, boxes, counts_bytes * DIPS_BOX_WORDS * max_boxes, sg.kOut);
        sg.add(h->stage_map, labels, counts_bytes * roi_w * roi_h, sg.kOut);
        DIPS_TRY(sg.begin());
        DIPS_TRY(run_components_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes,
                                       chunk_frames, counts, boxes, labels, h->stream));
        return sg.finish();
    });
}

dips_status dips_mask_shapes(dips_handle* h, const uint8_t* mask, const uint8_t* weights, uint32_t n_frames,
                             uint32_t roi_w, uint32_t roi_h, uint32_t connectivity, uint32_t min_area,
                             uint32_t max_boxes, uint32_t chunk_frames, uint32_t* counts, uint32_t* boxes,
                             uint32_t* shapes) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts || ((!boxes || !shapes) && max_boxes != 0u))
            return fail(h, DIPS_ERR_INVALID, "mask_shapes: null argument");
        DIPS_TRY(check_labelling(h, "mask_shapes", n_frames, roi_w, roi_h, connectivity, max_boxes));
        if (roi_w > 65536u || roi_h > 65536u)
            return fail(h, DIPS_ERR_INVALID, "mask_shapes: roi_w and roi_h must be at most 65536");
        if ((uint64_t)n_frames * max_boxes * DIPS_SHAPE_WORDS >= (1ull << 32))
            return fail(h, DIPS_ERR_INVALID, "mask_shapes: n_frames * max_boxes * 16 must stay below 2^32");
        if (max_boxes == 0u) boxes = shapes = nullptr;
        const size_t counts_bytes = sizeof(uint32_t) * (size_t)n_frames;
        // the weights (bytes) behind the mask, the shapes (8-byte aligned) in
        // front of boxes and counts
        HostStaging sg(h, "mask_shapes");
        sg.add(h->stage_frames, mask, mask_frame_bytes(roi_w, roi_h) * n_frames, sg.kIn);
        sg.add(h->stage_frames, weights, (size_t)roi_w * roi_h * n_frames, sg.kIn | sg.kAnyAlign);
        sg.add(h->stage_series, shapes, counts_bytes * DIPS_SHAPE_WORDS * max_boxes, sg.kOut | sg.kAnyAlign);
        sg.add(h->stage_series, boxes, counts_bytes * DIPS_BOX_WORDS * max_boxes, sg.kOut);
        sg.add(h->stage_series, counts, counts_bytes, sg.kOut);
        DIPS_TRY(sg.check_aligned4());
        if (sg.device() && ((uintptr_t)shapes & 7u) != 0)
            return fail(h, DIPS_ERR_INVALID, "mask_shapes: shapes must be 8-byte aligned");
        DIPS_TRY(sg.upload());
        DIPS_TRY(run_components_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes,
                                       chunk_frames, counts, boxes, nullptr, h->stream, weights, shapes));
        return sg.finish();
    });
}

dips_status dips_mask_tracks(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                             uint32_t connectivity, uint32_t min_area, uint32_t max_boxes, uint32_t chunk_frames,
                             const uint8_t* prev_mask, uint32_t* state, uint32_t* counts, uint32_t* boxes,
                             uint32_t* links) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts || !boxes || !links) return fail(h, DIPS_ERR_INVALID, "mask_tracks: null argument");
        if (max_boxes == 0u || max_boxes > DIPS_TRACK_MAX_BOXES)
            return fail(h, DIPS_ERR_INVALID, "mask_tracks: max_boxes must be 1 .. 256");
        if (prev_mask && !state) return fail(h, DIPS_ERR_INVALID, "mask_tracks: prev_mask needs state");
        DIPS_TRY(check_labelling(h, "mask_tracks", n_frames, roi_w, roi_h, connectivity, max_boxes));
        const size_t frame_bytes = mask_frame_bytes(roi_w, roi_h), counts_bytes = sizeof(uint32_t) * (size_t)n_frames;
        // the frame before the clip behind the mask, the outputs and the state in one buffer
        HostStaging sg(h, "mask_tracks");
        sg.add(h->stage_frames, mask, frame_bytes * n_frames, sg.kIn);
        sg.add(h->stage_frames, prev_mask, frame_bytes, sg.kIn);
        sg.add(h->stage_series, counts, counts_bytes, sg.kOut);
        sg.add(h->stage_series, boxes, counts_bytes * DIPS_BOX_WORDS * max_boxes, sg.kOut);
        sg.add(h->stage_series, links, counts_bytes * DIPS_LINK_WORDS * max_boxes, sg.kOut);
        sg.add(h->stage_series, state, sizeof(uint32_t) * (1u + 2u * (size_t)max_boxes), sg.kInOut);
        DIPS_TRY(sg.begin());
        DIPS_TRY(run_tracks_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes, chunk_frames,
                                   prev_mask, state, counts, boxes, links, h->stream));
        return sg.finish();
    });
}

dips_status dips_mask_morph(dips_handle* h, const uint8_t* mask_in, uint32_t n_frames, uint32_t roi_w,
                            uint32_t roi_h, uint32_t op, uint32_t shape, uint32_t rx, uint32_t ry,
                            uint8_t* mask_out) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        if (n_frames == 0) return DIPS_OK;
        if (!mask_in || !mask_out) return fail(h, DIPS_ERR_INVALID, "mask_morph: null argument");
        if (op > DIPS_MORPH_CLOSE) return fail(h, DIPS_ERR_INVALID, "mask_morph: op must be 0 .. 3");
        if (shape > DIPS_MORPH_DIAMOND) return fail(h, DIPS_ERR_INVALID, "mask_morph: shape must be 0 or 1");
        if (rx > DIPS_MORPH_MAX_RADIUS || ry > DIPS_MORPH_MAX_RADIUS)
            return fail(h, DIPS_ERR_INVALID, "mask_morph: rx and ry must be 0 .. 15");
        if (shape == DIPS_MORPH_DIAMOND && ry != rx)
            return fail(h, DIPS_ERR_INVALID, "mask_morph: a diamond needs ry == rx");
        DIPS_TRY(check_mask_region(h, "mask_morph", roi_w, roi_h));
        const size_t bytes = mask_frame_bytes(roi_w, roi_h) * n_frames;
        if (outputs_overlap({{mask_out, bytes}}, {{mask_in, bytes}}))
            return fail(h, DIPS_ERR_INVALID, "mask_morph: mask_in and mask_out must not overlap");
        HostStaging sg(h, "mask_morph");
        sg.add(h->stage_frames, mask_in, bytes, sg.kIn);
        sg.add(h->stage_map, mask_out, bytes, sg.kOut);
        DIPS_TRY(sg.begin());
        DIPS_TRY(run_morph_device(h, mask_in, n_frames, roi_w, roi_h, op, shape, rx, ry, mask_out, h->stream));
        return sg.finish();
    });
}

dips_status dips_mask_vote(dips_handle* h, const uint8_t* mask_in, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                           uint32_t window, uint32_t votes, const uint8_t* history_in, uint8_t* history_out,
                           uint8_t* mask_out) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        if (window == 0u || window > DIPS_VOTE_MAX_WINDOW) return fail(h, DIPS_ERR_INVALID, "mask_vote: window must be 1 .. 31");
        if (votes == 0u || votes > window) return fail(h, DIPS_ERR_INVALID, "mask_vote: votes must be 1 .. window");
        DIPS_TRY(check_mask_region(h, "mask_vote", roi_w, roi_h));
        if (n_frames >= (1u << 31)) return fail(h, DIPS_ERR_INVALID, "mask_vote: n_frames must stay below 2^31");
        if (n_frames != 0 && (!mask_in || !mask_out)) return fail(h, DIPS_ERR_INVALID, "mask_vote: null argument");
        if (window == 1u) history_in = history_out = nullptr;  // there is no history
        const size_t frame_bytes = mask_frame_bytes(roi_w, roi_h);
        const size_t bytes = frame_bytes * n_frames, hist_bytes = frame_bytes * (window - 1u);
        if (outputs_overlap({{mask_out, bytes}, {history_out, hist_bytes}}, {{mask_in, bytes}, {history_in, hist_bytes}}))
            return fail(h, DIPS_ERR_INVALID, "mask_vote: an output must not overlap an input or the other output");
        if (n_frames == 0) mask_in = mask_out = nullptr;
        // the history behind the mask, in and out alike
        HostStaging sg(h, "mask_vote");
        sg.add(h->stage_frames, mask_in, bytes, sg.kIn);
        sg.add(h->stage_frames, history_in, hist_bytes, sg.kIn);
        sg.add(h->stage_map, mask_out, bytes, sg.kOut);
        sg.add(h->stage_map, history_out, hist_bytes, sg.kOut);
        DIPS_TRY(sg.check_aligned4());
        if (n_frames == 0 && !history_out) return DIPS_OK;  // nothing to write: nothing is staged
        DIPS_TRY(sg.upload());
        DIPS_TRY(run_vote_device(h, mask_in, n_frames, roi_w, roi_h, window, votes, history_in, history_out, mask_out,
                                 h->stream));
        return sg.finish();
    });
}

dips_status dips_mask_select(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                             uint32_t connectivity, uint32_t min_area, uint32_t max_area, uint32_t select,
                             const uint8_t* marker, uint32_t marker_frames, uint32_t chunk_frames, uint8_t* mask_out,
                             uint32_t* counts) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !mask_out) return fail(h, DIPS_ERR_INVALID, "mask_select: null argument");
        DIPS_TRY(check_labelling(h, "mask_select", n_frames, roi_w, roi_h, connectivity, 0u));
        if ((select & ~(DIPS_SELECT_CLEAR_BORDER | DIPS_SELECT_DROPPED)) != 0u)
            return fail(h, DIPS_ERR_INVALID, "mask_select: unknown bits in select");
        if (max_area != 0u && max_area < min_area)
            return fail(h, DIPS_ERR_INVALID, "mask_select: max_area must be 0 or at least min_area");
        if (marker ? (marker_frames != 1u && marker_frames != n_frames) : marker_frames != 0u)
            return fail(h, DIPS_ERR_INVALID,
                        "mask_select: marker_frames must be 1 or n_frames with a marker and 0 without");
        const size_t frame_bytes = mask_frame_bytes(roi_w, roi_h);
        const size_t mask_bytes = frame_bytes * n_frames, marker_bytes = frame_bytes * marker_frames;
        const size_t counts_bytes = counts ? sizeof(uint32_t) * (size_t)n_frames : 0u;
        if (outputs_overlap({{mask_out, mask_bytes}, {counts, counts_bytes}}, {{mask, mask_bytes}, {marker, marker_bytes}}))
            return fail(h, DIPS_ERR_INVALID, "mask_select: an output must not overlap an input or the other output");
        // the marker behind the mask
        HostStaging sg(h, "mask_select");
        sg.add(h->stage_frames, mask, mask_bytes, sg.kIn);
        sg.add(h->stage_frames, marker, marker_bytes, sg.kIn);
        sg.add(h->stage_map, mask_out, mask_bytes, sg.kOut);
        sg.add(h->stage_series, counts, counts_bytes, sg.kOut);
        DIPS_TRY(sg.begin());
        DIPS_TRY(run_select_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_area, select, marker,
                                   marker_frames, chunk_frames, mask_out, counts, h->stream));
        return sg.finish();
    });
}

dips_status dips_mask_logic(dips_handle* h, const uint8_t* a, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                            uint32_t op, const uint8_t* b, uint32_t b_frames, uint8_t* mask_out) {
    return guard(h, [&]() -> dips_status {
        DIPS_TRY(bind(h));
        if (n_frames == 0) return DIPS_OK;
        if (!a || !mask_out) return fail(h, DIPS_ERR_INVALID, "mask_logic: null argument");
        if (op > DIPS_LOGIC_NOT) return fail(h, DIPS_ERR_INVALID, "mask_logic: op must be 0 .. 4");
        if (op == DIPS_LOGIC_NOT ? (b != nullptr || b_frames != 0u) : b == nullptr)
            return fail(h, DIPS_ERR_INVALID, "mask_logic: NOT takes no b, every other op needs one");
        if (b && b_frames != 1u && b_frames != n_frames)
            return fail(h, DIPS_ERR_INVALID, "mask_logic: b_frames must be 1 or n_frames");
        DIPS_TRY(check_mask_region(h, "mask_logic", roi_w, roi_h));
        const size_t frame_bytes = mask_frame_bytes(roi_w, roi_h);
        const size_t bytes = frame_bytes * n_frames, b_bytes = frame_bytes * b_frames;
        if (outputs_overlap({{mask_out, bytes}}, {{a, bytes}, {b, b_bytes}}))
            return fail(h, DIPS_ERR_INVALID, "mask_logic: mask_out must not overlap an input");
        // b behind a
        HostStaging sg(h, "mask_logic");
        sg.add(h->stage_frames, a, bytes, sg.kIn);
        sg.add(h->stage_frames, b, b_bytes, sg.kIn);
        sg.add(h->stage_map, mask_out, bytes, sg.kOut);
        DIPS_TRY(sg.begin());
        DIPS_TRY(run_logic_device(h, a, n_frames, roi_w, roi_h, op, b, b_frames, mask_out, h->stream));
        return sg.finish();
    });
}

}  // extern "C"
