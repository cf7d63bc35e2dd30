// mask_abi.hip -- host side of include/dips_hip.h, part 5: the products of a
// packed change mask -- its connected components and their shape records,
// the components linked across frames (tracks), the binary morphology, the
// temporal vote, the selection of components with the word-wise logic, and
// the statistics (grid counts, change times and per-pixel sums).  What they
// share with the series and the regional products is in series_host.h.
// Every extern "C" body runs inside dips_abi::guard (abi_guard.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <string>

#include "series_host.h"

using dips_abi::guard;
using namespace dips_internal;

namespace {

// ---------------------------------------------------------------------------
// The connected components of a mask and their shape records
// (dips_mask_components, dips_mask_shapes; kernels in mask_components.hip and
// mask_shapes.hip)
// ---------------------------------------------------------------------------

constexpr size_t kComponentsScratchBytes = (size_t)1 << 30;  // chunk_frames = 0 stays within this

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

// the device pointers of a call, all 4-byte aligned
dips_status check_aligned4(dips_handle* h, const char* name, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    if ((bits & 3u) != 0)
        return fail(h, DIPS_ERR_INVALID, std::string(name) + ": the device pointers must be 4-byte aligned");
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
    // per frame: parent, six statistics (two of 8 bytes) per slot, the block sums
    const size_t per_frame = 4u * (size_t)a.npx + 32u * (size_t)a.nslots + 4u * (size_t)a.bpf;
    uint64_t frames = chunk ? chunk : std::max<uint64_t>(1u, kComponentsScratchBytes / per_frame);
    frames = std::min<uint64_t>(frames, n_frames);
    frames = std::min<uint64_t>(frames, std::max<uint64_t>(1u, (1u << 25) / a.bpf));  // the launches' block counts
    const uint32_t F = (uint32_t)frames;
    // the scratch before the timed span (growing it synchronises)
    DIPS_HIP(h, h->cc_scratch.ensure(per_frame * F));
    uint8_t* base = h->cc_scratch.as<uint8_t>();
    a.sum_i = reinterpret_cast<uint64_t*>(base);
    a.sum_j = a.sum_i + (size_t)F * a.nslots;
    a.area = reinterpret_cast<uint32_t*>(a.sum_j + (size_t)F * a.nslots);
    a.min_x = a.area + (size_t)F * a.nslots;
    a.max_x = a.min_x + (size_t)F * a.nslots;
    a.max_y = a.max_x + (size_t)F * a.nslots;
    a.parent = a.max_y + (size_t)F * a.nslots;
    a.block_count = a.parent + (size_t)F * a.npx;

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

// tr_ids_kernel walks a chain back to the chunk's first frame at most: the
// cap keeps that walk, one dependent load per frame, short whatever the clip
constexpr uint32_t kTracksChunkFrames = 256;

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
    // per frame: the labelling's share, the overlap table, cprev and hrank, heads and base;
    // once: the plane in front of parent and of the labels, next id, a count, two carries
    const size_t per_frame =
        4u * (size_t)a.npx + 32u * (size_t)a.nslots + 4u * (size_t)a.bpf + 4u * (size_t)K * K + 8u * (size_t)K + 8u;
    const size_t fixed = 4u * (size_t)a.npx + 4u * (size_t)a.nslots + 16u * (size_t)K + 8u;
    uint64_t frames =
        chunk ? chunk
              : std::max<uint64_t>(1u, (kComponentsScratchBytes - std::min(fixed, kComponentsScratchBytes)) / per_frame);
    frames = std::min<uint64_t>(frames, n_frames);
    frames = std::min<uint64_t>(frames, std::max<uint64_t>(1u, (1u << 25) / a.bpf));  // the launches' block counts
    frames = std::min<uint64_t>(frames, kTracksChunkFrames);
    const uint32_t F = (uint32_t)frames;
    DIPS_HIP(h, h->cc_scratch.ensure(per_frame * F + fixed));
    uint8_t* base = h->cc_scratch.as<uint8_t>();
    a.sum_i = reinterpret_cast<uint64_t*>(base);
    a.sum_j = a.sum_i + (size_t)F * a.nslots;
    uint32_t* label0 = reinterpret_cast<uint32_t*>(a.sum_j + (size_t)F * a.nslots);  // F + 1 planes
    a.area = label0 + a.nslots;
    a.min_x = a.area + (size_t)F * a.nslots;
    a.max_x = a.min_x + (size_t)F * a.nslots;
    a.max_y = a.max_x + (size_t)F * a.nslots;
    uint32_t* parent0 = a.max_y + (size_t)F * a.nslots;  // F + 1 planes
    a.parent = parent0 + a.npx;
    a.block_count = a.parent + (size_t)F * a.npx;

    dips::TracksArgs tr{};
    tr.parent = parent0;
    tr.label = label0;
    tr.ov = a.block_count + (size_t)F * a.bpf;
    tr.cprev = tr.ov + (size_t)F * K * K;
    tr.hrank = tr.cprev + (size_t)F * K;
    tr.heads = tr.hrank + (size_t)F * K;
    tr.base = tr.heads + F;
    tr.next_id = tr.base + F;
    uint32_t* prev_count = tr.next_id + 1;
    uint32_t* carry[2] = {prev_count + 1, prev_count + 1 + 2u * (size_t)K};
    tr.w = a.w;
    tr.h = a.h;
    tr.npx = a.npx;
    tr.wpr = a.wpr;
    tr.hw = a.hw;
    tr.nslots = a.nslots;
    tr.wpf = a.wpf;
    tr.bpf = a.bpf;
    tr.K = K;

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

// whether two byte ranges share a byte
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && na != 0 && nb != 0 && pa < pb + nb && pb < pa + na;
}

// Label the frames of a device mask and write the components selected,
// asynchronously on `s`, `chunk` frames per round (0: automatic) in the
// handle's scratch, laid out as run_components_device lays it out.  marker
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
    const size_t per_frame = 4u * (size_t)a.npx + 32u * (size_t)a.nslots + 4u * (size_t)a.bpf;
    uint64_t frames = chunk ? chunk : std::max<uint64_t>(1u, kComponentsScratchBytes / per_frame);
    frames = std::min<uint64_t>(frames, n_frames);
    frames = std::min<uint64_t>(frames, std::max<uint64_t>(1u, (1u << 25) / a.bpf));  // the launches' block counts
    const uint32_t F = (uint32_t)frames;
    // the scratch before the timed span (growing it synchronises)
    DIPS_HIP(h, h->cc_scratch.ensure(per_frame * F));
    uint8_t* base = h->cc_scratch.as<uint8_t>();
    a.sum_i = reinterpret_cast<uint64_t*>(base);
    a.sum_j = a.sum_i + (size_t)F * a.nslots;
    a.area = reinterpret_cast<uint32_t*>(a.sum_j + (size_t)F * a.nslots);
    a.min_x = a.area + (size_t)F * a.nslots;
    a.max_x = a.min_x + (size_t)F * a.nslots;
    a.max_y = a.max_x + (size_t)F * a.nslots;
    a.parent = a.max_y + (size_t)F * a.nslots;
    a.block_count = a.parent + (size_t)F * a.npx;

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
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (roi_w == 0 || roi_h == 0) return fail(h, DIPS_ERR_INVALID, "mask_counts: roi_w and roi_h must not be 0");
        if ((uint64_t)roi_w * roi_h >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_counts: the region must stay below 2^30 pixels");
        if (rows == 0 || cols == 0) return fail(h, DIPS_ERR_INVALID, "mask_counts: rows and cols must be at least 1");
        if (rows > roi_h || cols > roi_w)
            return fail(h, DIPS_ERR_INVALID,
                        "mask_counts: more rows or cols than the region has pixels (a cell would be empty)");
        if ((uint64_t)n_frames * rows * cols >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_counts: n_frames * rows * cols must stay below 2^30");
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts) return fail(h, DIPS_ERR_INVALID, "mask_counts: null argument");
        const size_t mask_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h) * n_frames;
        const size_t counts_bytes = sizeof(uint32_t) * (size_t)n_frames * rows * cols;
        if (ranges_overlap(counts, counts_bytes, mask, mask_bytes))
            return fail(h, DIPS_ERR_INVALID, "mask_counts: counts must not overlap mask");
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            DIPS_TRY(check_aligned4(h, "mask_counts", {mask, counts}));
            return run_counts_device(h, mask, n_frames, roi_w, roi_h, rows, cols, counts, h->stream);
        }
        // host pointers: stage through HBM (synchronous call)
        DIPS_HIP(h, h->stage_frames.ensure(mask_bytes));
        DIPS_HIP(h, h->stage_series.ensure(counts_bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, mask, mask_bytes, hipMemcpyHostToDevice, h->stream));
        st = run_counts_device(h, h->stage_frames.as<uint8_t>(), n_frames, roi_w, roi_h, rows, cols,
                               h->stage_series.as<uint32_t>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(counts, h->stage_series.p, counts_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_pixel_times(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w,
                                  uint32_t roi_h, uint32_t t0, uint32_t accumulate, uint32_t* times, uint32_t* sums) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (!times && !sums) return fail(h, DIPS_ERR_INVALID, "mask_pixel_times: times and sums are both null");
        if (!mask && n_frames > 0) return fail(h, DIPS_ERR_INVALID, "mask_pixel_times: null argument");
        if (roi_w == 0 || roi_h == 0)
            return fail(h, DIPS_ERR_INVALID, "mask_pixel_times: roi_w and roi_h must not be 0");
        if ((uint64_t)roi_w * roi_h >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_pixel_times: the region must stay below 2^30 pixels");
        if (times && (uint64_t)t0 + n_frames > 0xFFFFFFFFull)
            return fail(h, DIPS_ERR_INVALID,
                        "mask_pixel_times: t0 + n_frames must stay below 2^32 (index 0xFFFFFFFF is DIPS_TIME_NONE)");
        const size_t npx = (size_t)roi_w * roi_h;
        const size_t mask_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h) * n_frames;
        const size_t times_bytes = times ? sizeof(uint32_t) * DIPS_TIMES_PLANES * npx : 0u;
        const size_t sums_bytes = sums ? sizeof(uint32_t) * npx : 0u;
        if (ranges_overlap(times, times_bytes, mask, mask_bytes) || ranges_overlap(sums, sums_bytes, mask, mask_bytes) ||
            ranges_overlap(times, times_bytes, sums, sums_bytes))
            return fail(h, DIPS_ERR_INVALID, "mask_pixel_times: an output must not overlap the mask or the other output");
        if (n_frames == 0) mask = nullptr;
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            DIPS_TRY(check_aligned4(h, "mask_pixel_times", {mask, times, sums}));
            return run_mask_times_device(h, mask, n_frames, roi_w, roi_h, t0, accumulate != 0u, times, sums, h->stream);
        }
        if (n_frames == 0 && accumulate != 0u) return DIPS_OK;
        // host pointers: stage through HBM (synchronous call); the sums behind
        // the times, the state uploaded first when accumulating
        if (mask_bytes) DIPS_HIP(h, h->stage_frames.ensure(mask_bytes));
        DIPS_HIP(h, h->stage_series.ensure(times_bytes + sums_bytes));
        uint32_t* times_dev = times ? h->stage_series.as<uint32_t>() : nullptr;
        uint32_t* sums_dev = sums ? h->stage_series.as<uint32_t>() + times_bytes / sizeof(uint32_t) : nullptr;
        if (mask_bytes) DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, mask, mask_bytes, hipMemcpyHostToDevice, h->stream));
        if (accumulate != 0u) {
            if (times) DIPS_HIP(h, hipMemcpyAsync(times_dev, times, times_bytes, hipMemcpyHostToDevice, h->stream));
            if (sums) DIPS_HIP(h, hipMemcpyAsync(sums_dev, sums, sums_bytes, hipMemcpyHostToDevice, h->stream));
        }
        st = run_mask_times_device(h, mask_bytes ? h->stage_frames.as<uint8_t>() : nullptr, n_frames, roi_w, roi_h, t0,
                                   accumulate != 0u, times_dev, sums_dev, h->stream);
        if (st != DIPS_OK) return st;
        if (times) DIPS_HIP(h, hipMemcpyAsync(times, times_dev, times_bytes, hipMemcpyDeviceToHost, h->stream));
        if (sums) DIPS_HIP(h, hipMemcpyAsync(sums, sums_dev, sums_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_components(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w,
                                 uint32_t roi_h, uint32_t connectivity, uint32_t min_area, uint32_t max_boxes,
                                 uint32_t chunk_frames, uint32_t* counts, uint32_t* boxes, uint32_t* labels) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts || (!boxes && max_boxes != 0u))
            return fail(h, DIPS_ERR_INVALID, "mask_components: null argument");
        DIPS_TRY(check_labelling(h, "mask_components", n_frames, roi_w, roi_h, connectivity, max_boxes));
        const uint64_t n_px = (uint64_t)roi_w * roi_h;
        if (max_boxes == 0u) boxes = nullptr;
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            DIPS_TRY(check_aligned4(h, "mask_components", {mask, counts, boxes, labels}));
            return run_components_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes,
                                         chunk_frames, counts, boxes, labels, h->stream);
        }
        // host pointers: stage through HBM (synchronous call); counts and
        // boxes share one buffer
        const size_t mask_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h) * n_frames;
        const size_t counts_bytes = sizeof(uint32_t) * (size_t)n_frames;
        const size_t boxes_bytes = sizeof(uint32_t) * DIPS_BOX_WORDS * (size_t)n_frames * max_boxes;
        const size_t labels_bytes = labels ? sizeof(uint32_t) * (size_t)n_px * n_frames : 0u;
        DIPS_HIP(h, h->stage_frames.ensure(mask_bytes));
        DIPS_HIP(h, h->stage_series.ensure(counts_bytes + boxes_bytes));
        if (labels) DIPS_HIP(h, h->stage_map.ensure(labels_bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, mask, mask_bytes, hipMemcpyHostToDevice, h->stream));
        uint32_t* counts_dev = h->stage_series.as<uint32_t>();
        uint32_t* boxes_dev = max_boxes != 0u ? counts_dev + n_frames : nullptr;
        st = run_components_device(h, h->stage_frames.as<uint8_t>(), n_frames, roi_w, roi_h, connectivity, min_area,
                                   max_boxes, chunk_frames, counts_dev, boxes_dev,
                                   labels ? h->stage_map.as<uint32_t>() : nullptr, h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(counts, counts_dev, counts_bytes, hipMemcpyDeviceToHost, h->stream));
        if (max_boxes != 0u)
            DIPS_HIP(h, hipMemcpyAsync(boxes, boxes_dev, boxes_bytes, hipMemcpyDeviceToHost, h->stream));
        if (labels) DIPS_HIP(h, hipMemcpyAsync(labels, h->stage_map.p, labels_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_shapes(dips_handle* h, const uint8_t* mask, const uint8_t* weights, uint32_t n_frames,
                             uint32_t roi_w, uint32_t roi_h, uint32_t connectivity, uint32_t min_area,
                             uint32_t max_boxes, uint32_t chunk_frames, uint32_t* counts, uint32_t* boxes,
                             uint32_t* shapes) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts || ((!boxes || !shapes) && max_boxes != 0u))
            return fail(h, DIPS_ERR_INVALID, "mask_shapes: null argument");
        DIPS_TRY(check_labelling(h, "mask_shapes", n_frames, roi_w, roi_h, connectivity, max_boxes));
        if (roi_w > 65536u || roi_h > 65536u)
            return fail(h, DIPS_ERR_INVALID, "mask_shapes: roi_w and roi_h must be at most 65536");
        if ((uint64_t)n_frames * max_boxes * DIPS_SHAPE_WORDS >= (1ull << 32))
            return fail(h, DIPS_ERR_INVALID, "mask_shapes: n_frames * max_boxes * 16 must stay below 2^32");
        if (max_boxes == 0u) boxes = shapes = nullptr;
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            DIPS_TRY(check_aligned4(h, "mask_shapes", {mask, counts, boxes}));
            if (((uintptr_t)shapes & 7u) != 0)
                return fail(h, DIPS_ERR_INVALID, "mask_shapes: shapes must be 8-byte aligned");
            return run_components_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes,
                                         chunk_frames, counts, boxes, nullptr, h->stream, weights, shapes);
        }
        // host pointers: stage through HBM (synchronous call); the weights
        // behind the mask, the shapes (8-byte aligned) in front of boxes and counts
        const size_t mask_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h) * n_frames;
        const size_t weights_bytes = weights ? (size_t)roi_w * roi_h * n_frames : 0u;
        const size_t counts_bytes = sizeof(uint32_t) * (size_t)n_frames;
        const size_t boxes_bytes = sizeof(uint32_t) * DIPS_BOX_WORDS * (size_t)n_frames * max_boxes;
        const size_t shapes_bytes = sizeof(uint32_t) * DIPS_SHAPE_WORDS * (size_t)n_frames * max_boxes;
        DIPS_HIP(h, h->stage_frames.ensure(mask_bytes + weights_bytes));
        DIPS_HIP(h, h->stage_series.ensure(shapes_bytes + boxes_bytes + counts_bytes));
        uint8_t* mask_dev = h->stage_frames.as<uint8_t>();
        uint8_t* weights_dev = weights ? mask_dev + mask_bytes : nullptr;
        uint32_t* shapes_dev = max_boxes != 0u ? h->stage_series.as<uint32_t>() : nullptr;
        uint32_t* boxes_dev = max_boxes != 0u ? shapes_dev + shapes_bytes / sizeof(uint32_t) : nullptr;
        uint32_t* counts_dev = h->stage_series.as<uint32_t>() + (shapes_bytes + boxes_bytes) / sizeof(uint32_t);
        DIPS_HIP(h, hipMemcpyAsync(mask_dev, mask, mask_bytes, hipMemcpyHostToDevice, h->stream));
        if (weights) DIPS_HIP(h, hipMemcpyAsync(weights_dev, weights, weights_bytes, hipMemcpyHostToDevice, h->stream));
        st = run_components_device(h, mask_dev, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes,
                                   chunk_frames, counts_dev, boxes_dev, nullptr, h->stream, weights_dev, shapes_dev);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(counts, counts_dev, counts_bytes, hipMemcpyDeviceToHost, h->stream));
        if (max_boxes != 0u) {
            DIPS_HIP(h, hipMemcpyAsync(boxes, boxes_dev, boxes_bytes, hipMemcpyDeviceToHost, h->stream));
            DIPS_HIP(h, hipMemcpyAsync(shapes, shapes_dev, shapes_bytes, hipMemcpyDeviceToHost, h->stream));
        }
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_tracks(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                             uint32_t connectivity, uint32_t min_area, uint32_t max_boxes, uint32_t chunk_frames,
                             const uint8_t* prev_mask, uint32_t* state, uint32_t* counts, uint32_t* boxes,
                             uint32_t* links) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts || !boxes || !links) return fail(h, DIPS_ERR_INVALID, "mask_tracks: null argument");
        if (max_boxes == 0u || max_boxes > DIPS_TRACK_MAX_BOXES)
            return fail(h, DIPS_ERR_INVALID, "mask_tracks: max_boxes must be 1 .. 256");
        if (prev_mask && !state) return fail(h, DIPS_ERR_INVALID, "mask_tracks: prev_mask needs state");
        DIPS_TRY(check_labelling(h, "mask_tracks", n_frames, roi_w, roi_h, connectivity, max_boxes));
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            DIPS_TRY(check_aligned4(h, "mask_tracks", {mask, prev_mask, state, counts, boxes, links}));
            return run_tracks_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes, chunk_frames,
                                     prev_mask, state, counts, boxes, links, h->stream);
        }
        // host pointers: stage through HBM (synchronous call); the frame
        // before the clip behind the mask, the outputs and the state in one buffer
        const size_t frame_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h);
        const size_t mask_bytes = frame_bytes * n_frames;
        const size_t counts_words = (size_t)n_frames;
        const size_t boxes_words = DIPS_BOX_WORDS * (size_t)n_frames * max_boxes;
        const size_t links_words = DIPS_LINK_WORDS * (size_t)n_frames * max_boxes;
        const size_t state_words = 1u + 2u * (size_t)max_boxes;
        DIPS_HIP(h, h->stage_frames.ensure(mask_bytes + frame_bytes));
        DIPS_HIP(h, h->stage_series.ensure(sizeof(uint32_t) * (counts_words + boxes_words + links_words + state_words)));
        uint8_t* mask_dev = h->stage_frames.as<uint8_t>();
        uint8_t* prev_dev = prev_mask ? mask_dev + mask_bytes : nullptr;
        uint32_t* counts_dev = h->stage_series.as<uint32_t>();
        uint32_t* boxes_dev = counts_dev + counts_words;
        uint32_t* links_dev = boxes_dev + boxes_words;
        uint32_t* state_dev = state ? links_dev + links_words : nullptr;
        DIPS_HIP(h, hipMemcpyAsync(mask_dev, mask, mask_bytes, hipMemcpyHostToDevice, h->stream));
        if (prev_mask) DIPS_HIP(h, hipMemcpyAsync(prev_dev, prev_mask, frame_bytes, hipMemcpyHostToDevice, h->stream));
        if (state)
            DIPS_HIP(h, hipMemcpyAsync(state_dev, state, sizeof(uint32_t) * state_words, hipMemcpyHostToDevice, h->stream));
        st = run_tracks_device(h, mask_dev, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes, chunk_frames,
                               prev_dev, state_dev, counts_dev, boxes_dev, links_dev, h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(counts, counts_dev, sizeof(uint32_t) * counts_words, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipMemcpyAsync(boxes, boxes_dev, sizeof(uint32_t) * boxes_words, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipMemcpyAsync(links, links_dev, sizeof(uint32_t) * links_words, hipMemcpyDeviceToHost, h->stream));
        if (state)
            DIPS_HIP(h, hipMemcpyAsync(state, state_dev, sizeof(uint32_t) * state_words, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_morph(dips_handle* h, const uint8_t* mask_in, uint32_t n_frames, uint32_t roi_w,
                            uint32_t roi_h, uint32_t op, uint32_t shape, uint32_t rx, uint32_t ry,
                            uint8_t* mask_out) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!mask_in || !mask_out) return fail(h, DIPS_ERR_INVALID, "mask_morph: null argument");
        if (op > DIPS_MORPH_CLOSE) return fail(h, DIPS_ERR_INVALID, "mask_morph: op must be 0 .. 3");
        if (shape > DIPS_MORPH_DIAMOND) return fail(h, DIPS_ERR_INVALID, "mask_morph: shape must be 0 or 1");
        if (rx > DIPS_MORPH_MAX_RADIUS || ry > DIPS_MORPH_MAX_RADIUS)
            return fail(h, DIPS_ERR_INVALID, "mask_morph: rx and ry must be 0 .. 15");
        if (shape == DIPS_MORPH_DIAMOND && ry != rx)
            return fail(h, DIPS_ERR_INVALID, "mask_morph: a diamond needs ry == rx");
        if (roi_w == 0 || roi_h == 0) return fail(h, DIPS_ERR_INVALID, "mask_morph: roi_w and roi_h must not be 0");
        if ((uint64_t)roi_w * roi_h >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_morph: the region must stay below 2^30 pixels");
        const size_t bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h) * n_frames;
        const uintptr_t pi = (uintptr_t)mask_in, po = (uintptr_t)mask_out;
        if (pi < po + bytes && po < pi + bytes)
            return fail(h, DIPS_ERR_INVALID, "mask_morph: mask_in and mask_out must not overlap");
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            if (((pi | po) & 3u) != 0)
                return fail(h, DIPS_ERR_INVALID, "mask_morph: the device pointers must be 4-byte aligned");
            return run_morph_device(h, mask_in, n_frames, roi_w, roi_h, op, shape, rx, ry, mask_out, h->stream);
        }
        // host pointers: stage through HBM (synchronous call)
        DIPS_HIP(h, h->stage_frames.ensure(bytes));
        DIPS_HIP(h, h->stage_map.ensure(bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, mask_in, bytes, hipMemcpyHostToDevice, h->stream));
        st = run_morph_device(h, h->stage_frames.as<uint8_t>(), n_frames, roi_w, roi_h, op, shape, rx, ry,
                              h->stage_map.as<uint8_t>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(mask_out, h->stage_map.p, bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_vote(dips_handle* h, const uint8_t* mask_in, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                           uint32_t window, uint32_t votes, const uint8_t* history_in, uint8_t* history_out,
                           uint8_t* mask_out) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (window == 0u || window > DIPS_VOTE_MAX_WINDOW) return fail(h, DIPS_ERR_INVALID, "mask_vote: window must be 1 .. 31");
        if (votes == 0u || votes > window) return fail(h, DIPS_ERR_INVALID, "mask_vote: votes must be 1 .. window");
        if (roi_w == 0 || roi_h == 0) return fail(h, DIPS_ERR_INVALID, "mask_vote: roi_w and roi_h must not be 0");
        if ((uint64_t)roi_w * roi_h >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_vote: the region must stay below 2^30 pixels");
        if (n_frames >= (1u << 31)) return fail(h, DIPS_ERR_INVALID, "mask_vote: n_frames must stay below 2^31");
        if (n_frames != 0 && (!mask_in || !mask_out)) return fail(h, DIPS_ERR_INVALID, "mask_vote: null argument");
        if (window == 1u) history_in = history_out = nullptr;  // there is no history
        const size_t frame_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h);
        const size_t bytes = frame_bytes * n_frames, hist_bytes = frame_bytes * (window - 1u);
        // no output may share a byte with an input or with the other output
        const auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
            const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
            return a && b && na != 0 && nb != 0 && pa < pb + nb && pb < pa + na;
        };
        if (overlap(mask_out, bytes, mask_in, bytes) || overlap(mask_out, bytes, history_in, hist_bytes) ||
            overlap(history_out, hist_bytes, mask_in, bytes) || overlap(history_out, hist_bytes, history_in, hist_bytes) ||
            overlap(mask_out, bytes, history_out, hist_bytes))
            return fail(h, DIPS_ERR_INVALID, "mask_vote: an output must not overlap an input or the other output");
        if (n_frames == 0) mask_in = mask_out = nullptr;
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            DIPS_TRY(check_aligned4(h, "mask_vote", {mask_in, mask_out, history_in, history_out}));
            return run_vote_device(h, mask_in, n_frames, roi_w, roi_h, window, votes, history_in, history_out, mask_out,
                                   h->stream);
        }
        if (n_frames == 0 && !history_out) return DIPS_OK;
        // host pointers: stage through HBM (synchronous call); the history
        // behind the mask, in and out alike
        DIPS_HIP(h, h->stage_frames.ensure(bytes + hist_bytes));
        DIPS_HIP(h, h->stage_map.ensure(bytes + hist_bytes));
        uint8_t* in_dev = h->stage_frames.as<uint8_t>();
        uint8_t* out_dev = h->stage_map.as<uint8_t>();
        if (bytes) DIPS_HIP(h, hipMemcpyAsync(in_dev, mask_in, bytes, hipMemcpyHostToDevice, h->stream));
        if (history_in)
            DIPS_HIP(h, hipMemcpyAsync(in_dev + bytes, history_in, hist_bytes, hipMemcpyHostToDevice, h->stream));
        st = run_vote_device(h, bytes ? in_dev : nullptr, n_frames, roi_w, roi_h, window, votes,
                             history_in ? in_dev + bytes : nullptr, history_out ? out_dev + bytes : nullptr,
                             bytes ? out_dev : nullptr, h->stream);
        if (st != DIPS_OK) return st;
        if (bytes) DIPS_HIP(h, hipMemcpyAsync(mask_out, out_dev, bytes, hipMemcpyDeviceToHost, h->stream));
        if (history_out)
            DIPS_HIP(h, hipMemcpyAsync(history_out, out_dev + bytes, hist_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_select(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                             uint32_t connectivity, uint32_t min_area, uint32_t max_area, uint32_t select,
                             const uint8_t* marker, uint32_t marker_frames, uint32_t chunk_frames, uint8_t* mask_out,
                             uint32_t* counts) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
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
        const size_t frame_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h);
        const size_t mask_bytes = frame_bytes * n_frames, marker_bytes = frame_bytes * marker_frames;
        const size_t counts_bytes = counts ? sizeof(uint32_t) * (size_t)n_frames : 0u;
        if (ranges_overlap(mask_out, mask_bytes, mask, mask_bytes) ||
            ranges_overlap(mask_out, mask_bytes, marker, marker_bytes) ||
            ranges_overlap(counts, counts_bytes, mask, mask_bytes) ||
            ranges_overlap(counts, counts_bytes, marker, marker_bytes) ||
            ranges_overlap(counts, counts_bytes, mask_out, mask_bytes))
            return fail(h, DIPS_ERR_INVALID, "mask_select: an output must not overlap an input or the other output");
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            DIPS_TRY(check_aligned4(h, "mask_select", {mask, marker, mask_out, counts}));
            return run_select_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_area, select, marker,
                                     marker_frames, chunk_frames, mask_out, counts, h->stream);
        }
        // host pointers: stage through HBM (synchronous call); the marker
        // behind the mask
        DIPS_HIP(h, h->stage_frames.ensure(mask_bytes + marker_bytes));
        DIPS_HIP(h, h->stage_map.ensure(mask_bytes));
        if (counts) DIPS_HIP(h, h->stage_series.ensure(counts_bytes));
        uint8_t* mask_dev = h->stage_frames.as<uint8_t>();
        uint8_t* marker_dev = marker ? mask_dev + mask_bytes : nullptr;
        uint32_t* counts_dev = counts ? h->stage_series.as<uint32_t>() : nullptr;
        DIPS_HIP(h, hipMemcpyAsync(mask_dev, mask, mask_bytes, hipMemcpyHostToDevice, h->stream));
        if (marker) DIPS_HIP(h, hipMemcpyAsync(marker_dev, marker, marker_bytes, hipMemcpyHostToDevice, h->stream));
        st = run_select_device(h, mask_dev, n_frames, roi_w, roi_h, connectivity, min_area, max_area, select,
                               marker_dev, marker_frames, chunk_frames, h->stage_map.as<uint8_t>(), counts_dev,
                               h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(mask_out, h->stage_map.p, mask_bytes, hipMemcpyDeviceToHost, h->stream));
        if (counts) DIPS_HIP(h, hipMemcpyAsync(counts, counts_dev, counts_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_logic(dips_handle* h, const uint8_t* a, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                            uint32_t op, const uint8_t* b, uint32_t b_frames, uint8_t* mask_out) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!a || !mask_out) return fail(h, DIPS_ERR_INVALID, "mask_logic: null argument");
        if (op > DIPS_LOGIC_NOT) return fail(h, DIPS_ERR_INVALID, "mask_logic: op must be 0 .. 4");
        if (op == DIPS_LOGIC_NOT ? (b != nullptr || b_frames != 0u) : b == nullptr)
            return fail(h, DIPS_ERR_INVALID, "mask_logic: NOT takes no b, every other op needs one");
        if (b && b_frames != 1u && b_frames != n_frames)
            return fail(h, DIPS_ERR_INVALID, "mask_logic: b_frames must be 1 or n_frames");
        if (roi_w == 0 || roi_h == 0) return fail(h, DIPS_ERR_INVALID, "mask_logic: roi_w and roi_h must not be 0");
        if ((uint64_t)roi_w * roi_h >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_logic: the region must stay below 2^30 pixels");
        const size_t frame_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h);
        const size_t bytes = frame_bytes * n_frames, b_bytes = frame_bytes * b_frames;
        if (ranges_overlap(mask_out, bytes, a, bytes) || ranges_overlap(mask_out, bytes, b, b_bytes))
            return fail(h, DIPS_ERR_INVALID, "mask_logic: mask_out must not overlap an input");
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            DIPS_TRY(check_aligned4(h, "mask_logic", {a, b, mask_out}));
            return run_logic_device(h, a, n_frames, roi_w, roi_h, op, b, b_frames, mask_out, h->stream);
        }
        // host pointers: stage through HBM (synchronous call); b behind a
        DIPS_HIP(h, h->stage_frames.ensure(bytes + b_bytes));
        DIPS_HIP(h, h->stage_map.ensure(bytes));
        uint8_t* a_dev = h->stage_frames.as<uint8_t>();
        uint8_t* b_dev = b ? a_dev + bytes : nullptr;
        DIPS_HIP(h, hipMemcpyAsync(a_dev, a, bytes, hipMemcpyHostToDevice, h->stream));
        if (b) DIPS_HIP(h, hipMemcpyAsync(b_dev, b, b_bytes, hipMemcpyHostToDevice, h->stream));
        st = run_logic_device(h, a_dev, n_frames, roi_w, roi_h, op, b_dev, b_frames, h->stage_map.as<uint8_t>(),
                              h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(mask_out, h->stage_map.p, bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

}  // extern "C"
