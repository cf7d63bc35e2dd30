// mask_scratch.h -- the scratch of the labelling family (mask_components.hip,
// mask_select.hip, mask_shapes.hip, mask_tracks.hip) as a function of plain
// numbers: how many frames a round takes and where every plane lies.  No HIP
// here (tests/test_mask_scratch_cpu.py compiles this header alone with g++);
// mask_abi.hip applies the offsets to the handle's cc_scratch.
#pragma once

#include <algorithm>
#include <cstdint>

namespace dips_sched {

constexpr uint64_t kComponentsScratchBytes = 1ull << 30;  // chunk_frames = 0 stays within this

// tr_ids_kernel walks a chain back to the chunk's first frame at most: the
// cap keeps that walk, one dependent load per frame, short whatever the clip
constexpr uint32_t kTracksChunkFrames = 256;

// F frames per round, `bytes` in all, and the byte offset of every plane in
// layout order.  Per frame and slot: sum_i, sum_j (8 bytes each), area, min_x,
// max_x, max_y; per frame and pixel: parent; per frame: bpf block sums.  The
// tracks (K != 0) have one more frame in front of area's plane and of
// parent's (label0, parent0: the predecessor of the round's first frame),
// and behind the block sums per frame the overlap table, cprev and hrank,
// heads and base; once the next id, a count and two carries of 2 K words.
// K == 0: label0 == area, parent0 == parent, and the tracks' planes are empty
// at the end.
struct LabelScratch {
    uint32_t F = 0;
    uint64_t bytes = 0;
    uint64_t sum_i = 0, sum_j = 0, label0 = 0, area = 0, min_x = 0, max_x = 0, max_y = 0, parent0 = 0, parent = 0,
             block_count = 0;
    uint64_t ov = 0, cprev = 0, hrank = 0, heads = 0, base = 0, next_id = 0, prev_count = 0, carry[2] = {0, 0};
};

// The plan for frames of npx pixels, nslots slots and bpf blocks: `chunk`
// frames per round, or with 0 as many as keep the scratch within
// kComponentsScratchBytes; never more than the clip has, than keeps a
// launch's block count (F * bpf) at 2^25, or, for the tracks (K = max_boxes
// != 0), than kTracksChunkFrames.
inline LabelScratch label_scratch(uint64_t npx, uint64_t nslots, uint64_t bpf, uint32_t n_frames, uint32_t chunk,
                                  uint64_t K) {
    const uint64_t front = K != 0 ? 1u : 0u;
    const uint64_t per_frame = 4u * npx + 32u * nslots + 4u * bpf + front * (4u * K * K + 8u * K + 8u);
    const uint64_t fixed = front * (4u * npx + 4u * nslots + 16u * K + 8u);
    uint64_t frames =
        chunk ? chunk
              : std::max<uint64_t>(1u, (kComponentsScratchBytes - std::min(fixed, kComponentsScratchBytes)) / per_frame);
    frames = std::min<uint64_t>(frames, n_frames);
    frames = std::min<uint64_t>(frames, std::max<uint64_t>(1u, (1u << 25) / bpf));  // the launches' block counts
    if (K != 0) frames = std::min<uint64_t>(frames, kTracksChunkFrames);
    LabelScratch p;
    p.F = (uint32_t)frames;
    const uint64_t F = frames;
    uint64_t at = 0;
    const auto take = [&at](uint64_t bytes) {
        const uint64_t off = at;
        at += bytes;
        return off;
    };
    p.sum_i = take(8u * F * nslots);
    p.sum_j = take(8u * F * nslots);
    p.label0 = take(front * 4u * nslots);
    p.area = take(4u * F * nslots);
    p.min_x = take(4u * F * nslots);
    p.max_x = take(4u * F * nslots);
    p.max_y = take(4u * F * nslots);
    p.parent0 = take(front * 4u * npx);
    p.parent = take(4u * F * npx);
    p.block_count = take(4u * F * bpf);
    p.ov = take(4u * F * K * K);
    p.cprev = take(4u * F * K);
    p.hrank = take(4u * F * K);
    p.heads = take(front * 4u * F);
    p.base = take(front * 4u * F);
    p.next_id = take(front * 4u);
    p.prev_count = take(front * 4u);
    p.carry[0] = take(8u * K);
    p.carry[1] = take(8u * K);
    p.bytes = at;  // == per_frame * F + fixed
    return p;
}

}  // namespace dips_sched
