// series_slots.h -- the slot geometry of the regional kernels as functions of
// plain numbers: which vec (4 horizontally consecutive pixels of one region
// row) a flat slot index names, where it lies in a frame, how many of its
// pixels belong to the region, and whether the fast kernels leave it to the
// generic kernel.  The fast kernels and the host walks (series_sched.h) both
// call these, and tests/test_region_slots_cpu.py
// compiles them with g++ alone: no HIP types here.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define DIPS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DIPS_HD inline
#endif

namespace dips_sched {

// An offset past every buffer descriptor (frames stay below 2^31 bytes):
// loads through it give 0, stores are dropped.
constexpr uint32_t kNoSlot = 0x80000000u;

// THE frame-end rule: a vec of `vec` units that starts at unit `first` of a
// frame of `frame` units would read past the frame's end.  The fast kernels
// leave such a vec out (bytes, u32) and the host hands it to the generic
// kernel (pixels, u64).
template <typename T>
DIPS_HD constexpr bool vec_crosses_frame_end(T first, T vec, T frame) {
    return first + vec > frame;
}

// How many of the 4 pixels of a vec that starts at region column x4 < w lie
// inside a region w pixels wide.
DIPS_HD uint32_t vec_px_inside(uint32_t w, uint32_t x4) { return w - x4 < 4u ? w - x4 : 4u; }

// One slot.  `in`: the slot names a vec of the region; `ok`: a fast kernel
// loads it (in, and not across the frame's end); `left`: how many of its 4
// pixels lie inside the region (0 for a slot that is not `in`).
struct Slot {
    uint32_t r, x4;  // region row, first column within the region
    uint32_t off;    // byte offset of the vec in a frame
    bool in, ok;
    uint32_t voff;  // where a fast kernel loads it from: off, or kNoSlot when !ok
    uint32_t left;
};

// The flat layout: vpr = flat_vpr(w) = ceil(w / 4) vecs per region row, (row,
// vec) flattened over the region's nvec = vpr * h.  `off` of a slot that is
// not `in` is meaningless.  (The kernels hoist vpr and nvec out of their
// loops and pass them in.)
DIPS_HD uint32_t flat_vpr(uint32_t w) { return (w + 3u) >> 2; }

template <typename Rect>
DIPS_HD Slot region_slot(const Rect& rc, uint32_t vpr, uint32_t nvec, uint32_t width, uint32_t C, uint32_t frame_bytes,
                         uint32_t idx) {
    Slot s;
    s.r = idx / vpr;
    s.x4 = (idx - s.r * vpr) * 4u;
    s.off = ((rc.y + s.r) * width + rc.x + s.x4) * C;
    s.in = idx < nvec;
    const bool cross = vec_crosses_frame_end(s.off, 4u * C, frame_bytes);
    s.ok = s.in && !cross;
    s.voff = s.ok ? s.off : kNoSlot;
    s.left = s.in ? vec_px_inside(rc.w, s.x4) : 0u;
    return s;
}

// The word-padded layout of the mask products: the vecs of a region row
// padded to whole mask words, vpr = word_vpr(w) = 8 * ceil(w / 32) per row, so
// that the 8 slots idx & ~7 .. idx | 7 are the 32 pixels of mask word idx >> 3
// of the frame.  A slot past the region's right edge inside the padded rows is
// not `in`, and its `off` is 0; its word exists when idx < nvec.
typedef Slot WordSlot;

DIPS_HD uint32_t word_vpr(uint32_t w) { return ((w + 31u) >> 5) << 3; }

template <typename Rect>
DIPS_HD WordSlot region_word_slot(const Rect& rc, uint32_t vpr, uint32_t nvec, uint32_t width, uint32_t C,
                                  uint32_t frame_bytes, uint32_t idx) {
    WordSlot s;
    s.r = idx / vpr;
    s.x4 = (idx - s.r * vpr) * 4u;
    s.in = idx < nvec && s.x4 < rc.w;
    s.off = s.in ? ((rc.y + s.r) * width + rc.x + s.x4) * C : 0u;
    const bool cross = vec_crosses_frame_end(s.off, 4u * C, frame_bytes);
    s.ok = s.in && !cross;
    s.voff = s.ok ? s.off : kNoSlot;
    s.left = s.in ? vec_px_inside(rc.w, s.x4) : 0u;
    return s;
}

// The slot's valid pixels as bits of its mask word: a nibble at 4 * (idx & 7).
DIPS_HD uint32_t slot_word_bits(uint32_t left, uint32_t shift) { return ((1u << left) - 1u) << shift; }

}  // namespace dips_sched
