// series_region.h -- device pieces the regional kernels share (series_grid,
// series_pixels, series_mask, series_times, series_background,
// series_sigma_delta): the decode of an item (frame part, tile) of the
// persistent grid, the raw buffer loads of a tile's slots (series_slots.h)
// through a wave-uniform descriptor over the whole frame, mask words, state
// planes, and the instantiation tables.  Each kernel writes its own 4-slot
// frame ring ("The regional skeleton").
#pragma once

#include <type_traits>

#include "series_slots.h"
#include "series_v2_frame.h"

namespace dips {

using dips_sched::kNoSlot;

// ---------------------------------------------------------------------------
// Items and slots
// ---------------------------------------------------------------------------

// Item `it` of the part-major schedule: frames [t0, t0 + n) of tile `tile`,
// n >= 1, the last of them tlast.
struct RegionItem {
    uint32_t part, tile, t0, n, tlast;
};

__device__ __forceinline__ uint64_t region_items(uint32_t n_frames, uint32_t part_frames, uint32_t n_tiles) {
    return (uint64_t)((n_frames + part_frames - 1) / part_frames) * n_tiles;
}

__device__ __forceinline__ RegionItem region_item(uint64_t it, uint32_t n_frames, uint32_t part_frames,
                                                  uint32_t n_tiles) {
    RegionItem i;
    i.part = (uint32_t)(it / n_tiles);
    i.tile = (uint32_t)(it - (uint64_t)i.part * n_tiles);
    i.t0 = i.part * part_frames;
    const uint32_t tend = min(n_frames, i.t0 + part_frames);
    i.n = tend - i.t0;
    i.tlast = tend - 1;
    return i;
}

// The reference of an item's first frame: the frame before the part in
// per-frame mode.
template <bool PF>
__device__ __forceinline__ const uint8_t* region_ref(const uint8_t* frames, const uint8_t* ref0, uint32_t t0,
                                                     uint32_t fb) {
    return PF ? (t0 == 0 ? ref0 : frames + (uint64_t)(t0 - 1) * fb) : ref0;
}

// ---------------------------------------------------------------------------
// Frame loads and the ring
// ---------------------------------------------------------------------------

// The vecs of a tile's slots out of one frame; frames past `tlast` repeat it
// (the ring loads ahead unconditionally).
template <int C, int U>
struct FrameLoader {
    static constexpr int NDW = Fmt<C>::NDW;
    const uint8_t* frames;
    uint32_t fb, tlast;
    const uint32_t (&voff)[U];

    __device__ __forceinline__ void at(const uint8_t* p, uint32_t (&dst)[U][NDW]) const {
        const __amdgpu_buffer_rsrc_t r = make_rsrc(p, fb);
#pragma unroll
        for (int u = 0; u < U; ++u) load_vec<C, kAuxNT>(r, voff[u], dst[u]);
    }
    __device__ __forceinline__ void frame(uint32_t tf, uint32_t (&dst)[U][NDW]) const {
        at(frames + (uint64_t)min(tf, tlast) * fb, dst);
    }
    // frames t0 .. t0 + 3 into ring slots 0 .. 3
    __device__ __forceinline__ void fill(uint32_t t0, uint32_t (&buf)[4][U][NDW]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) frame(t0 + (uint32_t)j, buf[j]);
    }
};

// The ring that also holds the reference bytes.  PF: frame k of the item in
// slot (k + 1) & 3, its reference (frame k - 1) in slot k & 3, reloaded with
// frame tf + 3; overall: frame k in slot k & 3, the fixed reference bytes in
// rb.  ref_ring_fill loads the reference from `rp` and the first frames, and
// returns where the reference bytes are.
template <bool PF, int C, int U>
__device__ __forceinline__ auto& ref_ring_fill(const FrameLoader<C, U>& ld, const uint8_t* rp, uint32_t t0,
                                               uint32_t (&buf)[4][U][Fmt<C>::NDW], uint32_t (&rb)[U][Fmt<C>::NDW]) {
    uint32_t (&dref)[U][Fmt<C>::NDW] = PF ? buf[0] : rb;
    ld.at(rp, dref);
    if constexpr (PF) {
        ld.frame(t0, buf[1]);
        ld.frame(t0 + 1, buf[2]);
        ld.frame(t0 + 2, buf[3]);
    } else {
        ld.fill(t0, buf);
    }
    return dref;
}

// ---------------------------------------------------------------------------
// Mask words and state planes
// ---------------------------------------------------------------------------

// A lane's nibble of decisions put at its place in the group's mask word and
// ORed over the group: the word, in all 8 lanes.
__device__ __forceinline__ uint32_t nibble_word(uint32_t nib, uint32_t sh, uint32_t nm) {
    return group8_or((nib << sh) & nm);
}

// The words of one frame's mask (`bytes` long at `mask`, the descriptor
// covers exactly it): woff < bytes for every storing lane.
template <int U>
__device__ __forceinline__ void store_words(uint8_t* mask, uint32_t bytes, const uint32_t (&woff)[U],
                                            const uint32_t (&word)[U]) {
    const __amdgpu_buffer_rsrc_t r = make_rsrc(mask, bytes);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (woff[u] != kNoSlot) __builtin_amdgcn_raw_buffer_store_b32(word[u], r, woff[u], 0, 0);
    }
}

// A slot's 4 u16 of a state plane as two dwords (pixels (0, 1) and (2, 3)),
// through the plane's own descriptor: 8 contiguous bytes for a whole vec
// (soff + 8 <= the plane's bytes), the region's spx pixels alone for a
// partial one.
__device__ __forceinline__ void load_state(__amdgpu_buffer_rsrc_t r, uint32_t soff, uint32_t spx, uint32_t& lo,
                                           uint32_t& hi) {
    lo = 0u;
    hi = 0u;
    if (spx == 4u) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, soff, 0, 0);
        lo = v[0];
        hi = v[1];
    } else {
        if (spx > 0u) lo = (uint32_t)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, soff, 0, 0);
        if (spx > 1u) lo |= (uint32_t)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, soff + 2u, 0, 0) << 16;
        if (spx > 2u) hi = (uint32_t)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, soff + 4u, 0, 0);
    }
}

// ---------------------------------------------------------------------------
// Instantiation tables (host)
// ---------------------------------------------------------------------------

// f(std::integral_constant<int, chroma>) for the chroma filters 0 .. 3, else
// nullptr; f(std::true_type / std::false_type) for a flag.
template <typename F>
const void* dispatch_chroma(int chroma, F&& f) {
    switch (chroma) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return nullptr;
    }
}

template <typename F>
const void* dispatch_flag(bool flag, F&& f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace dips
