// series_mask.hip -- the per-frame change mask of a region of interest
// (dips_diff_change_mask): bit (t, j, i) = |dI_t| > tau of region pixel
// (i, j), one bit per pixel, LSB first in little-endian u32 words, rows
// padded to whole words with zero bits.  One read of the batch, every word
// written exactly once.
//
// The fast kernel is the regional skeleton (series_region.h) over the
// word-padded slots with the frames-only ring (the slot decode is
// series_slots.h region_word_slot's, written out: DESIGN.md).  Per frame it
// does derive_v2, the subtract and the compare: no SAD, SJ, SI, no
// accumulator; only the reference state crosses frames (the reference bytes
// are dropped once their state is derived).
//
// One intensity form serves every tau: only the compare matters, and
// |dI2s| > tau * 2^23 in the I2s = 2 I * 2^22 domain is an exact power-of-two
// scaling of the reference's f32 compare for any tau (the x32 form exists for
// the integer intensity sum, which the mask does not have).
//
// Words.  A lane produces a nibble; a tile is 64 * U flat vecs and a
// lane-slot holds flat vec v0 + 64 u + lane, so the 8 lanes of a group
// (lane >> 3) always own one word: the nibbles, shifted to their place, are
// ORed across the group (DPP, no LDS) and the group's first lane stores the
// word.  Every word of every frame is written by exactly one wave: no
// atomics, no memset, any number of frame parts.  Slots past the region's
// right edge inside the padded row load nothing (zeros against zeros: the
// strict compare gives 0), the pixels of a partial vec beyond the edge are
// masked out of the nibble, so the pad bits are 0.
//
// A vec left out at the frame's end loads nothing either, and its bits come
// out 0 here; the host then has the generic kernel recompute and store the
// whole word that holds it, in a later launch of the same stream
// (run_mask_device, by for_frame_end_tail_rows).
#include <algorithm>

#include "series_region.h"

namespace dips {

// One frame of one tile: the mask word of every slot's 8-lane group (in all
// 8 lanes); `st` is the reference state (updated to this frame's in
// per-frame mode), `nm` the slot's valid-pixel nibble already shifted to the
// lane's place in the word.
template <int C, int CH, int U, bool PF>
__device__ __forceinline__ void frame_mask(float thr, St2 (&st)[U], const uint32_t (&cur)[U][Fmt<C>::NDW],
                                           const uint32_t (&nm)[U], uint32_t sh, uint32_t (&word)[U]) {
    using F = Fmt<C>;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        St2 n;
        {
            uint32_t cv[F::NDW];
#pragma unroll
            for (int k = 0; k < F::NDW; ++k) cv[k] = cur[u][k];
            derive_v2<C, CH, false>(cv, n);
        }
        uint32_t nib = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const f32x2 d = n.i[k] - st[u].i[k];
            nib |= (fabsf(d.x) > thr ? 1u : 0u) << (2 * k);
            nib |= (fabsf(d.y) > thr ? 1u : 0u) << (2 * k + 1);
        }
        word[u] = nibble_word(nib, sh, nm[u]);
        if constexpr (PF) st[u] = n;
    }
}

// Waves per SIMD asked of the register allocator (DIPS_MASK_WAVES: probe
// builds of the vecs-per-lane comparison).
#ifndef DIPS_MASK_WAVES
#define DIPS_MASK_WAVES 4
#endif

template <int C, int CH, int U, bool PF>
__global__ __launch_bounds__(256, DIPS_MASK_WAVES) void series_mask_kernel(MaskArgs a) {
    constexpr int NDW = Fmt<C>::NDW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    const uint32_t fb = a.frame_bytes;
    const uint32_t mfb = a.mask_frame_bytes;
    const uint32_t sh = (lane & 7u) * 4u;
    const uint32_t vpr8 = dips_sched::word_vpr(a.roi.w);  // vecs per padded region row
    const uint32_t nvec8 = vpr8 * a.roi.h;                // = mfb / 4 * 8

    const uint64_t pitems = region_items(a.n_frames, a.part_frames, a.n_tiles);
    for (uint64_t it = wave; it < pitems; it += a.n_waves) {
        const RegionItem i = region_item(it, a.n_frames, a.part_frames, a.n_tiles);
        // per lane-slot, once per tile: the frame offset, the valid pixels
        // of its nibble in the word, the word's byte offset in a frame's mask
        uint32_t voff[U], nm[U], woff[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t idx = i.tile * (uint32_t)(64 * U) + (uint32_t)(u * 64) + lane;
            const uint32_t r = idx / vpr8;
            const uint32_t x4 = (idx - r * vpr8) * 4u;
            const bool in = idx < nvec8 && x4 < a.roi.w;
            const uint32_t off = in ? ((a.roi.y + r) * a.width + a.roi.x + x4) * (uint32_t)C : 0u;
            const bool cross = dips_sched::vec_crosses_frame_end(off, (uint32_t)Fmt<C>::VB, fb);
            const bool ok = in && !cross;
            voff[u] = ok ? off : kNoSlot;
            const uint32_t left = in ? min(4u, a.roi.w - x4) : 0u;
            nm[u] = dips_sched::slot_word_bits(left, sh);
            woff[u] = ((lane & 7u) == 0u && idx < nvec8) ? (idx >> 3) * 4u : kNoSlot;
        }
        const FrameLoader<C, U> ld{a.frames, fb, i.tlast, voff};

        // the reference only leaves its state
        uint32_t buf[4][U][NDW];
        St2 st[U];
        {
            uint32_t rb[U][NDW];
            ld.at(region_ref<PF>(a.frames, a.ref0, i.t0, fb), rb);
            ld.fill(i.t0, buf);
#pragma unroll
            for (int u = 0; u < U; ++u) derive_v2<C, CH, false>(rb[u], st[u]);
        }
        // ring: frame k of the item in slot k & 3
        auto step = [&](const uint32_t (&cur)[U][NDW], uint32_t tf) {
            uint32_t word[U];
            frame_mask<C, CH, U, PF>(a.thr, st, cur, nm, sh, word);
            store_words<U>(a.mask + (uint64_t)tf * mfb, mfb, woff, word);
        };
        uint32_t k = 0;
        for (; k + 4 <= i.n; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t tf = i.t0 + k + (uint32_t)j;
                step(buf[j], tf);
                __builtin_amdgcn_sched_barrier(0);
                ld.frame(tf + 4, buf[j]);
            }
        }
        // tail: up to 3 frames, already in flight in their slots
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (k + (uint32_t)j < i.n) step(buf[j], i.t0 + k + (uint32_t)j);
        }
    }
}

// Generic path: any format, shape and alignment.  One thread per (frame, mask
// word) of a rectangle of words evaluates the word's up to 32 pixels with
// series_generic_kernel's per-pixel body (generic_intensity; the previous
// frame read as the reference in per-frame mode) and stores the word, pad
// bits 0.  It serves GRAY8, DIPS_FLAG_FORCE_GENERIC, DIPS_FLAG_CROSSCHECK,
// the shapes the fast kernel's geometry refuses and the words that hold a vec
// it leaves out; being independent of derive_v2 it is the fast kernel's
// on-device cross-check.
template <int C>
__global__ __launch_bounds__(256) void mask_generic_kernel(MaskGenericArgs a) {
    uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= (uint64_t)a.n_frames * a.n_rows * a.n_words) return;
    const uint32_t word = a.word0 + (uint32_t)(q % a.n_words);
    q /= a.n_words;
    const uint32_t row = a.row0 + (uint32_t)(q % a.n_rows);
    const uint32_t t = a.t0 + (uint32_t)(q / a.n_rows);
    const uint64_t fb = a.frame_bytes;
    const uint8_t* Fp = a.frames + (uint64_t)t * fb;
    const uint8_t* Rp = a.mode == 1u ? (t == 0 ? a.ref0 : a.frames + (uint64_t)(t - 1) * fb) : a.ref0;
    const uint32_t i0 = word * 32u;
    const uint32_t cnt = i0 < a.roi.w ? min(32u, a.roi.w - i0) : 0u;
    const uint64_t pb0 = ((uint64_t)(a.roi.y + row) * a.width + a.roi.x + i0) * (uint64_t)C;
    uint32_t bits = 0u;
    for (uint32_t b = 0; b < cnt; ++b) {
        const uint64_t pb = pb0 + (uint64_t)b * C;
        const float If = generic_intensity<C>(Fp, pb, a.chroma);
        const float Ir = generic_intensity<C>(Rp, pb, a.chroma);
        if (fabsf(If - Ir) > a.tau) bits |= 1u << b;
    }
    const uint32_t wpr = (a.roi.w + 31u) >> 5;
    uint32_t* out = reinterpret_cast<uint32_t*>(a.mask + (uint64_t)t * a.mask_frame_bytes);
    out[(uint64_t)row * wpr + word] = bits;
}

// ---------------------------------------------------------------------------
// Host-side launchers (instantiation table)
// ---------------------------------------------------------------------------
template <int C>
static const void* pick_mask(int chroma, bool pf) {
    return dispatch_chroma(chroma, [&](auto ch) {
        return dispatch_flag(pf, [&](auto p) {
            return reinterpret_cast<const void*>(&series_mask_kernel<C, ch.value, kUnrollMask, p.value>);
        });
    });
}

const void* series_mask_kernel_ptr(int channels, int chroma, bool per_frame) {
    switch (channels) {
        case 3: return pick_mask<3>(chroma, per_frame);
        case 4: return pick_mask<4>(chroma, per_frame);
        default: return nullptr;
    }
}

hipError_t launch_series_mask(const MaskArgs& a, int channels, int chroma, bool per_frame, uint32_t blocks,
                              hipStream_t s) {
    const void* k = series_mask_kernel_ptr(channels, chroma, per_frame);
    const uint64_t words = (uint64_t)((a.roi.w + 31u) >> 5) * a.roi.h;
    if (!k || blocks == 0 || a.part_frames == 0 || a.n_tiles == 0 || a.n_frames == 0 || !a.mask ||
        (uint64_t)a.mask_frame_bytes != words * 4u || ((uintptr_t)a.mask & 3u) != 0)
        return hipErrorInvalidValue;
    MaskArgs args = a;
    void* params[] = {&args};
    return hipLaunchKernel(k, dim3(blocks), dim3(256), params, 0, s);
}

hipError_t launch_mask_generic(const MaskGenericArgs& a, int channels, hipStream_t s) {
    const uint64_t wpr = ((uint64_t)a.roi.w + 31u) >> 5;
    const uint64_t per_frame = (uint64_t)a.n_rows * a.n_words;
    if (per_frame == 0 || a.n_frames == 0) return hipSuccess;
    if ((uint64_t)a.row0 + a.n_rows > a.roi.h || (uint64_t)a.word0 + a.n_words > wpr ||
        a.mask_frame_bytes != wpr * a.roi.h * 4u || ((uintptr_t)a.mask & 3u) != 0 || per_frame >= (1ull << 31))
        return hipErrorInvalidValue;
    // frames in chunks that keep a launch below 2^31 work-items
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(a.n_frames, (1ull << 31) / per_frame));
    for (uint32_t t = 0; t < a.n_frames; t += chunk) {
        MaskGenericArgs c = a;
        c.t0 = a.t0 + t;
        c.n_frames = std::min(chunk, a.n_frames - t);
        const uint32_t blocks = (uint32_t)((per_frame * c.n_frames + 255u) / 256u);
        switch (channels) {
            case 1: hipLaunchKernelGGL(mask_generic_kernel<1>, dim3(blocks), dim3(256), 0, s, c); break;
            case 3: hipLaunchKernelGGL(mask_generic_kernel<3>, dim3(blocks), dim3(256), 0, s, c); break;
            case 4: hipLaunchKernelGGL(mask_generic_kernel<4>, dim3(blocks), dim3(256), 0, s, c); break;
            default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dips
