// series_mask.hip -- the per-frame change mask of a region of interest
// (dips_diff_change_mask): bit (t, j, i) = |dI_t| > tau of region pixel
// (i, j), one bit per pixel, LSB first in little-endian u32 words, rows
// padded to whole words with zero bits.  One read of the batch, every word
// written exactly once.
//
// The fast kernel takes series_pixels_kernel's skeleton: a persistent grid,
// items (frame part, tile), per-slot byte offsets computed once per tile, raw
// buffer loads through a wave-uniform descriptor over the whole frame, the
// 4-slot frame ring and derive_v2.  Per frame it does derive_v2, the subtract
// and the compare: no SAD, SJ, SI, no accumulator; only the reference state
// crosses frames, so the ring holds frames alone in both modes (the reference
// bytes are dropped once their state is derived).
//
// One intensity form serves every tau: only the compare matters, and
// |dI2s| > tau * 2^23 in the I2s = 2 I * 2^22 domain is an exact power-of-two
// scaling of the reference's f32 compare for any tau (the x32 form exists for
// the integer intensity sum, which the mask does not have).
//
// Geometry.  A vec is 4 horizontally consecutive pixels of one region row, so
// a lane produces a nibble.  The vecs of a region row are padded to a
// multiple of 8, vpr8 = 8 * ceil(w / 32), and (row, vec) is flattened over
// vpr8 * h: 8 consecutive flat vecs starting at a multiple of 8 are the 32
// pixels of one mask word of one row, and flat word i >> 3 is that word's
// index in the frame's mask.  A tile is 64 * U flat vecs and a lane-slot holds
// flat vec v0 + 64 u + lane, so the 8 lanes of a group (lane >> 3) always own
// one word: the nibbles, shifted to their place, are ORed across lane ^ 1,
// lane ^ 2 and the 8-lane mirror (DPP, no LDS) and the group's first lane
// stores the word.  Every word of every frame is written by exactly one wave:
// no atomics, no memset, any number of frame parts.  Slots past the region's
// right edge inside the padded row load nothing (zeros against zeros: the
// strict compare gives 0), the pixels of a partial vec beyond the edge are
// masked out of the nibble, so the pad bits are 0.
//
// A partial vec that would read past the frame's end (the last vec of the
// frame's last row; in frames narrower than 3 pixels that of up to three rows
// before it) loads nothing either, and its bits come out 0 here; the host
// then has the generic kernel recompute and store the whole word that holds
// it, in a later launch of the same stream (run_mask_device applies the same
// test).
#include <algorithm>

#include "series_v2_frame.h"

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
        uint32_t w = (nib << sh) & nm[u];
        w |= DIPS_DPP(w, 0xB1);   // quad_perm [1,0,3,2]  (xor 1)
        w |= DIPS_DPP(w, 0x4E);   // quad_perm [2,3,0,1]  (xor 2)
        w |= DIPS_DPP(w, 0x141);  // row_half_mirror      (xor 7 inside 8 lanes)
        word[u] = w;
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
    using F = Fmt<C>;
    constexpr int NDW = F::NDW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    const uint32_t fb = a.frame_bytes;
    const uint32_t mfb = a.mask_frame_bytes;
    const GridRect rc = a.roi;
    const uint32_t vpr8 = ((rc.w + 31u) >> 5) << 3;  // vecs per padded region row
    const uint32_t nvec8 = vpr8 * rc.h;              // = mfb / 4 * 8
    const uint32_t sh = (lane & 7u) * 4u;

    const uint32_t plen = a.part_frames;
    const uint64_t pitems = (uint64_t)((a.n_frames + plen - 1) / plen) * a.n_tiles;
    for (uint64_t it = wave; it < pitems; it += a.n_waves) {
        const uint32_t part = (uint32_t)(it / a.n_tiles);
        const uint32_t tile = (uint32_t)(it - (uint64_t)part * a.n_tiles);
        const uint32_t v0 = tile * (uint32_t)(64 * U);
        const uint32_t t0 = part * plen;
        const uint32_t tend = min(a.n_frames, t0 + plen);
        const uint32_t n = tend - t0;  // frames of this item (>= 1)
        const uint32_t tlast = tend - 1;

        // per lane-slot, once per tile: the byte offset into a frame (past
        // the descriptor for a slot beyond the region's right edge or rows,
        // or the one vec that would cross the frame's end: its loads return
        // zeros), the valid pixels of its nibble, and for the first lane of a
        // group inside the mask the byte offset of the group's word
        uint32_t voff[U], nm[U], woff[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t idx = v0 + (uint32_t)(u * 64) + lane;
            const uint32_t r = idx / vpr8;
            const uint32_t x4 = (idx - r * vpr8) * 4u;
            const bool in = idx < nvec8 && x4 < rc.w;
            const uint32_t off = in ? ((rc.y + r) * a.width + rc.x + x4) * (uint32_t)C : 0u;
            const bool ok = in && off + (uint32_t)F::VB <= fb;
            voff[u] = ok ? off : 0x80000000u;
            const uint32_t left = in ? min(4u, rc.w - x4) : 0u;
            nm[u] = ((1u << left) - 1u) << sh;
            woff[u] = ((lane & 7u) == 0u && idx < nvec8) ? (idx >> 3) * 4u : 0x80000000u;
        }

        auto load_at = [&](const uint8_t* p, uint32_t (&dst)[U][NDW]) {
            const __amdgpu_buffer_rsrc_t r = make_rsrc(p, fb);
#pragma unroll
            for (int u = 0; u < U; ++u) load_vec<C, kAuxNT>(r, voff[u], dst[u]);
        };
        auto load_frame = [&](uint32_t tf, uint32_t (&dst)[U][NDW]) {
            load_at(a.frames + (uint64_t)min(tf, tlast) * fb, dst);
        };
        // words of frame tf: woff < mfb for every storing lane (idx < nvec8
        // = 2 * mfb), the descriptor covers exactly this frame's mask
        auto store_words = [&](uint32_t tf, const uint32_t (&word)[U]) {
            const __amdgpu_buffer_rsrc_t r = make_rsrc(a.mask + (uint64_t)tf * mfb, mfb);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (woff[u] != 0x80000000u) __builtin_amdgcn_raw_buffer_store_b32(word[u], r, woff[u], 0, 0);
            }
        };

        // ring: frame k of the item in slot k & 3; the reference (the frame
        // before the part in per-frame mode) only leaves its state
        uint32_t buf[4][U][NDW];
        St2 st[U];
        {
            const uint8_t* rp = PF ? (t0 == 0 ? a.ref0 : a.frames + (uint64_t)(t0 - 1) * fb) : a.ref0;
            uint32_t rb[U][NDW];
            load_at(rp, rb);
            load_frame(t0, buf[0]);
            load_frame(t0 + 1, buf[1]);
            load_frame(t0 + 2, buf[2]);
            load_frame(t0 + 3, buf[3]);
#pragma unroll
            for (int u = 0; u < U; ++u) derive_v2<C, CH, false>(rb[u], st[u]);
        }

        uint32_t k = 0;
        for (; k + 4 <= n; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t tf = t0 + k + (uint32_t)j;
                uint32_t word[U];
                frame_mask<C, CH, U, PF>(a.thr, st, buf[j], nm, sh, word);
                store_words(tf, word);
                __builtin_amdgcn_sched_barrier(0);
                load_frame(tf + 4, buf[j]);
            }
        }
        // tail: up to 3 frames, already in flight in their slots
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (k + (uint32_t)j < n) {
                uint32_t word[U];
                frame_mask<C, CH, U, PF>(a.thr, st, buf[j], nm, sh, word);
                store_words(t0 + k + (uint32_t)j, word);
            }
        }
    }
}

// Generic path: any format, shape and alignment.  One thread per (frame, mask
// word) of a rectangle of words evaluates the word's up to 32 pixels with
// series_generic_kernel's per-pixel body (the reference's own (cmax + cmin)
// / 2 intensity form, dips_shader.wgsl:73-81; the previous frame read as the
// reference in per-frame mode) and stores the word, pad bits 0.  It serves
// GRAY8, DIPS_FLAG_FORCE_GENERIC, DIPS_FLAG_CROSSCHECK, the shapes the fast
// kernel's geometry refuses and the words that hold a vec it leaves out;
// being independent of derive_v2 it is the fast kernel's on-device
// cross-check.
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
        uint32_t fv[4] = {0, 0, 0, 0}, rv[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            fv[c] = Fp[pb + c];
            rv[c] = Rp[pb + c];
        }
        if constexpr (C == 1) {
            fv[1] = fv[2] = fv[0];
            rv[1] = rv[2] = rv[0];
        }
        const float If = intensity_rgb(fv[0], fv[1], fv[2], a.chroma);
        const float Ir = intensity_rgb(rv[0], rv[1], rv[2], a.chroma);
        if (fabsf(If - Ir) > a.tau) bits |= 1u << b;
    }
    const uint32_t wpr = (a.roi.w + 31u) >> 5;
    uint32_t* out = reinterpret_cast<uint32_t*>(a.mask + (uint64_t)t * a.mask_frame_bytes);
    out[(uint64_t)row * wpr + word] = bits;
}

// ---------------------------------------------------------------------------
// Host-side launchers (instantiation table)
// ---------------------------------------------------------------------------
template <int C, int CH, bool PF>
static const void* mask_ptr() {
    return reinterpret_cast<const void*>(&series_mask_kernel<C, CH, kUnrollMask, PF>);
}

template <int C>
static const void* pick_mask(int chroma, bool pf) {
    switch (chroma) {
        case 0: return pf ? mask_ptr<C, 0, true>() : mask_ptr<C, 0, false>();
        case 1: return pf ? mask_ptr<C, 1, true>() : mask_ptr<C, 1, false>();
        case 2: return pf ? mask_ptr<C, 2, true>() : mask_ptr<C, 2, false>();
        case 3: return pf ? mask_ptr<C, 3, true>() : mask_ptr<C, 3, false>();
        default: return nullptr;
    }
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
