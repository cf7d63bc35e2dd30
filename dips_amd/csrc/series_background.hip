// series_background.hip -- the running-average background model of a region
// of interest and the change mask taken against it
// (dips_diff_background_mask).  Per pixel and channel a u16 B in 8.8 fixed
// point; for frame t, in order:
//   R[c]  = (B[c] + 128) >> 8                           the reference bytes
//   bit   = |I(F_t) - I(R)| > tau                       dips_diff_change_mask's compare
//   B'[c] = B[c] - ((B[c] + h) >> k) + (F[c] << (8 - k))  h = (1 << k) >> 1
// the update skipped for the whole pixel when DIPS_BG_SELECTIVE is set and
// bit = 1.  One read of the batch; every mask word and every state value has
// one final writer.
//
// The fast kernel is the regional skeleton (series_region.h) as
// series_mask_kernel uses it: word-padded slots, the frames-only ring, one
// store per word.  What differs:
//
//   One part always.  The recurrence is sequential in t and truncating: a
//   part cannot start without the state before it, so a wave owns every frame
//   of its tile and the only parallelism is tiles.  No combine pass, no
//   atomics, no memset, no wave waits for another.
//
//   The state is packed u16 pairs per channel in the layout pair_planes<C>
//   gives a frame's channels (pixels (0, 1) and (2, 3)): the update is five
//   packed 16-bit ops per pair (add h, shift right k, subtract, shift F left
//   8 - k, add; k and h wave-uniform run-time values), R two more, and R
//   comes out as u16 planes holding byte values, which derive_planes (the
//   planes-input sibling of derive_v2) consumes.  Two intensity derivations
//   per vec and frame, then the subtract and compare in the 2^22-scaled
//   domain; one form serves every tau (series_mask.hip).
//
//   The selective update is a per-half select (v_bfi_b32) built from the two
//   decision bits of a pair.  RGBA8's alpha has its own plane; it is tracked
//   like any channel and does not enter the intensity.
//
//   The state is read (accumulate) and written once per call, per channel: a
//   lane's 4 pixels are 8 contiguous bytes of a plane.  The pixels of a
//   partial vec beyond the region's right edge are neither loaded nor stored.
//
// A partial vec that would read past the frame's end (series_slots.h
// vec_crosses_frame_end) is left out: the fast kernel stores neither its
// pixels' state nor the mask word that holds it.  The generic kernel computes
// that whole word and those pixels' state in an EARLIER launch of the stream
// (run_background_device): it needs the initial state of all of the word's
// pixels, which an accumulating call keeps in the very buffer the fast kernel
// overwrites.  The two launches write disjoint addresses.
#include <algorithm>

#include "series_region.h"

namespace dips {

// derive_v2 (intensity_v2.h) from the pair planes instead of the vec's
// dwords: the scaled intensity pairs I2s of 4 pixels whose channels are u16
// planes holding byte values.
template <int CH>
__device__ __forceinline__ void derive_planes(const u16x2 (&r)[2], const u16x2 (&g)[2], const u16x2 (&b)[2], St2& s) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        h2 mx, mn;
        if constexpr (CH == 0) {
            const h2 rh = __builtin_bit_cast(h2, r[k]), gh = __builtin_bit_cast(h2, g[k]), bh = __builtin_bit_cast(h2, b[k]);
            mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(rh, gh), bh);
            mn = __builtin_elementwise_minimum(__builtin_elementwise_minimum(rh, gh), bh);
        } else {
            mx = mn = __builtin_bit_cast(h2, CH == 1 ? r[k] : (CH == 2 ? g[k] : b[k]));
        }
        const h2 xn = norm_h2(mx), nn = norm_h2(mn);
        const uint32_t jn = __builtin_bit_cast(uint32_t, xn + nn);  // J * 2^-9, exact
        const uint32_t e = __builtin_bit_cast(uint32_t, pow2_floor_h2(xn) + pow2_floor_h2(nn));
        s.i[k] = f32x2{fma_mix_lo(jn, kI2Mul, e), fma_mix_hi(jn, kI2Mul, e)};
    }
}

// The channel planes of one vec: pair_planes' r, g, b and RGBA8's alpha.
template <int C>
__device__ __forceinline__ void channel_planes(const uint32_t (&d)[Fmt<C>::NDW], u16x2 (&p)[C][2]) {
    pair_planes<C>(d, p[0], p[1], p[2]);
    if constexpr (C == 4) {
        p[3][0] = as_u16x2(__builtin_amdgcn_perm(d[1], d[0], 0x0C070C03u));
        p[3][1] = as_u16x2(__builtin_amdgcn_perm(d[3], d[2], 0x0C070C03u));
    }
}

// The wave-uniform constants of the update.
struct BgRate {
    u16x2 k, h, l;   // rate_shift, (1 << k) >> 1, 8 - k, in both halves
    uint32_t sel;    // ~0 with DIPS_BG_SELECTIVE, else 0
};

// One frame of one tile: the mask word of every slot's 8-lane group (in all
// 8 lanes) and the state `st` moved on by the frame; `nm` the slot's
// valid-pixel nibble already shifted to the lane's place in the word.
template <int C, int CH, int U>
__device__ __forceinline__ void frame_background(float thr, const BgRate& q, u16x2 (&st)[U][C][2],
                                                 const uint32_t (&cur)[U][Fmt<C>::NDW], const uint32_t (&nm)[U],
                                                 uint32_t sh, uint32_t (&word)[U]) {
    using F = Fmt<C>;
    const u16x2 half = {128, 128}, eight = {8, 8};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        u16x2 f[C][2];
        {
            uint32_t cv[F::NDW];
#pragma unroll
            for (int k = 0; k < F::NDW; ++k) cv[k] = cur[u][k];
            channel_planes<C>(cv, f);
        }
        u16x2 rp[3][2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int k = 0; k < 2; ++k) rp[c][k] = (st[u][c][k] + half) >> eight;
        }
        St2 sb, sf;
        derive_planes<CH>(rp[0], rp[1], rp[2], sb);
        derive_planes<CH>(f[0], f[1], f[2], sf);
        uint32_t nib = 0u, keep[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const f32x2 d = sf.i[k] - sb.i[k];
            const bool b0 = fabsf(d.x) > thr, b1 = fabsf(d.y) > thr;
            nib |= (b0 ? 1u : 0u) << (2 * k);
            nib |= (b1 ? 1u : 0u) << (2 * k + 1);
            keep[k] = ((b0 ? 0x0000FFFFu : 0u) | (b1 ? 0xFFFF0000u : 0u)) & q.sel;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const u16x2 b = st[u][c][k];
                const u16x2 nb = b - ((b + q.h) >> q.k) + (f[c][k] << q.l);
                st[u][c][k] = as_u16x2((as_u32(b) & keep[k]) | (as_u32(nb) & ~keep[k]));
            }
        }
        word[u] = nibble_word(nib, sh, nm[u]);
    }
}

// Waves per SIMD asked of the register allocator (probe builds of the
// vecs-per-lane comparison override it).
#ifndef DIPS_BG_WAVES
#define DIPS_BG_WAVES 4
#endif

template <int C, int CH, int U>
__global__ __launch_bounds__(256, DIPS_BG_WAVES) void series_background_kernel(BgArgs a) {
    using F = Fmt<C>;
    constexpr int NDW = F::NDW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    const uint32_t fb = a.frame_bytes;
    const uint32_t mfb = a.mask_frame_bytes;
    const GridRect rc = a.roi;
    const uint32_t vpr8 = dips_sched::word_vpr(rc.w);  // vecs per padded region row
    const uint32_t nvec8 = vpr8 * rc.h;              // = mfb / 4 * 8
    const uint32_t sh = (lane & 7u) * 4u;
    const uint32_t plane_bytes = rc.w * rc.h * 2u;   // < 2^31 (the region stays below 2^30 pixels)
    const uint32_t n = a.n_frames;                   // >= 1
    const uint32_t tlast = n - 1u;
    BgRate q;
    {
        const unsigned short k = (unsigned short)a.rate_shift;
        q.k = u16x2{k, k};
        q.h = u16x2{(unsigned short)((1u << k) >> 1), (unsigned short)((1u << k) >> 1)};
        q.l = u16x2{(unsigned short)(8u - k), (unsigned short)(8u - k)};
        q.sel = a.selective != 0u ? 0xFFFFFFFFu : 0u;
    }

    for (uint32_t tile = wave; tile < a.n_tiles; tile += a.n_waves) {
        const uint32_t v0 = tile * (uint32_t)(64 * U);

        // per lane-slot, once per tile: where it loads from, the valid pixels
        // of its nibble, the byte offset of its pixels in a state plane with
        // their count (0: none), and for the first lane of a group the byte
        // offset of the group's word -- kNoSlot when there is no mask or the
        // word holds a vec that was left out
        uint32_t voff[U], nm[U], woff[U], soff[U], spx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t idx = v0 + (uint32_t)(u * 64) + lane;
            const dips_sched::WordSlot q = dips_sched::region_word_slot(rc, vpr8, nvec8, a.width, (uint32_t)C, fb, idx);
            voff[u] = q.voff;
            nm[u] = dips_sched::slot_word_bits(q.left, sh);
            spx[u] = q.ok ? q.left : 0u;
            soff[u] = q.ok ? (q.r * rc.w + q.x4) * 2u : kNoSlot;
            const uint32_t out = group8_or((q.in && !q.ok) ? 1u : 0u);  // by all lanes: no branch around it
            woff[u] = ((lane & 7u) == 0u && idx < nvec8 && out == 0u && a.mask != nullptr) ? (idx >> 3) * 4u : kNoSlot;
        }

        const FrameLoader<C, U> ld{a.frames, fb, tlast, voff};
        // the initial state: what `background` holds, or 256 * the reference
        u16x2 st[U][C][2];
        uint32_t buf[4][U][NDW];
        if (a.accumulate != 0u) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                // plane c alone: soff + 8 <= plane_bytes for a whole vec,
                // soff + 2 * spx <= plane_bytes for a partial one
                const __amdgpu_buffer_rsrc_t r =
                    make_rsrc(reinterpret_cast<const uint8_t*>(a.background) + (uint64_t)c * plane_bytes, plane_bytes);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    uint32_t lo, hi;
                    load_state(r, soff[u], spx[u], lo, hi);
                    st[u][c][0] = as_u16x2(lo);
                    st[u][c][1] = as_u16x2(hi);
                }
            }
            ld.fill(0u, buf);
        } else {
            uint32_t rb[U][NDW];
            ld.at(a.ref0, rb);
            ld.fill(0u, buf);
            const u16x2 eight = {8, 8};
#pragma unroll
            for (int u = 0; u < U; ++u) {
                u16x2 p[C][2];
                channel_planes<C>(rb[u], p);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    st[u][c][0] = p[c][0] << eight;
                    st[u][c][1] = p[c][1] << eight;
                }
            }
        }

        // ring: frame k in slot k & 3
        uint32_t k = 0;
        for (; k + 4 <= n; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t tf = k + (uint32_t)j;
                uint32_t word[U];
                frame_background<C, CH, U>(a.thr, q, st, buf[j], nm, sh, word);
                store_words<U>(a.mask + (uint64_t)tf * mfb, a.mask != nullptr ? mfb : 0u, woff, word);
                __builtin_amdgcn_sched_barrier(0);
                ld.frame(tf + 4, buf[j]);
            }
        }
        // tail: up to 3 frames, already in flight in their slots
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (k + (uint32_t)j < n) {
                uint32_t word[U];
                frame_background<C, CH, U>(a.thr, q, st, buf[j], nm, sh, word);
                store_words<U>(a.mask + (uint64_t)(k + (uint32_t)j) * mfb, a.mask != nullptr ? mfb : 0u, woff, word);
            }
        }

        // the final state, per channel: 8 contiguous bytes of the plane for a
        // whole vec, the region's pixels alone for a partial one
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const __amdgpu_buffer_rsrc_t r =
                make_rsrc(reinterpret_cast<uint8_t*>(a.background) + (uint64_t)c * plane_bytes, plane_bytes);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t lo = as_u32(st[u][c][0]), hi = as_u32(st[u][c][1]);
                if (spx[u] == 4u) {
                    typedef uint32_t u32x2 __attribute__((vector_size(8)));
                    const u32x2 v = {lo, hi};
                    __builtin_amdgcn_raw_buffer_store_b64(v, r, soff[u], 0, 0);
                } else {
                    if (spx[u] > 0u) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)lo, r, soff[u], 0, 0);
                    if (spx[u] > 1u) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(lo >> 16), r, soff[u] + 2u, 0, 0);
                    if (spx[u] > 2u) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)hi, r, soff[u] + 4u, 0, 0);
                }
            }
        }
    }
}

// Generic path: any format, shape and alignment.  One thread per mask word of
// a rectangle of words takes the word's up to 32 pixels one after the other:
// the pixel's state in registers, the frames in order with
// series_generic_kernel's per-pixel body (the reference's own (cmax + cmin)
// / 2 intensity form, dips_shader.wgsl:73-81) on the frame's and on the
// reference bytes, the plain integer recurrence, the pixel's bit put into the
// word of each frame (the thread is the word's only writer: the first pixel
// stores, the later ones read, OR and store; pad bits stay 0), and at the end
// the state of the pixels from region column state_x0 on.  It serves GRAY8,
// DIPS_FLAG_FORCE_GENERIC, DIPS_FLAG_CROSSCHECK, the shapes the fast kernel's
// geometry refuses, the initial state of a call without frames and the words
// that hold a vec the fast kernel leaves out; being independent of the packed
// arithmetic it is the fast kernel's on-device cross-check.
template <int C>
__global__ __launch_bounds__(256) void background_generic_kernel(BgGenericArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= (uint64_t)a.n_rows * a.n_words) return;
    const uint32_t word = a.word0 + (uint32_t)(q % a.n_words);
    const uint32_t row = a.row0 + (uint32_t)(q / a.n_words);
    const uint64_t fb = a.frame_bytes;
    const uint32_t i0 = word * 32u;
    const uint32_t cnt = i0 < a.roi.w ? min(32u, a.roi.w - i0) : 0u;
    const uint64_t npx = (uint64_t)a.roi.w * a.roi.h;
    const uint64_t wpr = ((uint64_t)a.roi.w + 31u) >> 5;
    const uint32_t k = a.rate_shift, hh = (1u << k) >> 1;
    for (uint32_t b = 0; b < cnt; ++b) {
        const uint64_t pb = ((uint64_t)(a.roi.y + row) * a.width + a.roi.x + i0 + b) * (uint64_t)C;
        uint16_t* sp = a.background + (uint64_t)row * a.roi.w + i0 + b;
        uint32_t B[C];
#pragma unroll
        for (int c = 0; c < C; ++c) B[c] = a.accumulate != 0u ? (uint32_t)sp[(uint64_t)c * npx] : 256u * a.ref0[pb + c];
        for (uint32_t t = 0; t < a.n_frames; ++t) {
            const uint8_t* Fp = a.frames + (uint64_t)t * fb;
            uint32_t fv[4] = {0, 0, 0, 0}, rv[4] = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < C; ++c) {
                fv[c] = Fp[pb + c];
                rv[c] = (B[c] + 128u) >> 8;
            }
            const float If = C == 1 ? intensity_rgb(fv[0], fv[0], fv[0], 0u) : intensity_rgb(fv[0], fv[1], fv[2], a.chroma);
            const float Ir = C == 1 ? intensity_rgb(rv[0], rv[0], rv[0], 0u) : intensity_rgb(rv[0], rv[1], rv[2], a.chroma);
            const uint32_t bit = fabsf(If - Ir) > a.tau ? 1u : 0u;
            if (!(a.selective != 0u && bit != 0u)) {
#pragma unroll
                for (int c = 0; c < C; ++c) B[c] = B[c] - ((B[c] + hh) >> k) + (fv[c] << (8u - k));
            }
            if (a.mask != nullptr) {
                uint32_t* out = reinterpret_cast<uint32_t*>(a.mask + (uint64_t)t * a.mask_frame_bytes) + (uint64_t)row * wpr + word;
                *out = b == 0u ? bit : (*out | (bit << b));
            }
        }
        if (i0 + b >= a.state_x0) {
#pragma unroll
            for (int c = 0; c < C; ++c) sp[(uint64_t)c * npx] = (uint16_t)B[c];
        }
    }
}

// ---------------------------------------------------------------------------
// Host-side launchers (instantiation table)
// ---------------------------------------------------------------------------
template <int C>
static const void* pick_background(int chroma, bool small) {
    return dispatch_chroma(chroma, [&](auto ch) {
        return dispatch_flag(small, [&](auto sm) {
            return reinterpret_cast<const void*>(&series_background_kernel<C, ch.value, sm.value ? 1 : kUnrollBackground>);
        });
    });
}

const void* series_background_kernel_ptr(int channels, int chroma, bool small_tile) {
    switch (channels) {
        case 3: return pick_background<3>(chroma, small_tile);
        case 4: return pick_background<4>(chroma, small_tile);
        default: return nullptr;
    }
}

hipError_t launch_series_background(const BgArgs& a, int channels, int chroma, bool small_tile, uint32_t blocks,
                                    hipStream_t s) {
    const void* k = series_background_kernel_ptr(channels, chroma, small_tile);
    const uint64_t words = (uint64_t)((a.roi.w + 31u) >> 5) * a.roi.h;
    if (!k || blocks == 0 || a.n_tiles == 0 || a.n_frames == 0 || !a.background || ((uintptr_t)a.background & 1u) != 0 ||
        (uint64_t)a.roi.w * a.roi.h >= (1ull << 30) || a.rate_shift > 8u || (a.accumulate == 0u && !a.ref0) ||
        (a.mask && ((uint64_t)a.mask_frame_bytes != words * 4u || ((uintptr_t)a.mask & 3u) != 0)))
        return hipErrorInvalidValue;
    BgArgs args = a;
    void* params[] = {&args};
    return hipLaunchKernel(k, dim3(blocks), dim3(256), params, 0, s);
}

hipError_t launch_background_generic(const BgGenericArgs& a, int channels, hipStream_t s) {
    const uint64_t wpr = ((uint64_t)a.roi.w + 31u) >> 5;
    const uint64_t items = (uint64_t)a.n_rows * a.n_words;
    if (items == 0) return hipSuccess;
    if ((uint64_t)a.row0 + a.n_rows > a.roi.h || (uint64_t)a.word0 + a.n_words > wpr || !a.background ||
        ((uintptr_t)a.background & 1u) != 0 || a.rate_shift > 8u || (a.accumulate == 0u && !a.ref0) ||
        (a.n_frames > 0 && !a.frames) || (a.mask && (a.mask_frame_bytes != wpr * a.roi.h * 4u || ((uintptr_t)a.mask & 3u) != 0)) ||
        items >= (1ull << 31))
        return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)((items + 255u) / 256u);
    switch (channels) {
        case 1: hipLaunchKernelGGL(background_generic_kernel<1>, dim3(blocks), dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(background_generic_kernel<3>, dim3(blocks), dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(background_generic_kernel<4>, dim3(blocks), dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dips
