// series_sigma_delta.hip -- the Sigma-Delta background model of a region of
// interest and its per-pixel adaptive threshold mask
// (dips_diff_sigma_delta_mask; Manzanera & Richefeu 2007).  Per pixel two u16:
// a running median M of the integer intensity J (max + min of the R, G, B
// bytes, 0 .. 510; 2 * channel under a chroma filter) and a running estimate
// V of the pixel's own temporal activity; for frame t, in order:
//   M' = M + sgn(J_t - M)
//   D  = |J_t - M'|
//   V' = clamp(V + sgn(N * D - V), v_min, v_max)   if D != 0, else V' = V
//   bit = D > V'
// No f32, no multiply by a rate, no tau.  One read of the batch; every mask
// word and every state value has one final writer.
//
// Ranges the packed body relies on: 0 <= J, M <= 510 (M moves toward a J
// inside the range), D <= 510, N <= 15 so N * D <= 7650, V <= 510: every
// value and every difference fits a signed 16-bit lane.  The caller of an
// accumulating call promises that the held state is in range
// (include/dips_hip.h).
//
// The fast kernel has series_background_kernel's shape (the regional
// skeleton, series_region.h): word-padded slots with state, one part always
// (the recurrence is sequential in t, tiles are the only parallelism), the
// state read (accumulate) and written once per call and plane through the
// plane's own descriptor.  The body differs:
//
//   M and V of a vec are 4 VGPRs, packed i16 pairs in pair_planes<C>'s pixel
//   order (pixels (0, 1) and (2, 3)).  J is a packed max / min over the u16
//   channel planes and one packed add.  The +-1 steps are packed signed
//   clamps of a difference to [-1, 1]; "D != 0" is min(D, 1) as a multiplier
//   (under the promise v_min <= V <= v_max the clamp of an unmoved V is the
//   identity).  The decision is the sign of V' - D.  N, v_min and v_max are
//   wave-uniform run-time values.
//
// A partial vec that would read past the frame's end is left out exactly as
// in series_background.hip: the generic kernel computes its whole word and
// its pixels' state in an EARLIER launch of the stream
// (run_sigma_delta_device); the two launches write disjoint addresses.
#include <algorithm>

#include "series_region.h"
#include "series_sigma_delta.h"

namespace dips {

typedef short i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ i16x2 as_i16x2(uint32_t x) { return __builtin_bit_cast(i16x2, x); }
__device__ __forceinline__ i16x2 as_i16x2(u16x2 x) { return __builtin_bit_cast(i16x2, x); }
__device__ __forceinline__ uint32_t as_u32(i16x2 x) { return __builtin_bit_cast(uint32_t, x); }

__device__ __forceinline__ i16x2 clamp_unit(i16x2 d) {
    const i16x2 one = {1, 1}, neg = {-1, -1};
    return __builtin_elementwise_min(__builtin_elementwise_max(d, neg), one);
}

// The integer intensity J of the 4 pixels of one vec, as pairs.
template <int C, int CH>
__device__ __forceinline__ void intensity_j(const uint32_t (&d)[Fmt<C>::NDW], i16x2 (&j)[2]) {
    u16x2 r[2], g[2], b[2];
    pair_planes<C>(d, r, g, b);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if constexpr (CH == 0) {
            const u16x2 mx = __builtin_elementwise_max(__builtin_elementwise_max(r[k], g[k]), b[k]);
            const u16x2 mn = __builtin_elementwise_min(__builtin_elementwise_min(r[k], g[k]), b[k]);
            j[k] = as_i16x2(mx + mn);
        } else {
            const u16x2 x = CH == 1 ? r[k] : (CH == 2 ? g[k] : b[k]);
            j[k] = as_i16x2(x + x);
        }
    }
}

// The wave-uniform parameters, in both halves.
struct SdRate {
    i16x2 n, vmin, vmax;
};

// One frame of one tile: the mask word of every slot's 8-lane group (in all
// 8 lanes) and the state (m, v) moved on by the frame; `nm` the slot's
// valid-pixel nibble already shifted to the lane's place in the word.
template <int C, int CH, int U>
__device__ __forceinline__ void frame_sigma_delta(const SdRate& q, i16x2 (&m)[U][2], i16x2 (&v)[U][2],
                                                  const uint32_t (&cur)[U][Fmt<C>::NDW], const uint32_t (&nm)[U],
                                                  uint32_t sh, uint32_t (&word)[U]) {
    using F = Fmt<C>;
    const i16x2 one = {1, 1};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        i16x2 j[2];
        {
            uint32_t cv[F::NDW];
#pragma unroll
            for (int k = 0; k < F::NDW; ++k) cv[k] = cur[u][k];
            intensity_j<C, CH>(cv, j);
        }
        uint32_t nib = 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const i16x2 mk = m[u][k] + clamp_unit(j[k] - m[u][k]);
            const i16x2 e = j[k] - mk;
            const i16x2 d = __builtin_elementwise_max(e, -e);
            const i16x2 nz = __builtin_elementwise_min(d, one);
            const i16x2 step = clamp_unit(q.n * d - v[u][k]) * nz;
            const i16x2 vk = __builtin_elementwise_min(__builtin_elementwise_max(v[u][k] + step, q.vmin), q.vmax);
            m[u][k] = mk;
            v[u][k] = vk;
            const uint32_t neg = as_u32(vk - d);  // a half's sign bit: D > V'
            nib |= ((neg >> 15) & 1u) << (2 * k);
            nib |= (neg >> 31) << (2 * k + 1);
        }
        word[u] = nibble_word(nib, sh, nm[u]);
    }
}

// Waves per SIMD asked of the register allocator (probe builds of the
// vecs-per-lane comparison override it).
#ifndef DIPS_SD_WAVES
#define DIPS_SD_WAVES 4
#endif

template <int C, int CH, int U>
__global__ __launch_bounds__(256, DIPS_SD_WAVES) void series_sigma_delta_kernel(SdArgs a) {
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
    const uint32_t plane_bytes = rc.w * rc.h * 2u;   // < 2^31 (the region stays below 2^30 pixels)
    const uint32_t n = a.n_frames;                   // >= 1
    const uint32_t tlast = n - 1u;
    SdRate q;
    q.n = i16x2{(short)a.n_amp, (short)a.n_amp};
    q.vmin = i16x2{(short)a.v_min, (short)a.v_min};
    q.vmax = i16x2{(short)a.v_max, (short)a.v_max};

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
            const dips_sched::WordSlot s = dips_sched::region_word_slot(rc, vpr8, nvec8, a.width, (uint32_t)C, fb, idx);
            voff[u] = s.voff;
            nm[u] = dips_sched::slot_word_bits(s.left, sh);
            spx[u] = s.ok ? s.left : 0u;
            soff[u] = s.ok ? (s.r * rc.w + s.x4) * 2u : kNoSlot;
            const uint32_t out = group8_or((s.in && !s.ok) ? 1u : 0u);  // by all lanes: no branch around it
            woff[u] = ((lane & 7u) == 0u && idx < nvec8 && out == 0u && a.mask != nullptr) ? (idx >> 3) * 4u : kNoSlot;
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
            const __amdgpu_buffer_rsrc_t r = make_rsrc(a.mask + (uint64_t)tf * mfb, a.mask != nullptr ? mfb : 0u);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (woff[u] != kNoSlot) __builtin_amdgcn_raw_buffer_store_b32(word[u], r, woff[u], 0, 0);
            }
        };
        // plane p of the state alone: soff + 8 <= plane_bytes for a whole
        // vec, soff + 2 * spx <= plane_bytes for a partial one
        auto load_plane = [&](uint32_t p, i16x2 (&dst)[U][2]) {
            const __amdgpu_buffer_rsrc_t r =
                make_rsrc(reinterpret_cast<const uint8_t*>(a.state) + (uint64_t)p * plane_bytes, plane_bytes);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint32_t lo, hi;
                load_state(r, soff[u], spx[u], lo, hi);
                dst[u][0] = as_i16x2(lo);
                dst[u][1] = as_i16x2(hi);
            }
        };
        auto store_plane = [&](uint32_t p, const i16x2 (&src)[U][2]) {
            const __amdgpu_buffer_rsrc_t r =
                make_rsrc(reinterpret_cast<uint8_t*>(a.state) + (uint64_t)p * plane_bytes, plane_bytes);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t lo = as_u32(src[u][0]), hi = as_u32(src[u][1]);
                if (spx[u] == 4u) {
                    typedef uint32_t u32x2 __attribute__((vector_size(8)));
                    const u32x2 x = {lo, hi};
                    __builtin_amdgcn_raw_buffer_store_b64(x, r, soff[u], 0, 0);
                } else {
                    if (spx[u] > 0u) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)lo, r, soff[u], 0, 0);
                    if (spx[u] > 1u) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(lo >> 16), r, soff[u] + 2u, 0, 0);
                    if (spx[u] > 2u) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)hi, r, soff[u] + 4u, 0, 0);
                }
            }
        };

        // the initial state: what `state` holds, or M = J(ref), V = v_min
        i16x2 m[U][2], v[U][2];
        uint32_t buf[4][U][NDW];
        if (a.accumulate != 0u) {
            load_plane(0u, m);
            load_plane(1u, v);
            load_frame(0u, buf[0]);
            load_frame(1u, buf[1]);
            load_frame(2u, buf[2]);
            load_frame(3u, buf[3]);
        } else {
            uint32_t rb[U][NDW];
            load_at(a.ref0, rb);
            load_frame(0u, buf[0]);
            load_frame(1u, buf[1]);
            load_frame(2u, buf[2]);
            load_frame(3u, buf[3]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                intensity_j<C, CH>(rb[u], m[u]);
                v[u][0] = v[u][1] = q.vmin;
            }
        }

        // ring: frame k in slot k & 3
        uint32_t k = 0;
        for (; k + 4 <= n; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t tf = k + (uint32_t)j;
                uint32_t word[U];
                frame_sigma_delta<C, CH, U>(q, m, v, buf[j], nm, sh, word);
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
                frame_sigma_delta<C, CH, U>(q, m, v, buf[j], nm, sh, word);
                store_words(k + (uint32_t)j, word);
            }
        }

        // the final state, per plane: 8 contiguous bytes for a whole vec, the
        // region's pixels alone for a partial one
        store_plane(0u, m);
        store_plane(1u, v);
    }
}

// Generic path: any format, shape and alignment.  One thread per mask word of
// a rectangle of words takes the word's up to 32 pixels one after the other:
// the pixel's (M, V) in registers, the frames in order with the definition's
// plain integer steps, the pixel's bit put into the word of each frame (the
// thread is the word's only writer: the first pixel stores, the later ones
// read, OR and store; pad bits stay 0), and at the end the state of the
// pixels from region column state_x0 on.  It serves GRAY8,
// DIPS_FLAG_FORCE_GENERIC, DIPS_FLAG_CROSSCHECK, the shapes the fast kernel's
// geometry refuses, the initial state of a call without frames and the words
// that hold a vec the fast kernel leaves out; being independent of the packed
// arithmetic it is the fast kernel's on-device cross-check.
template <int C>
__device__ __forceinline__ int generic_j(const uint8_t* p, uint32_t chroma) {
    if constexpr (C == 1) {
        return 2 * (int)p[0];
    } else {
        const int r = p[0], g = p[1], b = p[2];
        if (chroma == 1u) return 2 * r;
        if (chroma == 2u) return 2 * g;
        if (chroma == 3u) return 2 * b;
        return max(max(r, g), b) + min(min(r, g), b);
    }
}

template <int C>
__global__ __launch_bounds__(256) void sigma_delta_generic_kernel(SdGenericArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= (uint64_t)a.n_rows * a.n_words) return;
    const uint32_t word = a.word0 + (uint32_t)(q % a.n_words);
    const uint32_t row = a.row0 + (uint32_t)(q / a.n_words);
    const uint64_t fb = a.frame_bytes;
    const uint32_t i0 = word * 32u;
    const uint32_t cnt = i0 < a.roi.w ? min(32u, a.roi.w - i0) : 0u;
    const uint64_t npx = (uint64_t)a.roi.w * a.roi.h;
    const uint64_t wpr = ((uint64_t)a.roi.w + 31u) >> 5;
    const int N = (int)a.n_amp, vmin = (int)a.v_min, vmax = (int)a.v_max;
    for (uint32_t b = 0; b < cnt; ++b) {
        const uint64_t pb = ((uint64_t)(a.roi.y + row) * a.width + a.roi.x + i0 + b) * (uint64_t)C;
        uint16_t* sp = a.state + (uint64_t)row * a.roi.w + i0 + b;
        int M, V;
        if (a.accumulate != 0u) {
            M = (int)sp[0];
            V = (int)sp[npx];
        } else {
            M = generic_j<C>(a.ref0 + pb, a.chroma);
            V = vmin;
        }
        for (uint32_t t = 0; t < a.n_frames; ++t) {
            const int J = generic_j<C>(a.frames + (uint64_t)t * fb + pb, a.chroma);
            if (J > M)
                ++M;
            else if (J < M)
                --M;
            const int D = J > M ? J - M : M - J;
            if (D != 0) {
                const int x = N * D;
                if (x > V)
                    ++V;
                else if (x < V)
                    --V;
                V = V < vmin ? vmin : (V > vmax ? vmax : V);
            }
            const uint32_t bit = D > V ? 1u : 0u;
            if (a.mask != nullptr) {
                uint32_t* out = reinterpret_cast<uint32_t*>(a.mask + (uint64_t)t * a.mask_frame_bytes) + (uint64_t)row * wpr + word;
                *out = b == 0u ? bit : (*out | (bit << b));
            }
        }
        if (i0 + b >= a.state_x0) {
            sp[0] = (uint16_t)M;
            sp[npx] = (uint16_t)V;
        }
    }
}

// ---------------------------------------------------------------------------
// Host-side launchers (instantiation table)
// ---------------------------------------------------------------------------
template <int C>
static const void* pick_sigma_delta(int chroma, bool small) {
    return dispatch_chroma(chroma, [&](auto ch) {
        return dispatch_flag(small, [&](auto sm) {
            return reinterpret_cast<const void*>(&series_sigma_delta_kernel<C, ch.value, sm.value ? 1 : kUnrollSigmaDelta>);
        });
    });
}

const void* series_sigma_delta_kernel_ptr(int channels, int chroma, bool small_tile) {
    switch (channels) {
        case 3: return pick_sigma_delta<3>(chroma, small_tile);
        case 4: return pick_sigma_delta<4>(chroma, small_tile);
        default: return nullptr;
    }
}

static bool sd_params_ok(uint32_t n_amp, uint32_t v_min, uint32_t v_max) {
    return n_amp >= 1u && n_amp <= 15u && v_min <= v_max && v_max <= 510u;
}

hipError_t launch_series_sigma_delta(const SdArgs& a, int channels, int chroma, bool small_tile, uint32_t blocks,
                                     hipStream_t s) {
    const void* k = series_sigma_delta_kernel_ptr(channels, chroma, small_tile);
    const uint64_t words = (uint64_t)((a.roi.w + 31u) >> 5) * a.roi.h;
    if (!k || blocks == 0 || a.n_tiles == 0 || a.n_frames == 0 || !a.frames || !a.state || ((uintptr_t)a.state & 1u) != 0 ||
        (uint64_t)a.roi.w * a.roi.h >= (1ull << 30) || !sd_params_ok(a.n_amp, a.v_min, a.v_max) ||
        (a.accumulate == 0u && !a.ref0) ||
        (a.mask && ((uint64_t)a.mask_frame_bytes != words * 4u || ((uintptr_t)a.mask & 3u) != 0)))
        return hipErrorInvalidValue;
    SdArgs args = a;
    void* params[] = {&args};
    return hipLaunchKernel(k, dim3(blocks), dim3(256), params, 0, s);
}

hipError_t launch_sigma_delta_generic(const SdGenericArgs& a, int channels, hipStream_t s) {
    const uint64_t wpr = ((uint64_t)a.roi.w + 31u) >> 5;
    const uint64_t items = (uint64_t)a.n_rows * a.n_words;
    if (items == 0) return hipSuccess;
    if ((uint64_t)a.row0 + a.n_rows > a.roi.h || (uint64_t)a.word0 + a.n_words > wpr || !a.state ||
        ((uintptr_t)a.state & 1u) != 0 || !sd_params_ok(a.n_amp, a.v_min, a.v_max) || (a.accumulate == 0u && !a.ref0) ||
        (a.n_frames > 0 && !a.frames) || (a.mask && (a.mask_frame_bytes != wpr * a.roi.h * 4u || ((uintptr_t)a.mask & 3u) != 0)) ||
        items >= (1ull << 31))
        return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)((items + 255u) / 256u);
    switch (channels) {
        case 1: hipLaunchKernelGGL(sigma_delta_generic_kernel<1>, dim3(blocks), dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(sigma_delta_generic_kernel<3>, dim3(blocks), dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(sigma_delta_generic_kernel<4>, dim3(blocks), dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dips
