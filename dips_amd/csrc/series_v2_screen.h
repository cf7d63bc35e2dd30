// series_v2_screen.h -- the screened form of frame_v2 (series_v2_frame.h) for
// RGB8 without chroma filter, map or realignment, in the integer-sum range of
// tau (>= 2^-5): the same 4 per-lane values and count, with the exact f32
// intensity computed only where a pixel can be selected.
//
// SAD is a byte sum and SJ per lane IS the integer sum of |dJ|, J = max + min
// (frame_v2's f32 sum is within 0.015 of it and truncated after + 0.5), so
// neither needs an intensity.  count and SI take only selected pixels, and
// 255 * |dI2| = |dJ| + err, |err| < 1.1e-4 (series_v2_frame.h), so a pixel
// with |dJ| <= s is never selected (s = series_screen_level(tau),
// series_screen_rule.h; exhaustive over all (max, min) pairs in
// tests/test_screen_bound.py).  Per vec (4 px of each of 64 lanes) the kernel
// therefore keeps the two packed u16 J pairs as state (2 VGPRs, St2 takes 4),
// forms SJ by v_sad_u16 and tests |dJ| > s on the packed pairs; one ballot
// per vec decides, wave-uniformly, whether the vec runs frame_v2's exact
// arithmetic (derive_v2 of the reference and the current bytes, subtract,
// compare with a.thr, ballot count, integer a sums).  Lanes of such a vec
// without a hit run it too: their pixels fail the compare by the bound.
#pragma once

#include "series_v2_frame.h"

namespace dips {

// The packed u16 J = max + min pairs of one RGB8 vec (j[0] = pixels 0, 1;
// j[1] = pixels 2, 3): max / min as derive_v2 takes them, on the u16 planes
// read as f16 denormals, and one packed integer add.
__device__ __forceinline__ void derive_j(const uint32_t (&d)[3], uint32_t (&j)[2]) {
    u16x2 r[2], g[2], b[2];
    pair_planes<3>(d, r, g, b);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const h2 rh = __builtin_bit_cast(h2, r[k]), gh = __builtin_bit_cast(h2, g[k]), bh = __builtin_bit_cast(h2, b[k]);
        const h2 mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(rh, gh), bh);
        const h2 mn = __builtin_elementwise_minimum(__builtin_elementwise_minimum(rh, gh), bh);
        j[k] = as_u32(__builtin_bit_cast(u16x2, mx) + __builtin_bit_cast(u16x2, mn));
    }
}

// The screen level in both u16 halves and twice that: |dJ| <= s exactly when
// (Jc - Jr + s) mod 2^16 <= 2 s (|dJ| <= 510 and s <= 510: no wrap back).
struct ScreenLevel {
    uint32_t s, s2;
};
__device__ __forceinline__ ScreenLevel screen_level(const SeriesArgs& a) {
    const uint32_t s = __builtin_amdgcn_readfirstlane(a.screen);
    return {s * 0x00010001u, s * 0x00020002u};
}

// frame_v2 for <3, 0, U, PF, false> with ISI = 1: `jst` the J pairs of the
// reference (updated to this frame's in per-frame mode), `rb` / `cur` the
// reference's and the frame's bytes.
template <int U, bool PF>
__device__ __forceinline__ void frame_v2_screen(const SeriesArgs& a, ScreenLevel lv, uint32_t (&jst)[U][2],
                                                const uint32_t (&rb)[U][3], const uint32_t (&cur)[U][3],
                                                uint32_t* vals, uint32_t& cnt) {
    uint32_t sad = 0, sj = 0, c = 0;
    uint32_t si0 = 0, si1 = 0;  // sum of a over vecs 0 .. U/2-1 and U/2 .. U-1, as frame_v2
    // the fast path of all vecs first, one block of straight code whose five
    // chains interleave, then the branches on the ballots it left in SGPRs
    // (a branch right after its vec's compare waits for the VALU each time)
    uint64_t hit[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sad = __builtin_amdgcn_sad_u8(cur[u][k], rb[u][k], sad);
        uint32_t jc[2];
        derive_j(cur[u], jc);
        u16x2 far = {0, 0};  // max over the vec of (dJ + s) mod 2^16
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            // (volatile: the compiler otherwise sinks the five vecs' SJ adds
            // below the branches and keeps the old and the new J pairs of
            // the whole tile live at once)
            asm volatile("v_sad_u16 %0, %1, %2, %0" : "+v"(sj) : "v"(jc[k]), "v"(jst[u][k]));
            const u16x2 d = as_u16x2(jc[k]) - as_u16x2(jst[u][k]) + as_u16x2(lv.s);
            far = k == 0 ? d : __builtin_elementwise_max(far, d);
        }
        const uint32_t over = as_u32(__builtin_elementwise_sub_sat(far, as_u16x2(lv.s2)));
        hit[u] = __ballot(over != 0u);
        if constexpr (PF) {
            jst[u][0] = jc[0];
            jst[u][1] = jc[1];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (hit[u] != 0ull) {
            // a pixel of this vec may be selected: frame_v2's arithmetic
            // (the bytes enter through an empty volatile asm: without it the
            // compiler moves intensity arithmetic out of the branch -- the
            // fixed reference's out of the frame loop, a frame's into the
            // fast path for the next frame to reuse -- and the registers
            // that holds cost a wave per SIMD or spill)
            uint32_t rv[3], cv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                rv[k] = rb[u][k];
                cv[k] = cur[u][k];
                asm volatile("" : "+v"(rv[k]), "+v"(cv[k]));
            }
            St2 r, n;
            derive_v2<3, 0, true>(rv, r);
            derive_v2<3, 0, true>(cv, n);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const f32x2 d = n.i[k] - r.i[k];
                const float a0 = fabsf(d.x), a1 = fabsf(d.y);
                const bool s0 = a0 > a.thr, s1 = a1 > a.thr;
                const uint64_t m0 = __ballot(s0), m1 = __ballot(s1);
                c += (uint32_t)__builtin_popcountll(m0) + (uint32_t)__builtin_popcountll(m1);
                const uint32_t v = (uint32_t)(s0 ? a0 : 0.0f) + (uint32_t)(s1 ? a1 : 0.0f);
                if (u < U / 2)
                    si0 += v;
                else
                    si1 += v;
            }
        }
    }
    vals[0] = sad;
    vals[1] = sj;
    // n = 16 (si0 + si1): H = n >> 15, L = n mod 2^15, as frame_v2
    const uint64_t s64 = (uint64_t)si0 + (uint64_t)si1;
    vals[2] = (uint32_t)(s64 >> 11);
    vals[3] = ((uint32_t)s64 & 0x7FFu) << 4;
    cnt = c;
}

}  // namespace dips
