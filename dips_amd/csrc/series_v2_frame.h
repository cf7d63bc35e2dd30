// series_v2_frame.h -- the per-(tile, frame) arithmetic of the RGB8 / RGBA8
// series kernels: frame_v2 (one frame of one tile against its reference
// state), its constants and the record stores.  Shared by series_v2.hip (a
// tile = a flat run of vecs of the frame) and series_grid.hip (a tile = vecs
// of one cell of a spatial grid); both produce the same 16-byte records.
#pragma once

#include "intensity_v2.h"

namespace dips {

// SJ from the intensity difference: 255 * |dI2| = |dJ| + err, |err| < 1.1e-4
// (u() rounds up by < 2^-24, the sum and difference round by <= 2^-24 each;
// exhaustive in tests/test_oracle.py), so the per-lane f32 sum of
// |dI2s| * 255 * 2^-22 (exact multiplier, <= 20 px x 510 < 16384: rounding
// <= 2^-11 per add) is within 0.015 of the integer SJ.
constexpr float kSjMul = 255.0f / 4194304.0f;

// The integer intensity sum (ISI): for tau >= 2^-5 every selected dI is an
// f32 in [2^-5, 1] whose ulp is >= 2^-28, so a = |dI| * 2^28 -- the
// intensities taken 32 times as large (derive_v2<X32>, an exact power-of-two
// scaling of the reference's f32 arithmetic; threshold and SJ multiplier
// scaled with them) -- is an integer <= 2^28 for every selected pixel: one
// v_cvt_u32_f32 and an integer add per pixel replace v_cvt_f64_f32 +
// v_add_f64 (the f64 add is the most power-hungry VALU class this kernel
// issues, profiles/r02_energy_per_instruction.jsonl), for one packed f16
// multiply per pixel pair.  Two u32 accumulators of <= 12 pixels each stay
// below 2^32 (U = 5: 8 and 12).  The record carries n = sum dI * 2^32 = 16 sum a as H = n >> 15,
// L = n mod 2^15, exactly as the f64 form.
constexpr float kIsiMinTau = 0.03125f;  // 2^-5

// One frame of one tile: accumulate against the reference state `st`
// (updated to this frame's state in per-frame mode) and the reference bytes
// `rb`; produce the 4 per-lane values {SAD, SJ, H, L} and the wave-wide count.
// rb / cur rows hold LR / LC dwords, the first Fmt<C>::NDW of which are the
// vec's bytes (LC = NDW + 1 in the aligned-load form, see load_at).
template <int C, int CH, int U, bool PF, bool MAP, int SAUX = kAuxNT, int LR = Fmt<C>::NDW, int LC = Fmt<C>::NDW,
          int ISI = 0>
__device__ __forceinline__ void frame_v2(const SeriesArgs& a, St2 (&st)[U], const uint32_t (&rb)[U][LR],
                                         const uint32_t (&cur)[U][LC], uint32_t voff, uint32_t t,
                                         uint32_t* vals, uint32_t& cnt) {
    using F = Fmt<C>;
    uint32_t sad = 0, c = 0;
    float sj = 0.5f;  // + 0.5: the final truncation rounds to nearest
    constexpr float sj_mul = ISI ? kSjMul / 32.0f : kSjMul;
    // exact per-lane intensity sum, offset by 2^43 so that the f64's low 52
    // mantissa bits ARE the fixed-point value n = sum(a_s) * 2^9 (ulp(2^43)
    // = 2^-9, the a_s granularity; n < 2^37 keeps every add exact)
    double si = 0x1p43;
    uint32_t si0 = 0, si1 = 0;  // ISI: sum of a over vecs 0 .. U/2-1 and U/2 .. U-1
    uint32_t map[U][F::NDW];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < F::NDW; ++k) {
            sad = __builtin_amdgcn_sad_u8(cur[u][k], rb[u][k], sad);
            if constexpr (MAP) map[u][k] = absdiff_bytes(cur[u][k], rb[u][k]);
        }
        St2 n;
        {
            uint32_t cv[F::NDW];
#pragma unroll
            for (int k = 0; k < F::NDW; ++k) cv[k] = cur[u][k];
            derive_v2<C, CH, (ISI != 0)>(cv, n);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const f32x2 d = n.i[k] - st[u].i[k];
            const float a0 = fabsf(d.x), a1 = fabsf(d.y);
            sj = __builtin_fmaf(a0, sj_mul, sj);
            sj = __builtin_fmaf(a1, sj_mul, sj);
            const bool s0 = a0 > a.thr, s1 = a1 > a.thr;
            const uint64_t m0 = __ballot(s0), m1 = __ballot(s1);
            c += (uint32_t)__builtin_popcountll(m0) + (uint32_t)__builtin_popcountll(m1);
            // (a wave-uniform skip of this exact sum when no lane has a pixel
            // above the threshold measured slower: if-converted by hipcc, or
            // as a forced branch it costs registers and occupancy)
            // (the lane-predicated form `if (s0) si += a0` compiles to an
            // unconditional add and two 32-bit selects of the f64: slower)
            if constexpr (ISI == 1) {
                const uint32_t v = (uint32_t)(s0 ? a0 : 0.0f) + (uint32_t)(s1 ? a1 : 0.0f);
                if (u < U / 2)
                    si0 += v;
                else
                    si1 += v;
            } else {
                si += (double)(s0 ? a0 : 0.0f) + (double)(s1 ? a1 : 0.0f);
            }
        }
        if constexpr (PF) st[u] = n;
    }
    if constexpr (MAP) {
        const __amdgpu_buffer_rsrc_t rm = make_rsrc(a.dmap + (uint64_t)t * a.frame_bytes, a.vec_bytes);
#pragma unroll
        for (int u = 0; u < U; ++u) store_vec<C, SAUX>(rm, voff + (uint32_t)(u * 64 * F::VB), map[u]);
    }
    vals[0] = sad;
    vals[1] = (uint32_t)sj;
    if constexpr (ISI == 1) {
        // n = 16 (si0 + si1): H = n >> 15, L = n mod 2^15 (the 33-bit sum
        // through the carry: add, add-with-carry, alignbit)
        const uint64_t s64 = (uint64_t)si0 + (uint64_t)si1;
        vals[2] = (uint32_t)(s64 >> 11);
        vals[3] = ((uint32_t)s64 & 0x7FFu) << 4;
    } else {
        const uint64_t yb = __builtin_bit_cast(uint64_t, si);
        const uint32_t lo = (uint32_t)yb, hi = (uint32_t)(yb >> 32);
        vals[2] = __builtin_amdgcn_alignbit(hi, lo, 15);  // H = n >> 15 (n < 2^37: no exponent bits)
        vals[3] = lo & 0x7FFFu;                           // L = n mod 2^15
    }
    cnt = c;
}

// Records of frames t, t+1 from their 8 reduced values (lanes 8v hold v);
// the SJ word (1) carries count << 20.
__device__ __forceinline__ void store_pair(__amdgpu_buffer_rsrc_t rpart, uint32_t t, uint32_t rec_off8,
                                           uint32_t lane, uint32_t y, uint32_t cnt0, uint32_t cnt1) {
    const uint32_t add = lane == 8u ? (cnt0 << 20) : (lane == 40u ? (cnt1 << 20) : 0u);
    __builtin_amdgcn_raw_buffer_store_b32(y + add, rpart, rec_off8, t * 16u, 0);
}

__device__ __forceinline__ void store_one(__amdgpu_buffer_rsrc_t rpart, uint32_t t, uint32_t rec_off4,
                                          uint32_t lane, uint32_t y, uint32_t cnt) {
    const uint32_t add = lane == 16u ? (cnt << 20) : 0u;
    __builtin_amdgcn_raw_buffer_store_b32(y + add, rpart, rec_off4, t * 16u, 0);
}

}  // namespace dips
