// series_pixels.hip -- the difference series summed over time per pixel of a
// region of interest (dips_diff_pixel_sums): one read of the batch, one entry
// per pixel, written once.
//
// The fast kernel is the regional skeleton (series_region.h) over the flat
// slots of the region (series_slots.h region_slot) with the ring that holds
// the reference bytes; derive_v2 and the 2^22-scaled intensity domain are
// those of frame_v2.  Its own is the per-frame step (frame_pix below): nothing
// is reduced across lanes, every pixel has its own accumulators, and they
// live across the frames of the part.
//
// Accumulators, per pixel (4 VGPRs; 16 per vec):
//   sad   u32: <= 1020 per frame, exact for 2^22 frames;
//   sjc   u32: SJ in bits 0..19, count in bits 20..31.  |dJ| per pixel and
//         frame is taken to its integer at once ((uint32_t)(a * kSjMul + 0.5),
//         255 * |dI2| = |dJ| + err with |err| < 1.1e-4, series_v2_frame.h), so
//         no f32 sum has to stay near an integer; 510 * 2048 < 2^20 and a
//         count of 2048 fits 12 bits: exact for parts of <= 2048 frames;
//   si    the integer form (tau >= 2^-5): a u64 sum of a = |dI| * 2^28 <= 2^28
//         (add + add-with-carry), si_fixed = 16 * si; the general form: an f64
//         sum of a = |dI2s|, a multiple of 2^-9 that is <= 2^23, so the sum is
//         exact below 2^53 * 2^-9 (2^21 frames) and si_fixed = si * 2^9.
// Parts are capped at kPixMaxPart = 2048 frames, so no accumulator is flushed
// inside a part.
//
// No masks.  The pixels of a partial vec beyond the region's right edge are
// computed from the bytes that follow (the neighbouring pixels of the frame
// row, or the next row's first pixels: inside the frame) and never stored.
// Only a partial vec that would read past the frame's end is left out: the
// last vec of the frame's last row, and in frames narrower than 3 pixels
// that of up to three rows before it; the host gives the <= 3 pixels of each
// to the generic kernel (run_pixels_device, by for_frame_end_tail_rows).
//
// Schedule: a persistent grid, items (frame part, tile) dealt part-major with
// stride n_waves.  With one part a wave owns every frame of its pixels and
// writes their entries with plain stores (or load-add-store when the call
// accumulates); with several parts every part adds its share with u64
// atomics, the host having zeroed the map in an earlier launch when the call
// does not accumulate.
#include "series_region.h"

namespace dips {

static_assert(kPixMaxPart * 510u < (1u << 20), "SJ of a part must fit 20 bits");

template <int ISI>
struct PixAcc {
    using Si = typename std::conditional<ISI != 0, uint64_t, double>::type;
    uint32_t sad[4];
    uint32_t sjc[4];
    Si si[4];
};

// The four pixels of a vec as one dword each: r | g << 8 | b << 16 (RGB8; the
// 12 bytes realigned by byte permutes) or the RGBA8 texel itself (alpha
// counts in SAD, as in the series).
template <int C>
__device__ __forceinline__ void pixel_dwords(const uint32_t (&d)[Fmt<C>::NDW], uint32_t (&p)[4]) {
    if constexpr (C == 3) {
        // d0 = r0 g0 b0 r1 | d1 = g1 b1 r2 g2 | d2 = b2 r3 g3 b3 (byte 0 first)
        p[0] = d[0] & 0x00FFFFFFu;
        p[1] = __builtin_amdgcn_perm(d[1], d[0], 0x0C050403u);
        p[2] = __builtin_amdgcn_perm(d[2], d[1], 0x0C040302u);
        p[3] = d[2] >> 8;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = d[k];
    }
}

// One frame of one tile: add every pixel's {SAD, |dJ|, selected, dI} to its
// accumulators; `st` is the reference state (updated to this frame's in
// per-frame mode), `rb` the reference bytes.
template <int C, int CH, int U, bool PF, int ISI>
__device__ __forceinline__ void frame_pix(float thr, St2 (&st)[U], const uint32_t (&rb)[U][Fmt<C>::NDW],
                                          const uint32_t (&cur)[U][Fmt<C>::NDW], PixAcc<ISI> (&acc)[U]) {
    using F = Fmt<C>;
    constexpr float sj_mul = ISI ? kSjMul / 32.0f : kSjMul;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint32_t pc[4], pr[4];
        pixel_dwords<C>(cur[u], pc);
        pixel_dwords<C>(rb[u], pr);
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[u].sad[p] = __builtin_amdgcn_sad_u8(pc[p], pr[p], acc[u].sad[p]);
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
            const float a[2] = {fabsf(d.x), fabsf(d.y)};
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int p = 2 * k + q;
                const bool s = a[q] > thr;
                acc[u].sjc[p] += (uint32_t)__builtin_fmaf(a[q], sj_mul, 0.5f) + (s ? (1u << 20) : 0u);
                const float sel = s ? a[q] : 0.0f;
                if constexpr (ISI != 0)
                    acc[u].si[p] += (uint64_t)(uint32_t)sel;
                else
                    acc[u].si[p] += (double)sel;
            }
        }
        if constexpr (PF) st[u] = n;
    }
}

// Waves per SIMD asked of the register allocator: U = 2 fits the 128 VGPRs of
// 4 waves (103-114, no spill); U = 3 spills there and gets the 168 of 3.
template <int U>
constexpr int pix_min_waves() {
    return U <= 2 ? 4 : 3;
}

template <int C, int CH, int U, bool PF, int ISI>
__global__ __launch_bounds__(256, (pix_min_waves<U>())) void series_pixels_kernel(PixArgs a) {
    using F = Fmt<C>;
    constexpr int NDW = F::NDW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    const uint32_t fb = a.frame_bytes;
    const GridRect rc = a.roi;
    const uint32_t vpr = (rc.w + 3u) >> 2;  // vecs per region row
    const uint32_t nvec = vpr * rc.h;

    const uint64_t pitems = region_items(a.n_frames, a.part_frames, a.n_tiles);
    for (uint64_t it = wave; it < pitems; it += a.n_waves) {
        const RegionItem i = region_item(it, a.n_frames, a.part_frames, a.n_tiles);
        const uint32_t t0 = i.t0, n = i.n, tlast = i.tlast;
        const uint32_t v0 = i.tile * (uint32_t)(64 * U);

        // per lane-slot, once per tile: where it loads from (series_slots.h)
        uint32_t voff[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            voff[u] =
                dips_sched::region_slot(rc, vpr, nvec, a.width, (uint32_t)C, fb, v0 + (uint32_t)(u * 64) + lane).voff;
        }

        const FrameLoader<C, U> ld{a.frames, fb, tlast, voff};

        // ring: PF -- frame k of the item in slot (k+1)&3, its reference
        // (frame k-1) in slot k&3; overall -- frame k in slot k&3, the fixed
        // reference bytes in rb
        uint32_t buf[4][U][NDW];
        uint32_t rb[U][NDW];  // overall mode only
        St2 st[U];
        PixAcc<ISI> acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                acc[u].sad[p] = 0u;
                acc[u].sjc[p] = 0u;
                acc[u].si[p] = 0;
            }
        }
        {
            const uint8_t* rp = region_ref<PF>(a.frames, a.ref0, t0, fb);
            auto& dref = ref_ring_fill<PF>(ld, rp, t0, buf, rb);
#pragma unroll
            for (int u = 0; u < U; ++u) derive_v2<C, CH, (ISI != 0)>(dref[u], st[u]);
        }

        uint32_t k = 0;
        for (; k + 4 <= n; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t tf = t0 + k + (uint32_t)j;
                if constexpr (PF) {
                    frame_pix<C, CH, U, PF, ISI>(a.thr, st, buf[j], buf[(j + 1) & 3], acc);
                    __builtin_amdgcn_sched_barrier(0);
                    ld.frame(tf + 3, buf[j]);
                } else {
                    frame_pix<C, CH, U, PF, ISI>(a.thr, st, rb, buf[j], acc);
                    __builtin_amdgcn_sched_barrier(0);
                    ld.frame(tf + 4, buf[j]);
                }
            }
        }
        // tail: up to 3 frames, already in flight in their slots
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (k + (uint32_t)j < n) {
                if constexpr (PF)
                    frame_pix<C, CH, U, PF, ISI>(a.thr, st, buf[j], buf[j + 1], acc);
                else
                    frame_pix<C, CH, U, PF, ISI>(a.thr, st, rb, buf[j], acc);
            }
        }

        // the entries of this item's pixels: a lane's four are 128
        // contiguous bytes of the map
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (voff[u] == kNoSlot) continue;
            const dips_sched::Slot sl =
                dips_sched::region_slot(rc, vpr, nvec, a.width, (uint32_t)C, fb, v0 + (uint32_t)(u * 64) + lane);
            const uint32_t r = sl.r, x4 = sl.x4;
            dips_series_entry* e = a.sums + ((uint64_t)r * rc.w + x4);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (x4 + (uint32_t)p >= rc.w) continue;
                dips_series_entry v;
                v.sad = acc[u].sad[p];
                v.sj = acc[u].sjc[p] & 0xFFFFFu;
                v.count = acc[u].sjc[p] >> 20;
                if constexpr (ISI != 0)
                    v.si_fixed = acc[u].si[p] << 4;
                else
                    v.si_fixed = (uint64_t)(acc[u].si[p] * 512.0);
                if (a.out_mode == 2u) {
                    unsigned long long* q = reinterpret_cast<unsigned long long*>(e + p);
                    atomicAdd(q + 0, (unsigned long long)v.sad);
                    atomicAdd(q + 1, (unsigned long long)v.sj);
                    atomicAdd(q + 2, (unsigned long long)v.count);
                    atomicAdd(q + 3, (unsigned long long)v.si_fixed);
                } else {
                    if (a.out_mode == 1u) {
                        const dips_series_entry o = e[p];
                        v.sad += o.sad;
                        v.sj += o.sj;
                        v.count += o.count;
                        v.si_fixed += o.si_fixed;
                    }
                    e[p] = v;
                }
            }
        }
    }
}

// Generic path: any format, shape and alignment.  One thread per pixel of
// `rect` walks the frames with series_generic_kernel's per-pixel body (the
// reference's own (cmax + cmin) / 2 intensity form, dips_shader.wgsl:73-81)
// and u64 sums, and writes (or adds to) that pixel's entry; no two threads
// share an entry.  It serves GRAY8, DIPS_FLAG_FORCE_GENERIC,
// DIPS_FLAG_CROSSCHECK, the shapes the fast kernel's geometry refuses and the
// pixels it leaves out; being independent of derive_v2 it is the fast
// kernel's on-device cross-check.
template <int C>
__global__ __launch_bounds__(256) void pixels_generic_kernel(PixGenericArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= (uint64_t)a.rect.w * a.rect.h) return;
    const uint32_t py = a.rect.y + (uint32_t)(q / a.rect.w);
    const uint32_t px = a.rect.x + (uint32_t)(q % a.rect.w);
    const uint64_t pb = ((uint64_t)py * a.width + px) * (uint64_t)C;
    auto load_px = [&](const uint8_t* base, uint32_t (&v)[4], uint32_t& j, float& I) {
        v[0] = v[1] = v[2] = v[3] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = base[pb + c];
        uint32_t r = v[0], g = C == 1 ? v[0] : v[1], b = C == 1 ? v[0] : v[2];
        I = intensity_rgb(r, g, b, a.chroma);
        if (a.chroma >= 1u && a.chroma <= 3u)
            j = 2u * (a.chroma == 1u ? r : (a.chroma == 2u ? g : b));
        else
            j = max(max(r, g), b) + min(min(r, g), b);
    };
    uint32_t rv[4], jr;
    float Ir;
    load_px(a.ref0, rv, jr, Ir);
    uint64_t sad = 0, sj = 0, cnt = 0, sif = 0;
    for (uint32_t t = 0; t < a.n_frames; ++t) {
        uint32_t fv[4], jf;
        float If;
        load_px(a.frames + (uint64_t)t * a.frame_bytes, fv, jf, If);
#pragma unroll
        for (int c = 0; c < C; ++c) sad += fv[c] > rv[c] ? fv[c] - rv[c] : rv[c] - fv[c];
        sj += jf > jr ? jf - jr : jr - jf;
        const float dI = fabsf(If - Ir);
        if (dI > a.tau) {
            cnt += 1;
            sif += (uint64_t)((double)dI * 4294967296.0);
        }
        if (a.mode == 1u) {
#pragma unroll
            for (int c = 0; c < 4; ++c) rv[c] = fv[c];
            jr = jf;
            Ir = If;
        }
    }
    dips_series_entry* e = a.sums + ((uint64_t)(py - a.roi_y) * a.roi_w + (px - a.roi_x));
    if (a.accumulate != 0u) {
        sad += e->sad;
        sj += e->sj;
        cnt += e->count;
        sif += e->si_fixed;
    }
    e->sad = sad;
    e->sj = sj;
    e->count = cnt;
    e->si_fixed = sif;
}

// ---------------------------------------------------------------------------
// Host-side launchers (instantiation table)
// ---------------------------------------------------------------------------
template <int C, int ISI>
static const void* pick_pix(int chroma, bool pf) {
    return dispatch_chroma(chroma, [&](auto ch) {
        return dispatch_flag(pf, [&](auto p) {
            return reinterpret_cast<const void*>(&series_pixels_kernel<C, ch.value, kUnrollPix, p.value, ISI>);
        });
    });
}

const void* series_pixels_kernel_ptr(int channels, int chroma, bool per_frame, int isi) {
    switch (channels) {
        case 3: return isi == 1 ? pick_pix<3, 1>(chroma, per_frame) : pick_pix<3, 0>(chroma, per_frame);
        case 4: return isi == 1 ? pick_pix<4, 1>(chroma, per_frame) : pick_pix<4, 0>(chroma, per_frame);
        default: return nullptr;
    }
}

hipError_t launch_series_pixels(const PixArgs& a, int channels, int chroma, bool per_frame, int isi, uint32_t blocks,
                                hipStream_t s) {
    const void* k = series_pixels_kernel_ptr(channels, chroma, per_frame, isi);
    if (!k || blocks == 0 || a.part_frames == 0 || a.part_frames > kPixMaxPart || a.n_tiles == 0)
        return hipErrorInvalidValue;
    PixArgs args = a;
    void* params[] = {&args};
    return hipLaunchKernel(k, dim3(blocks), dim3(256), params, 0, s);
}

hipError_t launch_pixels_generic(const PixGenericArgs& a, int channels, hipStream_t s) {
    const uint64_t npx = (uint64_t)a.rect.w * a.rect.h;
    const uint64_t blocks = (npx + 255u) / 256u;
    if (blocks == 0 || a.n_frames == 0) return hipSuccess;
    if (blocks >= (1ull << 23)) return hipErrorInvalidValue;
    switch (channels) {
        case 1: hipLaunchKernelGGL(pixels_generic_kernel<1>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(pixels_generic_kernel<3>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(pixels_generic_kernel<4>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dips
