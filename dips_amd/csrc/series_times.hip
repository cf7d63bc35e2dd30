// series_times.hip -- the change times per pixel of a region of interest
// (dips_diff_pixel_times): with bit(t, j, i) = |dI_t| > tau the bit of
// dips_diff_change_mask, per pixel the global index of the first and of the
// last frame whose bit is 1, the longest run of consecutive 1 bits and the
// run that ends at the newest frame -- four u32 planes of roi_w * roi_h, one
// read of the batch, every value written once.
//
// The fold of frame g (a global index, wave-uniform) into a pixel's state
// {first, last, run_max, run_cur}, initially {NONE, NONE, 0, 0}:
//   bit = 1: first = min(first, g)  (g only grows and NONE is the largest u32)
//            last = g, run_cur += 1, run_max = max(run_max, run_cur)
//   bit = 0: run_cur = 0
//
// The fast kernel takes series_mask_kernel's per-frame step (derive_v2, the
// subtract and the strict compare in the 2^22-scaled domain; one intensity
// form serves every tau, so there is no integer-sum axis) and
// series_pixels_kernel's ownership and output: the regional skeleton
// (series_region.h) over the flat slots of the region (series_slots.h
// region_slot) with the frames-only ring, and the state of a lane's pixels in
// registers across the frames of the item, stored by that lane with plain
// stores.  The pixels of a partial vec beyond the region's right edge are
// computed from the bytes that follow and never stored; a partial vec that
// would read past the frame's end is left out (its <= 3 pixels go to the
// generic kernel: run_times_device, by for_frame_end_tail_rows).
//
// One part (MP = false): a wave owns every frame of its pixels.  It starts
// from the initial state, or when the call accumulates from the state the
// output holds (load-fold-store), and writes the four planes.
//
// Several parts (MP = true; regions with too few tiles to fill the wave
// slots): a run may span a part boundary, so parts cannot be combined with
// atomics.  Each part folds its own frames from the initial state, keeps a
// fifth value per pixel -- the length of its leading run -- and writes a
// summary {first, last, run_max, leading, trailing = run_cur} to five planes
// of a scratch buffer.  times_combine_kernel, a later launch of the same
// stream, folds the summaries in order onto the initial or accumulated state,
// one thread per pixel:
//   first    = state.first == NONE ? part.first : state.first
//   last     = part.last == NONE ? state.last : part.last
//   run_max  = max(state.run_max, part.run_max, state.run_cur + part.leading)
//   run_cur  = part.leading == len ? state.run_cur + len : part.trailing
// with len the part's frame count, known from the geometry.  In per-frame
// mode a part's first reference is the frame before it, so a part's bits are
// those of the whole clip and the result does not depend on the part count.
#include "series_region.h"

namespace dips {

constexpr uint32_t kTimeNone = 0xFFFFFFFFu;  // DIPS_TIME_NONE

template <bool MP>
struct TimesAcc {
    uint32_t first[4], last[4], rmax[4], rcur[4];
    uint32_t lead[MP ? 4 : 1];  // several parts only
};

// One frame of one tile: fold every pixel's bit of global frame `g` into its
// state; `kk` the frames of the item folded so far, this one included (the
// leading run is the current run as long as that spans them all); `st` is the
// reference state (updated to this frame's in per-frame mode).
template <int C, int CH, int U, bool PF, bool MP>
__device__ __forceinline__ void frame_times(float thr, uint32_t g, uint32_t kk, St2 (&st)[U],
                                            const uint32_t (&cur)[U][Fmt<C>::NDW], TimesAcc<MP> (&acc)[U]) {
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
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const f32x2 d = n.i[k] - st[u].i[k];
            const bool s[2] = {fabsf(d.x) > thr, fabsf(d.y) > thr};
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int p = 2 * k + q;
                acc[u].first[p] = min(acc[u].first[p], s[q] ? g : kTimeNone);
                acc[u].last[p] = s[q] ? g : acc[u].last[p];
                acc[u].rcur[p] = s[q] ? acc[u].rcur[p] + 1u : 0u;
                acc[u].rmax[p] = max(acc[u].rmax[p], acc[u].rcur[p]);
                if constexpr (MP) acc[u].lead[p] = acc[u].rcur[p] == kk ? kk : acc[u].lead[p];
            }
        }
        if constexpr (PF) st[u] = n;
    }
}

// Waves per SIMD asked of the register allocator (DIPS_TIMES_WAVES: probe
// builds of the vecs-per-lane comparison).
#ifndef DIPS_TIMES_WAVES
#define DIPS_TIMES_WAVES 4
#endif

template <int C, int CH, int U, bool PF, bool MP>
__global__ __launch_bounds__(256, DIPS_TIMES_WAVES) void series_times_kernel(TimesArgs a) {
    using F = Fmt<C>;
    constexpr int NDW = F::NDW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    const uint32_t fb = a.frame_bytes;
    const GridRect rc = a.roi;
    const uint32_t vpr = (rc.w + 3u) >> 2;  // vecs per region row
    const uint32_t nvec = vpr * rc.h;
    const uint64_t npx = (uint64_t)rc.w * rc.h;  // u32 per plane

    const uint64_t pitems = region_items(a.n_frames, a.part_frames, a.n_tiles);
    for (uint64_t it = wave; it < pitems; it += a.n_waves) {
        const RegionItem i = region_item(it, a.n_frames, a.part_frames, a.n_tiles);
        const uint32_t part = i.part, t0 = i.t0, n = i.n, tlast = i.tlast;
        const uint32_t v0 = i.tile * (uint32_t)(64 * U);

        // per lane-slot, once per tile: where it loads from, the index of
        // its first pixel in a plane and how many of its pixels are stored
        uint32_t voff[U], pbase[U], left[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const dips_sched::Slot s =
                dips_sched::region_slot(rc, vpr, nvec, a.width, (uint32_t)C, fb, v0 + (uint32_t)(u * 64) + lane);
            voff[u] = s.voff;
            pbase[u] = s.ok ? s.r * rc.w + s.x4 : 0u;
            left[u] = s.ok ? dips_sched::vec_px_inside(rc.w, s.x4) : 0u;
        }

        const FrameLoader<C, U> ld{a.frames, fb, tlast, voff};

        // ring: frame k of the item in slot k & 3; the reference (the frame
        // before the part in per-frame mode) only leaves its state
        uint32_t buf[4][U][NDW];
        St2 st[U];
        TimesAcc<MP> acc[U];
        {
            const uint8_t* rp = PF ? (t0 == 0 ? a.ref0 : a.frames + (uint64_t)(t0 - 1) * fb) : a.ref0;
            uint32_t rb[U][NDW];
            ld.at(rp, rb);
            ld.fill(t0, buf);
            // the state the fold starts from, while the frames are in flight
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    acc[u].first[p] = kTimeNone;
                    acc[u].last[p] = kTimeNone;
                    acc[u].rmax[p] = 0u;
                    acc[u].rcur[p] = 0u;
                    if constexpr (MP) acc[u].lead[p] = 0u;
                }
                if constexpr (!MP) {
                    if (a.accumulate != 0u) {
                        const uint32_t* o = a.out + pbase[u];
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            if ((uint32_t)p >= left[u]) continue;
                            acc[u].first[p] = o[p];
                            acc[u].last[p] = o[npx + p];
                            acc[u].rmax[p] = o[2u * npx + p];
                            acc[u].rcur[p] = o[3u * npx + p];
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) derive_v2<C, CH, false>(rb[u], st[u]);
        }

        const uint32_t g0 = a.t0 + t0;  // global index of the item's first frame
        uint32_t k = 0;
        for (; k + 4 <= n; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t kj = k + (uint32_t)j;
                frame_times<C, CH, U, PF, MP>(a.thr, g0 + kj, kj + 1u, st, buf[j], acc);
                __builtin_amdgcn_sched_barrier(0);
                ld.frame(t0 + kj + 4u, buf[j]);
            }
        }
        // tail: up to 3 frames, already in flight in their slots
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t kj = k + (uint32_t)j;
            if (kj < n) frame_times<C, CH, U, PF, MP>(a.thr, g0 + kj, kj + 1u, st, buf[j], acc);
        }

        // the planes of this item's pixels: a lane's four are 16 contiguous
        // bytes of each plane (one part: the output; several: this part's
        // five summary planes)
        uint32_t* const out = a.out + (MP ? (uint64_t)part * 5u * npx : 0u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint32_t* o = out + pbase[u];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if ((uint32_t)p >= left[u]) continue;
                o[p] = acc[u].first[p];
                o[npx + p] = acc[u].last[p];
                o[2u * npx + p] = acc[u].rmax[p];
                if constexpr (MP) {
                    o[3u * npx + p] = acc[u].lead[p];
                    o[4u * npx + p] = acc[u].rcur[p];
                } else {
                    o[3u * npx + p] = acc[u].rcur[p];
                }
            }
        }
    }
}

// The fold of the parts' summaries, one thread per pixel of the region, in a
// launch after series_times_kernel<MP = true>.  The pixels of the vecs that
// kernel leaves out have no summaries and are not touched here (the generic
// kernel writes them).
__global__ __launch_bounds__(256) void times_combine_kernel(TimesCombineArgs a) {
    const uint64_t npx = (uint64_t)a.roi.w * a.roi.h;
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= npx) return;
    const uint32_t j = (uint32_t)(q / a.roi.w);
    const uint32_t i = (uint32_t)(q - (uint64_t)j * a.roi.w);
    const uint32_t off = ((a.roi.y + j) * a.width + a.roi.x + (i & ~3u)) * a.channels;
    if (dips_sched::vec_crosses_frame_end(off, 4u * a.channels, a.frame_bytes)) return;
    uint32_t first = kTimeNone, last = kTimeNone, rmax = 0u, rcur = 0u;
    if (a.accumulate != 0u) {
        first = a.times[q];
        last = a.times[npx + q];
        rmax = a.times[2u * npx + q];
        rcur = a.times[3u * npx + q];
    }
    for (uint32_t part = 0, t = 0; t < a.n_frames; ++part, t += a.part_frames) {
        const uint32_t len = min(a.part_frames, a.n_frames - t);
        const uint32_t* s = a.parts + (uint64_t)part * 5u * npx + q;
        const uint32_t pf = s[0], pl = s[npx], pm = s[2u * npx], lead = s[3u * npx], trail = s[4u * npx];
        first = first == kTimeNone ? pf : first;
        last = pl == kTimeNone ? last : pl;
        rmax = max(max(rmax, pm), rcur + lead);
        rcur = lead == len ? rcur + len : trail;
    }
    a.times[q] = first;
    a.times[npx + q] = last;
    a.times[2u * npx + q] = rmax;
    a.times[3u * npx + q] = rcur;
}

// Generic path: any format, shape and alignment.  One thread per pixel of
// `rect` walks the frames with series_generic_kernel's per-pixel body (the
// reference's own (cmax + cmin) / 2 intensity form, dips_shader.wgsl:73-81),
// folds each bit as it comes and writes (or updates) that pixel's four
// values; no two threads share a pixel, there are no atomics.  It serves
// GRAY8, DIPS_FLAG_FORCE_GENERIC, DIPS_FLAG_CROSSCHECK, the shapes the fast
// kernel's geometry refuses and the pixels it leaves out; being independent
// of derive_v2 it is the fast kernel's on-device cross-check.
template <int C>
__global__ __launch_bounds__(256) void times_generic_kernel(TimesGenericArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= (uint64_t)a.rect.w * a.rect.h) return;
    const uint32_t py = a.rect.y + (uint32_t)(q / a.rect.w);
    const uint32_t px = a.rect.x + (uint32_t)(q % a.rect.w);
    const uint64_t pb = ((uint64_t)py * a.width + px) * (uint64_t)C;
    auto load_px = [&](const uint8_t* base) -> float { return generic_intensity<C>(base, pb, a.chroma); };
    const uint64_t npx = (uint64_t)a.roi.w * a.roi.h;
    uint32_t* e = a.times + ((uint64_t)(py - a.roi.y) * a.roi.w + (px - a.roi.x));
    uint32_t first = kTimeNone, last = kTimeNone, rmax = 0u, rcur = 0u;
    if (a.accumulate != 0u) {
        first = e[0];
        last = e[npx];
        rmax = e[2u * npx];
        rcur = e[3u * npx];
    }
    float Ir = load_px(a.ref0);
    for (uint32_t t = 0; t < a.n_frames; ++t) {
        const float If = load_px(a.frames + (uint64_t)t * a.frame_bytes);
        if (fabsf(If - Ir) > a.tau) {
            const uint32_t g = a.t0 + t;
            first = first == kTimeNone ? g : first;
            last = g;
            rcur += 1u;
            rmax = max(rmax, rcur);
        } else {
            rcur = 0u;
        }
        if (a.mode == 1u) Ir = If;
    }
    e[0] = first;
    e[npx] = last;
    e[2u * npx] = rmax;
    e[3u * npx] = rcur;
}

// ---------------------------------------------------------------------------
// Host-side launchers (instantiation table)
// ---------------------------------------------------------------------------
template <int C>
static const void* pick_times(int chroma, bool pf, bool mp) {
    return dispatch_chroma(chroma, [&](auto ch) {
        return dispatch_flag(pf, [&](auto p) {
            return dispatch_flag(mp, [&](auto m) {
                return reinterpret_cast<const void*>(&series_times_kernel<C, ch.value, kUnrollTimes, p.value, m.value>);
            });
        });
    });
}

const void* series_times_kernel_ptr(int channels, int chroma, bool per_frame, bool parts) {
    switch (channels) {
        case 3: return pick_times<3>(chroma, per_frame, parts);
        case 4: return pick_times<4>(chroma, per_frame, parts);
        default: return nullptr;
    }
}

hipError_t launch_series_times(const TimesArgs& a, int channels, int chroma, bool per_frame, bool parts,
                               uint32_t blocks, hipStream_t s) {
    const void* k = series_times_kernel_ptr(channels, chroma, per_frame, parts);
    if (!k || blocks == 0 || a.part_frames == 0 || a.n_tiles == 0 || a.n_frames == 0 || !a.out ||
        ((uintptr_t)a.out & 3u) != 0 || (uint64_t)a.t0 + a.n_frames > 0xFFFFFFFFull ||
        (!parts && a.part_frames < a.n_frames) || (parts && a.accumulate != 0u))
        return hipErrorInvalidValue;
    TimesArgs args = a;
    void* params[] = {&args};
    return hipLaunchKernel(k, dim3(blocks), dim3(256), params, 0, s);
}

hipError_t launch_times_combine(const TimesCombineArgs& a, hipStream_t s) {
    const uint64_t npx = (uint64_t)a.roi.w * a.roi.h;
    const uint64_t blocks = (npx + 255u) / 256u;
    if (blocks == 0 || blocks >= (1ull << 23) || a.part_frames == 0 || a.n_frames == 0 || !a.parts || !a.times ||
        (a.channels != 3u && a.channels != 4u))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(times_combine_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_times_generic(const TimesGenericArgs& a, int channels, hipStream_t s) {
    const uint64_t npx = (uint64_t)a.rect.w * a.rect.h;
    const uint64_t blocks = (npx + 255u) / 256u;
    if (blocks == 0 || a.n_frames == 0) return hipSuccess;
    if (blocks >= (1ull << 23) || a.rect.x < a.roi.x || a.rect.y < a.roi.y ||
        (uint64_t)a.rect.x + a.rect.w > (uint64_t)a.roi.x + a.roi.w ||
        (uint64_t)a.rect.y + a.rect.h > (uint64_t)a.roi.y + a.roi.h)
        return hipErrorInvalidValue;
    switch (channels) {
        case 1: hipLaunchKernelGGL(times_generic_kernel<1>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(times_generic_kernel<3>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(times_generic_kernel<4>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dips
