// series_host.h -- what the host units of the series (series_abi.hip), the
// regional products (region_abi.hip) and the mask products (mask_abi.hip)
// share: the wave slots of a kernel, the environment's schedule knobs, the
// choice between a product's fast and generic kernel, and the staging of host
// frames.  Internal to libdips_hip.so; the schedules themselves are in
// series_sched.h.
#pragma once

#include <cstdlib>

#include "dips_handle.h"
#include "dips_kernels.h"
#include "series_sched.h"
#include "series_screen_rule.h"

namespace dips_internal {

using dips_sched::mask_words_per_row;

// Resident waves per SIMD for a kernel of `occupancy` waves per SIMD, capped
// by DIPS_SERIES_WAVES_PER_SIMD where `env_cap` (a deployment knob; every
// launch applies it, dips_shard_plan also reports the uncapped count).  No
// launch caps itself: leaving a slot per SIMD free for the halo's RCCL
// kernels beside the sharded 'per-frame' launch cost 2-5 ms per 2,000-5,000
// 4K frames, where the full grid lets the exchange through at +0.03-0.07 ms
// (profiles/r06/halo_contention/).
inline uint64_t waves_per_simd(uint64_t occupancy, bool env_cap) {
    if (env_cap) {
        if (const char* cap = std::getenv("DIPS_SERIES_WAVES_PER_SIMD")) {
            const unsigned long c = std::strtoul(cap, nullptr, 10);
            if (c >= 1 && c < occupancy) return c;
        }
    }
    return occupancy;
}

// The wave slots of the device at `occupancy` waves per SIMD (4 SIMDs per CU).
inline uint64_t resident_at(const dips_handle* h, uint64_t occupancy, bool env_cap = true) {
    return waves_per_simd(occupancy, env_cap) * (uint64_t)h->cu_count * 4u;
}

// The wave slots `kernel` (256-thread blocks) has resident; 0: no such kernel.
inline uint64_t resident_waves(dips_handle* h, const void* kernel, bool env_cap = true) {
    return kernel ? resident_at(h, (uint64_t)occupancy_blocks(h, kernel), env_cap) : 0u;
}

// DIPS_PIXEL_PART_FRAMES: the pinned part length of the pixel sums and the
// change times (0: none; series_sched.h cut_parts_unless_full)
inline uint64_t pixel_part_pin() {
    const char* pin = std::getenv("DIPS_PIXEL_PART_FRAMES");
    return pin ? std::strtoul(pin, nullptr, 10) : 0u;
}

// The intensity-sum form of the RGB8 / RGBA8 series kernel for the handle's
// tau (series_v2.hip ISI): 1 (the integer sum) for tau >= 2^-5, 0 (the exact
// f64 sum) below that or with DIPS_FLAG_CROSSCHECK.
inline int series_isi_form(const dips_handle* h) {
    const int C = (int)h->p.format;
    if (C == 1 || h->crosscheck() || !dips::series_v2_isi(h->p.tau)) return 0;
    return 1;
}

// The form series_v2_kernel_ptr is asked for: series_isi_form, with the
// integer sum as 3 (no screen, series_v2_screen.h) where the handle was
// created with the screen switched off (DIPS_SERIES_SCREEN=0).
inline int series_v2_form(const dips_handle* h) {
    const int isi = series_isi_form(h);
    return isi == 1 && !h->series_screen ? 3 : isi;
}

// Whether a regional product may run its fast kernel: GRAY8 has no fast
// form; DIPS_FLAG_CROSSCHECK asks for the plain kernel
inline bool regional_fast_path(const dips_handle* h) {
    return h->p.format != DIPS_FMT_GRAY8 && !(h->p.flags & DIPS_FLAG_FORCE_GENERIC) && !h->crosscheck();
}

inline uint64_t frame_bytes(const dips_handle* h, uint32_t width, uint32_t height) {
    return (uint64_t)width * height * (uint64_t)h->p.format;
}

// series_sched.h for_frame_end_tail_rows over a region: the generic launches
// for the vecs a fast regional kernel leaves out
template <typename Row>
dips_status for_frame_end_tail_rows(uint32_t width, uint32_t height, const dips::GridSpec& g, Row&& row) {
    return dips_sched::for_frame_end_tail_rows(width, height, g.x, g.y, g.w, g.h, row);
}

// Host-pointer calls stage through HBM: `total` bytes of frames into
// stage_frames and, where given, the reference frame into stage_ref, on the
// handle's stream; `out` is the call's output staging, grown to `out_bytes`
// before anything is copied.  *frames_dev: the staged frames (NULL for none);
// *ref_dev: the staged reference, else the staged frames (their first frame).
inline dips_status stage_host_frames(dips_handle* h, const uint8_t* frames, size_t total, const uint8_t* ref, size_t fb,
                                     dips_host::DevBuf& out, size_t out_bytes, const uint8_t** frames_dev,
                                     const uint8_t** ref_dev) {
    DIPS_HIP(h, h->stage_frames.ensure(total));
    DIPS_HIP(h, out.ensure(out_bytes));
    if (total) DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, frames, total, hipMemcpyHostToDevice, h->stream));
    *frames_dev = total ? h->stage_frames.as<uint8_t>() : nullptr;
    *ref_dev = h->stage_frames.as<uint8_t>();
    if (ref) {
        DIPS_HIP(h, h->stage_ref.ensure(fb));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_ref.p, ref, fb, hipMemcpyHostToDevice, h->stream));
        *ref_dev = h->stage_ref.as<uint8_t>();
    }
    return DIPS_OK;
}

}  // namespace dips_internal
