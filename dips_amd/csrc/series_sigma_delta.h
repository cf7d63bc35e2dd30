// series_sigma_delta.h -- arguments and launchers of the Sigma-Delta
// background model and its per-pixel adaptive threshold mask
// (dips_diff_sigma_delta_mask; kernels in series_sigma_delta.hip).
#pragma once

#include "dips_kernels.h"

namespace dips {

// series_sigma_delta_kernel: the background kernel's geometry (rows padded to
// 8 vecs per mask word, one part always: a wave owns every frame of its tile)
// with the state of its pixels -- the u16 pair (M, V) -- in registers.
#ifndef DIPS_UNROLL_SIGMA_DELTA
#define DIPS_UNROLL_SIGMA_DELTA 4
#endif
constexpr int kUnrollSigmaDelta = DIPS_UNROLL_SIGMA_DELTA;  // vecs per lane: 1024 px / wave / frame
struct SdArgs {
    const uint8_t* frames;   // n_frames * frame_bytes, contiguous
    const uint8_t* ref0;     // accumulate == 0: the initial M is J of its pixels
    uint16_t* state;         // 2 planes (M, V) of roi.w * roi.h u16, 2-byte aligned
    uint8_t* mask;           // n_frames * mask_frame_bytes, 4-byte aligned, or NULL
    uint32_t frame_bytes;
    uint32_t mask_frame_bytes;  // roi.h * 4 * ceil(roi.w / 32)
    uint32_t width;
    uint32_t n_frames;       // >= 1
    uint32_t n_tiles;
    uint32_t n_waves;
    uint32_t n_amp;          // 1 .. 15
    uint32_t v_min, v_max;   // 0 <= v_min <= v_max <= 510
    uint32_t accumulate;     // continue the state `state` holds
    GridRect roi;
};

// sigma_delta_generic_kernel: one thread per mask word of rows [row0, row0 +
// n_rows) x words [word0, word0 + n_words) of the region walks the word's
// pixels and, per pixel, the frames; it stores the state of the pixels from
// region column state_x0 on.  n_frames may be 0 (the initial state alone).
struct SdGenericArgs {
    const uint8_t* frames;
    const uint8_t* ref0;
    uint16_t* state;
    uint8_t* mask;           // or NULL
    uint64_t frame_bytes;
    uint64_t mask_frame_bytes;
    uint32_t width;
    uint32_t n_frames;
    uint32_t chroma;
    uint32_t n_amp, v_min, v_max;
    uint32_t accumulate;
    uint32_t row0, n_rows, word0, n_words;
    uint32_t state_x0;
    GridRect roi;
};

// RGB8 / RGBA8 fast kernel (tiles of kUnrollSigmaDelta vecs per lane, or of
// one for small regions) and the any-format generic kernel
const void* series_sigma_delta_kernel_ptr(int channels, int chroma, bool small_tile);
hipError_t launch_series_sigma_delta(const SdArgs& a, int channels, int chroma, bool small_tile, uint32_t blocks,
                                     hipStream_t s);
hipError_t launch_sigma_delta_generic(const SdGenericArgs& a, int channels, hipStream_t s);

}  // namespace dips
