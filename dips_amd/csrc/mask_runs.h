// mask_runs.h -- the word-local runs of a 32-bit mask word, shared by the
// kernels that name a run by its first bit (mask_components.hip,
// mask_tracks.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dips {

// The first run of `rem` (non-zero): bits [s, e); `rem` loses them.
__device__ __forceinline__ void next_run(uint32_t& rem, uint32_t& s, uint32_t& e) {
    s = (uint32_t)__ffs((int)rem) - 1u;
    const uint32_t clear = ~rem & (~0u << s);
    e = clear ? (uint32_t)__ffs((int)clear) - 1u : 32u;
    rem = e < 32u ? rem & (~0u << e) : 0u;
}

// Start of the word-local run of `word` that holds set bit b.
__device__ __forceinline__ uint32_t local_start(uint32_t word, uint32_t b) {
    const uint32_t below = ~word & ((1u << b) - 1u);
    return below ? 32u - (uint32_t)__clz((int)below) : 0u;
}

}  // namespace dips
