// mask_labelling.h -- what the kernels behind the labelling share with it
// (mask_components.hip, mask_select.hip, mask_shapes.hip): the thread's word
// of a chunk, the mask word with its pad bits cleared, the statistics slot of
// a node and the relaxed load of a parent.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dips_kernels.h"

namespace dips {

__device__ __forceinline__ uint32_t ld_parent(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The thread's word of the chunk: frame f, row j, word k of the row; false
// for the threads past the frame's last word.
struct WordPos {
    uint32_t f, j, k;
    bool active;
};

__device__ __forceinline__ WordPos word_pos(const ComponentsArgs& a) {
    WordPos q;
    q.f = blockIdx.x / a.bpf;
    const uint32_t wi = (blockIdx.x - q.f * a.bpf) * 256u + threadIdx.x;
    q.active = wi < a.wpf;
    q.j = q.active ? wi / a.wpr : 0u;
    q.k = q.active ? wi - q.j * a.wpr : 0u;
    return q;
}

// Word k of row j of frame f with the pad bits of the row's last word cleared.
__device__ __forceinline__ uint32_t mask_word(const ComponentsArgs& a, uint32_t f, uint32_t j, uint32_t k) {
    uint32_t v = a.mask[((size_t)f * a.h + j) * a.wpr + k];
    if (k == a.wpr - 1u && (a.w & 31u) != 0u) v &= (1u << (a.w & 31u)) - 1u;
    return v;
}

__device__ __forceinline__ size_t slot_of(const ComponentsArgs& a, uint32_t f, uint32_t j, uint32_t i) {
    return (size_t)f * a.nslots + (size_t)j * a.hw + (i >> 1);
}

}  // namespace dips
