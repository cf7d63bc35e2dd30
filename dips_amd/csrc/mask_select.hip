// mask_select.hip -- the selection of components of a change mask
// (dips_mask_select) and the word-wise logic of two masks (dips_mask_logic).
// The reference has no counterpart; inputs and outputs are bits, so both are
// exact.
//
// dips_mask_select gives the labelling's knowledge back as a mask: the union
// of the components of a frame that pass a predicate on area, on a marker
// mask (reconstruction by marker) and on the region's border.  It runs behind
// launches 1-3 of mask_components.hip (launch_mask_labelling) on the same
// ComponentsArgs: after them parent[node] is the root of every node and the
// root's slot holds area, min_x, max_x and max_y; the anchor's row is
// root / w.  Two launches follow, one thread per mask word each:
//   sel_mark_kernel   (only with a marker) every run of the mask word that
//                     meets marker & mask sets bit 31 of its root's area slot.
//                     Areas stay below 2^30, cc_rows_kernel has cleared the
//                     bit, so the flag needs no plane of its own.  The flag is
//                     read first (a relaxed load) and the lanes of a wave that
//                     share a root issue one fetch-or between them: a full
//                     frame under a full marker costs at most one atomic per
//                     wave, and none once the flag is visible.
//   sel_write_kernel  per run the predicate from the root's slot, the output
//                     word built from the runs kept (or, DIPS_SELECT_DROPPED,
//                     from the others) and stored plainly: the thread is the
//                     word's only writer.  With counts: the kept roots of the
//                     block's words, summed in the block, one integer add per
//                     block onto counts[f], which the host cleared in the
//                     stream; a block lies inside one frame (bpf blocks per
//                     frame) and integer adds commute, so the count is exact.
// Termination: see mask_components.hip; neither kernel waits for another
// thread, the run loops clear at least one bit per step and the wave loop
// retires at least its leader per step.
//
// dips_mask_logic: one launch, a grid stride over the words of all frames.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dips_kernels.h"
#include "mask_labelling.h"  // word_pos, mask_word, slot_of, ld_parent
#include "mask_runs.h"       // next_run

namespace dips {

namespace {

constexpr uint32_t kHitBit = 1u << 31;  // of a root's area slot: a marker pixel lies in the component

__device__ __forceinline__ uint32_t run_bits(uint32_t s, uint32_t e) {
    return (e < 32u ? 1u << e : 0u) - (1u << s);  // bits [s, e)
}

}  // namespace

__global__ __launch_bounds__(256) void sel_mark_kernel(SelectArgs g) {
    const ComponentsArgs& a = g.cc;
    const WordPos q = word_pos(a);  // no early return: every lane takes part in the wave's ballots
    uint32_t word = 0u, hit = 0u;
    if (q.active) {
        word = mask_word(a, q.f, q.j, q.k);
        hit = word & g.marker[(size_t)q.f * g.marker_stride + (size_t)q.j * a.wpr + q.k];
    }
    uint32_t rem = hit ? word : 0u;  // a word no marker bit meets has nothing to report
    const uint32_t* parent = a.parent + (size_t)q.f * a.npx;
    const uint32_t lane = threadIdx.x & 63u;
    while (__ballot(rem != 0u)) {
        bool has = false;
        uint32_t root = 0u;
        size_t sl = 0;
        if (rem != 0u) {
            uint32_t s, e;
            next_run(rem, s, e);
            if (hit & run_bits(s, e)) {
                root = ld_parent(parent + q.j * a.w + q.k * 32u + s);  // a root since cc_stats_kernel
                sl = slot_of(a, q.f, root / a.w, root % a.w);
                has = (ld_parent(a.area + sl) & kHitBit) == 0u;  // set already: nothing to do
            }
        }
        unsigned long long pending = __ballot(has);
        while (pending) {  // loses at least the leader's bit per step
            const int leader = __ffsll(pending) - 1;
            const uint32_t lroot = (uint32_t)__shfl((int)root, leader);
            if ((int)lane == leader) atomicOr(a.area + sl, kHitBit);
            has = has && root != lroot;  // same frame too: the wave's frame is one
            pending = __ballot(has);
        }
    }
}

__global__ __launch_bounds__(256) void sel_write_kernel(SelectArgs g) {
    __shared__ uint32_t sh[4];
    const ComponentsArgs& a = g.cc;
    const WordPos q = word_pos(a);
    uint32_t kept_roots = 0u;
    if (q.active) {
        const uint32_t word = mask_word(a, q.f, q.j, q.k);
        const uint32_t* parent = a.parent + (size_t)q.f * a.npx;
        const bool border = (g.select & DIPS_SELECT_CLEAR_BORDER) != 0u;
        uint32_t rem = word, out = 0u;
        uint32_t last_root = ~0u;
        bool last_keep = false;
        while (rem) {
            uint32_t s, e;
            next_run(rem, s, e);
            const uint32_t node = q.j * a.w + q.k * 32u + s;
            const uint32_t root = parent[node];  // a root since cc_stats_kernel
            if (root != last_root) {
                const uint32_t rj = root / a.w;
                const size_t sl = slot_of(a, q.f, rj, root - rj * a.w);
                const uint32_t raw = a.area[sl], area = raw & ~kHitBit;
                bool keep = area >= a.min_area && (g.max_area == 0u || area <= g.max_area) &&
                            (g.marker == nullptr || (raw & kHitBit) != 0u);
                if (keep && border)
                    keep = !(a.min_x[sl] == 0u || a.max_x[sl] == a.w - 1u || rj == 0u || a.max_y[sl] == a.h - 1u);
                last_root = root;
                last_keep = keep;
            }
            if (last_keep) {
                out |= run_bits(s, e);
                if (root == node) kept_roots += 1u;
            }
        }
        if (g.select & DIPS_SELECT_DROPPED) out = word & ~out;
        g.out[((size_t)q.f * a.h + q.j) * a.wpr + q.k] = out;
    }
    if (g.counts == nullptr) return;  // uniform over the block
    for (int d = 32; d > 0; d >>= 1) kept_roots += (uint32_t)__shfl_xor((int)kept_roots, d);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = kept_roots;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t total = sh[0] + sh[1] + sh[2] + sh[3];
        if (total != 0u) atomicAdd(g.counts + blockIdx.x / a.bpf, total);
    }
}

// One word per thread and step; `r`, the word's index inside its frame,
// advances with it, so the loop has no 64-bit division.
__global__ __launch_bounds__(256) void mask_logic_kernel(LogicArgs g) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= g.words) return;
    uint32_t r = (uint32_t)(i % g.wpf);                 // the word of its frame
    const uint32_t dr = (uint32_t)(stride % g.wpf);
    const uint32_t tail = g.w & 31u;
    const uint32_t last_mask = tail ? (1u << tail) - 1u : ~0u;
    for (; i < g.words; i += stride) {
        const uint32_t x = g.a[i];
        const uint32_t y = g.b ? g.b[g.b_bcast ? (uint64_t)r : i] : 0u;
        uint32_t v;
        switch (g.op) {
            case DIPS_LOGIC_AND: v = x & y; break;
            case DIPS_LOGIC_OR: v = x | y; break;
            case DIPS_LOGIC_XOR: v = x ^ y; break;
            case DIPS_LOGIC_ANDNOT: v = x & ~y; break;
            default: v = ~x; break;  // DIPS_LOGIC_NOT
        }
        if (r % g.wpr == g.wpr - 1u) v &= last_mask;
        g.out[i] = v;
        r += dr;
        if (r >= g.wpf) r -= g.wpf;
    }
}

hipError_t launch_mask_select(const SelectArgs& g, hipStream_t s) {
    const ComponentsArgs& a = g.cc;
    const uint64_t word_blocks = (uint64_t)a.n_frames * a.bpf;
    if (a.n_frames == 0 || a.w == 0 || a.h == 0 || a.npx != a.w * a.h || a.npx >= (1u << 30) ||
        a.wpr != (a.w + 31u) / 32u || a.hw != (a.w + 1u) / 2u || a.nslots != a.hw * a.h || a.wpf != a.wpr * a.h ||
        a.bpf != (a.wpf + 255u) / 256u || word_blocks >= (1ull << 31) || !a.mask || !a.parent || !a.area ||
        !a.min_x || !a.max_x || !a.max_y || !g.out || (g.marker && g.marker_stride != 0u && g.marker_stride != a.wpf) ||
        (g.select & ~(DIPS_SELECT_CLEAR_BORDER | DIPS_SELECT_DROPPED)) != 0u)
        return hipErrorInvalidValue;
    const dim3 wg((uint32_t)word_blocks), tb(256);
    if (g.marker) hipLaunchKernelGGL(sel_mark_kernel, wg, tb, 0, s, g);
    hipLaunchKernelGGL(sel_write_kernel, wg, tb, 0, s, g);
    return hipGetLastError();
}

hipError_t launch_mask_logic(const LogicArgs& g, hipStream_t s) {
    if (g.words == 0 || g.w == 0 || g.wpr != (g.w + 31u) / 32u || g.wpf == 0 || g.wpf % g.wpr != 0u ||
        g.wpf >= (1u << 30) || g.words % g.wpf != 0u || !g.a || !g.out || g.op > DIPS_LOGIC_NOT ||
        (g.op == DIPS_LOGIC_NOT) != (g.b == nullptr))
        return hipErrorInvalidValue;
    constexpr uint64_t kMaxBlocks = 1u << 15;  // beyond: the grid stride
    const uint64_t blocks = std::min<uint64_t>((g.words + 255u) / 256u, kMaxBlocks);
    hipLaunchKernelGGL(mask_logic_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, g);
    return hipGetLastError();
}

}  // namespace dips
