// mask_components.hip -- connected components of the change mask
// (dips_mask_components): per frame of a bit mask in dips_diff_change_mask's
// layout the components under 4- or 8-connectivity, their count, one record
// per component (box, area, anchor, centroid) in the order of their first
// pixel, and optionally the label image.  The reference has no counterpart;
// the input is bits and the answer is combinatorial, so it is exact.
//
// Union-find by smallest linear index, frames independent.  The nodes are the
// word-local runs: a maximal run of set bits inside one 32-bit mask word,
// named by the linear index p = j*w + i of its first pixel.  parent[p] <= p
// always and parent[p] == p marks a root, so the root of a component is its
// first pixel in row-major order: the anchor.  Two starts of a row are at
// least two pixels apart, so the statistics of a node live in slot
// j*ceil(w/2) + i/2: half a value per pixel instead of one.
//
// Six launches per chunk of frames, each one thread per mask word unless
// noted; a later launch of the same stream sees all of an earlier one:
//   1 cc_rows_kernel    every node gets parent = itself, or, where its run
//                       continues the previous word's, the start of that run
//                       (found by walking back over all-ones words, at most
//                       kBackWords of them: beyond that the parent is bit 0
//                       of the word reached, a node of the same run); its
//                       statistics slot is cleared.  Nothing else of the
//                       scratch is ever read, so there is no memset.
//   2 cc_merge_kernel   a run and the bits above it (for 8: also up-left and
//                       up-right) as one 34-bit window: one union per set
//                       fragment of the window, i.e. per run-to-run adjacency.
//   3 cc_stats_kernel   root of every node (written back: every parent is a
//                       root afterwards); per run {len, sum i, sum j, min i,
//                       max i, max j}, summed over the lanes of the wave that
//                       share a root before one lane adds them to the root's
//                       slot: an all-ones frame costs one set of atomics per
//                       wave, not per pixel or run.  min j is the anchor's row.
//   4 cc_count_kernel   kept roots (area >= min_area) per block of 256 words
//     cc_offsets_kernel one block per frame: exclusive scan of those sums,
//                       counts[t] = the total
//     cc_select_kernel  rank of every kept root = block offset + scan inside
//                       the block + position in the word: ascending anchor.
//                       Records with rank < max_boxes are written; the area
//                       slot becomes the label (rank + 1, 0 for a dropped
//                       component).
//   5 cc_labels_kernel  (only when labels are asked for) one thread per pixel:
//                       the label of its node's root.
// The records not written are zeros: the host clears `boxes` first.
//
// Termination: no loop waits for another thread.  find follows parent, which
// strictly decreases until the root; a union that loses its atomicMin goes on
// from the value the atomic returned, which is strictly smaller than the root
// it tried; the run loops clear at least one bit of a word per step; the
// wave-sum loop retires at least its leader per step; the walk back is
// bounded by the row and by kBackWords.  Stale reads of parent are harmless:
// every value a node ever held is a node of its own component, and only the
// atomicMin's return decides whether a union is done.
//
// dips_mask_select runs launches 1-3 (launch_mask_labelling) and then its own
// two (mask_select.hip).  Those add no new kind of loop: sel_mark_kernel's
// run loop clears at least one bit of a word per step and its wave loop
// retires at least its leader per step, like cc_stats_kernel's; its one
// atomic is a fetch-or whose return nobody waits for; sel_write_kernel has
// the run loop only.  Both read parent after launch 3, when it is final.
#include <hip/hip_runtime.h>

#include "dips_kernels.h"
#include "mask_labelling.h"  // word_pos, mask_word, slot_of, ld_parent
#include "mask_runs.h"       // next_run, local_start

namespace dips {

namespace {

constexpr uint32_t kBackWords = 64;  // all-ones words a continuing run walks back over

__device__ __forceinline__ void st_parent(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t find_root(const uint32_t* parent, uint32_t x) {
    uint32_t p = ld_parent(parent + x);
    while (p != x) {  // p < x: strictly decreasing
        x = p;
        p = ld_parent(parent + x);
    }
    return x;
}

__device__ __forceinline__ void unite(uint32_t* parent, uint32_t x, uint32_t y) {
    for (;;) {
        x = find_root(parent, x);
        y = find_root(parent, y);
        if (x == y) return;
        if (x < y) {
            const uint32_t t = x;
            x = y;
            y = t;
        }
        // y < x: hang x under y if x is still a root
        const uint32_t old = atomicMin(parent + x, y);
        if (old == x) return;
        x = old;  // someone else hung x under old < x: unite old and y
    }
}

// Exclusive prefix sum of v over the block's 256 threads; *total = the sum.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1u; d < 256u; d <<= 1) {
        const uint32_t add = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const uint32_t incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

// Kept roots among the nodes of word `word` at (f, j, k).
__device__ __forceinline__ uint32_t kept_in_word(const ComponentsArgs& a, const WordPos& q, uint32_t word) {
    const uint32_t* parent = a.parent + (size_t)q.f * a.npx;
    uint32_t rem = word, n = 0;
    while (rem) {
        uint32_t s, e;
        next_run(rem, s, e);
        const uint32_t i = q.k * 32u + s, p = q.j * a.w + i;
        if (parent[p] == p && a.area[slot_of(a, q.f, q.j, i)] >= a.min_area) n += 1u;
    }
    return n;
}

}  // namespace

__global__ __launch_bounds__(256) void cc_rows_kernel(ComponentsArgs a) {
    const WordPos q = word_pos(a);
    if (!q.active) return;
    uint32_t rem = mask_word(a, q.f, q.j, q.k);
    if (!rem) return;
    uint32_t* parent = a.parent + (size_t)q.f * a.npx;
    const uint32_t row = q.j * a.w;
    while (rem) {
        uint32_t s, e;
        next_run(rem, s, e);
        const uint32_t i = q.k * 32u + s;
        uint32_t up = row + i;
        if (s == 0u && q.k > 0u) {
            uint32_t kk = q.k - 1u;
            uint32_t prev = mask_word(a, q.f, q.j, kk);
            if (prev >> 31) {
                // the run continues the previous word's
                for (uint32_t n = 0; prev == ~0u && kk > 0u && n < kBackWords; ++n) {
                    kk -= 1u;
                    prev = mask_word(a, q.f, q.j, kk);
                }
                up = row + kk * 32u + (prev == ~0u ? 0u : 32u - (uint32_t)__clz((int)~prev));
            }
        }
        parent[row + i] = up;
        const size_t sl = slot_of(a, q.f, q.j, i);
        a.sum_i[sl] = 0ull;
        a.sum_j[sl] = 0ull;
        a.area[sl] = 0u;
        a.min_x[sl] = ~0u;
        a.max_x[sl] = 0u;
        a.max_y[sl] = 0u;
    }
}

__global__ __launch_bounds__(256) void cc_merge_kernel(ComponentsArgs a) {
    const WordPos q = word_pos(a);
    if (!q.active || q.j == 0u) return;
    uint32_t rem = mask_word(a, q.f, q.j, q.k);
    if (!rem) return;
    const bool c8 = a.connectivity == 8u;
    const uint32_t above = mask_word(a, q.f, q.j - 1u, q.k);
    const uint32_t above_l = c8 && q.k > 0u ? mask_word(a, q.f, q.j - 1u, q.k - 1u) : 0u;
    const uint32_t above_r = c8 && q.k + 1u < a.wpr ? mask_word(a, q.f, q.j - 1u, q.k + 1u) : 0u;
    // bit b of the window is the pixel above local position b - 1
    const uint64_t win = (uint64_t)(above_l >> 31) | ((uint64_t)above << 1) | ((uint64_t)(above_r & 1u) << 33);
    if (!win) return;
    uint32_t* parent = a.parent + (size_t)q.f * a.npx;
    const uint32_t row = q.j * a.w, row_up = row - a.w;
    while (rem) {
        uint32_t s, e;
        next_run(rem, s, e);
        // 8: local positions s - 1 .. e, 4: s .. e - 1
        const uint32_t lo = c8 ? s : s + 1u, n = c8 ? e - s + 2u : e - s;
        uint64_t u = win & (((1ull << n) - 1ull) << lo);
        const uint32_t node = row + q.k * 32u + s;
        while (u) {
            // one fragment of set bits: one run of the row above
            const uint32_t b = (uint32_t)__ffsll((unsigned long long)u) - 1u;
            const uint64_t clear = ~u & (~0ull << b);
            const uint32_t eb = clear ? (uint32_t)__ffsll((unsigned long long)clear) - 1u : 64u;
            u = eb < 64u ? u & (~0ull << eb) : 0ull;
            uint32_t ka = q.k, ba = b - 1u, wa = above;
            if (b == 0u) {
                ka = q.k - 1u;
                ba = 31u;
                wa = above_l;
            } else if (b == 33u) {
                ka = q.k + 1u;
                ba = 0u;
                wa = above_r;
            }
            unite(parent, node, row_up + ka * 32u + local_start(wa, ba));
        }
    }
}

__global__ __launch_bounds__(256) void cc_stats_kernel(ComponentsArgs a) {
    const WordPos q = word_pos(a);  // no early return: every lane takes part in the wave sums
    uint32_t rem = q.active ? mask_word(a, q.f, q.j, q.k) : 0u;
    uint32_t* parent = a.parent + (size_t)q.f * a.npx;
    const uint32_t lane = threadIdx.x & 63u;
    while (__ballot(rem != 0u)) {
        bool has = rem != 0u;
        uint32_t root = 0u, len = 0u, x0 = 0u;
        if (has) {
            uint32_t s, e;
            next_run(rem, s, e);
            x0 = q.k * 32u + s;
            len = e - s;
            const uint32_t node = q.j * a.w + x0;
            root = find_root(parent, node);
            if (root != node) st_parent(parent + node, root);
        }
        unsigned long long pending = __ballot(has);
        while (pending) {  // loses at least the leader's bit per step
            const int leader = __ffsll(pending) - 1;
            const uint32_t lroot = (uint32_t)__shfl((int)root, leader);
            const bool m = has && root == lroot;  // same frame too: the wave's frame is one (bpf blocks per frame)
            uint32_t ar = m ? len : 0u;
            unsigned long long si = m ? ((unsigned long long)len * (2ull * x0 + len - 1ull)) / 2ull : 0ull;
            unsigned long long sj = m ? (unsigned long long)len * q.j : 0ull;
            uint32_t mn = m ? x0 : ~0u, mx = m ? x0 + len - 1u : 0u, my = m ? q.j : 0u;
            for (int d = 32; d > 0; d >>= 1) {
                ar += (uint32_t)__shfl_xor((int)ar, d);
                si += __shfl_xor(si, d);
                sj += __shfl_xor(sj, d);
                mn = min(mn, (uint32_t)__shfl_xor((int)mn, d));
                mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
                my = max(my, (uint32_t)__shfl_xor((int)my, d));
            }
            if ((int)lane == leader) {
                const size_t sl = slot_of(a, q.f, lroot / a.w, lroot % a.w);
                atomicAdd(a.area + sl, ar);
                atomicAdd((unsigned long long*)(a.sum_i + sl), si);
                atomicAdd((unsigned long long*)(a.sum_j + sl), sj);
                atomicMin(a.min_x + sl, mn);
                atomicMax(a.max_x + sl, mx);
                atomicMax(a.max_y + sl, my);
            }
            has = has && !m;
            pending = __ballot(has);
        }
    }
}

__global__ __launch_bounds__(256) void cc_count_kernel(ComponentsArgs a) {
    __shared__ uint32_t sh[256];
    const WordPos q = word_pos(a);
    const uint32_t n = q.active ? kept_in_word(a, q, mask_word(a, q.f, q.j, q.k)) : 0u;
    uint32_t total;
    (void)block_exclusive_scan(n, sh, &total);
    if (threadIdx.x == 0u) a.block_count[blockIdx.x] = total;
}

// One block per frame: block_count becomes its exclusive scan, counts[f] the total.
__global__ __launch_bounds__(256) void cc_offsets_kernel(ComponentsArgs a) {
    __shared__ uint32_t sh[256];
    uint32_t* bc = a.block_count + (size_t)blockIdx.x * a.bpf;
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < a.bpf; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < a.bpf ? bc[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, sh, &total);
        if (i < a.bpf) bc[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0u) a.counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void cc_select_kernel(ComponentsArgs a) {
    __shared__ uint32_t sh[256];
    const WordPos q = word_pos(a);
    const uint32_t word = q.active ? mask_word(a, q.f, q.j, q.k) : 0u;
    const uint32_t n = q.active ? kept_in_word(a, q, word) : 0u;
    uint32_t total;
    uint32_t rank = a.block_count[blockIdx.x] + block_exclusive_scan(n, sh, &total);
    const uint32_t* parent = a.parent + (size_t)q.f * a.npx;
    uint32_t rem = word;
    while (rem) {
        uint32_t s, e;
        next_run(rem, s, e);
        const uint32_t i = q.k * 32u + s, p = q.j * a.w + i;
        if (parent[p] != p) continue;
        const size_t sl = slot_of(a, q.f, q.j, i);
        const uint32_t area = a.area[sl];
        if (area < a.min_area) {
            a.area[sl] = 0u;  // the slot is the label from here on: dropped
            continue;
        }
        a.area[sl] = rank + 1u;
        if (rank < a.max_boxes) {
            const unsigned long long si = a.sum_i[sl], sj = a.sum_j[sl];
            uint32_t* r = a.boxes + ((size_t)q.f * a.max_boxes + rank) * DIPS_BOX_WORDS;
            r[DIPS_BOX_X0] = a.min_x[sl];
            r[DIPS_BOX_Y0] = q.j;
            r[DIPS_BOX_X1] = a.max_x[sl] + 1u;
            r[DIPS_BOX_Y1] = a.max_y[sl] + 1u;
            r[DIPS_BOX_AREA] = area;
            r[DIPS_BOX_ANCHOR] = p;
            r[DIPS_BOX_CX256] = (uint32_t)((si / area) * 256ull + ((si % area) * 256ull) / area);
            r[DIPS_BOX_CY256] = (uint32_t)((sj / area) * 256ull + ((sj % area) * 256ull) / area);
        }
        rank += 1u;
    }
}

__global__ __launch_bounds__(256) void cc_labels_kernel(ComponentsArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)a.n_frames * a.npx) return;
    const uint32_t f = (uint32_t)(t / a.npx), p = (uint32_t)(t - (uint64_t)f * a.npx);
    const uint32_t j = p / a.w, i = p - j * a.w;
    const uint32_t word = mask_word(a, f, j, i >> 5);
    uint32_t label = 0u;
    if ((word >> (i & 31u)) & 1u) {
        const uint32_t node = j * a.w + (i & ~31u) + local_start(word, i & 31u);
        const uint32_t root = a.parent[(size_t)f * a.npx + node];  // a root since cc_stats_kernel
        label = a.area[slot_of(a, f, root / a.w, root % a.w)];
    }
    a.labels[t] = label;
}

// Whether `a` describes a chunk the labelling's launches can take.
static bool labelling_args_ok(const ComponentsArgs& a) {
    const uint64_t word_blocks = (uint64_t)a.n_frames * a.bpf;
    return !(a.n_frames == 0 || a.w == 0 || a.h == 0 || a.npx != a.w * a.h || a.npx >= (1u << 30) ||
             a.wpr != (a.w + 31u) / 32u || a.hw != (a.w + 1u) / 2u || a.nslots != a.hw * a.h ||
             a.wpf != a.wpr * a.h || a.bpf != (a.wpf + 255u) / 256u || word_blocks >= (1ull << 31) ||
             (a.connectivity != 4u && a.connectivity != 8u) || !a.mask || !a.parent || !a.sum_i || !a.sum_j ||
             !a.area || !a.min_x || !a.max_x || !a.max_y);
}

// Launches 1-3: afterwards every parent is a root and the root's slot holds
// the component's statistics.
hipError_t launch_mask_labelling(const ComponentsArgs& a, hipStream_t s) {
    if (!labelling_args_ok(a)) return hipErrorInvalidValue;
    const dim3 wg((uint32_t)((uint64_t)a.n_frames * a.bpf)), tb(256);
    hipLaunchKernelGGL(cc_rows_kernel, wg, tb, 0, s, a);
    hipLaunchKernelGGL(cc_merge_kernel, wg, tb, 0, s, a);
    hipLaunchKernelGGL(cc_stats_kernel, wg, tb, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mask_components(const ComponentsArgs& a, hipStream_t s) {
    const uint64_t pixel_blocks = ((uint64_t)a.n_frames * a.npx + 255u) / 256u;
    if (!labelling_args_ok(a) || pixel_blocks >= (1ull << 31) || !a.block_count || !a.counts ||
        (a.max_boxes != 0u && !a.boxes))
        return hipErrorInvalidValue;
    const hipError_t e = launch_mask_labelling(a, s);
    if (e != hipSuccess) return e;
    const dim3 wg((uint32_t)((uint64_t)a.n_frames * a.bpf)), tb(256);
    hipLaunchKernelGGL(cc_count_kernel, wg, tb, 0, s, a);
    hipLaunchKernelGGL(cc_offsets_kernel, dim3(a.n_frames), tb, 0, s, a);
    hipLaunchKernelGGL(cc_select_kernel, wg, tb, 0, s, a);
    if (a.labels) hipLaunchKernelGGL(cc_labels_kernel, dim3((uint32_t)pixel_blocks), tb, 0, s, a);
    return hipGetLastError();
}

}  // namespace dips
