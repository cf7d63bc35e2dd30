// mask_tracks.hip -- the components of a change mask linked across frames
// (dips_mask_tracks): per record of frame t the record of frame t - 1 it
// shares the most pixels with, that overlap, and the identity and age of its
// track.  The reference has no counterpart; the input is bits and the answer
// is combinatorial, so it is exact.
//
// The frames are labelled by launch_mask_components first.  After its
// cc_select_kernel every word-local run knows its root (parent[node]) and the
// root's area slot holds the label, record index + 1.  The links therefore
// read two mask words and two planes of the labelling scratch per pixel word
// and never a label image.  The planes carry one more frame in front (plane
// 0: the frame before the chunk), so a chunk's first frame links like any
// other.
//
// Four launches per chunk behind the clear of the overlap table, and a fifth
// (tr_keep_kernel) that moves the labelling of the chunk's last frame into
// plane 0 where another chunk follows:
//   1 tr_overlap_kernel  one thread per mask word of every frame.  A maximal
//                        fragment of set bits of cur & prev lies inside one
//                        run of each frame, so it has one (a, b) pair and a
//                        length.  The lanes of a wave with the same pair sum
//                        their lengths by shuffles before one lane adds the
//                        sum to ov[f][a][b]: two all-ones frames cost one
//                        atomic per wave.  The sums are integer, so the order
//                        of the atomics does not show.
//   2 tr_link_kernel     one block per frame, thread k = record k: the row
//                        argmax (PREV, OVERLAP), the column argmax (NEXT), the
//                        mutual test, the rank of a head among its frame's
//                        heads (a block scan) and the frame's head count.
//   3 tr_scan_kernel     one block: the exclusive scan of the head counts on
//                        top of the carried next id, which it advances.
//   4 tr_ids_kernel      one thread per record: walk back along the
//                        continuations to the head of the chain, or to the
//                        frame before the chunk, whose TRACK and AGE are
//                        carried.  The id is the head's frame base plus its
//                        rank: position, never an atomic, decides it.
//
// Termination: no loop waits for another thread and there is no grid barrier,
// spin flag or cooperative launch.  Bounds: the fragment loop clears at least
// one bit of a 32-bit word per step (<= 16 fragments); the wave-sum loop
// retires at least its leader per step (<= 64 steps, 6 shuffle steps each);
// the argmax loops run K <= 256 steps; the block scans 8 steps; the scan of
// the head counts ceil(n_frames / 256) rounds; the walk back goes one frame
// towards the chunk's start per step (<= n_frames steps, and the host keeps a
// chunk at 256 frames or fewer); tr_keep_kernel's run
// loop clears at least one bit of a word per step.
#include <hip/hip_runtime.h>

#include "dips_kernels.h"
#include "mask_runs.h"  // next_run, local_start

namespace dips {

namespace {

// Word wi of the frame at `m` with the pad bits of a row's last word cleared.
__device__ __forceinline__ uint32_t frame_word(const TracksArgs& a, const uint32_t* m, uint32_t wi, uint32_t k) {
    uint32_t v = m[wi];
    if (k == a.wpr - 1u && (a.w & 31u) != 0u) v &= (1u << (a.w & 31u)) - 1u;
    return v;
}

// The label (record index + 1, 0: dropped) of the run of `word` (word k of
// row j) that holds bit b, in plane `pl`.
__device__ __forceinline__ uint32_t run_label(const TracksArgs& a, uint32_t pl, uint32_t j, uint32_t k, uint32_t word,
                                              uint32_t b) {
    const uint32_t node = j * a.w + k * 32u + local_start(word, b);
    const uint32_t root = a.parent[(size_t)pl * a.npx + node];  // a root since cc_stats_kernel
    const uint32_t rj = root / a.w, ri = root - rj * a.w;
    return a.label[(size_t)pl * a.nslots + (size_t)rj * a.hw + (ri >> 1)];
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

}  // namespace

__global__ __launch_bounds__(256) void tr_overlap_kernel(TracksArgs a) {
    // no early return: every lane takes part in the wave sums
    const uint32_t f = blockIdx.x / a.bpf;
    const uint32_t wi = (blockIdx.x - f * a.bpf) * 256u + threadIdx.x;
    const uint32_t* cur_m = a.mask + (size_t)f * a.wpf;
    const uint32_t* prev_m = f ? cur_m - a.wpf : a.prev0;  // one per block
    uint32_t cur = 0u, prev = 0u, j = 0u, k = 0u;
    if (wi < a.wpf && prev_m) {
        j = wi / a.wpr;
        k = wi - j * a.wpr;
        cur = frame_word(a, cur_m, wi, k);
        prev = frame_word(a, prev_m, wi, k);
    }
    uint32_t rem = cur & prev;
    uint32_t* ov = a.ov + (size_t)f * a.K * a.K;
    const uint32_t lane = threadIdx.x & 63u;
    while (__ballot(rem != 0u)) {
        bool has = rem != 0u;
        uint32_t key = 0u, len = 0u;
        if (has) {
            uint32_t s, e;
            next_run(rem, s, e);
            len = e - s;
            const uint32_t la = run_label(a, f + 1u, j, k, cur, s);
            const uint32_t lb = run_label(a, f, j, k, prev, s);
            // dropped by min_area, or beyond the K records: takes no part
            has = la != 0u && la <= a.K && lb != 0u && lb <= a.K;
            key = has ? (la - 1u) * a.K + (lb - 1u) : 0u;
        }
        unsigned long long pending = __ballot(has);
        while (pending) {  // loses at least the leader's bit per step
            const int leader = __ffsll(pending) - 1;
            const uint32_t lkey = (uint32_t)__shfl((int)key, leader);
            const bool m = has && key == lkey;  // the wave's frame is one (bpf blocks per frame)
            uint32_t n = m ? len : 0u;
            for (int d = 32; d > 0; d >>= 1) n += (uint32_t)__shfl_xor((int)n, d);
            if ((int)lane == leader) atomicAdd(ov + lkey, n);
            has = has && !m;
            pending = __ballot(has);
        }
    }
}

__global__ __launch_bounds__(256) void tr_link_kernel(TracksArgs a) {
    __shared__ uint32_t s_next[256];
    __shared__ uint32_t s_scan[256];
    const uint32_t f = blockIdx.x, k = threadIdx.x, K = a.K;
    const uint32_t m = min(a.counts[f], K);
    const bool has_prev = f != 0u || a.prev0 != nullptr;
    const uint32_t* ov = a.ov + (size_t)f * K * K;
    // strict > keeps the smallest index on a tie
    uint32_t best = 0u, arg = DIPS_LINK_NONE;
    if (has_prev && k < m)
        for (uint32_t b = 0u; b < K; ++b) {
            const uint32_t v = ov[k * K + b];
            if (v > best) {
                best = v;
                arg = b;
            }
        }
    uint32_t nbest = 0u, narg = DIPS_LINK_NONE;
    if (has_prev && k < K)
        for (uint32_t r = 0u; r < m; ++r) {
            const uint32_t v = ov[r * K + k];
            if (v > nbest) {
                nbest = v;
                narg = r;
            }
        }
    s_next[k] = narg;
    __syncthreads();
    const bool cont = arg != DIPS_LINK_NONE && s_next[arg] == k;
    const bool head = k < m && !cont;
    uint32_t total;
    const uint32_t rank = block_exclusive_scan(head ? 1u : 0u, s_scan, &total);
    if (k < K) {
        a.cprev[(size_t)f * K + k] = cont ? arg : DIPS_LINK_NONE;
        a.hrank[(size_t)f * K + k] = rank;
        uint32_t* r = a.links + ((size_t)f * K + k) * DIPS_LINK_WORDS;
        r[DIPS_LINK_PREV] = arg;  // NONE beyond the records: arg was never set
        r[DIPS_LINK_OVERLAP] = best;
        if (k >= m) {
            r[DIPS_LINK_TRACK] = DIPS_LINK_NONE;
            r[DIPS_LINK_AGE] = 0u;
        }
    }
    if (k == 0u) a.heads[f] = total;
}

// One block: heads becomes base, the id of every frame's first head.
__global__ __launch_bounds__(256) void tr_scan_kernel(TracksArgs a) {
    __shared__ uint32_t sh[256];
    uint32_t carry = *a.next_id;  // every thread reads it before the scans' barriers, thread 0 writes it after them
    for (uint32_t b0 = 0u; b0 < a.n_frames; b0 += 256u) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < a.n_frames ? a.heads[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, sh, &total);
        if (i < a.n_frames) a.base[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0u) *a.next_id = carry;
}

__global__ __launch_bounds__(256) void tr_ids_kernel(TracksArgs a) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, K = a.K;
    if (t >= a.n_frames * K) return;
    const uint32_t f = t / K, k = t - f * K;
    uint32_t track = DIPS_LINK_NONE, age = 0u;
    if (k < min(a.counts[f], K)) {
        uint32_t ff = f, kk = k;
        for (uint32_t step = 0u; step <= a.n_frames; ++step) {  // ff falls by one per step: ends at step f at the latest
            const uint32_t b = a.cprev[(size_t)ff * K + kk];
            if (b == DIPS_LINK_NONE) {
                track = a.base[ff] + a.hrank[(size_t)ff * K + kk];
                break;
            }
            age += 1u;
            if (ff == 0u) {  // continues a record of the frame before the chunk
                track = a.carry_in[b];
                age += a.carry_in[K + b];
                break;
            }
            ff -= 1u;
            kk = b;
        }
        uint32_t* r = a.links + (size_t)t * DIPS_LINK_WORDS;
        r[DIPS_LINK_TRACK] = track;
        r[DIPS_LINK_AGE] = age;
    }
    if (f == a.n_frames - 1u) {
        a.carry_out[k] = track;
        a.carry_out[K + k] = age;
    }
}

// One thread per mask word of `frame`: the parent of every run and, where the
// run is a root, its label go from plane `plane` to plane 0.  Nothing else of
// plane 0 is ever read: tr_overlap_kernel looks up runs of this frame only.
__global__ __launch_bounds__(256) void tr_keep_kernel(TracksArgs a, const uint32_t* frame, uint32_t plane) {
    const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
    if (wi >= a.wpf) return;
    const uint32_t j = wi / a.wpr, k = wi - j * a.wpr;
    uint32_t rem = frame_word(a, frame, wi, k);
    while (rem) {  // clears at least one bit per step
        uint32_t s, e;
        next_run(rem, s, e);
        const uint32_t i = k * 32u + s, node = j * a.w + i;
        const uint32_t root = a.parent[(size_t)plane * a.npx + node];
        a.parent[node] = root;
        if (root == node) {
            const size_t sl = (size_t)j * a.hw + (i >> 1);
            a.label[sl] = a.label[(size_t)plane * a.nslots + sl];
        }
    }
}

hipError_t launch_mask_tracks_keep(const TracksArgs& a, const uint32_t* frame, uint32_t plane, hipStream_t s) {
    if (!frame || plane == 0u || !a.parent || !a.label || a.wpf == 0u || a.bpf != (a.wpf + 255u) / 256u ||
        a.npx != a.w * a.h || a.wpr != (a.w + 31u) / 32u || a.hw != (a.w + 1u) / 2u || a.nslots != a.hw * a.h ||
        a.wpf != a.wpr * a.h)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(tr_keep_kernel, dim3(a.bpf), dim3(256), 0, s, a, frame, plane);
    return hipGetLastError();
}

hipError_t launch_mask_tracks(const TracksArgs& a, hipStream_t s) {
    const uint64_t word_blocks = (uint64_t)a.n_frames * a.bpf;
    const uint64_t records = (uint64_t)a.n_frames * a.K;
    if (a.n_frames == 0 || a.w == 0 || a.h == 0 || a.npx != a.w * a.h || a.npx >= (1u << 30) ||
        a.wpr != (a.w + 31u) / 32u || a.hw != (a.w + 1u) / 2u || a.nslots != a.hw * a.h || a.wpf != a.wpr * a.h ||
        a.bpf != (a.wpf + 255u) / 256u || word_blocks >= (1ull << 31) || a.K == 0u || a.K > DIPS_TRACK_MAX_BOXES ||
        records >= (1ull << 30) || !a.mask || !a.parent || !a.label || !a.counts || !a.ov || !a.cprev || !a.hrank ||
        !a.heads || !a.base || !a.next_id || !a.carry_in || !a.carry_out || a.carry_in == a.carry_out || !a.links)
        return hipErrorInvalidValue;
    const dim3 tb(256);
    hipError_t e = hipMemsetAsync(a.ov, 0, sizeof(uint32_t) * (size_t)records * a.K, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tr_overlap_kernel, dim3((uint32_t)word_blocks), tb, 0, s, a);
    hipLaunchKernelGGL(tr_link_kernel, dim3(a.n_frames), tb, 0, s, a);
    hipLaunchKernelGGL(tr_scan_kernel, dim3(1), tb, 0, s, a);
    hipLaunchKernelGGL(tr_ids_kernel, dim3((uint32_t)((records + 255u) / 256u)), tb, 0, s, a);
    return hipGetLastError();
}

}  // namespace dips
