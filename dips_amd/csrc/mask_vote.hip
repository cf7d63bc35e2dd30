// mask_vote.hip -- the temporal m-of-k vote on the change mask
// (dips_mask_vote): output bit (t, j, i) is set when at least m of the k
// input frames t - k + 1 .. t have bit (j, i) set; the frames before the clip
// come from a history of k - 1 frames or are clear.  Masks in
// dips_diff_change_mask's layout.  The reference has no counterpart; the input
// is bits and the answer is exact.
//
// Ownership.  A lane owns kVoteWords words of the frame (one, as built; word
// 64 u + lane of its tile in general: a wave's loads and stores are 256
// contiguous bytes each) and walks time.  The count of the window of each of a word's 32 pixels lives in five
// bit planes c[0..4] (plane i holds bit i of all 32 counts): k <= 31 fits.
// Per frame, with nw the word that enters the window and od the one that
// leaves it:
//   a ripple increment by nw & ~od and a ripple decrement by od & ~nw in one
//   pass over the planes (the two sets are disjoint, so are their carries and
//   borrows: c[i] ^= carry | borrow);
//   the bit-sliced compare count >= m against the wave-uniform m, from the low
//   plane up: ge = m_i ? c[i] & ge : c[i] | ge, starting from all ones;
//   one store.
// No atomics, no LDS, no scratch; every output word is written once by one
// lane, whatever the part count.
//
// The leaving word is read again from memory, k frames after it entered
// (DESIGN.md has the reasons and the numbers): the window of a frame part is
// at most 31 frames of mask, 31 MB at 4K, far inside the 256 MiB last-level
// cache, the second read travels in the same batch of loads as the first, and
// the kernel keeps no state that grows with k, so its occupancy is the same
// for every window.
//
// Schedule (series_sched.h vote_geometry).  Time is cut into parts; an item
// is (part, tile) and the items are dealt to the resident waves part-major, as
// in series_mask.hip.  A part that starts at frame s primes its counters from
// X_{s-k+1} .. X_{s-1} (increments only); the first frame of a part has no
// leaving word.  Frames with a negative index come from the history, or are
// clear.  Loads are issued kGroup frames at a time (2 * kGroup * kVoteWords
// in flight per lane) before the first is used.
//
// Pad bits: every loaded word is masked to the region, so the counts of the
// pad bits stay 0 and, m being at least 1, their output bits are 0.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dips_kernels.h"

namespace dips {

namespace {

constexpr int kGroup = 8;               // frames whose loads are in flight together
constexpr uint32_t kHistBlocks = 2048;  // the history launch's grid; the words beyond are looped over

// The bits of word idx of a frame that lie in the region.
__device__ __forceinline__ uint32_t vote_region_bits(const VoteArgs& a, size_t idx) {
    const uint32_t col = (uint32_t)(idx % a.wpr);
    return (col == a.wpr - 1u && (a.w & 31u) != 0u) ? (1u << (a.w & 31u)) - 1u : ~0u;
}

// Frame t of the sequence history ++ input, t >= -(k - 1); NULL: a clear frame
__device__ __forceinline__ const uint32_t* vote_frame(const VoteArgs& a, int64_t t) {
    if (t >= 0) return a.in + (size_t)t * a.wpf;
    return a.hist_in ? a.hist_in + (size_t)(t + (int64_t)a.window - 1) * a.wpf : nullptr;
}

}  // namespace

template <int W>
__global__ __launch_bounds__(256, 8) void mask_vote_kernel(VoteArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    const int64_t k = a.window;
    // plane i of the compare: all ones where bit i of m is clear
    uint32_t nm[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) nm[i] = ((a.votes >> i) & 1u) ? 0u : ~0u;

    const uint64_t items = (uint64_t)a.parts * a.n_tiles;
    for (uint64_t it = wave; it < items; it += a.n_waves) {
        const uint32_t part = (uint32_t)(it / a.n_tiles);
        const uint32_t tile = (uint32_t)(it - (uint64_t)part * a.n_tiles);
        const int64_t t0 = (int64_t)part * a.part_frames;
        const int64_t tend = min((int64_t)a.n_frames, t0 + (int64_t)a.part_frames);

        // per lane-slot, once per item: the word's index in a frame (inside
        // the frame or not loaded and not stored) and its region bits
        size_t idx[W];
        uint32_t pm[W];
        bool in[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
            idx[u] = (size_t)tile * (64u * W) + (size_t)(u * 64) + lane;
            in[u] = idx[u] < a.wpf;
            pm[u] = in[u] ? vote_region_bits(a, idx[u]) : 0u;
        }
        auto fetch = [&](const uint32_t* p, uint32_t (&v)[W]) {
#pragma unroll
            for (int u = 0; u < W; ++u) {
                v[u] = 0u;
                if (p && in[u]) v[u] = p[idx[u]] & pm[u];
            }
        };

        uint32_t c[W][5];
#pragma unroll
        for (int u = 0; u < W; ++u)
#pragma unroll
            for (int i = 0; i < 5; ++i) c[u][i] = 0u;

        // priming: the k - 1 frames before the part, increments only
        for (int64_t t = t0 - k + 1; t < t0; t += kGroup) {
            uint32_t nw[kGroup][W];
#pragma unroll
            for (int j = 0; j < kGroup; ++j) fetch(t + j < t0 ? vote_frame(a, t + j) : nullptr, nw[j]);
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
#pragma unroll
                for (int u = 0; u < W; ++u) {
                    uint32_t carry = nw[j][u];
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        const uint32_t tc = c[u][i] & carry;
                        c[u][i] ^= carry;
                        carry = tc;
                    }
                }
            }
        }

        for (int64_t t = t0; t < tend; t += kGroup) {
            uint32_t nw[kGroup][W], od[kGroup][W];
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                const bool live = t + j < tend;
                fetch(live ? vote_frame(a, t + j) : nullptr, nw[j]);
                // the part's first frame has no leaving word
                fetch(live && t + j > t0 ? vote_frame(a, t + j - k) : nullptr, od[j]);
            }
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                if (t + j < tend) {
                    uint32_t* o = a.out + (size_t)(t + j) * a.wpf;
#pragma unroll
                    for (int u = 0; u < W; ++u) {
                        uint32_t carry = nw[j][u] & ~od[j][u], borrow = od[j][u] & ~nw[j][u];
                        uint32_t ge = ~0u;
#pragma unroll
                        for (int i = 0; i < 5; ++i) {
                            const uint32_t tc = c[u][i] & carry, tb = ~c[u][i] & borrow;
                            c[u][i] ^= carry | borrow;
                            carry = tc;
                            borrow = tb;
                            ge = (c[u][i] & ge) | ((c[u][i] | ge) & nm[i]);
                        }
                        if (in[u]) o[idx[u]] = ge & pm[u];
                    }
                }
            }
        }
    }
}

// The next history: frame q of hist_out is frame n_frames - (k - 1) + q of the
// sequence history ++ input, pad bits 0.
__global__ __launch_bounds__(256) void mask_vote_history_kernel(VoteArgs a) {
    const uint64_t total = (uint64_t)(a.window - 1u) * a.wpf;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        const uint64_t q = i / a.wpf;
        const size_t idx = (size_t)(i - q * a.wpf);
        const uint32_t* p = vote_frame(a, (int64_t)a.n_frames - (int64_t)(a.window - 1u) + (int64_t)q);
        a.hist_out[i] = p ? p[idx] & vote_region_bits(a, idx) : 0u;
    }
}

namespace {

bool vote_args_ok(const VoteArgs& a) {
    return a.w != 0 && a.wpr == (a.w + 31u) / 32u && a.wpf != 0 && a.wpf % a.wpr == 0 && a.wpf < (1u << 30) &&
           a.window >= 1u && a.window <= DIPS_VOTE_MAX_WINDOW && a.votes >= 1u && a.votes <= a.window &&
           (a.in || a.n_frames == 0);
}

}  // namespace

const void* mask_vote_kernel_ptr() { return reinterpret_cast<const void*>(&mask_vote_kernel<kVoteWords>); }

hipError_t launch_mask_vote(const VoteArgs& a, uint32_t blocks, hipStream_t s) {
    if (!vote_args_ok(a) || !a.out || a.n_frames == 0 || blocks == 0 || a.part_frames == 0 ||
        (uint64_t)a.parts != ((uint64_t)a.n_frames + a.part_frames - 1u) / a.part_frames ||
        a.n_tiles != (a.wpf + 64u * kVoteWords - 1u) / (64u * kVoteWords) || a.n_waves == 0 ||
        (uint64_t)blocks * 4u < a.n_waves)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_vote_kernel<kVoteWords>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_mask_vote_history(const VoteArgs& a, hipStream_t s) {
    if (!vote_args_ok(a) || !a.hist_out || a.window < 2u) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)(a.window - 1u) * a.wpf;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255u) / 256u, kHistBlocks);
    hipLaunchKernelGGL(mask_vote_history_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dips
