// mask_stats.hip -- the statistics of a packed change mask: the set bits per
// frame and grid cell (dips_mask_counts), and per pixel the change times and
// the number of set frames (dips_mask_pixel_times).  Masks in
// dips_diff_change_mask's layout.  The reference has no counterpart; the input
// is bits, every sum is an integer, and the answers are exact whatever the
// schedule.
//
// Counts.  An item (series_sched.h mask_counts_geometry) is (frame, grid row,
// chunk of at most kCountsChunkCells grid columns, band of mask rows of that
// grid row).  A block of 256 threads is TH rows of TW word columns (TW the
// chunk's word count rounded up to a power of two, at most 64: a wave's load
// is up to 256 contiguous bytes).  A thread keeps its word column and walks
// the band's rows, so the cells its word meets and their column masks are
// computed once: a word that lies in one cell or straddles two is summed in
// two registers and added to the block's LDS counters once per thread; a word
// that holds more cells (cells narrower than 32 pixels, down to one) adds
// popcount(word & cell mask) per cell and row to LDS.  Then one store per
// cell (one band per grid row) or one integer atomic add per block and cell
// onto counts cleared on the stream before the launch.  The column masks
// cover region pixels only, so the pad bits never count.
//
// Times and sums.  A lane owns the kMaskTimesPx pixels of one slot -- a byte
// of the frame, or half of one -- and walks time, as mask_vote.hip does: the
// state {first, last, run_max, run_cur} (and the count) of its pixels stays in
// registers over the frames of the item and is stored once, by that lane, with
// plain stores.  A wave's load of one frame is 64 (or 32) contiguous bytes, so
// the loads of kGroup frames are issued before the first is used.  Pixels
// beyond the region's width are computed and never stored.  The kernel is
// bound by the fold's vector instructions, not by traffic, so the fold is
// mask arithmetic without compares or selects (at the lambda `fold`;
// DESIGN.md has the numbers).
// One part: the fold starts from the initial state, or when the call
// accumulates from what the outputs hold, and writes them.
// Several parts (series_sched.h mask_times_geometry: regions with too few
// tiles to fill the wave slots): a run may span a part boundary, so each part
// folds its frames from the initial state, keeps the length of its leading run
// and writes {first, last, run_max, leading, trailing} and its count to the
// handle's scratch; mask_times_combine_kernel folds the parts in order onto the
// initial or accumulated state with series_times.hip's rule:
//   first    = state.first == NONE ? part.first : state.first
//   last     = part.last == NONE ? state.last : part.last
//   run_max  = max(state.run_max, part.run_max, state.run_cur + part.leading)
//   run_cur  = part.leading == len ? state.run_cur + len : part.trailing
// No atomics; the scratch is the parts' summaries and does not grow with the
// frames of a part.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dips_kernels.h"

namespace dips {

namespace {

constexpr int kGroup = 8;                    // frames whose loads are in flight together
constexpr uint32_t kNone = 0xFFFFFFFFu;      // DIPS_TIME_NONE

// bits [lo, hi) of a word, 0 <= lo < hi <= 32
__device__ __forceinline__ uint32_t bit_range(uint32_t lo, uint32_t hi) {
    const uint32_t n = hi - lo;
    return (n >= 32u ? ~0u : (1u << n) - 1u) << lo;
}

// the grid column that holds region pixel x: the largest c with c * w / cols <= x
__device__ __forceinline__ uint32_t col_of(uint32_t x, uint32_t w, uint32_t cols) {
    return (uint32_t)((((uint64_t)x + 1u) * cols - 1u) / w);
}

}  // namespace

__global__ __launch_bounds__(256) void mask_counts_kernel(MaskCountsArgs a) {
    __shared__ uint32_t cell[kCountsChunkCells];
    const uint32_t tid = threadIdx.x;
    const size_t wpf = (size_t)a.wpr * a.h;
    for (uint64_t it = blockIdx.x; it < a.items; it += gridDim.x) {
        const uint32_t band = (uint32_t)(it % a.bands);
        uint64_t q = it / a.bands;
        const uint32_t chunk = (uint32_t)(q % a.col_chunks);
        q /= a.col_chunks;
        const uint32_t r = (uint32_t)(q % a.rows);
        const uint32_t t = (uint32_t)(q / a.rows);
        const uint32_t c0 = chunk * kCountsChunkCells;
        const uint32_t c1 = min(a.cols, c0 + kCountsChunkCells);
        const uint32_t nc = c1 - c0;
        for (uint32_t i = tid; i < nc; i += 256u) cell[i] = 0u;
        __syncthreads();

        const uint32_t y0 = grid_edge(0u, a.h, a.rows, r) + band * a.band_rows;
        const uint32_t y1 = min(grid_edge(0u, a.h, a.rows, r + 1u), y0 + a.band_rows);
        if (y0 < y1) {
            const uint32_t x0 = grid_edge(0u, a.w, a.cols, c0), x1 = grid_edge(0u, a.w, a.cols, c1);
            const uint32_t w0 = x0 >> 5, w1 = (x1 + 31u) >> 5;  // the chunk's words; x0 < x1
            uint32_t ltw = 0;
            while (ltw < 6u && (1u << ltw) < w1 - w0) ++ltw;
            const uint32_t tw = 1u << ltw, th = 256u >> ltw;
            const uint32_t tx = tid & (tw - 1u), ty = tid >> ltw;
            const uint32_t* frame = a.mask + (size_t)t * wpf;
            for (uint32_t wx = w0 + tx; wx < w1; wx += tw) {
                const uint32_t p0 = wx << 5;
                const uint32_t lo = max(p0, x0), hi = min(p0 + 32u, x1);  // the chunk's pixels of this word
                const uint32_t cf = col_of(lo, a.w, a.cols), cl = col_of(hi - 1u, a.w, a.cols);
                if (cl - cf <= 1u) {
                    const uint32_t m0 = bit_range(lo - p0, min(hi, grid_edge(0u, a.w, a.cols, cf + 1u)) - p0);
                    const uint32_t m1 = cl != cf ? bit_range(grid_edge(0u, a.w, a.cols, cl) - p0, hi - p0) : 0u;
                    uint32_t s0 = 0u, s1 = 0u;
#pragma unroll 4
                    for (uint32_t y = y0 + ty; y < y1; y += th) {
                        const uint32_t v = frame[(size_t)y * a.wpr + wx];
                        s0 += __popc(v & m0);
                        s1 += __popc(v & m1);
                    }
                    if (s0) atomicAdd(&cell[cf - c0], s0);
                    if (s1) atomicAdd(&cell[cl - c0], s1);
                } else {
                    for (uint32_t y = y0 + ty; y < y1; y += th) {
                        const uint32_t v = frame[(size_t)y * a.wpr + wx];
                        uint32_t e0 = lo;
                        for (uint32_t c = cf; c <= cl; ++c) {
                            const uint32_t e1 = min(hi, grid_edge(0u, a.w, a.cols, c + 1u));
                            const uint32_t k = __popc(v & bit_range(e0 - p0, e1 - p0));
                            if (k) atomicAdd(&cell[c - c0], k);
                            e0 = e1;
                        }
                    }
                }
            }
        }
        __syncthreads();
        uint32_t* out = a.counts + ((size_t)t * a.rows + r) * a.cols + c0;
        for (uint32_t i = tid; i < nc; i += 256u) {
            if (a.bands == 1u)
                out[i] = cell[i];
            else if (cell[i])
                atomicAdd(&out[i], cell[i]);
        }
        __syncthreads();
    }
}

template <int PX>
struct MaskTimesAcc {
    uint32_t nfirst[PX], last[PX], rmax[PX], rcur[PX], lead[PX], cnt[PX];
};

template <int PX, bool TIMES, bool SUMS, bool MP>
__global__ __launch_bounds__(256) void mask_times_kernel(MaskTimesArgs a) {
    static_assert(PX == 4 || PX == 8, "a slot is a byte or half of one");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    const uint64_t npx = (uint64_t)a.w * a.h;
    const uint64_t slots = (uint64_t)a.frame_bytes * (8 / PX);
    constexpr uint32_t kPlanes = (TIMES ? 5u : 0u) + (SUMS ? 1u : 0u);  // of a part's summary

    const uint64_t items = (uint64_t)a.n_parts * a.n_tiles;
    for (uint64_t it = wave; it < items; it += a.n_waves) {
        const uint32_t part = (uint32_t)(it / a.n_tiles);
        const uint32_t tile = (uint32_t)(it - (uint64_t)part * a.n_tiles);
        const uint64_t ts = (uint64_t)part * a.part_frames;  // 64 bits: t + kGroup may pass 2^32
        const uint64_t tend = min((uint64_t)a.n_frames, ts + a.part_frames);

        // once per item: the slot's byte in a frame, its shift in that byte,
        // its first pixel in a plane and how many of its pixels are stored
        const uint64_t slot = (uint64_t)tile * 64u + lane;
        const bool in = slot < slots;
        const uint32_t byte = in ? (uint32_t)(slot * PX >> 3) : 0u;
        const uint32_t sh = (uint32_t)(slot * PX) & 7u;
        const uint32_t row = byte / a.row_bytes;
        const uint32_t x = (byte - row * a.row_bytes) * 8u + sh;
        const uint32_t left = in && x < a.w ? min((uint32_t)PX, a.w - x) : 0u;
        const uint64_t pbase = (uint64_t)row * a.w + x;

        // nfirst is ~first: none is 0 and an earlier frame is larger, so the
        // fold is a max of masked values like the others
        MaskTimesAcc<PX> acc;
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            acc.nfirst[p] = ~kNone;
            acc.last[p] = kNone;
            acc.rmax[p] = acc.rcur[p] = acc.lead[p] = acc.cnt[p] = 0u;
        }
        if constexpr (!MP) {
            if (a.accumulate != 0u) {
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    if ((uint32_t)p >= left) continue;
                    if constexpr (TIMES) {
                        const uint32_t* o = a.times + pbase + p;
                        acc.nfirst[p] = ~o[0];
                        acc.last[p] = o[npx];
                        acc.rmax[p] = o[2u * npx];
                        acc.rcur[p] = o[3u * npx];
                    }
                    if constexpr (SUMS) acc.cnt[p] = a.sums[pbase + p];
                }
            }
        }

        // One frame: with m all ones where the pixel's bit is set, else 0
        // (one sign-extending bit-field extract), every update is mask
        // arithmetic, no compare and no select:
        //   nfirst = max(nfirst, ~g & m)     ~g >= 1, as g <= 0xFFFFFFFE
        //   last   = (g & m) | (last & ~m)   one bit-field insert
        //   rcur   = (rcur + 1) & m,  rmax = max(rmax, rcur),  cnt -= m
        auto fold = [&](uint32_t byte_of_frame, uint64_t t) {
            const uint32_t g = a.t0 + (uint32_t)t;        // the frame's global index
            const uint32_t kk = (uint32_t)(t - ts) + 1u;  // frames of the item so far
            const uint32_t bits = byte_of_frame >> sh;
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)bits, (uint32_t)p, 1u);
                // the compiler is not to know that m is 0 or all ones: it
                // would turn the arithmetic back into compares and selects
                asm("" : "+v"(m));
                if constexpr (TIMES) {
                    acc.nfirst[p] = max(acc.nfirst[p], ~g & m);
                    acc.last[p] = (g & m) | (acc.last[p] & ~m);
                    acc.rcur[p] = (acc.rcur[p] + 1u) & m;
                    acc.rmax[p] = max(acc.rmax[p], acc.rcur[p]);
                    if constexpr (MP) acc.lead[p] = acc.rcur[p] == kk ? kk : acc.lead[p];
                }
                if constexpr (SUMS) acc.cnt[p] -= m;
            }
        };
        // whole groups: kGroup loads in flight, then kGroup folds with no
        // branch between them; the last frames, fewer than kGroup, likewise
        // under a wave-uniform test each
        uint64_t t = ts;
        for (; t + kGroup <= tend; t += kGroup) {
            uint32_t v[kGroup];
#pragma unroll
            for (int j = 0; j < kGroup; ++j) v[j] = in ? a.mask[(size_t)(t + (uint32_t)j) * a.frame_bytes + byte] : 0u;
#pragma unroll
            for (int j = 0; j < kGroup; ++j) fold(v[j], t + (uint32_t)j);
        }
        if (t < tend) {
            uint32_t v[kGroup];
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                v[j] = 0u;
                if (in && t + (uint32_t)j < tend) v[j] = a.mask[(size_t)(t + (uint32_t)j) * a.frame_bytes + byte];
            }
#pragma unroll
            for (int j = 0; j < kGroup; ++j)
                if (t + (uint32_t)j < tend) fold(v[j], t + (uint32_t)j);
        }

#pragma unroll
        for (int p = 0; p < PX; ++p) {
            if ((uint32_t)p >= left) continue;
            if constexpr (MP) {
                uint32_t* o = a.parts + (uint64_t)part * kPlanes * npx + pbase + p;
                if constexpr (TIMES) {
                    o[0] = ~acc.nfirst[p];
                    o[npx] = acc.last[p];
                    o[2u * npx] = acc.rmax[p];
                    o[3u * npx] = acc.lead[p];
                    o[4u * npx] = acc.rcur[p];
                }
                if constexpr (SUMS) o[(kPlanes - 1u) * npx] = acc.cnt[p];
            } else {
                if constexpr (TIMES) {
                    uint32_t* o = a.times + pbase + p;
                    o[0] = ~acc.nfirst[p];
                    o[npx] = acc.last[p];
                    o[2u * npx] = acc.rmax[p];
                    o[3u * npx] = acc.rcur[p];
                }
                if constexpr (SUMS) a.sums[pbase + p] = acc.cnt[p];
            }
        }
    }
}

// The fold of the parts' summaries, one thread per pixel of the region, in a
// launch after mask_times_kernel<MP = true> on the same stream.
__global__ __launch_bounds__(256) void mask_times_combine_kernel(MaskTimesArgs a) {
    const uint64_t npx = (uint64_t)a.w * a.h;
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= npx) return;
    const uint32_t planes = (a.times ? 5u : 0u) + (a.sums ? 1u : 0u);
    uint32_t first = kNone, last = kNone, rmax = 0u, rcur = 0u, cnt = 0u;
    if (a.accumulate != 0u) {
        if (a.times) {
            first = a.times[q];
            last = a.times[npx + q];
            rmax = a.times[2u * npx + q];
            rcur = a.times[3u * npx + q];
        }
        if (a.sums) cnt = a.sums[q];
    }
    for (uint32_t part = 0; part < a.n_parts; ++part) {
        const uint32_t ts = part * a.part_frames;
        const uint32_t len = min(a.part_frames, a.n_frames - ts);
        const uint32_t* s = a.parts + (uint64_t)part * planes * npx + q;
        if (a.times) {
            const uint32_t pf = s[0], pl = s[npx], pm = s[2u * npx], lead = s[3u * npx], trail = s[4u * npx];
            first = first == kNone ? pf : first;
            last = pl == kNone ? last : pl;
            rmax = max(max(rmax, pm), rcur + lead);
            rcur = lead == len ? rcur + len : trail;
        }
        if (a.sums) cnt += s[(uint64_t)(planes - 1u) * npx];
    }
    if (a.times) {
        a.times[q] = first;
        a.times[npx + q] = last;
        a.times[2u * npx + q] = rmax;
        a.times[3u * npx + q] = rcur;
    }
    if (a.sums) a.sums[q] = cnt;
}

// ---------------------------------------------------------------------------
// Host-side launchers
// ---------------------------------------------------------------------------
const void* mask_counts_kernel_ptr() { return reinterpret_cast<const void*>(&mask_counts_kernel); }

hipError_t launch_mask_counts(const MaskCountsArgs& a, uint32_t blocks, hipStream_t s) {
    if (!a.mask || !a.counts || a.w == 0 || a.h == 0 || a.wpr != (a.w + 31u) / 32u || a.n_frames == 0 || a.rows == 0 ||
        a.cols == 0 || a.rows > a.h || a.cols > a.w || blocks == 0 || a.bands == 0 || a.band_rows == 0 ||
        a.col_chunks != (a.cols + kCountsChunkCells - 1u) / kCountsChunkCells ||
        (uint64_t)a.bands * a.band_rows < ((uint64_t)a.h + a.rows - 1u) / a.rows ||
        a.items != (uint64_t)a.n_frames * a.rows * a.col_chunks * a.bands)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_counts_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <bool MP>
static const void* mask_times_ptr(bool times, bool sums) {
    if (times && sums) return reinterpret_cast<const void*>(&mask_times_kernel<kMaskTimesPx, true, true, MP>);
    if (times) return reinterpret_cast<const void*>(&mask_times_kernel<kMaskTimesPx, true, false, MP>);
    if (sums) return reinterpret_cast<const void*>(&mask_times_kernel<kMaskTimesPx, false, true, MP>);
    return nullptr;
}

const void* mask_times_kernel_ptr(bool times, bool sums, bool parts) {
    return parts ? mask_times_ptr<true>(times, sums) : mask_times_ptr<false>(times, sums);
}

namespace {

bool mask_times_args_ok(const MaskTimesArgs& a) {
    return a.mask && (a.times || a.sums) && a.w != 0 && a.h != 0 && a.row_bytes == 4u * ((a.w + 31u) / 32u) &&
           (uint64_t)a.row_bytes * a.h == a.frame_bytes && a.n_frames != 0 && a.part_frames != 0 &&
           (uint64_t)a.n_parts == ((uint64_t)a.n_frames + a.part_frames - 1u) / a.part_frames &&
           (a.n_parts == 1u || a.parts) && (!a.times || (uint64_t)a.t0 + a.n_frames <= 0xFFFFFFFFull);
}

}  // namespace

hipError_t launch_mask_times(const MaskTimesArgs& a, uint32_t blocks, hipStream_t s) {
    const void* k = mask_times_kernel_ptr(a.times != nullptr, a.sums != nullptr, a.n_parts > 1u);
    if (!k || !mask_times_args_ok(a) || blocks == 0 || a.n_waves == 0 || (uint64_t)blocks * 4u < a.n_waves ||
        (uint64_t)a.n_tiles != ((uint64_t)a.frame_bytes * (8 / kMaskTimesPx) + 63u) / 64u)
        return hipErrorInvalidValue;
    MaskTimesArgs args = a;
    void* params[] = {&args};
    return hipLaunchKernel(k, dim3(blocks), dim3(256), params, 0, s);
}

hipError_t launch_mask_times_combine(const MaskTimesArgs& a, hipStream_t s) {
    const uint64_t blocks = ((uint64_t)a.w * a.h + 255u) / 256u;
    if (!mask_times_args_ok(a) || !a.parts || blocks == 0 || blocks >= (1ull << 23)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_times_combine_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dips
