// mask_morph.hip -- binary morphology of the change mask (dips_mask_morph):
// erode, dilate, open, close of every frame of a bit mask in
// dips_diff_change_mask's layout by a box or a diamond of radius <= 15.  The
// reference has no counterpart; the input is bits and the answer is exact.
//
// One launch per call.  A workgroup of 256 threads takes one tile of kTH rows
// x kTW words (32 x 1024 pixels) of one frame at a time (a grid-stride loop
// over the flattened 64-bit tile index: frames never sit in a grid
// dimension), holds it in LDS with its halo and runs every pass there; open
// and close compose their two operations on chip.  The input is read once
// apart from the halo, every output word is stored once by one thread, there
// are no atomics and no scratch.
//
// Everything is a dilation with 0 outside the region D: erode(X) =
// D \ dilate(D \ X), so an erosion loads the complement (and D's own
// complement -- rows and words outside the frame, the pad bits of a row's
// last word -- stays 0: the structuring element is clipped to D), dilates,
// and complements again on the way out.  open = erode, dilate and close =
// dilate, erode therefore complement exactly once between their two
// dilations, masked to D again, which is where the intermediate's outside
// value differs from the input's.  Edges are data: no pass tests for a frame
// or row end, it reads zeros.
//
// The tile in LDS: rows j0 - H .. j0 + th + H with H = ry (one operation) or
// 2 ry (open / close), at most 32 + 60; columns 1 .. kTW + 2 hold words k0 - 1
// .. k0 + kTW, columns 0 and kTW + 3 are zero guards so that the horizontal
// pass of a halo word reads a left and a right neighbour like any other.  A
// halo word is then wrong in the bits nearer than the radius to its guard,
// and right in the rest: two passes reach 2 * 15 = 30 < 32 bits sideways, so
// a tile word never depends on more than its two neighbour words, and what it
// takes from a halo word of the intermediate (the <= 15 bits next to the
// tile) depends on that halo word's bits at least 32 - 30 = 2 away from the
// guard.  That is the reason for DIPS_MORPH_MAX_RADIUS.
//
// Passes, each from one LDS buffer to the other with a __syncthreads() after
// it, the last one of the call to global memory:
//   box      horizontal: the 32 + 2 rx bits around a word as one 64-bit
//            window (funnel of left, centre, right), OR of its 2 rx + 1
//            shifts by doubling (1, 2, 4, 8, then the remainder);
//            vertical: OR of the 2 ry + 1 rows around.
//   diamond  r rounds of the 5-point cross (centre, the two one-bit funnel
//            shifts, the rows above and below); r applications of the
//            radius-1 diamond are the radius-r diamond, also at the border,
//            because D is a rectangle.  Radius 0 runs as the 0 x 0 box.
// Each pass shrinks the valid rows by its vertical reach; the last one is
// left with exactly the tile's rows.
//
// Bank conflicts: every pass walks the tile row-major, a lane per word, so
// the 32 lanes of an LDS lane group read consecutive words of one row (or of
// two rows end to end): distinct banks whatever the pitch.  The pitch of 36
// words is kTW plus the halo and guard words, not padding.
#include <hip/hip_runtime.h>

#include "dips_kernels.h"

namespace dips {

namespace {

constexpr uint32_t kTH = 32;                                  // tile rows
constexpr uint32_t kTW = 32;                                  // tile words
constexpr uint32_t kMaxHalo = 2u * DIPS_MORPH_MAX_RADIUS;     // rows above and below, open / close
constexpr uint32_t kRows = kTH + 2u * kMaxHalo;               // 92
constexpr uint32_t kPitch = kTW + 4u;                         // halo word and guard word per side
constexpr uint32_t kThreads = 256;
constexpr uint32_t kLoads = 8;                                // global loads in flight per thread
constexpr uint32_t kMaxBlocks = 4096;                         // the grid; the tiles beyond are looped over

// The bits of word gk of row gj that lie in the region: 0 outside it.
__device__ __forceinline__ uint32_t region_bits(const MorphArgs& a, int32_t gj, int32_t gk) {
    if ((uint32_t)gj >= a.h || (uint32_t)gk >= a.wpr) return 0u;  // negative: far above either
    return ((uint32_t)gk == a.wpr - 1u && (a.w & 31u) != 0u) ? (1u << (a.w & 31u)) - 1u : ~0u;
}

// Bit b of the result = OR of bits b - rad .. b + rad of the row, of which
// l, c, r are three consecutive words.
__device__ __forceinline__ uint32_t dilate_row(uint32_t l, uint32_t c, uint32_t r, uint32_t rad) {
    // bit i of the window = bit i - rad of c's word; above bit 31 + 2 rad it is never used
    uint64_t win = ((((uint64_t)c << 32) | l) >> (32u - rad)) | ((uint64_t)r << (32u + rad));
    const uint32_t n = 2u * rad + 1u;
    uint32_t span = 1u;  // bit i of win covers bits i .. i + span - 1 of the window
    while (2u * span <= n) {
        win |= win >> span;
        span *= 2u;
    }
    win |= win >> (n - span);
    return (uint32_t)win;
}

// The tile a workgroup is working on.
struct Tile {
    size_t frame_word;  // first word of the frame
    int32_t j0, k0;     // first row and word of the tile
    uint32_t th;        // its rows
    uint32_t halo;      // rows loaded above and below
};

// What a pass does with the result `res` of local row lr, column col.
// Intermediate: the complement inside the region, 0 outside, to LDS.  Last:
// the tile's own words to global memory, complemented for an erosion, pad
// bits 0.
template <bool LAST>
__device__ __forceinline__ void emit(const MorphArgs& a, const Tile& t, uint32_t* dst, uint32_t lr, uint32_t col,
                                     uint32_t res, bool inv_last) {
    const int32_t gj = t.j0 - (int32_t)t.halo + (int32_t)lr, gk = t.k0 - 2 + (int32_t)col;
    const uint32_t m = region_bits(a, gj, gk);
    if (LAST) {
        if (m) a.out[t.frame_word + (size_t)gj * a.wpr + (size_t)gk] = (inv_last ? ~res : res) & m;
    } else {
        dst[lr * kPitch + col] = ~res & m;
    }
}

// Rows [lo, hi), columns 1 .. kTW + 2: the horizontal dilation by rad.
__device__ __forceinline__ void pass_rows(const uint32_t* src, uint32_t* dst, uint32_t lo, uint32_t hi, uint32_t rad) {
    constexpr uint32_t kCols = kTW + 2u;
    for (uint32_t i = threadIdx.x; i < (hi - lo) * kCols; i += kThreads) {
        const uint32_t rr = i / kCols, p = (lo + rr) * kPitch + 1u + (i - rr * kCols);
        dst[p] = dilate_row(src[p - 1u], src[p], src[p + 1u], rad);
    }
}

// Rows [lo, hi): the vertical dilation by rad (the rows lo - rad .. hi + rad
// - 1 of src are valid).
template <bool LAST>
__device__ __forceinline__ void pass_cols(const MorphArgs& a, const Tile& t, const uint32_t* src, uint32_t* dst,
                                          uint32_t lo, uint32_t hi, uint32_t rad, bool inv_last) {
    constexpr uint32_t kCols = LAST ? kTW : kTW + 2u, kFirst = LAST ? 2u : 1u;
    for (uint32_t i = threadIdx.x; i < (hi - lo) * kCols; i += kThreads) {
        const uint32_t rr = i / kCols, lr = lo + rr, col = kFirst + (i - rr * kCols);
        const uint32_t* s = src + (lr - rad) * kPitch + col;
        uint32_t acc = 0u;
        for (uint32_t e = 0u; e <= 2u * rad; ++e) acc |= s[e * kPitch];
        emit<LAST>(a, t, dst, lr, col, acc, inv_last);
    }
}

// Rows [lo, hi): one round of the 5-point cross.  PLAIN: to LDS as it is
// (between the rounds of one operation).
template <bool LAST, bool PLAIN>
__device__ __forceinline__ void pass_cross(const MorphArgs& a, const Tile& t, const uint32_t* src, uint32_t* dst,
                                           uint32_t lo, uint32_t hi, bool inv_last) {
    constexpr uint32_t kCols = LAST ? kTW : kTW + 2u, kFirst = LAST ? 2u : 1u;
    for (uint32_t i = threadIdx.x; i < (hi - lo) * kCols; i += kThreads) {
        const uint32_t rr = i / kCols, lr = lo + rr, col = kFirst + (i - rr * kCols), p = lr * kPitch + col;
        const uint32_t c = src[p], l = src[p - 1u], r = src[p + 1u];
        const uint32_t res = c | (c << 1) | (l >> 31) | (c >> 1) | (r << 31) | src[p - kPitch] | src[p + kPitch];
        if (PLAIN)
            dst[p] = res;
        else
            emit<LAST>(a, t, dst, lr, col, res, inv_last);
    }
}

}  // namespace

__global__ __launch_bounds__(kThreads) void mask_morph_kernel(MorphArgs a) {
    __shared__ uint32_t lds[2][kRows * kPitch];
    const bool two = a.op >= DIPS_MORPH_OPEN;
    const bool box = a.shape == DIPS_MORPH_BOX || a.rx == 0u;  // the diamond of radius 0 is the 0 x 0 box
    // the first operation is an erosion: the complement is loaded
    const bool inv_first = a.op == DIPS_MORPH_ERODE || a.op == DIPS_MORPH_OPEN;
    const bool inv_last = two ? !inv_first : inv_first;
    const uint32_t n_ops = two ? 2u : 1u;
    const uint64_t tiles_per_frame = (uint64_t)a.tiles_x * a.tiles_y;

    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const uint64_t f = item / tiles_per_frame;
        const uint32_t rem = (uint32_t)(item - f * tiles_per_frame);
        const uint32_t ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
        Tile t;
        t.frame_word = (size_t)f * a.h * a.wpr;
        t.j0 = (int32_t)(ty * kTH);
        t.k0 = (int32_t)(tx * kTW);
        t.th = min(kTH, a.h - ty * kTH);
        t.halo = a.ry * n_ops;
        const uint32_t rows = t.th + 2u * t.halo;  // <= kRows
        uint32_t* cur = lds[0];
        uint32_t* nxt = lds[1];

        // the tile and its halo: the region's bits (complemented for an
        // erosion), 0 for everything outside it and for the guards
        // (kLoads words per thread and round, all loads issued before the
        // first is used: the tile is a few loads per thread, and one at a
        // time they are its latency several times over)
        for (uint32_t base = threadIdx.x; base < rows * kPitch; base += kThreads * kLoads) {
            uint32_t v[kLoads], m[kLoads];
#pragma unroll
            for (uint32_t u = 0u; u < kLoads; ++u) {
                const uint32_t i = base + u * kThreads, lr = i / kPitch, col = i - lr * kPitch;
                const int32_t gj = t.j0 - (int32_t)t.halo + (int32_t)lr, gk = t.k0 - 2 + (int32_t)col;
                const bool guard = col == 0u || col == kPitch - 1u;
                m[u] = guard || i >= rows * kPitch ? 0u : region_bits(a, gj, gk);
                v[u] = 0u;
                if (m[u]) v[u] = a.in[t.frame_word + (size_t)gj * a.wpr + (size_t)gk];
            }
#pragma unroll
            for (uint32_t u = 0u; u < kLoads; ++u) {
                const uint32_t i = base + u * kThreads;
                if (i < rows * kPitch) {
                    cur[i] = (inv_first ? ~v[u] : v[u]) & m[u];
                    const uint32_t col = i % kPitch;
                    if (col == 0u || col == kPitch - 1u) nxt[i] = 0u;
                }
            }
        }
        __syncthreads();

        uint32_t lo = 0u, hi = rows;  // the valid rows of cur
        for (uint32_t k = 0u; k < n_ops; ++k) {
            const bool last = k + 1u == n_ops;
            if (box) {
                pass_rows(cur, nxt, lo, hi, a.rx);
                __syncthreads();
                lo += a.ry;
                hi -= a.ry;
                if (last)
                    pass_cols<true>(a, t, nxt, nullptr, lo, hi, a.ry, inv_last);
                else
                    pass_cols<false>(a, t, nxt, cur, lo, hi, a.ry, inv_last);
                __syncthreads();  // cur holds the next operation's input (or is free for the next tile)
            } else {
                for (uint32_t round = 0u; round < a.rx; ++round) {
                    lo += 1u;
                    hi -= 1u;
                    if (round + 1u < a.rx)
                        pass_cross<false, true>(a, t, cur, nxt, lo, hi, inv_last);
                    else if (last)
                        pass_cross<true, false>(a, t, cur, nullptr, lo, hi, inv_last);
                    else
                        pass_cross<false, false>(a, t, cur, nxt, lo, hi, inv_last);
                    __syncthreads();
                    uint32_t* s = cur;
                    cur = nxt;
                    nxt = s;
                }
            }
        }
    }
}

hipError_t launch_mask_morph(const MorphArgs& a, hipStream_t s) {
    if (!a.in || !a.out || a.n_frames == 0 || a.w == 0 || a.h == 0 || (uint64_t)a.w * a.h >= (1ull << 30) ||
        a.wpr != (a.w + 31u) / 32u || a.op > DIPS_MORPH_CLOSE || a.shape > DIPS_MORPH_DIAMOND ||
        a.rx > DIPS_MORPH_MAX_RADIUS || a.ry > DIPS_MORPH_MAX_RADIUS ||
        (a.shape == DIPS_MORPH_DIAMOND && a.rx != a.ry) || a.tiles_x != (a.wpr + kTW - 1u) / kTW ||
        a.tiles_y != (a.h + kTH - 1u) / kTH || a.items != (uint64_t)a.n_frames * a.tiles_x * a.tiles_y)
        return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)(a.items < kMaxBlocks ? a.items : kMaxBlocks);
    hipLaunchKernelGGL(mask_morph_kernel, dim3(blocks), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

void mask_morph_tiling(uint32_t w, uint32_t h, uint32_t* tiles_x, uint32_t* tiles_y) {
    *tiles_x = ((w + 31u) / 32u + kTW - 1u) / kTW;
    *tiles_y = (h + kTH - 1u) / kTH;
}

}  // namespace dips
