// mask_shapes.hip -- the shape record of every component of a change mask
// (dips_mask_shapes): the exact second-order moments, the sum and the peak of
// a caller's weight plane, the crack counts (perimeter) and the Euler number
// (1 - holes).  The reference has no counterpart; every field is an integer
// sum over the set bits of a component, so it is exact.
//
// One launch behind launch_mask_components on the same ComponentsArgs, one
// thread per mask word: after cc_stats_kernel parent[node] is the root of
// every node, and after cc_select_kernel the root's area slot is the label,
// rank + 1, or 0 for a dropped component.  A run finds its record with those
// two loads; a run whose label is 0 or beyond max_boxes contributes nothing.
//
// Per run [s, e) of row j, with rm its bits in the word x:
//   SX, SXX   closed forms in the run's ends; SY, SYY, SXY from them and j.
//   cracks    l and r are the row shifted by one pixel (the carry bit from the
//             neighbour word), u and d the rows above and below, zero outside
//             the region: CRACKS_V = popc(rm & ~l) + popc(rm & ~r), CRACKS_H =
//             popc(rm & ~u) + popc(rm & ~d).
//   EULER     the Euler number of a cell complex on the pixels, every cell
//             charged to its pixel of the lowest row, and there the rightmost
//             but for the up-right cells.  A cell lies inside one 2 x 2
//             window and its pixels are pairwise adjacent under the call's
//             connectivity, so they are one component: the count needs no
//             root comparison, only the bits.  With ul and ur the rows above
//             shifted like l and r:
//               4: pixels - edges (x&l, x&u) + squares (x&l&u&ul);
//               8: the clique complex of the 8-adjacency: pixels - edges
//                  (x&l, x&u, x&ul, x&ur) + triangles (x&l&u, x&l&ul, x&u&ul,
//                  x&u&ur) - tetrahedra (x&l&u&ul).
//             Each is homotopy equivalent to the component as a plane set
//             (closed pixels for 8, open for 4), whose Euler number is 1 -
//             holes with the holes taken under the dual connectivity.
//   weights   the bytes under the run: aligned dwords between a head and a
//             tail of single bytes, so the plane may start at any address and
//             roi_w need not be a multiple of 4.  The kernel is a template on
//             whether weights are given: the other form reads no plane.
// A lane first sums the runs of its word that share the record of the first
// of them; then the lanes of the wave that share a record are summed over the
// wave (as cc_stats_kernel sums over a root); the wave's first such sum is
// staged in LDS, where the sums of the block's four waves that share a record
// become one, and one thread adds it to the output record, which the host
// cleared in the stream.  A wave's further sums of the round go straight to
// their records, and the runs of a word that belong to other records than
// its first wait for the next round.  So a frame that is one component costs
// one set of atomics per block, whether its words are one run each (all
// ones) or many (a component that percolates through noise).  Integer adds
// and max commute, so the record does not depend on the order.
//
// Termination: see mask_components.hip.  The kernel waits for no other
// thread but at its barriers, which every thread of the block reaches the
// same number of times: the round loop's condition is the barrier's own OR
// over the block, and nothing returns or breaks inside it.  Its atomics'
// returns are not read.  The run loop clears at least one bit of the word
// per step; a round takes the lane's first run out of the word, so the word
// it leaves for the next round has fewer bits; the wave loop retires at least
// its leader per step; the weight loops advance a pointer to the run's end.
// parent and the labels are read after the launches that wrote them, when
// they are final.
#include <hip/hip_runtime.h>

#include "dips_kernels.h"
#include "mask_labelling.h"  // word_pos, mask_word, slot_of
#include "mask_runs.h"       // next_run

namespace dips {

namespace {

// sum of i^2 over 0 <= i < n; n <= 65536, so the product stays below 2^50
__device__ __forceinline__ unsigned long long squares_below(unsigned long long n) {
    return n ? ((n - 1ull) * n * (2ull * n - 1ull)) / 6ull : 0ull;
}

__device__ __forceinline__ void weigh_byte(uint32_t v, uint32_t& sum, uint32_t& peak) {
    sum += v;
    peak = max(peak, v);
}

// sum and peak of the n <= 32 bytes at p
__device__ __forceinline__ void weigh_run(const uint8_t* p, uint32_t n, uint32_t& sum, uint32_t& peak) {
    const uint8_t* const end = p + n;
    while (p < end && ((uintptr_t)p & 3u) != 0u) weigh_byte(*p++, sum, peak);
    for (; p + 4 <= end; p += 4) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
        weigh_byte(v & 0xFFu, sum, peak);
        weigh_byte((v >> 8) & 0xFFu, sum, peak);
        weigh_byte((v >> 16) & 0xFFu, sum, peak);
        weigh_byte(v >> 24, sum, peak);
    }
    while (p < end) weigh_byte(*p++, sum, peak);
}

constexpr uint32_t kNoRecord = ~0u;

// What the runs of one record add up to: SX, SY, SXX, SYY, SXY, WSUM, then
// WMAX, CRACKS_V, CRACKS_H, EULER.
struct Partial {
    unsigned long long q[6];
    uint32_t wmax, cv, ch, eu;
};

__device__ __forceinline__ Partial no_partial() {
    return Partial{{0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, 0u, 0u, 0u, 0u};
}

template <bool kWeights>
__device__ __forceinline__ void merge(Partial& p, const Partial& o) {
#pragma unroll
    for (int i = 0; i < (kWeights ? 6 : 5); ++i) p.q[i] += o.q[i];
    if (kWeights) p.wmax = max(p.wmax, o.wmax);
    p.cv += o.cv;
    p.ch += o.ch;
    p.eu += o.eu;
}

// the partials of all lanes merged, in every lane
template <bool kWeights>
__device__ __forceinline__ void wave_merge(Partial& p) {
    for (int d = 32; d > 0; d >>= 1) {
        Partial o;
#pragma unroll
        for (int i = 0; i < 6; ++i) o.q[i] = i < (kWeights ? 6 : 5) ? __shfl_xor(p.q[i], d) : 0ull;
        o.wmax = kWeights ? (uint32_t)__shfl_xor((int)p.wmax, d) : 0u;
        o.cv = (uint32_t)__shfl_xor((int)p.cv, d);
        o.ch = (uint32_t)__shfl_xor((int)p.ch, d);
        o.eu = (uint32_t)__shfl_xor((int)p.eu, d);
        merge<kWeights>(p, o);
    }
}

// onto the output record `rw` (8-byte aligned: checked by the host)
template <bool kWeights>
__device__ __forceinline__ void add_to_record(uint32_t* rw, const Partial& p) {
    unsigned long long* rq = reinterpret_cast<unsigned long long*>(rw);
#pragma unroll
    for (int i = 0; i < (kWeights ? 6 : 5); ++i) atomicAdd(rq + i, p.q[i]);  // DIPS_SHAPE_SX .. DIPS_SHAPE_WSUM, in order
    if (kWeights) atomicMax(rw + DIPS_SHAPE_WMAX, p.wmax);
    atomicAdd(rw + DIPS_SHAPE_CRACKS_V, p.cv);
    atomicAdd(rw + DIPS_SHAPE_CRACKS_H, p.ch);
    atomicAdd(rw + DIPS_SHAPE_EULER, p.eu);
}

static_assert(DIPS_SHAPE_SX == 0u && DIPS_SHAPE_SY == 2u && DIPS_SHAPE_SXX == 4u && DIPS_SHAPE_SYY == 6u &&
                  DIPS_SHAPE_SXY == 8u && DIPS_SHAPE_WSUM == 10u && DIPS_SHAPE_WORDS == 16u,
              "Partial::q is the record's 64-bit fields in order");

}  // namespace

template <bool kWeights>
__global__ __launch_bounds__(256) void shapes_kernel(ShapesArgs g) {
    __shared__ Partial sh_part[4];
    __shared__ uint32_t sh_rec[4];
    const ComponentsArgs& a = g.cc;
    const WordPos q = word_pos(a);  // no early return: every thread takes part in the wave sums and the barriers
    uint32_t x = 0u, l = 0u, r = 0u, u = 0u, d = 0u, ul = 0u, ur = 0u;
    if (q.active) {
        x = mask_word(a, q.f, q.j, q.k);
        if (x) {
            const bool left = q.k > 0u, right = q.k + 1u < a.wpr;
            l = (x << 1) | (left ? mask_word(a, q.f, q.j, q.k - 1u) >> 31 : 0u);
            r = (x >> 1) | (right ? mask_word(a, q.f, q.j, q.k + 1u) << 31 : 0u);
            if (q.j > 0u) {
                u = mask_word(a, q.f, q.j - 1u, q.k);
                ul = (u << 1) | (left ? mask_word(a, q.f, q.j - 1u, q.k - 1u) >> 31 : 0u);
                ur = (u >> 1) | (right ? mask_word(a, q.f, q.j - 1u, q.k + 1u) << 31 : 0u);
            }
            if (q.j + 1u < a.h) d = mask_word(a, q.f, q.j + 1u, q.k);
        }
    }
    const bool c8 = a.connectivity == 8u;
    const uint32_t* parent = a.parent + (size_t)q.f * a.npx;
    uint32_t* const records = g.shapes + (size_t)q.f * a.max_boxes * DIPS_SHAPE_WORDS;  // the block's frame is one
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t rem = x;
    while (__syncthreads_or(rem != 0u)) {  // a round of the block; the barrier also orders the rounds' use of sh_*
        // the lane's round: the record of its first run that has one, and
        // every run of the word with that record; the runs of other records
        // stay in rem for the next round, the runs without a record leave it
        bool has = false;
        uint32_t rec = 0u, left = 0u;
        Partial mine = no_partial();
        while (rem != 0u) {  // clears at least one bit per step
            uint32_t s, e;
            next_run(rem, s, e);
            const uint32_t x0 = q.k * 32u + s, len = e - s;
            const uint32_t rm = (e < 32u ? 1u << e : 0u) - (1u << s);  // bits [s, e)
            const uint32_t root = parent[q.j * a.w + x0];  // a root since cc_stats_kernel
            const uint32_t label = a.area[slot_of(a, q.f, root / a.w, root % a.w)];  // since cc_select_kernel
            if (label == 0u || label > a.max_boxes) continue;
            if (!has) {
                has = true;
                rec = label - 1u;
            } else if (label - 1u != rec) {
                left |= rm;
                continue;
            }
            const unsigned long long n = len, j = q.j;
            const unsigned long long si = (n * (2ull * x0 + n - 1ull)) / 2ull;
            mine.q[0] += si;
            mine.q[1] += n * j;
            mine.q[2] += squares_below((unsigned long long)x0 + n) - squares_below(x0);
            mine.q[3] += n * j * j;
            mine.q[4] += si * j;
            mine.cv += (uint32_t)(__popc(rm & ~l) + __popc(rm & ~r));
            mine.ch += (uint32_t)(__popc(rm & ~u) + __popc(rm & ~d));
            // two's complement: a partial count may be negative, the sum over a component is not wrapped
            mine.eu += len - (uint32_t)(__popc(rm & l) + __popc(rm & u));
            if (c8)
                mine.eu += (uint32_t)(__popc(rm & l & u) + __popc(rm & l & ul) + __popc(rm & u & ul) + __popc(rm & u & ur)) -
                           (uint32_t)(__popc(rm & ul) + __popc(rm & ur) + __popc(rm & l & u & ul));
            else
                mine.eu += (uint32_t)__popc(rm & l & u & ul);
            if (kWeights) {
                uint32_t sum = 0u;
                weigh_run(g.weights + (size_t)q.f * a.npx + (size_t)q.j * a.w + x0, len, sum, mine.wmax);
                mine.q[5] += sum;
            }
        }
        rem = left;  // has lost its first run at least
        // the wave: one sum per record among its lanes; the first goes to
        // the block's stage, any other straight to its record
        unsigned long long pending = __ballot(has);
        if (pending == 0ull && lane == 0u) sh_rec[wave] = kNoRecord;
        bool first = true;
        while (pending) {  // loses at least the leader's bit per step
            const int leader = __ffsll(pending) - 1;
            const uint32_t lrec = (uint32_t)__shfl((int)rec, leader);
            const bool m = has && rec == lrec;
            Partial t = m ? mine : no_partial();
            wave_merge<kWeights>(t);
            if ((int)lane == leader) {
                if (first) {
                    sh_part[wave] = t;
                    sh_rec[wave] = lrec;
                } else {
                    add_to_record<kWeights>(records + (size_t)lrec * DIPS_SHAPE_WORDS, t);
                }
            }
            first = false;
            has = has && !m;
            pending = __ballot(has);
        }
        __syncthreads();
        // the block: thread v < 4 owns wave v's staged sum unless an earlier
        // wave staged the same record, and adds the later waves' to it: one
        // set of atomics per block where its waves agree
        if (threadIdx.x < 4u) {
            const uint32_t v = threadIdx.x, vrec = sh_rec[v];
            bool own = vrec != kNoRecord;
            for (uint32_t o = 0u; o < v; ++o) own = own && sh_rec[o] != vrec;
            if (own) {
                Partial t = sh_part[v];
                for (uint32_t o = v + 1u; o < 4u; ++o)
                    if (sh_rec[o] == vrec) merge<kWeights>(t, sh_part[o]);
                add_to_record<kWeights>(records + (size_t)vrec * DIPS_SHAPE_WORDS, t);
            }
        }
    }
}

hipError_t launch_mask_shapes(const ShapesArgs& g, hipStream_t s) {
    const ComponentsArgs& a = g.cc;
    const uint64_t word_blocks = (uint64_t)a.n_frames * a.bpf;
    if (a.n_frames == 0 || a.w == 0 || a.h == 0 || a.w > 65536u || a.h > 65536u || a.npx != a.w * a.h ||
        a.npx >= (1u << 30) || a.wpr != (a.w + 31u) / 32u || a.hw != (a.w + 1u) / 2u || a.nslots != a.hw * a.h ||
        a.wpf != a.wpr * a.h || a.bpf != (a.wpf + 255u) / 256u || word_blocks >= (1ull << 31) ||
        (a.connectivity != 4u && a.connectivity != 8u) || !a.mask || !a.parent || !a.area || a.max_boxes == 0u ||
        !g.shapes || ((uintptr_t)g.shapes & 7u) != 0u)
        return hipErrorInvalidValue;
    const dim3 wg((uint32_t)word_blocks), tb(256);
    if (g.weights)
        hipLaunchKernelGGL(shapes_kernel<true>, wg, tb, 0, s, g);
    else
        hipLaunchKernelGGL(shapes_kernel<false>, wg, tb, 0, s, g);
    return hipGetLastError();
}

}  // namespace dips
