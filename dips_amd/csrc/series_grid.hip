// series_grid.hip -- the difference series resolved per cell of a spatial
// grid over a region of interest (dips_diff_series_grid): one read of the
// batch, rows * cols entries per frame.
//
// series_v2.hip treats a frame as a flat run of vecs, so its tiles have no
// rectangle.  Here a tile is 64 * U vecs of ONE cell (GridArgs,
// dips_kernels.h): a vec is 4 horizontally consecutive pixels starting at
// cell_x + 4 v in row cell_y + r, and the (row, vec-in-row) index is flattened
// over the cell, so narrow cells still fill the lanes: the flat slots of the
// regional skeleton (series_slots.h, series_region.h), one cell at a time.
// The per-pixel arithmetic is frame_v2 (series_v2_frame.h), unchanged:
// same unroll, one call per (tile, frame), same 16-byte records.
//
// Masking.  The last vec of a cell row covers w % 4 valid pixels when that is
// not 0; the bytes after them belong to the neighbouring cell (or the next
// frame row).  Both the frame dwords and the reference dwords of such a slot
// are ANDed with a mask of valid_px * C bytes before frame_v2 / derive_v2 see
// them.  A pixel whose bytes are zero on both sides adds 0 to SAD and SJ and
// has dI = 0, and the threshold compare is strict, so it is never counted,
// not even at tau = 0.  Slots past the cell's last vec get an offset past the
// descriptor: the hardware returns zeros for them.  The mask is applied in
// place in the ring slot at the frame's first use, so in 'per-frame' mode the
// masked dwords are what the next frame sees as its reference.  The masks
// live in registers (U * NDW per lane, computed once per tile) and the pass is
// unconditional: U * NDW v_and per frame.  (Recomputing them per frame from a
// packed pixel count behind a wave-uniform "tile has a partial slot" branch
// needed fewer live registers on paper, but hipcc hoisted the masks out of
// the frame loop anyway and the branch doubled the ring's live ranges: 250+
// VGPRs.)
//
// A few vecs are left out: a partial last vec of a cell row that starts
// within 3 pixels of the frame's end would read past it (in the frame's last
// row the corner cell when its width is no multiple of 4 and cells narrower
// than a vec next to it; in frames narrower than 3 pixels also vecs of up to
// three rows before the last).  Such a slot is invalid here and the host adds
// its <= 3 pixels with the generic kernel below, as series_abi.hip does for
// the ragged tail of a whole frame.
//
// Schedule: a persistent grid, items (frame part, tile) dealt part-major with
// stride n_waves as in series_v2_body, a 4-slot register ring of frames (three
// frames of loads in flight), one record per (tile, frame), summed per (cell,
// frame) by grid_reduce_kernel.
#include "series_region.h"

namespace dips {

// Mask of dword k of a vec whose first nb bytes are valid.
__device__ __forceinline__ uint32_t head_mask(uint32_t nb, int k) {
    const int32_t left = (int32_t)nb - 4 * k;
    return left >= 4 ? 0xFFFFFFFFu : (left <= 0 ? 0u : (0xFFFFFFFFu >> (32 - 8 * left)));
}

// Waves per SIMD asked of the register allocator.  Beside series_v2_body's
// state a lane holds U offsets and U * NDW masks: RGB8 (U = 5) needs 138-141
// VGPRs and spills at the 128 of 4 waves, so it runs 3; RGBA8 fits 4
// (119-125).  Three frames of loads in flight per wave keep 3 x 3 x 3.75 KiB
// outstanding per SIMD.
template <int C>
constexpr int grid_min_waves() {
    return C == 3 ? 3 : 4;
}

template <int C, int CH, int U, bool PF, int ISI>
__global__ __launch_bounds__(256, (grid_min_waves<C>())) void series_grid_kernel(GridArgs a) {
    constexpr int NDW = Fmt<C>::NDW;
    if (a.zero != nullptr) {
        const uint32_t stride = gridDim.x * blockDim.x;
        for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < a.zero_n; j += stride) a.zero[j] = 0u;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_waves) return;
    const uint32_t fb = a.frame_bytes;
    SeriesArgs sa{};  // frame_v2 reads the threshold from it (no map here)
    sa.thr = a.thr;
    // record dword offsets of the lanes that store reduced values; other
    // lanes point past the descriptor and their stores are dropped
    const uint32_t rec_off8 = (lane & 7u) == 0u ? (lane >> 5) * 16u + ((lane >> 3) & 3u) * 4u : kNoSlot;
    const uint32_t rec_off4 = (lane & 15u) == 0u ? (lane >> 4) * 4u : kNoSlot;

    const uint64_t pitems = region_items(a.n_frames, a.part_frames, a.n_tiles);
    for (uint64_t it = wave; it < pitems; it += a.n_waves) {
        const RegionItem i = region_item(it, a.n_frames, a.part_frames, a.n_tiles);
        const uint32_t tile = i.tile, t0 = i.t0, n = i.n;
        const uint32_t cell = tile / a.tiles_per_cell;
        const uint32_t v0 = (tile - cell * a.tiles_per_cell) * (uint32_t)(64 * U);
        const uint32_t crow = cell / a.g.cols;
        const GridRect rc = grid_cell_rect(a.g, crow, cell - crow * a.g.cols);
        const uint32_t vpr = dips_sched::flat_vpr(rc.w);  // vecs per cell row
        const uint32_t nvec = vpr * rc.h;
        if (v0 >= nvec) continue;  // a tile id past this cell's last tile

        // per lane-slot, once per tile: the frame offset and the byte mask of
        // its valid pixels (all ones for a slot that loads nothing)
        uint32_t voff[U];
        uint32_t msk[U][NDW];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const dips_sched::Slot s =
                dips_sched::region_slot(rc, vpr, nvec, a.width, (uint32_t)C, fb, v0 + (uint32_t)(u * 64) + lane);
            const uint32_t nb = (s.ok ? dips_sched::vec_px_inside(rc.w, s.x4) : 4u) * (uint32_t)C;
            voff[u] = s.voff;
#pragma unroll
            for (int k = 0; k < NDW; ++k) msk[u][k] = head_mask(nb, k);
        }
        const FrameLoader<C, U> ld{a.frames, fb, i.tlast, voff};

        const __amdgpu_buffer_rsrc_t rpart =
            make_rsrc(a.partials + 2 * (uint64_t)tile * a.n_frames, a.n_frames * 16u);
        // the mask pass of one ring slot (or the reference), in place
        auto settle = [&](uint32_t (&v)[U][NDW]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int k = 0; k < NDW; ++k) v[u][k] &= msk[u][k];
            }
        };

        // the ring that also holds the reference bytes (ref_ring_fill); the
        // loop pairs two frames per cross-lane reduction
        uint32_t buf[4][U][NDW];
        uint32_t rb[U][NDW];  // overall mode only
        St2 st[U];
        {
            auto& dref = ref_ring_fill<PF>(ld, region_ref<PF>(a.frames, a.ref0, t0, fb), t0, buf, rb);
            settle(dref);
#pragma unroll
            for (int u = 0; u < U; ++u) derive_v2<C, CH, (ISI != 0)>(dref[u], st[u]);
        }

        uint32_t k = 0;
        for (; k + 4 <= n; k += 4) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint32_t v[8], c0, c1;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int j = 2 * h + q;
                    const uint32_t tf = t0 + k + (uint32_t)j;
                    if constexpr (PF) {
                        settle(buf[(j + 1) & 3]);
                        frame_v2<C, CH, U, PF, false, kAuxNT, NDW, NDW, ISI>(sa, st, buf[j], buf[(j + 1) & 3], 0u, tf,
                                                                            v + 4 * q, q ? c1 : c0);
                        __builtin_amdgcn_sched_barrier(0);
                        ld.frame(tf + 3, buf[j]);
                    } else {
                        settle(buf[j]);
                        frame_v2<C, CH, U, PF, false, kAuxNT, NDW, NDW, ISI>(sa, st, rb, buf[j], 0u, tf, v + 4 * q,
                                                                            q ? c1 : c0);
                        __builtin_amdgcn_sched_barrier(0);
                        ld.frame(tf + 4, buf[j]);
                    }
                }
                const uint32_t y = wave_sum8_lanes(v, lane);
                store_pair(rpart, t0 + k + 2 * h, rec_off8, lane, y, c0, c1);
            }
        }
        // tail: up to 3 frames, already in flight in their slots
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (k + (uint32_t)j < n) {
                uint32_t v[4], c;
                const uint32_t tf = t0 + k + (uint32_t)j;
                if constexpr (PF) {
                    settle(buf[j + 1]);
                    frame_v2<C, CH, U, PF, false, kAuxNT, NDW, NDW, ISI>(sa, st, buf[j], buf[j + 1], 0u, tf, v, c);
                } else {
                    settle(buf[j]);
                    frame_v2<C, CH, U, PF, false, kAuxNT, NDW, NDW, ISI>(sa, st, rb, buf[j], 0u, tf, v, c);
                }
                const uint32_t y = wave_sum4_lanes(v);
                store_one(rpart, tf, rec_off4, lane, y, c);
            }
        }
    }
}

// Sum the records {SAD, SJ + count << 20, H, L} of one cell's tiles
// [tile0, tile1) for frame t and add them to the cell's entry (u64 atomics:
// order-independent; one thread per (cell, frame, chunk of tiles), not one
// per wave of the series kernel).  Threads run along t, so a tile's records
// are read coalesced; blockIdx.x = cell * ceil(n_frames / 256) + frame block,
// blockIdx.y = the chunk of tiles.
__global__ __launch_bounds__(256) void grid_reduce_kernel(const uint64_t* __restrict__ partials, uint32_t n_frames,
                                                          uint32_t frame_blocks, uint32_t tiles_per_cell,
                                                          uint32_t tiles_per_block, uint32_t vecs_per_tile, GridSpec g,
                                                          dips_series_entry* __restrict__ cells) {
    const uint32_t cell = blockIdx.x / frame_blocks;
    const uint32_t t = (blockIdx.x - cell * frame_blocks) * 256u + threadIdx.x;
    if (t >= n_frames) return;
    const uint32_t crow = cell / g.cols;
    const GridRect rc = grid_cell_rect(g, crow, cell - crow * g.cols);
    const uint32_t nvec = ((rc.w + 3u) >> 2) * rc.h;
    const uint32_t nt = (nvec + vecs_per_tile - 1u) / vecs_per_tile;  // this cell's tiles
    const uint32_t tile0 = blockIdx.y * tiles_per_block;
    const uint32_t tile1 = min(nt, tile0 + tiles_per_block);
    if (tile0 >= tile1) return;
    const u32x4* p =
        reinterpret_cast<const u32x4*>(partials) + ((uint64_t)(cell * tiles_per_cell + tile0) * n_frames + t);
    uint64_t sad = 0, sj = 0, cnt = 0, h = 0;
    int64_t l = 0;
    auto add = [&](const u32x4 rec) {
        sad += rec.x;
        sj += rec.y & 0xFFFFFu;
        cnt += rec.y >> 20;
        h += rec.z;
        l += (int64_t)(int32_t)rec.w;
    };
    uint32_t tile = tile0;
    for (; tile + 8u <= tile1; tile += 8u, p += 8u * (uint64_t)n_frames) {
        u32x4 rec[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) rec[k] = __builtin_nontemporal_load(p + (uint64_t)k * n_frames);
#pragma unroll
        for (int k = 0; k < 8; ++k) add(rec[k]);
    }
    for (; tile < tile1; ++tile, p += n_frames) add(__builtin_nontemporal_load(p));
    dips_series_entry* e = cells + ((uint64_t)t * (g.rows * g.cols) + cell);
    atomicAdd(reinterpret_cast<unsigned long long*>(&e->sad), (unsigned long long)sad);
    atomicAdd(reinterpret_cast<unsigned long long*>(&e->sj), (unsigned long long)sj);
    atomicAdd(reinterpret_cast<unsigned long long*>(&e->count), (unsigned long long)cnt);
    atomicAdd(reinterpret_cast<unsigned long long*>(&e->si_fixed), (unsigned long long)((h << 15) + (uint64_t)l));
}

// Generic path: any format, shape and alignment.  series_generic_kernel's
// per-pixel body (the reference's own (cmax + cmin) / 2 intensity form,
// dips_shader.wgsl:73-81) with 2-D addressing: a workgroup walks 256-pixel
// segments of ONE cell of one frame, so its reduction never mixes cells, and
// adds four u64 atomics into that cell's entry.  It serves GRAY8,
// DIPS_FLAG_FORCE_GENERIC, DIPS_FLAG_CROSSCHECK, the shapes the fast kernel's
// geometry refuses and the one vec the fast kernel leaves out; being
// independent of frame_v2 it is the fast kernel's on-device cross-check.
template <int C>
__global__ __launch_bounds__(256) void grid_generic_kernel(GridGenericArgs a) {
    __shared__ uint64_t red[4][4];
    const uint32_t n_cells = a.g.rows * a.g.cols;
    const uint64_t per_frame = (uint64_t)n_cells * a.segs_per_cell;
    const uint64_t n_seg = per_frame * a.n_frames;
    for (uint64_t seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        const uint32_t t = (uint32_t)(seg / per_frame);
        const uint64_t rem = seg - (uint64_t)t * per_frame;
        const uint32_t cell = (uint32_t)(rem / a.segs_per_cell);
        const uint32_t s = (uint32_t)(rem - (uint64_t)cell * a.segs_per_cell);
        const uint32_t crow = cell / a.g.cols;
        const GridRect rc = grid_cell_rect(a.g, crow, cell - crow * a.g.cols);
        const uint64_t npx = (uint64_t)rc.w * rc.h;
        if ((uint64_t)s * 256u >= npx) continue;  // a segment id past this cell (uniform in the workgroup)
        const uint64_t q = (uint64_t)s * 256u + threadIdx.x;
        const uint64_t fb = a.frame_bytes;
        const uint8_t* F = a.frames + (uint64_t)t * fb;
        const uint8_t* R = a.mode == 1u ? (t == 0 ? a.ref0 : a.frames + (uint64_t)(t - 1) * fb) : a.ref0;
        uint64_t sad = 0, sj = 0, cnt = 0, sif = 0;
        if (q < npx) {
            const uint32_t py = (uint32_t)(q / rc.w);
            const uint32_t px = (uint32_t)(q - (uint64_t)py * rc.w);
            const uint64_t p = (uint64_t)(rc.y + py) * a.width + rc.x + px;
            uint32_t fv[4] = {0, 0, 0, 0}, rv[4] = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < C; ++c) {
                fv[c] = F[p * C + c];
                rv[c] = R[p * C + c];
                sad += fv[c] > rv[c] ? fv[c] - rv[c] : rv[c] - fv[c];
            }
            if constexpr (C == 1) {
                fv[1] = fv[2] = fv[0];
                rv[1] = rv[2] = rv[0];
            }
            const float If = intensity_rgb(fv[0], fv[1], fv[2], a.chroma);
            const float Ir = intensity_rgb(rv[0], rv[1], rv[2], a.chroma);
            uint32_t jf, jr;
            if (a.chroma >= 1u && a.chroma <= 3u) {
                jf = 2u * fv[a.chroma - 1u];
                jr = 2u * rv[a.chroma - 1u];
            } else {
                jf = max(max(fv[0], fv[1]), fv[2]) + min(min(fv[0], fv[1]), fv[2]);
                jr = max(max(rv[0], rv[1]), rv[2]) + min(min(rv[0], rv[1]), rv[2]);
            }
            sj = jf > jr ? jf - jr : jr - jf;
            const float dI = fabsf(If - Ir);
            if (dI > a.tau) {
                cnt = 1;
                sif = (uint64_t)((double)dI * 4294967296.0);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sad += __shfl_xor(sad, o, 64);
            sj += __shfl_xor(sj, o, 64);
            cnt += __shfl_xor(cnt, o, 64);
            sif += __shfl_xor(sif, o, 64);
        }
        const uint32_t w = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0) {
            red[w][0] = sad;
            red[w][1] = sj;
            red[w][2] = cnt;
            red[w][3] = sif;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const uint64_t v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
            dips_series_entry* e = a.cells + ((uint64_t)t * a.out_stride + a.out_base + cell);
            atomicAdd(reinterpret_cast<unsigned long long*>(e) + threadIdx.x, (unsigned long long)v);
        }
        __syncthreads();  // red is reused by the next segment
    }
}

// ---------------------------------------------------------------------------
// Host-side launchers (instantiation table)
// ---------------------------------------------------------------------------
template <int C, int ISI>
static const void* pick_grid(int chroma, bool pf) {
    return dispatch_chroma(chroma, [&](auto ch) {
        return dispatch_flag(pf, [&](auto p) {
            return reinterpret_cast<const void*>(&series_grid_kernel<C, ch.value, v2_unroll<C>(), p.value, ISI>);
        });
    });
}

const void* series_grid_kernel_ptr(int channels, int chroma, bool per_frame, int isi) {
    switch (channels) {
        case 3: return isi == 1 ? pick_grid<3, 1>(chroma, per_frame) : pick_grid<3, 0>(chroma, per_frame);
        case 4: return isi == 1 ? pick_grid<4, 1>(chroma, per_frame) : pick_grid<4, 0>(chroma, per_frame);
        default: return nullptr;
    }
}

hipError_t launch_series_grid(const GridArgs& a, int channels, int chroma, bool per_frame, int isi, uint32_t blocks,
                              hipStream_t s) {
    const void* k = series_grid_kernel_ptr(channels, chroma, per_frame, isi);
    if (!k || blocks == 0 || a.part_frames == 0 || a.tiles_per_cell == 0) return hipErrorInvalidValue;
    GridArgs args = a;
    void* params[] = {&args};
    return hipLaunchKernel(k, dim3(blocks), dim3(256), params, 0, s);
}

hipError_t launch_grid_reduce(const GridArgs& a, int channels, dips_series_entry* cells, hipStream_t s) {
    // tiles per thread as launch_series_reduce picks them: 64 when that still
    // gives >= 2048 groups, else down to 8
    const uint32_t n_cells = a.g.rows * a.g.cols;
    const uint32_t gx = (a.n_frames + 255u) / 256u;
    const uint64_t bx = (uint64_t)gx * n_cells;
    if (bx == 0 || bx >= (1ull << 31)) return hipErrorInvalidValue;
    uint32_t tpb = 64;
    while (tpb > 8u && bx * ((a.tiles_per_cell + tpb - 1u) / tpb) < 2048u) tpb >>= 1;
    while ((a.tiles_per_cell + tpb - 1u) / tpb > 65535u) tpb <<= 1;
    dim3 grid((uint32_t)bx, (a.tiles_per_cell + tpb - 1u) / tpb);
    hipLaunchKernelGGL(grid_reduce_kernel, grid, dim3(256), 0, s, a.partials, a.n_frames, gx, a.tiles_per_cell, tpb,
                       64u * (uint32_t)fast_unroll(channels), a.g, cells);
    return hipGetLastError();
}

hipError_t launch_grid_generic(const GridGenericArgs& a, int channels, hipStream_t s) {
    const uint64_t n_seg = (uint64_t)a.g.rows * a.g.cols * a.segs_per_cell * a.n_frames;
    const uint64_t blocks = n_seg < (1ull << 22) ? n_seg : (1ull << 22);
    if (blocks == 0) return hipSuccess;
    switch (channels) {
        case 1: hipLaunchKernelGGL(grid_generic_kernel<1>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(grid_generic_kernel<3>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL(grid_generic_kernel<4>, dim3((uint32_t)blocks), dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dips
