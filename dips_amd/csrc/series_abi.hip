// series_abi.hip -- host side of include/dips_hip.h, part 3: the north-star
// per-frame difference series ('overall' against frame 0 or a given
// reference, 'per-frame' against the previous frame; the per-pixel math of
// dips_shader.wgsl:64-82), its host feeds, the synthetic frames and the
// measurement legs bench.py reads (read ceilings, geometry).  Every
// extern "C" body runs inside dips_abi::guard (abi_guard.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "dips_handle.h"
#include "dips_kernels.h"
#include "series_sigma_delta.h"

using dips_abi::guard;
using namespace dips_internal;

namespace {

struct FastGeom {
    bool ok = false;
    uint64_t n_tiles = 0, items = 0, n_waves = 0, blocks = 0;
    uint64_t vec_bytes = 0;    // whole vecs of a frame (the vectorised kernel's range)
    uint64_t tail_px0 = 0;     // first pixel of the ragged tail (npx: none)
    uint32_t part_frames = 0;  // part-major schedule: frames per part (0: contiguous ranges)
};

// Resident waves per SIMD for a kernel of `occupancy` waves per SIMD, capped
// by DIPS_SERIES_WAVES_PER_SIMD where `env_cap` (a deployment knob; every
// launch applies it, dips_shard_plan also reports the uncapped count).  No
// launch caps itself: leaving a slot per SIMD free for the halo's RCCL
// kernels beside the sharded 'per-frame' launch cost 2-5 ms per 2,000-5,000
// 4K frames, where the full grid lets the exchange through at +0.03-0.07 ms
// (profiles/r06/halo_contention/).
uint64_t waves_per_simd(uint64_t occupancy, bool env_cap) {
    if (env_cap) {
        if (const char* cap = std::getenv("DIPS_SERIES_WAVES_PER_SIMD")) {
            const unsigned long c = std::strtoul(cap, nullptr, 10);
            if (c >= 1 && c < occupancy) return c;
        }
    }
    return occupancy;
}

// The part-major schedule of the series kernels (series_v2.hip,
// series_gray.hip): the batch's frames cut into P parts of L, items (part,
// tile) dealt to the waves with stride n_waves, so that concurrent waves read
// adjacent tiles of the same frames.  Measured 0.3-1.1 points above one
// contiguous (tile, frame) range per wave on each of four frame buffers,
// 0.7-1.2 % less energy per frame (tools/alloc_policy_ab.hip,
// profiles/r03/alloc/); per-frame 77.3 % against 75.4 % of 8 TB/s, 'overall'
// 74.1 against 72.05 % (profiles/r03/parts/, profiles/r04/l/).  Parts of at
// least 128 frames (each item re-reads its reference tile: +1/L of the
// traffic), P from the one that gives every resident wave slot an item up to
// 4x that: the smallest whose items fill >= 98 % of the slots (k items per
// slot), else the best-filling one (98 rather than 95 %: 8K's 3 parts fill
// 99.9 % against 2 parts' 97.4 %, +0.5 points in alternated runs,
// profiles/r05/ab_fill/; every other config keeps its part count); the
// waves then get ceil(items / n_waves) or one fewer items each (4K RGB8, 5000
// frames, U = 5: L = 1000, 4,050 waves).
// Batches of fewer than 256 frames keep the contiguous ranges.
void part_geometry(FastGeom& g, uint64_t n_frames, uint64_t resident) {
    if (n_frames < 256 || g.n_tiles == 0 || resident == 0) return;
    const uint64_t p_min = std::max<uint64_t>((resident + g.n_tiles - 1) / g.n_tiles, (n_frames + 1249) / 1250);
    const uint64_t p_max = std::min<uint64_t>(4 * p_min, n_frames / 128);
    if (p_max < p_min) return;
    uint64_t best_p = 0;
    double best_fill = -1.0;
    for (uint64_t p = p_min; p <= p_max; ++p) {
        const uint64_t L = (n_frames + p - 1) / p;
        const uint64_t parts = (n_frames + L - 1) / L;
        const uint64_t items = parts * g.n_tiles;
        const uint64_t k = (items + resident - 1) / resident;
        const double fill = (double)items / (double)(k * resident);
        if (fill > best_fill + 1e-9) {
            best_fill = fill;
            best_p = p;
        }
        if (fill >= 0.98) break;
    }
    const uint64_t L = (n_frames + best_p - 1) / best_p;
    const uint64_t items = ((n_frames + L - 1) / L) * g.n_tiles;
    const uint64_t k = (items + resident - 1) / resident;
    g.part_frames = (uint32_t)L;
    g.n_waves = (items + k - 1) / k;
    g.blocks = (g.n_waves + 3) / 4;
}

FastGeom fast_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf,
                       bool map, bool align = false, int isi = 0, bool env_cap = true) {
    FastGeom g;
    const uint64_t npx = (uint64_t)width * height;
    const uint64_t fb = npx * (uint64_t)C;
    const int ppv = dips::pixels_per_vec(C);
    // any alignment and pixel count: the vectorised kernel takes the whole
    // vecs of every frame (unaligned frames through unaligned buffer loads,
    // exact on gfx950: tests/test_gpu_series.py::test_unaligned_device_batches), the generic kernel the
    // < ppv trailing pixels
    const uint64_t nvec = npx / (uint64_t)ppv;
    if (nvec == 0 || fb >= (1ull << 31) || n_frames == 0) return g;
    const uint64_t U = (uint64_t)dips::fast_unroll(C);
    g.vec_bytes = nvec * (uint64_t)ppv * (uint64_t)C;
    g.tail_px0 = nvec * (uint64_t)ppv;
    g.n_tiles = (nvec + 64 * U - 1) / (64 * U);
    g.items = g.n_tiles * n_frames;
    const void* k = dips::series_fast_kernel_ptr(C, C == 1 ? 0 : (int)h->p.chroma_filter, pf, map, align, isi);
    if (!k) return g;
    const uint64_t resident = waves_per_simd((uint64_t)occupancy_blocks(h, k), env_cap) * (uint64_t)h->cu_count * 4u;
    g.n_waves = g.items < resident ? g.items : resident;
    g.blocks = (g.n_waves + 3) / 4;
    if (C == 3 || C == 4) part_geometry(g, n_frames, resident);
    g.ok = g.n_tiles < (1ull << 32) && g.blocks < (1ull << 31);
    return g;
}

// GRAY8 runs on the table kernel (series_gray.hip, table layout 4: layout 5
// or 2 per workgroup from a sample of its own items, or the one that
// DIPS_FLAG_GRAY_BAND_TABLE / _PAIR_TABLE pins) unless DIPS_FLAG_CROSSCHECK
// asks for the f32 kernel series_fast_kernel.
//
// Layout 4's choice: layout 5 when the band holds at least kGrayAutoMin of
// the sampled pixels and either kGrayAutoHi of them or the sampled waves'
// frame bytes span kGrayAutoSpread levels on average, else layout 2.  From
// the layouts measured in one process over five 4K contents
// (profiles/r04/d/gray_layout_ab.jsonl; band
// fraction / mean spread of a wave's 1024 pixels; % of 8 TB/s):
//   synthetic (0.64 / 247): layout 5 71.8-72.3, 3 64-70, 2 63-66;
//   random (0.03 / 248): 2 61-63, 5 62-63, 3 60;
//   flat 128 +- 3 (0.51 / 6): 2 70-71, 3 69, 5 58 (bank conflicts);
//   gradient (0.80 / 70): all 69-70;  moving (0.80 / 70): 5 72.2-72.4, 2, 3 68-71.
constexpr double kGrayAutoMin = 0.25, kGrayAutoHi = 0.9;
constexpr uint32_t kGrayAutoSpread = 48;
constexpr int kGrayLayout = 4;

bool gray_lut_enabled(const dips_handle* h) { return !h->crosscheck(); }

FastGeom gray_lut_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, bool env_cap = true) {
    FastGeom g;
    const uint64_t npx = (uint64_t)width * height;
    const uint64_t nvec = npx / 16u;
    if (nvec == 0 || npx >= (1ull << 31) || n_frames == 0) return g;
    const uint64_t U = (uint64_t)dips::kUnrollGrayLut;
    const uint64_t gw = dips::kGrayLutWaves;
    g.vec_bytes = nvec * 16u;
    g.tail_px0 = nvec * 16u;
    g.n_tiles = (nvec + 64 * U - 1) / (64 * U);
    g.items = g.n_tiles * n_frames;
    // one group per CU (the tables fill its LDS): 4 waves per SIMD
    const uint64_t resident = waves_per_simd(gw / 4u, env_cap) * 4u * (uint64_t)h->cu_count;
    g.n_waves = g.items < resident ? g.items : resident;
    // 'per-frame' batches: the part-major schedule, as for RGB8 (part_geometry)
    if (h->p.mode == DIPS_MODE_PER_FRAME) part_geometry(g, n_frames, resident);
    g.blocks = (g.n_waves + gw - 1) / gw;
    g.ok = g.n_tiles < (1ull << 32) && g.blocks < (1ull << 31);
    return g;
}

// The T_d / T_c tables of the GRAY8 table kernel for the handle's tau.
dips_status ensure_gray_lut(dips_handle* h, hipStream_t s) {
    if (h->gray_lut_valid && h->gray_lut_tau == h->p.tau) return DIPS_OK;
    DIPS_HIP(h, h->gray_lut.ensure(2 * dips::kGrayLutAllocBytes));
    DIPS_HIP(h, dips::launch_gray_lut(h->gray_lut.as<uint8_t>(), h->p.tau, kGrayLayout, s));
    h->gray_lut_valid = true;
    h->gray_lut_tau = h->p.tau;
    return DIPS_OK;
}

// The intensity-sum form of the RGB8 / RGBA8 series kernel for the handle's
// tau (series_v2.hip ISI): 1 (the integer sum) for tau >= 2^-5, 0 (the exact
// f64 sum) below that or with DIPS_FLAG_CROSSCHECK.
int series_isi_form(const dips_handle* h) {
    const int C = (int)h->p.format;
    if (C == 1 || h->crosscheck() || !dips::series_v2_isi(h->p.tau)) return 0;
    return 1;
}

// The timing events of a launch (DIPS_FLAG_TIME_KERNEL), back to the handle's
// free list when the launch function returns without having queued them.
struct EventReturn {
    dips_handle* h;
    hipEvent_t* e0;
    hipEvent_t* e1;
    ~EventReturn() {
        try {
            if (*e0) h->ev_free.push_back(*e0);
            if (*e1) h->ev_free.push_back(*e1);
        } catch (...) {
        }
    }
};

}  // namespace

namespace dips_internal {

// Run the series on device pointers, asynchronously on `s`.
dips_status run_series_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                              uint32_t n_frames, const uint8_t* ref0, dips_series_entry* series, uint8_t* map,
                              hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t npx = (uint64_t)width * height;
    const uint64_t fb = npx * (uint64_t)C;
    FastGeom g;
    const bool glut = C == 1 && gray_lut_enabled(h);
    // RGB8 / RGBA8 frames off a 4-byte boundary (an odd frame stride or an
    // offset pointer) run the aligned-load form of the kernel (series_v2.hip
    // ALIGN)
    const bool align = (C == 3 || C == 4) && ((((uintptr_t)frames | (uintptr_t)fb | (uintptr_t)ref0) & 3u) != 0u);
    const int isi = series_isi_form(h);
    if (!(h->p.flags & DIPS_FLAG_FORCE_GENERIC))
        g = glut ? gray_lut_geometry(h, width, height, n_frames)
                 : fast_geometry(h, width, height, n_frames, C, pf, map != nullptr, align, isi);
    // the series starts at zero: the table and RGB(A) kernels clear it
    // themselves (SeriesArgs::zero), saving a fill launch; the others after a
    // fill
    const bool kzero = g.ok && (glut || C != 1) && n_frames < (1u << 30);
    if (!kzero) DIPS_HIP(h, hipMemsetAsync(series, 0, sizeof(dips_series_entry) * (size_t)n_frames, s));
    auto launch_generic = [&](uint64_t px0) -> dips_status {
        const uint64_t bpf = (npx - px0 + 255u) / 256u;  // 256-pixel segments per frame
        if (bpf >= (1ull << 32))
            return fail(h, DIPS_ERR_INVALID, "frame too large for the generic kernel (2^40 pixels)");
        dips::GenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.dmap = map;
        a.series = series;
        a.frame_bytes = fb;
        a.n_px = npx;
        a.px0 = px0;
        a.n_frames = n_frames;
        a.blocks_per_frame = (uint32_t)bpf;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        DIPS_HIP(h, dips::launch_series_generic(a, C, s));
        return DIPS_OK;
    };

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    dips_status st = DIPS_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // the timing events go back to the free list on every early return; they
    // join ev_pending only once both are recorded
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
    }
    if (g.ok && glut) {
        st = ensure_gray_lut(h, s);  // before e0: the table is not part of the series launch
        if (st != DIPS_OK) return st;
    }
    if (timing) DIPS_HIP(h, hipEventRecord(e0, s));
    if (g.ok) {
        DIPS_HIP(h, h->partials.ensure((size_t)g.items * 16u));
        dips::SeriesArgs a{};
        if (glut) {
            // layout 4's thresholds in 1/1024 of the sampled pixels (each
            // workgroup samples its own items, series_gray.hip gray_sample);
            // a pinned layout: probe_min 0 (always 5) or 1025 (always 2)
            a.probe_min = std::max(1u, (uint32_t)std::ceil(kGrayAutoMin * 1024.0));
            if (h->p.flags & DIPS_FLAG_GRAY_BAND_TABLE) a.probe_min = 0u;
            else if (h->p.flags & DIPS_FLAG_GRAY_PAIR_TABLE) a.probe_min = 1025u;
            a.probe_hi = (uint32_t)std::ceil(kGrayAutoHi * 1024.0);
            a.probe_spread = kGrayAutoSpread;
        }
        if (kzero) {
            a.zero = reinterpret_cast<uint64_t*>(series);
            a.zero_n = 4u * n_frames;
        }
        a.frames = frames;
        a.ref0 = ref0;
        a.dmap = map;
        a.partials = h->partials.as<uint64_t>();
        a.items = g.items;
        a.frame_bytes = (uint32_t)fb;
        a.vec_bytes = (uint32_t)g.vec_bytes;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)g.n_tiles;
        a.n_waves = (uint32_t)g.n_waves;
        a.thr = dips::series_threshold(C, h->p.tau, isi);
        a.part_frames = g.part_frames;  // 0: contiguous ranges (part_geometry)
        if (glut) {
            a.lut = h->gray_lut.p;
            DIPS_HIP(h, dips::launch_series_gray_lut(a, pf, map != nullptr, (uint32_t)g.blocks, s));
        } else {
            DIPS_HIP(h, dips::launch_series_fast(a, C, C == 1 ? 0 : (int)h->p.chroma_filter, pf, map != nullptr,
                                                 (uint32_t)g.blocks, s, align, isi));
        }
        // the ragged tail (< pixels_per_vec pixels per frame): its sums go
        // straight into the series by atomics, so the order is free
        if (g.tail_px0 < npx) {
            st = launch_generic(g.tail_px0);
            if (st != DIPS_OK) return st;
        }
    } else {
        st = launch_generic(0);
        if (st != DIPS_OK) return st;
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    if (g.ok)
        DIPS_HIP(h, dips::launch_series_reduce(h->partials.as<uint64_t>(), n_frames, (uint32_t)g.n_tiles,
                                               C == 1 ? (glut ? 2 : 1) : 0, series, s));
    return DIPS_OK;
}

// Waves of the series launch an aligned batch of this shape runs (0 if the
// shape is not eligible for the fast kernels), with or without the
// DIPS_SERIES_WAVES_PER_SIMD cap.
uint64_t series_waves(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, bool env_cap) {
    const int C = (int)h->p.format;
    FastGeom g = C == 1 && gray_lut_enabled(h)
                     ? gray_lut_geometry(h, width, height, n_frames, env_cap)
                     : fast_geometry(h, width, height, n_frames, C, h->p.mode == DIPS_MODE_PER_FRAME, false, false,
                                     series_isi_form(h), env_cap);
    return g.ok ? g.n_waves : 0;
}

// The series of `n_frames` HOST frames staged through pooled pinned buffers
// and copied to a triple-buffered HBM ring on the side stream, each chunk's
// copy overlapping the previous chunk's series launch (next-1 of SURVEY.md
// s8f); `ref_dev` = the DEVICE reference of the first frame (NULL: overall
// -> the first frame, per-frame -> the first frame itself).  Series into
// the device array `series_dev`, asynchronously on the handle's stream once
// the last chunk is queued (the host frames are all read when it returns).
dips_status run_series_streamed(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* host_frames,
                                uint32_t n_frames, const uint8_t* ref_dev, dips_series_entry* series_dev,
                                uint32_t chunk_frames) {
    if (n_frames == 0) return DIPS_OK;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const size_t fb = (size_t)width * height * (size_t)h->p.format;
    uint32_t chunk = chunk_frames;
    if (chunk == 0) {
        const size_t target = 256u << 20;  // ~256 MiB per DMA chunk
        chunk = (uint32_t)(target / fb);
        if (chunk < 1) chunk = 1;
    }
    if (chunk > n_frames) chunk = n_frames;
    const size_t cbytes = fb * chunk;
    for (auto& r : h->ring) DIPS_HIP(h, r.ensure(cbytes));
    DIPS_HIP(h, h->ring_ref.ensure(fb));
    for (auto& pn : h->pinned) DIPS_HIP(h, pn.ensure(cbytes));
    DIPS_HIP(h, hipStreamSynchronize(h->copy_stream));
    // the ring and the pinned buffers are free once the stream's earlier
    // work (a previous streamed call's kernels) is done
    DIPS_HIP(h, hipStreamSynchronize(h->stream));
    const uint32_t n_chunks = (n_frames + chunk - 1) / chunk;
    for (uint32_t k = 0; k < n_chunks; ++k) {
        const uint32_t b = k % 3u, hb = k % 2u;
        const uint32_t f0 = k * chunk;
        const uint32_t nk = (f0 + chunk <= n_frames) ? chunk : n_frames - f0;
        // pinned[hb] was last read by the DMA of chunk k-2
        if (k >= 2) DIPS_HIP(h, hipEventSynchronize(h->copy_done[(k - 2) % 3u]));
        dips_host::staged_copy(static_cast<uint8_t*>(h->pinned[hb].p), host_frames + (size_t)f0 * fb,
                               (size_t)nk * fb);
        // ring[b] was read by kernel k-3 (frames) and kernel k-2 (per-frame ref)
        if (k >= 2) DIPS_HIP(h, hipStreamWaitEvent(h->copy_stream, h->kernel_done[(k - 2) % 3u], 0));
        // the upload by a copy kernel (1.00-1.15x the DMA engine's rate here)
        DIPS_HIP(h, dips_host::pipe_h2d(h->ring[b].p, h->pinned[hb].p, (size_t)nk * fb, h->copy_stream, true));
        DIPS_HIP(h, hipEventRecord(h->copy_done[b], h->copy_stream));
        DIPS_HIP(h, hipStreamWaitEvent(h->stream, h->copy_done[b], 0));
        const uint8_t* frames_dev = h->ring[b].as<uint8_t>();
        const uint8_t* ref;
        if (pf) {
            if (k == 0) ref = ref_dev ? ref_dev : frames_dev;
            else ref = h->ring[(k - 1) % 3u].as<uint8_t>() + (size_t)(chunk - 1) * fb;
        } else {
            if (k == 0 && !ref_dev)
                DIPS_HIP(h, hipMemcpyAsync(h->ring_ref.p, frames_dev, fb, hipMemcpyDeviceToDevice, h->stream));
            ref = ref_dev ? ref_dev : h->ring_ref.as<uint8_t>();
        }
        dips_status st = run_series_device(h, width, height, frames_dev, nk, ref, series_dev + f0, nullptr, h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipEventRecord(h->kernel_done[b], h->stream));
    }
    return DIPS_OK;
}

}  // namespace dips_internal

namespace {

// ---------------------------------------------------------------------------
// The grid form (dips_diff_series_grid; kernels in series_grid.hip)
// ---------------------------------------------------------------------------

// The grid of a call, validated: nullptr, or why it is refused.
const char* grid_spec(uint32_t width, uint32_t height, const uint32_t* roi, uint32_t rows, uint32_t cols,
                      dips::GridSpec* g) {
    if (width == 0 || height == 0) return "empty frame";
    g->x = roi ? roi[0] : 0u;
    g->y = roi ? roi[1] : 0u;
    g->w = roi ? roi[2] : width;
    g->h = roi ? roi[3] : height;
    g->rows = rows;
    g->cols = cols;
    if (g->w == 0 || g->h == 0) return "the region of interest has zero extent";
    if ((uint64_t)g->x + g->w > width || (uint64_t)g->y + g->h > height)
        return "the region of interest leaves the frame";
    if (rows == 0 || cols == 0) return "rows and cols must be at least 1";
    if (rows > g->h || cols > g->w) return "more rows or cols than the region has pixels (a cell would be empty)";
    return nullptr;
}

struct GridGeom {
    bool ok = false;
    uint32_t tiles_per_cell = 0, part_frames = 0;
    uint64_t n_tiles = 0, n_waves = 0, blocks = 0;
};

// Geometry of the fast grid kernel: every cell owns the tile count of the
// largest cell; a persistent grid of occupancy x CUs waves (fast_geometry's
// sizing), frames cut into parts as part_geometry cuts them, or for batches
// it leaves alone into enough parts of >= 16 frames to give every wave slot
// an item.  Refused (the generic kernel runs): frames of 2^31 bytes or more,
// 2^28 frames, and grids whose records would outweigh the batch -- cells of a
// few pixels, where a 16-byte record per (tile, frame) is most of the traffic.
GridGeom grid_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf, int isi,
                       const dips::GridSpec& g) {
    GridGeom q;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    if (fb >= (1ull << 31) || n_frames == 0 || n_frames >= (1u << 28)) return q;
    const void* k = dips::series_grid_kernel_ptr(C, (int)h->p.chroma_filter, pf, isi);
    if (!k) return q;
    const uint64_t vpt = 64u * (uint64_t)dips::fast_unroll(C);  // vecs per tile
    const uint64_t max_w = ((uint64_t)g.w + g.cols - 1) / g.cols, max_h = ((uint64_t)g.h + g.rows - 1) / g.rows;
    const uint64_t tpc = (((max_w + 3) / 4) * max_h + vpt - 1) / vpt;
    const uint64_t n_cells = (uint64_t)g.rows * g.cols;
    const uint64_t n_tiles = n_cells * tpc;
    if (n_tiles >= (1ull << 31)) return q;
    const uint64_t rec_bytes = n_tiles * n_frames * 16u;
    if (rec_bytes > (64ull << 20) && rec_bytes > fb * n_frames) return q;
    const uint64_t resident = waves_per_simd((uint64_t)occupancy_blocks(h, k), true) * (uint64_t)h->cu_count * 4u;
    if (resident == 0) return q;
    FastGeom f;
    f.n_tiles = n_tiles;
    part_geometry(f, n_frames, resident);
    if (f.part_frames != 0) {
        q.part_frames = f.part_frames;
        q.n_waves = f.n_waves;
    } else {
        const uint64_t want = (resident + n_tiles - 1) / n_tiles;
        const uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>(want, n_frames / 16u));
        q.part_frames = (uint32_t)((n_frames + parts - 1) / parts);
        const uint64_t items = ((n_frames + q.part_frames - 1) / q.part_frames) * n_tiles;
        q.n_waves = std::min(items, resident);
    }
    q.blocks = (q.n_waves + 3) / 4;
    q.tiles_per_cell = (uint32_t)tpc;
    q.n_tiles = n_tiles;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Run the grid series on device pointers, asynchronously on `s`.
dips_status run_grid_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                            const uint8_t* ref0, const dips::GridSpec& g, dips_series_entry* cells, hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    const uint32_t n_cells = g.rows * g.cols;
    const int isi = series_isi_form(h);
    GridGeom q;
    // GRAY8 has no fast grid kernel; DIPS_FLAG_CROSSCHECK asks for the plain one
    if (C != 1 && !(h->p.flags & DIPS_FLAG_FORCE_GENERIC) && !h->crosscheck())
        q = grid_geometry(h, width, height, n_frames, C, pf, isi, g);
    // the cells start at zero: the fast kernel clears them itself (GridArgs::zero)
    if (!q.ok) DIPS_HIP(h, hipMemsetAsync(cells, 0, sizeof(dips_series_entry) * (size_t)n_frames * n_cells, s));
    auto launch_generic = [&](const dips::GridSpec& gs, uint32_t out_base) -> dips_status {
        const uint64_t max_w = ((uint64_t)gs.w + gs.cols - 1) / gs.cols, max_h = ((uint64_t)gs.h + gs.rows - 1) / gs.rows;
        const uint64_t spc = (max_w * max_h + 255u) / 256u;
        if (spc >= (1ull << 32)) return fail(h, DIPS_ERR_INVALID, "diff_series_grid: cell too large for the generic kernel");
        dips::GridGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.cells = cells;
        a.frame_bytes = fb;
        a.width = width;
        a.n_frames = n_frames;
        a.segs_per_cell = (uint32_t)spc;
        a.out_stride = n_cells;
        a.out_base = out_base;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.g = gs;
        DIPS_HIP(h, dips::launch_grid_generic(a, C, s));
        return DIPS_OK;
    };

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    dips::GridArgs a{};
    if (q.ok) {
        DIPS_HIP(h, h->partials.ensure((size_t)q.n_tiles * n_frames * 16u));
        a.frames = frames;
        a.ref0 = ref0;
        a.partials = h->partials.as<uint64_t>();
        a.zero = reinterpret_cast<uint64_t*>(cells);
        a.zero_n = 4u * n_frames * n_cells;
        a.frame_bytes = (uint32_t)fb;
        a.width = width;
        a.n_frames = n_frames;
        a.tiles_per_cell = q.tiles_per_cell;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.part_frames = q.part_frames;
        a.thr = dips::series_threshold(C, h->p.tau, isi);
        a.g = g;
        DIPS_HIP(h, dips::launch_series_grid(a, C, (int)h->p.chroma_filter, pf, isi, (uint32_t)q.blocks, s));
        // the vecs the fast kernel leaves out (series_grid.hip): a partial
        // last vec of a cell row that starts within 3 pixels of the frame's
        // end would read past it.  A full vec ends inside its row, so these
        // lie in the frame's last row, and in frames narrower than 3 pixels
        // in up to three rows before it (run_pixels_device applies the same
        // test).  Their <= 3 pixels go into their cells by atomics (after the
        // kernel's zeroing); cell edges decrease with the column, so at most
        // three cells of a row qualify
        const uint64_t npx = (uint64_t)width * height;
        uint32_t crow = g.rows - 1u;  // the grid row of region row y
        for (uint32_t y = g.y + g.h; y-- > g.y;) {
            if (((uint64_t)y + 1u) * width + 3u <= npx) break;  // every vec of this and the earlier rows fits
            while (dips::grid_cell_rect(g, crow, 0u).y > y) --crow;
            for (uint32_t c = g.cols; c-- > 0;) {
                const dips::GridRect rc = dips::grid_cell_rect(g, crow, c);
                if ((uint64_t)y * width + rc.x + rc.w + 3u <= npx) break;  // so does every vec of the earlier columns
                const uint32_t x0 = rc.x + ((rc.w - 1u) & ~3u);  // the cell row's last vec
                if (rc.w % 4u == 0u || (uint64_t)y * width + x0 + 4u <= npx) continue;
                const dips::GridSpec tail{x0, y, rc.x + rc.w - x0, 1u, 1u, 1u};
                dips_status st = launch_generic(tail, crow * g.cols + c);
                if (st != DIPS_OK) return st;
            }
        }
    } else {
        dips_status st = launch_generic(g, 0u);
        if (st != DIPS_OK) return st;
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    if (q.ok) DIPS_HIP(h, dips::launch_grid_reduce(a, C, cells, s));
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The per-pixel sums over time (dips_diff_pixel_sums; kernels in
// series_pixels.hip)
// ---------------------------------------------------------------------------

struct PixGeom {
    bool ok = false;
    uint32_t part_frames = 0, parts = 0;
    uint64_t n_tiles = 0, n_waves = 0, blocks = 0;
};

// Geometry of the fast per-pixel kernel: a persistent grid of occupancy x CUs
// waves over items (frame part, tile).  One part -- every wave owns all
// frames of its pixels and stores their entries -- unless the tiles are too
// few to give every wave slot an item (then enough parts of >= 16 frames to
// do so) or the batch exceeds the kPixMaxPart frames the in-register
// accumulators hold; the parts then add their shares with atomics.  Refused
// (the generic kernel runs): frames of 2^31 bytes or more, 2^28 frames.
PixGeom pix_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf, int isi,
                     const dips::GridSpec& g) {
    PixGeom q;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    if (fb >= (1ull << 31) || n_frames == 0 || n_frames >= (1u << 28)) return q;
    const void* k = dips::series_pixels_kernel_ptr(C, (int)h->p.chroma_filter, pf, isi);
    if (!k) return q;
    const uint64_t vpt = 64u * (uint64_t)dips::kUnrollPix;  // vecs per tile
    const uint64_t n_tiles = ((((uint64_t)g.w + 3) / 4) * g.h + vpt - 1) / vpt;
    const uint64_t resident = waves_per_simd((uint64_t)occupancy_blocks(h, k), true) * (uint64_t)h->cu_count * 4u;
    if (resident == 0 || n_tiles == 0 || n_tiles >= (1ull << 31)) return q;
    // tiles that fill 98 % of the slots are left in one part (part_geometry's
    // fill rule): a second part would buy 2 % and cost the memset and atomics
    const uint64_t want = n_tiles * 100u >= resident * 98u ? 1u : (resident + n_tiles - 1) / n_tiles;
    uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>(want, n_frames / 16u));
    parts = std::max<uint64_t>(parts, ((uint64_t)n_frames + dips::kPixMaxPart - 1) / dips::kPixMaxPart);
    q.part_frames = (uint32_t)((n_frames + parts - 1) / parts);
    // DIPS_PIXEL_PART_FRAMES = 1 .. kPixMaxPart pins the part length (the
    // tests run the accumulators at their limit on a small frame with it)
    if (const char* pin = std::getenv("DIPS_PIXEL_PART_FRAMES")) {
        const unsigned long L = std::strtoul(pin, nullptr, 10);
        if (L >= 1 && L <= dips::kPixMaxPart) q.part_frames = (uint32_t)std::min<uint64_t>(L, n_frames);
    }
    q.parts = (uint32_t)((n_frames + q.part_frames - 1) / q.part_frames);
    q.n_tiles = n_tiles;
    q.n_waves = std::min((uint64_t)q.parts * n_tiles, resident);
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Run the per-pixel sums on device pointers, asynchronously on `s`.
dips_status run_pixels_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                              const uint8_t* ref0, const dips::GridSpec& g, bool accumulate, dips_series_entry* sums,
                              hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    const int isi = series_isi_form(h);
    PixGeom q;
    // GRAY8 has no fast form; DIPS_FLAG_CROSSCHECK asks for the plain kernel
    if (C != 1 && !(h->p.flags & DIPS_FLAG_FORCE_GENERIC) && !h->crosscheck())
        q = pix_geometry(h, width, height, n_frames, C, pf, isi, g);
    auto launch_generic = [&](const dips::GridRect& rect) -> dips_status {
        dips::PixGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.sums = sums;
        a.frame_bytes = fb;
        a.width = width;
        a.n_frames = n_frames;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.accumulate = accumulate ? 1u : 0u;
        a.roi_x = g.x;
        a.roi_y = g.y;
        a.roi_w = g.w;
        a.rect = rect;
        DIPS_HIP(h, dips::launch_pixels_generic(a, C, s));
        return DIPS_OK;
    };

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    if (q.ok) {
        // several parts add with atomics: the map is zeroed in this earlier
        // launch (waves of one launch are not ordered against each other)
        if (q.parts > 1 && !accumulate)
            DIPS_HIP(h, hipMemsetAsync(sums, 0, sizeof(dips_series_entry) * (size_t)g.w * g.h, s));
        dips::PixArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.sums = sums;
        a.frame_bytes = (uint32_t)fb;
        a.width = width;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.part_frames = q.part_frames;
        a.out_mode = q.parts > 1 ? 2u : (accumulate ? 1u : 0u);
        a.thr = dips::series_threshold(C, h->p.tau, isi);
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_series_pixels(a, C, (int)h->p.chroma_filter, pf, isi, (uint32_t)q.blocks, s));
        // the vecs the fast kernel leaves out (series_pixels.hip): those that
        // would read past the frame's end, i.e. that start within 3 pixels of
        // it.  Vecs of a row are 4 pixels apart and a full vec ends inside its
        // row, so that is at most the partial last vec of each of the region's
        // last rows: one row for frames 3 or more pixels wide, up to 4 for
        // narrower ones.  Their <= 3 pixels each are nobody else's
        if (g.w % 4u != 0u) {
            const uint32_t x0 = g.x + ((g.w - 1u) & ~3u);  // the last vec of a region row
            const uint64_t npx = (uint64_t)width * height;
            for (uint32_t r = g.h; r-- > 0 && g.h - r <= 4u;) {
                if ((uint64_t)(g.y + r) * width + x0 + 4u <= npx) break;  // it and every earlier row fit
                dips_status st = launch_generic(dips::GridRect{x0, g.y + r, g.x + g.w - x0, 1u});
                if (st != DIPS_OK) return st;
            }
        }
    } else {
        dips_status st = launch_generic(dips::GridRect{g.x, g.y, g.w, g.h});
        if (st != DIPS_OK) return st;
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The per-frame change mask (dips_diff_change_mask; kernels in
// series_mask.hip)
// ---------------------------------------------------------------------------

uint64_t mask_words_per_row(uint32_t roi_w) { return ((uint64_t)roi_w + 31u) / 32u; }

struct MaskGeom {
    bool ok = false;
    uint32_t part_frames = 0, parts = 0;
    uint64_t n_tiles = 0, n_waves = 0, blocks = 0;
};

// Geometry of the fast mask kernel: a persistent grid of occupancy x CUs
// waves over items (frame part, tile), a tile = 64 * kUnrollMask vecs of the
// region rows padded to whole mask words.  Parts as the grid cuts them: as
// part_geometry cuts them, or for the batches it leaves alone as many parts
// of >= 16 frames as give every wave slot an item; no upper cap on a part
// (nothing is accumulated), and every word has one writer whatever the part
// count.  Refused
// (the generic kernel runs): frames of 2^31 bytes or more, 2^28 frames,
// regions whose padded rows hold 2^31 vecs or more.
MaskGeom mask_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf,
                       const dips::GridSpec& g) {
    MaskGeom q;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    if (fb >= (1ull << 31) || n_frames == 0 || n_frames >= (1u << 28)) return q;
    const void* k = dips::series_mask_kernel_ptr(C, (int)h->p.chroma_filter, pf);
    if (!k) return q;
    const uint64_t vpt = 64u * (uint64_t)dips::kUnrollMask;  // vecs per tile
    const uint64_t nvec8 = 8u * mask_words_per_row(g.w) * g.h;
    if (nvec8 >= (1ull << 31)) return q;
    const uint64_t n_tiles = (nvec8 + vpt - 1) / vpt;
    const uint64_t resident = waves_per_simd((uint64_t)occupancy_blocks(h, k), true) * (uint64_t)h->cu_count * 4u;
    if (resident == 0 || n_tiles == 0) return q;
    FastGeom f;
    f.n_tiles = n_tiles;
    part_geometry(f, n_frames, resident);
    if (f.part_frames != 0) {
        q.part_frames = f.part_frames;
        q.parts = (uint32_t)((n_frames + q.part_frames - 1) / q.part_frames);
        q.n_waves = f.n_waves;
    } else {
        const uint64_t want = (resident + n_tiles - 1) / n_tiles;
        const uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>(want, n_frames / 16u));
        q.part_frames = (uint32_t)((n_frames + parts - 1) / parts);
        q.parts = (uint32_t)((n_frames + q.part_frames - 1) / q.part_frames);
        q.n_waves = std::min((uint64_t)q.parts * n_tiles, resident);
    }
    q.n_tiles = n_tiles;
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Run the change mask on device pointers, asynchronously on `s`.
dips_status run_mask_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                            const uint8_t* ref0, const dips::GridSpec& g, uint8_t* mask, hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    const uint64_t wpr = mask_words_per_row(g.w);
    const uint64_t mfb = wpr * g.h * 4u;
    MaskGeom q;
    // GRAY8 has no fast form; DIPS_FLAG_CROSSCHECK asks for the plain kernel
    if (C != 1 && !(h->p.flags & DIPS_FLAG_FORCE_GENERIC) && !h->crosscheck())
        q = mask_geometry(h, width, height, n_frames, C, pf, g);
    auto launch_generic = [&](uint32_t row0, uint32_t n_rows, uint32_t word0, uint32_t n_words) -> dips_status {
        dips::MaskGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.mask = mask;
        a.frame_bytes = fb;
        a.mask_frame_bytes = mfb;
        a.width = width;
        a.t0 = 0u;
        a.n_frames = n_frames;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.row0 = row0;
        a.n_rows = n_rows;
        a.word0 = word0;
        a.n_words = n_words;
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_mask_generic(a, C, s));
        return DIPS_OK;
    };

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    if (q.ok) {
        dips::MaskArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.mask = mask;
        a.frame_bytes = (uint32_t)fb;
        a.mask_frame_bytes = (uint32_t)mfb;
        a.width = width;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.part_frames = q.part_frames;
        a.thr = dips::series_threshold(C, h->p.tau, 0);
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_series_mask(a, C, (int)h->p.chroma_filter, pf, (uint32_t)q.blocks, s));
        // the vecs the fast kernel leaves out (series_mask.hip): those that
        // would read past the frame's end, i.e. the partial last vec of the
        // region's last rows where it starts within 3 pixels of the frame's
        // end (run_pixels_device's test): one row for frames 3 or more pixels
        // wide, up to 4 for narrower ones.  The fast kernel stored the word
        // that holds such a vec with zeros in its place; this later launch
        // recomputes and stores the whole word, so no two launches race for
        // it and nothing is ORed into memory
        if (g.w % 4u != 0u) {
            const uint32_t x0 = g.x + ((g.w - 1u) & ~3u);  // the last vec of a region row
            const uint64_t npx = (uint64_t)width * height;
            for (uint32_t r = g.h; r-- > 0 && g.h - r <= 4u;) {
                if ((uint64_t)(g.y + r) * width + x0 + 4u <= npx) break;  // it and every earlier row fit
                dips_status st = launch_generic(r, 1u, (g.w - 1u) >> 5, 1u);
                if (st != DIPS_OK) return st;
            }
        }
    } else {
        if ((uint64_t)g.h * wpr >= (1ull << 31))
            return fail(h, DIPS_ERR_INVALID, "diff_change_mask: region too large for the generic kernel");
        dips_status st = launch_generic(0u, g.h, 0u, (uint32_t)wpr);
        if (st != DIPS_OK) return st;
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The running-average background and its change mask
// (dips_diff_background_mask; kernels in series_background.hip)
// ---------------------------------------------------------------------------

struct BgGeom {
    bool ok = false;
    bool small_tile = false;
    uint64_t n_tiles = 0, n_waves = 0, blocks = 0;
};

// Geometry of the fast background kernel: a persistent grid of occupancy x
// CUs waves over the tiles of the region rows padded to whole mask words.
// One part always (the recurrence is sequential in t), so tiles are the only
// parallelism: a region whose tiles of 64 * kUnrollBackground vecs would fill
// under half of the wave slots takes tiles of 64 vecs instead.  (Choosing the
// tile by how full the rounds of resident waves are -- 4K RGB8: 16,200 small
// tiles fill two rounds to 98.9 %, 8,100 large ones to 56.5 % -- measured 3-5 %
// slower at 4K than this rule, DESIGN.md.)  Refused (the
// generic kernel runs): frames of 2^31 bytes or more, 2^28 frames, regions
// whose padded rows hold 2^31 vecs or more.
// `kernel_ptr` / `unroll`: the kernel family and its vecs per lane (the
// Sigma-Delta model shares the schedule, sigma_delta_geometry).
BgGeom background_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C,
                           const dips::GridSpec& g,
                           const void* (*kernel_ptr)(int, int, bool) = dips::series_background_kernel_ptr,
                           int unroll = dips::kUnrollBackground) {
    BgGeom q;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    if (fb >= (1ull << 31) || n_frames == 0 || n_frames >= (1u << 28)) return q;
    const uint64_t nvec8 = 8u * mask_words_per_row(g.w) * g.h;
    if (nvec8 == 0 || nvec8 >= (1ull << 31)) return q;
    auto resident_of = [&](bool small_tile) -> uint64_t {
        const void* k = kernel_ptr(C, (int)h->p.chroma_filter, small_tile);
        if (!k) return 0;
        return waves_per_simd((uint64_t)occupancy_blocks(h, k), true) * (uint64_t)h->cu_count * 4u;
    };
    uint64_t vpt = 64u * (uint64_t)unroll;  // vecs per tile
    uint64_t resident = resident_of(false);
    if (resident == 0) return q;
    if (unroll > 1 && 2u * ((nvec8 + vpt - 1) / vpt) < resident) {
        q.small_tile = true;
        vpt = 64u;
        resident = resident_of(true);
        if (resident == 0) return q;
    }
    q.n_tiles = (nvec8 + vpt - 1) / vpt;
    q.n_waves = std::min(q.n_tiles, resident);
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Run the background model on device pointers, asynchronously on `s`.  ref0:
// the initial state's bytes (accumulate false), else unused.  n_frames may be
// 0 (accumulate false: the initial state is written).
dips_status run_background_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                  uint32_t n_frames, const uint8_t* ref0, const dips::GridSpec& g, uint32_t rate_shift,
                                  bool selective, bool accumulate, uint16_t* background, uint8_t* mask, hipStream_t s) {
    const int C = (int)h->p.format;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    const uint64_t wpr = mask_words_per_row(g.w);
    const uint64_t mfb = wpr * g.h * 4u;
    BgGeom q;
    // GRAY8 has no fast form; DIPS_FLAG_CROSSCHECK asks for the plain kernel
    if (C != 1 && !(h->p.flags & DIPS_FLAG_FORCE_GENERIC) && !h->crosscheck())
        q = background_geometry(h, width, height, n_frames, C, g);
    auto launch_generic = [&](uint32_t row0, uint32_t n_rows, uint32_t word0, uint32_t n_words,
                              uint32_t state_x0) -> dips_status {
        dips::BgGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.background = background;
        a.mask = mask;
        a.frame_bytes = fb;
        a.mask_frame_bytes = mfb;
        a.width = width;
        a.n_frames = n_frames;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.rate_shift = rate_shift;
        a.selective = selective ? 1u : 0u;
        a.accumulate = accumulate ? 1u : 0u;
        a.row0 = row0;
        a.n_rows = n_rows;
        a.word0 = word0;
        a.n_words = n_words;
        a.state_x0 = state_x0;
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_background_generic(a, C, s));
        return DIPS_OK;
    };

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    if (q.ok) {
        // the vecs the fast kernel leaves out (series_background.hip): those
        // that would read past the frame's end, i.e. the partial last vec of
        // the region's last rows (run_mask_device's test).  The generic
        // kernel computes the whole mask word that holds such a vec and the
        // state of the vec's pixels BEFORE the fast kernel runs: it starts
        // every pixel of the word from its initial state, which an
        // accumulating call keeps in the buffer the fast kernel overwrites.
        // The fast kernel stores neither that word nor those pixels' state,
        // so each word and each state value has one writer
        if (g.w % 4u != 0u) {
            const uint32_t i0 = (g.w - 1u) & ~3u;  // the last vec of a region row
            const uint64_t npx = (uint64_t)width * height;
            for (uint32_t r = g.h; r-- > 0 && g.h - r <= 4u;) {
                if ((uint64_t)(g.y + r) * width + g.x + i0 + 4u <= npx) break;  // it and every earlier row fit
                dips_status st = launch_generic(r, 1u, (g.w - 1u) >> 5, 1u, i0);
                if (st != DIPS_OK) return st;
            }
        }
        dips::BgArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.background = background;
        a.mask = mask;
        a.frame_bytes = (uint32_t)fb;
        a.mask_frame_bytes = (uint32_t)mfb;
        a.width = width;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.rate_shift = rate_shift;
        a.selective = selective ? 1u : 0u;
        a.accumulate = accumulate ? 1u : 0u;
        a.thr = dips::series_threshold(C, h->p.tau, 0);
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_series_background(a, C, (int)h->p.chroma_filter, q.small_tile, (uint32_t)q.blocks, s));
    } else {
        if ((uint64_t)g.h * wpr >= (1ull << 31))
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: region too large for the generic kernel");
        dips_status st = launch_generic(0u, g.h, 0u, (uint32_t)wpr, 0u);
        if (st != DIPS_OK) return st;
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The Sigma-Delta background and its per-pixel adaptive threshold mask
// (dips_diff_sigma_delta_mask; kernels in series_sigma_delta.hip)
// ---------------------------------------------------------------------------

// Run the Sigma-Delta model on device pointers, asynchronously on `s`: the
// schedule of run_background_device (background_geometry with this kernel
// family and its vecs per lane; the generic kernel first for the words whose
// vecs the fast kernel leaves out).  ref0: the frame the initial M is taken
// from (accumulate false), else unused.  n_frames may be 0 (accumulate false:
// the initial state is written).
dips_status run_sigma_delta_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                   uint32_t n_frames, const uint8_t* ref0, const dips::GridSpec& g, uint32_t n_amp,
                                   uint32_t v_min, uint32_t v_max, bool accumulate, uint16_t* state, uint8_t* mask,
                                   hipStream_t s) {
    const int C = (int)h->p.format;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    const uint64_t wpr = mask_words_per_row(g.w);
    const uint64_t mfb = wpr * g.h * 4u;
    BgGeom q;
    // GRAY8 has no fast form; DIPS_FLAG_CROSSCHECK asks for the plain kernel
    if (C != 1 && !(h->p.flags & DIPS_FLAG_FORCE_GENERIC) && !h->crosscheck())
        q = background_geometry(h, width, height, n_frames, C, g, dips::series_sigma_delta_kernel_ptr,
                                dips::kUnrollSigmaDelta);
    auto launch_generic = [&](uint32_t row0, uint32_t n_rows, uint32_t word0, uint32_t n_words,
                              uint32_t state_x0) -> dips_status {
        dips::SdGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.state = state;
        a.mask = mask;
        a.frame_bytes = fb;
        a.mask_frame_bytes = mfb;
        a.width = width;
        a.n_frames = n_frames;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.n_amp = n_amp;
        a.v_min = v_min;
        a.v_max = v_max;
        a.accumulate = accumulate ? 1u : 0u;
        a.row0 = row0;
        a.n_rows = n_rows;
        a.word0 = word0;
        a.n_words = n_words;
        a.state_x0 = state_x0;
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_sigma_delta_generic(a, C, s));
        return DIPS_OK;
    };

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    if (q.ok) {
        // the partial last vec of the region's last rows that would read past
        // the frame's end: its whole mask word and its pixels' state come
        // from the generic kernel, launched BEFORE the fast kernel overwrites
        // the state an accumulating call continues (run_background_device)
        if (g.w % 4u != 0u) {
            const uint32_t i0 = (g.w - 1u) & ~3u;  // the last vec of a region row
            const uint64_t npx = (uint64_t)width * height;
            for (uint32_t r = g.h; r-- > 0 && g.h - r <= 4u;) {
                if ((uint64_t)(g.y + r) * width + g.x + i0 + 4u <= npx) break;  // it and every earlier row fit
                dips_status st = launch_generic(r, 1u, (g.w - 1u) >> 5, 1u, i0);
                if (st != DIPS_OK) return st;
            }
        }
        dips::SdArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.state = state;
        a.mask = mask;
        a.frame_bytes = (uint32_t)fb;
        a.mask_frame_bytes = (uint32_t)mfb;
        a.width = width;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.n_amp = n_amp;
        a.v_min = v_min;
        a.v_max = v_max;
        a.accumulate = accumulate ? 1u : 0u;
        a.roi = dips::GridRect{g.x, g.y, g.w, g.h};
        DIPS_HIP(h, dips::launch_series_sigma_delta(a, C, (int)h->p.chroma_filter, q.small_tile, (uint32_t)q.blocks, s));
    } else {
        if ((uint64_t)g.h * wpr >= (1ull << 31))
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: region too large for the generic kernel");
        dips_status st = launch_generic(0u, g.h, 0u, (uint32_t)wpr, 0u);
        if (st != DIPS_OK) return st;
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The change times per pixel (dips_diff_pixel_times; kernels in
// series_times.hip)
// ---------------------------------------------------------------------------

struct TimesGeom {
    bool ok = false;
    uint32_t part_frames = 0, parts = 0;
    uint64_t n_tiles = 0, n_waves = 0, blocks = 0;
};

// Geometry of the fast change-times kernel: pix_geometry's -- a persistent
// grid of occupancy x CUs waves over items (frame part, tile), one part
// unless the tiles fill less than 98 % of the wave slots, then enough parts
// of >= 16 frames to give every slot an item -- without a cap on the frames
// of a part (the state is u32 indices and run lengths, nothing overflows),
// and with the parts limited to what keeps their summaries (20 bytes per
// pixel and part) within kTimesPartsBytes.  DIPS_PIXEL_PART_FRAMES pins the
// part length as it does there.  Refused (the generic kernel runs): frames of
// 2^31 bytes or more, 2^28 frames.
constexpr uint64_t kTimesPartsBytes = 1ull << 30;

TimesGeom times_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames, int C, bool pf,
                         const dips::GridSpec& g) {
    TimesGeom q;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    if (fb >= (1ull << 31) || n_frames == 0 || n_frames >= (1u << 28)) return q;
    const uint64_t vpt = 64u * (uint64_t)dips::kUnrollTimes;  // vecs per tile
    const uint64_t n_tiles = ((((uint64_t)g.w + 3) / 4) * g.h + vpt - 1) / vpt;
    if (n_tiles == 0 || n_tiles >= (1ull << 31)) return q;
    const uint64_t sum_bytes = 20u * (uint64_t)g.w * g.h;  // one part's summaries
    const uint64_t max_parts = std::max<uint64_t>(1, kTimesPartsBytes / sum_bytes);
    // the slots of the several-parts form (its fifth register per pixel may
    // cost it occupancy): that is the form the parts would run
    const void* kp = dips::series_times_kernel_ptr(C, (int)h->p.chroma_filter, pf, true);
    if (!kp) return q;
    const uint64_t res_p = waves_per_simd((uint64_t)occupancy_blocks(h, kp), true) * (uint64_t)h->cu_count * 4u;
    if (res_p == 0) return q;
    const uint64_t want = n_tiles * 100u >= res_p * 98u ? 1u : (res_p + n_tiles - 1) / n_tiles;
    const uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>(std::min(want, max_parts), n_frames / 16u));
    q.part_frames = (uint32_t)((n_frames + parts - 1) / parts);
    if (const char* pin = std::getenv("DIPS_PIXEL_PART_FRAMES")) {
        const unsigned long L = std::strtoul(pin, nullptr, 10);
        if (L >= 1 && ((uint64_t)n_frames + L - 1) / L <= max_parts)
            q.part_frames = (uint32_t)std::min<uint64_t>(L, n_frames);
    }
    q.parts = (uint32_t)((n_frames + q.part_frames - 1) / q.part_frames);
    const void* k = dips::series_times_kernel_ptr(C, (int)h->p.chroma_filter, pf, q.parts > 1);
    if (!k) return q;
    const uint64_t resident = waves_per_simd((uint64_t)occupancy_blocks(h, k), true) * (uint64_t)h->cu_count * 4u;
    if (resident == 0) return q;
    q.n_tiles = n_tiles;
    q.n_waves = std::min((uint64_t)q.parts * n_tiles, resident);
    q.blocks = (q.n_waves + 3) / 4;
    q.ok = q.blocks < (1ull << 31);
    return q;
}

// Run the change times on device pointers, asynchronously on `s`.
dips_status run_times_device(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames, uint32_t n_frames,
                             const uint8_t* ref0, const dips::GridSpec& g, uint32_t t0, bool accumulate,
                             uint32_t* times, hipStream_t s) {
    const int C = (int)h->p.format;
    const bool pf = h->p.mode == DIPS_MODE_PER_FRAME;
    const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
    const dips::GridRect roi{g.x, g.y, g.w, g.h};
    TimesGeom q;
    // GRAY8 has no fast form; DIPS_FLAG_CROSSCHECK asks for the plain kernel
    if (C != 1 && !(h->p.flags & DIPS_FLAG_FORCE_GENERIC) && !h->crosscheck())
        q = times_geometry(h, width, height, n_frames, C, pf, g);
    auto launch_generic = [&](const dips::GridRect& rect) -> dips_status {
        dips::TimesGenericArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.times = times;
        a.frame_bytes = fb;
        a.width = width;
        a.n_frames = n_frames;
        a.mode = h->p.mode;
        a.chroma = C == 1 ? 0u : h->p.chroma_filter;
        a.tau = h->p.tau;
        a.t0 = t0;
        a.accumulate = accumulate ? 1u : 0u;
        a.roi = roi;
        a.rect = rect;
        DIPS_HIP(h, dips::launch_times_generic(a, C, s));
        return DIPS_OK;
    };
    // the summaries' buffer before the timed span (growing it synchronises)
    if (q.ok && q.parts > 1) DIPS_HIP(h, h->times_parts.ensure((size_t)q.parts * 20u * (size_t)g.w * g.h));

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    if (q.ok) {
        const bool mp = q.parts > 1;
        dips::TimesArgs a{};
        a.frames = frames;
        a.ref0 = ref0;
        a.out = mp ? h->times_parts.as<uint32_t>() : times;
        a.frame_bytes = (uint32_t)fb;
        a.width = width;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)q.n_tiles;
        a.n_waves = (uint32_t)q.n_waves;
        a.part_frames = q.part_frames;
        a.t0 = t0;
        a.accumulate = !mp && accumulate ? 1u : 0u;
        a.thr = dips::series_threshold(C, h->p.tau, 0);
        a.roi = roi;
        DIPS_HIP(h, dips::launch_series_times(a, C, (int)h->p.chroma_filter, pf, mp, (uint32_t)q.blocks, s));
        if (mp) {
            // the parts in order onto the initial or accumulated state: a
            // later launch, so every summary is written before it is read
            dips::TimesCombineArgs c{};
            c.parts = h->times_parts.as<uint32_t>();
            c.times = times;
            c.frame_bytes = (uint32_t)fb;
            c.width = width;
            c.channels = (uint32_t)C;
            c.n_frames = n_frames;
            c.part_frames = q.part_frames;
            c.accumulate = accumulate ? 1u : 0u;
            c.roi = roi;
            DIPS_HIP(h, dips::launch_times_combine(c, s));
        }
        // the vecs the fast kernel leaves out (series_times.hip): those that
        // would read past the frame's end (run_pixels_device's test): the
        // partial last vec of the region's last rows, one row for frames 3 or
        // more pixels wide, up to 4 for narrower ones.  Neither the fast
        // kernel nor the combine touches their <= 3 pixels each
        if (g.w % 4u != 0u) {
            const uint32_t x0 = g.x + ((g.w - 1u) & ~3u);  // the last vec of a region row
            const uint64_t npx = (uint64_t)width * height;
            for (uint32_t r = g.h; r-- > 0 && g.h - r <= 4u;) {
                if ((uint64_t)(g.y + r) * width + x0 + 4u <= npx) break;  // it and every earlier row fit
                dips_status st = launch_generic(dips::GridRect{x0, g.y + r, g.x + g.w - x0, 1u});
                if (st != DIPS_OK) return st;
            }
        }
    } else {
        dips_status st = launch_generic(roi);
        if (st != DIPS_OK) return st;
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The connected components of a mask (dips_mask_components; kernels in
// mask_components.hip)
// ---------------------------------------------------------------------------

constexpr size_t kComponentsScratchBytes = (size_t)1 << 30;  // chunk_frames = 0 stays within this

// Label the frames of a device mask, asynchronously on `s`, `chunk` frames
// per round (0: automatic) in the handle's scratch.
dips_status run_components_device(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t w, uint32_t hgt,
                                  uint32_t connectivity, uint32_t min_area, uint32_t max_boxes, uint32_t chunk,
                                  uint32_t* counts, uint32_t* boxes, uint32_t* labels, hipStream_t s) {
    dips::ComponentsArgs a{};
    a.w = w;
    a.h = hgt;
    a.npx = w * hgt;
    a.wpr = (uint32_t)mask_words_per_row(w);
    a.hw = (w + 1u) / 2u;
    a.nslots = a.hw * hgt;
    a.wpf = a.wpr * hgt;
    a.bpf = (a.wpf + 255u) / 256u;
    a.connectivity = connectivity;
    a.min_area = min_area;
    a.max_boxes = max_boxes;
    // per frame: parent, six statistics (two of 8 bytes) per slot, the block sums
    const size_t per_frame = 4u * (size_t)a.npx + 32u * (size_t)a.nslots + 4u * (size_t)a.bpf;
    uint64_t frames = chunk ? chunk : std::max<uint64_t>(1u, kComponentsScratchBytes / per_frame);
    frames = std::min<uint64_t>(frames, n_frames);
    frames = std::min<uint64_t>(frames, std::max<uint64_t>(1u, (1u << 25) / a.bpf));  // the launches' block counts
    const uint32_t F = (uint32_t)frames;
    // the scratch before the timed span (growing it synchronises)
    DIPS_HIP(h, h->cc_scratch.ensure(per_frame * F));
    uint8_t* base = h->cc_scratch.as<uint8_t>();
    a.sum_i = reinterpret_cast<uint64_t*>(base);
    a.sum_j = a.sum_i + (size_t)F * a.nslots;
    a.area = reinterpret_cast<uint32_t*>(a.sum_j + (size_t)F * a.nslots);
    a.min_x = a.area + (size_t)F * a.nslots;
    a.max_x = a.min_x + (size_t)F * a.nslots;
    a.max_y = a.max_x + (size_t)F * a.nslots;
    a.parent = a.max_y + (size_t)F * a.nslots;
    a.block_count = a.parent + (size_t)F * a.npx;

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    // the records no component fills are zeros
    if (max_boxes != 0u)
        DIPS_HIP(h, hipMemsetAsync(boxes, 0, sizeof(uint32_t) * DIPS_BOX_WORDS * (size_t)n_frames * max_boxes, s));
    const size_t frame_words = (size_t)a.wpf;
    for (uint32_t t = 0; t < n_frames; t += F) {
        a.n_frames = std::min(F, n_frames - t);
        a.mask = reinterpret_cast<const uint32_t*>(mask) + (size_t)t * frame_words;
        a.counts = counts + t;
        a.boxes = max_boxes != 0u ? boxes + (size_t)t * max_boxes * DIPS_BOX_WORDS : nullptr;
        a.labels = labels ? labels + (size_t)t * a.npx : nullptr;
        DIPS_HIP(h, dips::launch_mask_components(a, s));
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The components of a mask linked across frames (dips_mask_tracks; kernels in
// mask_components.hip and mask_tracks.hip)
// ---------------------------------------------------------------------------

// tr_ids_kernel walks a chain back to the chunk's first frame at most: the
// cap keeps that walk, one dependent load per frame, short whatever the clip
constexpr uint32_t kTracksChunkFrames = 256;

// Label and link the frames of a device mask, asynchronously on `s`, `chunk`
// frames per round (0: automatic) in the handle's scratch.  The parent and
// label planes have one more frame in front, the predecessor of the chunk's
// first frame: prev_mask is labelled into it, and what the runs of a chunk's
// last frame own is copied there for the next chunk.  The next id and the last frame's tracks
// and ages stay in the scratch from chunk to chunk (two buffers, swapped) and
// move from and to `state` by copies in the stream.
dips_status run_tracks_device(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t w, uint32_t hgt,
                              uint32_t connectivity, uint32_t min_area, uint32_t K, uint32_t chunk,
                              const uint8_t* prev_mask, uint32_t* state, uint32_t* counts, uint32_t* boxes,
                              uint32_t* links, hipStream_t s) {
    dips::ComponentsArgs a{};
    a.w = w;
    a.h = hgt;
    a.npx = w * hgt;
    a.wpr = (uint32_t)mask_words_per_row(w);
    a.hw = (w + 1u) / 2u;
    a.nslots = a.hw * hgt;
    a.wpf = a.wpr * hgt;
    a.bpf = (a.wpf + 255u) / 256u;
    a.connectivity = connectivity;
    a.min_area = min_area;
    // per frame: the labelling's share, the overlap table, cprev and hrank, heads and base;
    // once: the plane in front of parent and of the labels, next id, a count, two carries
    const size_t per_frame =
        4u * (size_t)a.npx + 32u * (size_t)a.nslots + 4u * (size_t)a.bpf + 4u * (size_t)K * K + 8u * (size_t)K + 8u;
    const size_t fixed = 4u * (size_t)a.npx + 4u * (size_t)a.nslots + 16u * (size_t)K + 8u;
    uint64_t frames =
        chunk ? chunk
              : std::max<uint64_t>(1u, (kComponentsScratchBytes - std::min(fixed, kComponentsScratchBytes)) / per_frame);
    frames = std::min<uint64_t>(frames, n_frames);
    frames = std::min<uint64_t>(frames, std::max<uint64_t>(1u, (1u << 25) / a.bpf));  // the launches' block counts
    frames = std::min<uint64_t>(frames, kTracksChunkFrames);
    const uint32_t F = (uint32_t)frames;
    DIPS_HIP(h, h->cc_scratch.ensure(per_frame * F + fixed));
    uint8_t* base = h->cc_scratch.as<uint8_t>();
    a.sum_i = reinterpret_cast<uint64_t*>(base);
    a.sum_j = a.sum_i + (size_t)F * a.nslots;
    uint32_t* label0 = reinterpret_cast<uint32_t*>(a.sum_j + (size_t)F * a.nslots);  // F + 1 planes
    a.area = label0 + a.nslots;
    a.min_x = a.area + (size_t)F * a.nslots;
    a.max_x = a.min_x + (size_t)F * a.nslots;
    a.max_y = a.max_x + (size_t)F * a.nslots;
    uint32_t* parent0 = a.max_y + (size_t)F * a.nslots;  // F + 1 planes
    a.parent = parent0 + a.npx;
    a.block_count = a.parent + (size_t)F * a.npx;

    dips::TracksArgs tr{};
    tr.parent = parent0;
    tr.label = label0;
    tr.ov = a.block_count + (size_t)F * a.bpf;
    tr.cprev = tr.ov + (size_t)F * K * K;
    tr.hrank = tr.cprev + (size_t)F * K;
    tr.heads = tr.hrank + (size_t)F * K;
    tr.base = tr.heads + F;
    tr.next_id = tr.base + F;
    uint32_t* prev_count = tr.next_id + 1;
    uint32_t* carry[2] = {prev_count + 1, prev_count + 1 + 2u * (size_t)K};
    tr.w = a.w;
    tr.h = a.h;
    tr.npx = a.npx;
    tr.wpr = a.wpr;
    tr.hw = a.hw;
    tr.nslots = a.nslots;
    tr.wpf = a.wpf;
    tr.bpf = a.bpf;
    tr.K = K;

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    const size_t frame_words = (size_t)a.wpf;
    if (state)
        DIPS_HIP(h, hipMemcpyAsync(tr.next_id, state, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    else
        DIPS_HIP(h, hipMemsetAsync(tr.next_id, 0, sizeof(uint32_t), s));
    if (prev_mask) {
        DIPS_HIP(h, hipMemcpyAsync(carry[0], state + 1, sizeof(uint32_t) * 2u * K, hipMemcpyDeviceToDevice, s));
        // the same labels as the call that held this frame gave it: they do not depend on max_boxes
        a.n_frames = 1;
        a.mask = reinterpret_cast<const uint32_t*>(prev_mask);
        a.counts = prev_count;
        a.boxes = nullptr;
        a.max_boxes = 0;
        DIPS_HIP(h, dips::launch_mask_components(a, s));
        DIPS_HIP(h, dips::launch_mask_tracks_keep(tr, a.mask, 1u, s));
    }
    a.max_boxes = K;
    // the records no component fills are zeros
    DIPS_HIP(h, hipMemsetAsync(boxes, 0, sizeof(uint32_t) * DIPS_BOX_WORDS * (size_t)n_frames * K, s));
    tr.prev0 = reinterpret_cast<const uint32_t*>(prev_mask);
    uint32_t cin = 0;
    for (uint32_t t = 0; t < n_frames; t += F) {
        const uint32_t n = std::min(F, n_frames - t);
        a.n_frames = n;
        a.mask = reinterpret_cast<const uint32_t*>(mask) + (size_t)t * frame_words;
        a.counts = counts + t;
        a.boxes = boxes + (size_t)t * K * DIPS_BOX_WORDS;
        DIPS_HIP(h, dips::launch_mask_components(a, s));
        tr.n_frames = n;
        tr.mask = a.mask;
        tr.counts = a.counts;
        tr.links = links + (size_t)t * K * DIPS_LINK_WORDS;
        tr.carry_in = carry[cin];
        tr.carry_out = carry[cin ^ 1u];
        DIPS_HIP(h, dips::launch_mask_tracks(tr, s));
        cin ^= 1u;
        if (t + n < n_frames) {
            tr.prev0 = a.mask + (size_t)(n - 1u) * frame_words;
            DIPS_HIP(h, dips::launch_mask_tracks_keep(tr, tr.prev0, n, s));
        }
    }
    if (state) {
        DIPS_HIP(h, hipMemcpyAsync(state, tr.next_id, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        DIPS_HIP(h, hipMemcpyAsync(state + 1, carry[cin], sizeof(uint32_t) * 2u * K, hipMemcpyDeviceToDevice, s));
    }
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    return DIPS_OK;
}

// ---------------------------------------------------------------------------
// The binary morphology of a mask (dips_mask_morph; kernel in mask_morph.hip)
// ---------------------------------------------------------------------------

// One launch over the frames of a device mask, asynchronously on `s`.
dips_status run_morph_device(dips_handle* h, const uint8_t* mask_in, uint32_t n_frames, uint32_t w, uint32_t hgt,
                             uint32_t op, uint32_t shape, uint32_t rx, uint32_t ry, uint8_t* mask_out,
                             hipStream_t s) {
    dips::MorphArgs a{};
    a.in = reinterpret_cast<const uint32_t*>(mask_in);
    a.out = reinterpret_cast<uint32_t*>(mask_out);
    a.w = w;
    a.h = hgt;
    a.wpr = (uint32_t)mask_words_per_row(w);
    a.n_frames = n_frames;
    a.op = op;
    a.shape = shape;
    a.rx = rx;
    a.ry = ry;
    dips::mask_morph_tiling(w, hgt, &a.tiles_x, &a.tiles_y);
    a.items = (uint64_t)n_frames * a.tiles_x * a.tiles_y;

    const bool timing = (h->p.flags & DIPS_FLAG_TIME_KERNEL) != 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventReturn ev_return{h, &e0, &e1};
    if (timing) {
        e0 = take_event(h);
        e1 = take_event(h);
        if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
        DIPS_HIP(h, hipEventRecord(e0, s));
    }
    DIPS_HIP(h, dips::launch_mask_morph(a, s));
    if (timing) {
        DIPS_HIP(h, hipEventRecord(e1, s));
        h->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
    }
    return DIPS_OK;
}

// One timed launch of a read-only leg on the handle's stream: *ms = its
// hipEvent duration (synchronous).
template <typename Launch>
dips_status time_leg(dips_handle* h, double* ms, Launch&& launch) {
    DIPS_HIP(h, h->probe_out.ensure(256));
    hipEvent_t e0 = take_event(h), e1 = take_event(h);
    if (!e0 || !e1) return fail(h, DIPS_ERR_HIP, "hipEventCreate failed");
    DIPS_HIP(h, hipEventRecord(e0, h->stream));
    DIPS_HIP(h, launch());
    DIPS_HIP(h, hipEventRecord(e1, h->stream));
    DIPS_HIP(h, hipEventSynchronize(e1));
    float t = 0.0f;
    DIPS_HIP(h, hipEventElapsedTime(&t, e0, e1));
    *ms = t;
    h->ev_free.push_back(e0);
    h->ev_free.push_back(e1);
    return DIPS_OK;
}

}  // namespace

extern "C" {

dips_status dips_diff_series(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                             uint32_t n_frames, const uint8_t* ref, dips_series_entry* series, uint8_t* map) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!frames || !series || width == 0 || height == 0)
            return fail(h, DIPS_ERR_INVALID, "diff_series: null or empty argument");
        const int C = (int)h->p.format;
        const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS)
            return run_series_device(h, width, height, frames, n_frames, ref ? ref : frames, series, map, h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        DIPS_HIP(h, h->stage_frames.ensure(total));
        DIPS_HIP(h, h->stage_series.ensure(sizeof(dips_series_entry) * (size_t)n_frames));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, frames, total, hipMemcpyHostToDevice, h->stream));
        const uint8_t* ref_dev = h->stage_frames.as<uint8_t>();
        if (ref) {
            DIPS_HIP(h, h->stage_ref.ensure(fb));
            DIPS_HIP(h, hipMemcpyAsync(h->stage_ref.p, ref, fb, hipMemcpyHostToDevice, h->stream));
            ref_dev = h->stage_ref.as<uint8_t>();
        }
        uint8_t* map_dev = nullptr;
        if (map) {
            DIPS_HIP(h, h->stage_map.ensure(total));
            map_dev = h->stage_map.as<uint8_t>();
        }
        st = run_series_device(h, width, height, h->stage_frames.as<uint8_t>(), n_frames, ref_dev,
                               h->stage_series.as<dips_series_entry>(), map_dev, h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(series, h->stage_series.p, sizeof(dips_series_entry) * (size_t)n_frames,
                                   hipMemcpyDeviceToHost, h->stream));
        if (map) DIPS_HIP(h, hipMemcpyAsync(map, map_dev, total, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_diff_series_streamed(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* host_frames,
                                      uint32_t n_frames, const uint8_t* host_ref, dips_series_entry* series,
                                      uint32_t chunk_frames) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!host_frames || !series || width == 0 || height == 0)
            return fail(h, DIPS_ERR_INVALID, "diff_series_streamed: null or empty argument");
        const size_t fb = (size_t)width * height * (size_t)h->p.format;
        DIPS_HIP(h, h->stage_series.ensure(sizeof(dips_series_entry) * (size_t)n_frames));
        dips_series_entry* series_dev = h->stage_series.as<dips_series_entry>();
        const uint8_t* ref_dev = nullptr;
        if (host_ref) {
            DIPS_HIP(h, hipStreamSynchronize(h->stream));  // ring_ref may still be read by earlier work
            DIPS_HIP(h, h->ring_ref.ensure(fb));
            DIPS_HIP(h, h->pinned[1].ensure(fb));
            DIPS_HIP(h, hipStreamSynchronize(h->copy_stream));
            std::memcpy(h->pinned[1].p, host_ref, fb);
            DIPS_HIP(h, hipMemcpyAsync(h->ring_ref.p, h->pinned[1].p, fb, hipMemcpyHostToDevice, h->copy_stream));
            DIPS_HIP(h, hipStreamSynchronize(h->copy_stream));
            ref_dev = h->ring_ref.as<uint8_t>();
        }
        st = run_series_streamed(h, width, height, host_frames, n_frames, ref_dev, series_dev, chunk_frames);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(series, series_dev, sizeof(dips_series_entry) * (size_t)n_frames,
                                   hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_grid_cell(uint32_t width, uint32_t height, const uint32_t* roi, uint32_t rows, uint32_t cols,
                           uint32_t row, uint32_t col, uint32_t* rect) {
    return guard(nullptr, [&]() -> dips_status {
        dips::GridSpec g{};
        if (!rect || grid_spec(width, height, roi, rows, cols, &g) != nullptr || row >= rows || col >= cols)
            return DIPS_ERR_INVALID;
        const dips::GridRect r = dips::grid_cell_rect(g, row, col);
        rect[0] = r.x;
        rect[1] = r.y;
        rect[2] = r.w;
        rect[3] = r.h;
        return DIPS_OK;
    });
}

dips_status dips_diff_series_grid(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                  uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t rows,
                                  uint32_t cols, dips_series_entry* cells) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!frames || !cells) return fail(h, DIPS_ERR_INVALID, "diff_series_grid: null argument");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, rows, cols, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_series_grid: ") + why);
        const uint64_t n_cells = (uint64_t)rows * cols;
        if (n_cells >= (1ull << 30) || n_cells * n_frames >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_series_grid: n_frames * rows * cols must stay below 2^30 entries");
        const int C = (int)h->p.format;
        const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS)
            return run_grid_device(h, width, height, frames, n_frames, ref ? ref : frames, g, cells, h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        const size_t out_bytes = sizeof(dips_series_entry) * (size_t)(n_cells * n_frames);
        DIPS_HIP(h, h->stage_frames.ensure(total));
        DIPS_HIP(h, h->stage_series.ensure(out_bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, frames, total, hipMemcpyHostToDevice, h->stream));
        const uint8_t* ref_dev = h->stage_frames.as<uint8_t>();
        if (ref) {
            DIPS_HIP(h, h->stage_ref.ensure(fb));
            DIPS_HIP(h, hipMemcpyAsync(h->stage_ref.p, ref, fb, hipMemcpyHostToDevice, h->stream));
            ref_dev = h->stage_ref.as<uint8_t>();
        }
        st = run_grid_device(h, width, height, h->stage_frames.as<uint8_t>(), n_frames, ref_dev, g,
                             h->stage_series.as<dips_series_entry>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(cells, h->stage_series.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_diff_pixel_sums(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                 uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t accumulate,
                                 dips_series_entry* sums) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (!sums || (!frames && n_frames > 0)) return fail(h, DIPS_ERR_INVALID, "diff_pixel_sums: null argument");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_pixel_sums: ") + why);
        const uint64_t n_px = (uint64_t)g.w * g.h;
        if (n_px >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_pixel_sums: the region must stay below 2^30 pixels");
        const size_t out_bytes = sizeof(dips_series_entry) * (size_t)n_px;
        const bool dev = (h->p.flags & DIPS_FLAG_DEVICE_PTRS) != 0;
        if (n_frames == 0) {
            // nothing to add: an overwriting call leaves zeros
            if (accumulate != 0u) return DIPS_OK;
            if (dev)
                DIPS_HIP(h, hipMemsetAsync(sums, 0, out_bytes, h->stream));
            else
                std::memset(sums, 0, out_bytes);
            return DIPS_OK;
        }
        const int C = (int)h->p.format;
        const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
        if (dev)
            return run_pixels_device(h, width, height, frames, n_frames, ref ? ref : frames, g, accumulate != 0u, sums,
                                     h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        DIPS_HIP(h, h->stage_frames.ensure(total));
        DIPS_HIP(h, h->stage_series.ensure(out_bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, frames, total, hipMemcpyHostToDevice, h->stream));
        if (accumulate != 0u)
            DIPS_HIP(h, hipMemcpyAsync(h->stage_series.p, sums, out_bytes, hipMemcpyHostToDevice, h->stream));
        const uint8_t* ref_dev = h->stage_frames.as<uint8_t>();
        if (ref) {
            DIPS_HIP(h, h->stage_ref.ensure(fb));
            DIPS_HIP(h, hipMemcpyAsync(h->stage_ref.p, ref, fb, hipMemcpyHostToDevice, h->stream));
            ref_dev = h->stage_ref.as<uint8_t>();
        }
        st = run_pixels_device(h, width, height, h->stage_frames.as<uint8_t>(), n_frames, ref_dev, g, accumulate != 0u,
                               h->stage_series.as<dips_series_entry>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(sums, h->stage_series.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

uint32_t dips_mask_row_bytes(uint32_t roi_w) {
    return guard(nullptr, [&]() -> uint32_t { return (uint32_t)(4u * mask_words_per_row(roi_w)); });
}

dips_status dips_diff_change_mask(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                  uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint8_t* mask) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!frames || !mask) return fail(h, DIPS_ERR_INVALID, "diff_change_mask: null argument");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_change_mask: ") + why);
        if ((uint64_t)g.w * g.h >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_change_mask: the region must stay below 2^30 pixels");
        const int C = (int)h->p.format;
        const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            if (((uintptr_t)mask & 3u) != 0)
                return fail(h, DIPS_ERR_INVALID, "diff_change_mask: the device mask must be 4-byte aligned");
            return run_mask_device(h, width, height, frames, n_frames, ref ? ref : frames, g, mask, h->stream);
        }
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        const size_t out_bytes = (size_t)(4u * mask_words_per_row(g.w) * g.h) * n_frames;
        DIPS_HIP(h, h->stage_frames.ensure(total));
        DIPS_HIP(h, h->stage_map.ensure(out_bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, frames, total, hipMemcpyHostToDevice, h->stream));
        const uint8_t* ref_dev = h->stage_frames.as<uint8_t>();
        if (ref) {
            DIPS_HIP(h, h->stage_ref.ensure(fb));
            DIPS_HIP(h, hipMemcpyAsync(h->stage_ref.p, ref, fb, hipMemcpyHostToDevice, h->stream));
            ref_dev = h->stage_ref.as<uint8_t>();
        }
        st = run_mask_device(h, width, height, h->stage_frames.as<uint8_t>(), n_frames, ref_dev, g,
                             h->stage_map.as<uint8_t>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(mask, h->stage_map.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_diff_pixel_times(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                  uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t t0,
                                  uint32_t accumulate, uint32_t* times) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (!times || (!frames && n_frames > 0)) return fail(h, DIPS_ERR_INVALID, "diff_pixel_times: null argument");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_pixel_times: ") + why);
        const uint64_t n_px = (uint64_t)g.w * g.h;
        if (n_px >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_pixel_times: the region must stay below 2^30 pixels");
        if ((uint64_t)t0 + n_frames > 0xFFFFFFFFull)
            return fail(h, DIPS_ERR_INVALID,
                        "diff_pixel_times: t0 + n_frames must stay below 2^32 (index 0xFFFFFFFF is DIPS_TIME_NONE)");
        const bool dev = (h->p.flags & DIPS_FLAG_DEVICE_PTRS) != 0;
        if (dev && ((uintptr_t)times & 3u) != 0)
            return fail(h, DIPS_ERR_INVALID, "diff_pixel_times: the device times must be 4-byte aligned");
        const size_t plane_bytes = sizeof(uint32_t) * (size_t)n_px;
        const size_t out_bytes = DIPS_TIMES_PLANES * plane_bytes;
        if (n_frames == 0) {
            // nothing to fold: an overwriting call leaves the initial state
            if (accumulate != 0u) return DIPS_OK;
            uint8_t* b = reinterpret_cast<uint8_t*>(times);
            if (dev) {
                DIPS_HIP(h, hipMemsetAsync(b, 0xFF, 2u * plane_bytes, h->stream));
                DIPS_HIP(h, hipMemsetAsync(b + 2u * plane_bytes, 0, 2u * plane_bytes, h->stream));
            } else {
                std::memset(b, 0xFF, 2u * plane_bytes);
                std::memset(b + 2u * plane_bytes, 0, 2u * plane_bytes);
            }
            return DIPS_OK;
        }
        const int C = (int)h->p.format;
        const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
        if (dev)
            return run_times_device(h, width, height, frames, n_frames, ref ? ref : frames, g, t0, accumulate != 0u,
                                    times, h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        DIPS_HIP(h, h->stage_frames.ensure(total));
        DIPS_HIP(h, h->stage_series.ensure(out_bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, frames, total, hipMemcpyHostToDevice, h->stream));
        if (accumulate != 0u)
            DIPS_HIP(h, hipMemcpyAsync(h->stage_series.p, times, out_bytes, hipMemcpyHostToDevice, h->stream));
        const uint8_t* ref_dev = h->stage_frames.as<uint8_t>();
        if (ref) {
            DIPS_HIP(h, h->stage_ref.ensure(fb));
            DIPS_HIP(h, hipMemcpyAsync(h->stage_ref.p, ref, fb, hipMemcpyHostToDevice, h->stream));
            ref_dev = h->stage_ref.as<uint8_t>();
        }
        st = run_times_device(h, width, height, h->stage_frames.as<uint8_t>(), n_frames, ref_dev, g, t0,
                              accumulate != 0u, h->stage_series.as<uint32_t>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(times, h->stage_series.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_diff_background_mask(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                      uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t rate_shift,
                                      uint32_t bg_flags, uint32_t accumulate, uint16_t* background, uint8_t* mask) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (rate_shift > DIPS_BG_MAX_RATE_SHIFT)
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: rate_shift must be 0 .. 8");
        if ((bg_flags & ~DIPS_BG_SELECTIVE) != 0u)
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: unknown bg_flags bits");
        if (!background || (!frames && n_frames > 0))
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: null argument");
        const bool acc = accumulate != 0u;
        if (acc && ref)
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: ref must be NULL when accumulating");
        if (!acc && !ref && n_frames == 0)
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: the initial state needs ref or a frame");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_background_mask: ") + why);
        const uint64_t n_px = (uint64_t)g.w * g.h;
        if (n_px >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: the region must stay below 2^30 pixels");
        const bool dev = (h->p.flags & DIPS_FLAG_DEVICE_PTRS) != 0;
        if (dev && ((uintptr_t)background & 1u) != 0)
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: the device background must be 2-byte aligned");
        if (dev && ((uintptr_t)mask & 3u) != 0)
            return fail(h, DIPS_ERR_INVALID, "diff_background_mask: the device mask must be 4-byte aligned");
        if (n_frames == 0 && acc) return DIPS_OK;  // nothing to fold
        const bool selective = (bg_flags & DIPS_BG_SELECTIVE) != 0u;
        const int C = (int)h->p.format;
        const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
        if (dev)
            return run_background_device(h, width, height, frames, n_frames, acc ? nullptr : (ref ? ref : frames), g,
                                         rate_shift, selective, acc, background, mask, h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        const size_t state_bytes = sizeof(uint16_t) * (size_t)C * (size_t)n_px;
        const size_t mask_bytes = mask ? (size_t)(4u * mask_words_per_row(g.w) * g.h) * n_frames : 0u;
        if (total) DIPS_HIP(h, h->stage_frames.ensure(total));
        DIPS_HIP(h, h->stage_series.ensure(state_bytes));
        if (mask_bytes) DIPS_HIP(h, h->stage_map.ensure(mask_bytes));
        if (total) DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, frames, total, hipMemcpyHostToDevice, h->stream));
        if (acc) DIPS_HIP(h, hipMemcpyAsync(h->stage_series.p, background, state_bytes, hipMemcpyHostToDevice, h->stream));
        const uint8_t* ref_dev = acc ? nullptr : h->stage_frames.as<uint8_t>();
        if (ref) {
            DIPS_HIP(h, h->stage_ref.ensure(fb));
            DIPS_HIP(h, hipMemcpyAsync(h->stage_ref.p, ref, fb, hipMemcpyHostToDevice, h->stream));
            ref_dev = h->stage_ref.as<uint8_t>();
        }
        st = run_background_device(h, width, height, total ? h->stage_frames.as<uint8_t>() : nullptr, n_frames, ref_dev,
                                   g, rate_shift, selective, acc, h->stage_series.as<uint16_t>(),
                                   mask_bytes ? h->stage_map.as<uint8_t>() : nullptr, h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(background, h->stage_series.p, state_bytes, hipMemcpyDeviceToHost, h->stream));
        if (mask_bytes) DIPS_HIP(h, hipMemcpyAsync(mask, h->stage_map.p, mask_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_diff_sigma_delta_mask(dips_handle* h, uint32_t width, uint32_t height, const uint8_t* frames,
                                       uint32_t n_frames, const uint8_t* ref, const uint32_t* roi, uint32_t n_amp,
                                       uint32_t v_min, uint32_t v_max, uint32_t accumulate, uint16_t* state,
                                       uint8_t* mask) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_amp == 0u || n_amp > DIPS_SD_MAX_AMP)
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: n_amp must be 1 .. 15");
        if (v_min > v_max || v_max > DIPS_SD_MAX_V)
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: 0 <= v_min <= v_max <= 510 is required");
        if (!state || (!frames && n_frames > 0))
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: null argument");
        const bool acc = accumulate != 0u;
        if (acc && ref)
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: ref must be NULL when accumulating");
        if (!acc && !ref && n_frames == 0)
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: the initial state needs ref or a frame");
        dips::GridSpec g{};
        if (const char* why = grid_spec(width, height, roi, 1u, 1u, &g))
            return fail(h, DIPS_ERR_INVALID, std::string("diff_sigma_delta_mask: ") + why);
        const uint64_t n_px = (uint64_t)g.w * g.h;
        if (n_px >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: the region must stay below 2^30 pixels");
        const bool dev = (h->p.flags & DIPS_FLAG_DEVICE_PTRS) != 0;
        if (dev && ((uintptr_t)state & 1u) != 0)
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: the device state must be 2-byte aligned");
        if (dev && ((uintptr_t)mask & 3u) != 0)
            return fail(h, DIPS_ERR_INVALID, "diff_sigma_delta_mask: the device mask must be 4-byte aligned");
        if (n_frames == 0 && acc) return DIPS_OK;  // nothing to fold
        const int C = (int)h->p.format;
        const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
        if (dev)
            return run_sigma_delta_device(h, width, height, frames, n_frames, acc ? nullptr : (ref ? ref : frames), g,
                                          n_amp, v_min, v_max, acc, state, mask, h->stream);
        // host pointers: stage through HBM (synchronous call)
        const size_t total = (size_t)fb * n_frames;
        const size_t state_bytes = sizeof(uint16_t) * (size_t)DIPS_SD_PLANES * (size_t)n_px;
        const size_t mask_bytes = mask ? (size_t)(4u * mask_words_per_row(g.w) * g.h) * n_frames : 0u;
        if (total) DIPS_HIP(h, h->stage_frames.ensure(total));
        DIPS_HIP(h, h->stage_series.ensure(state_bytes));
        if (mask_bytes) DIPS_HIP(h, h->stage_map.ensure(mask_bytes));
        if (total) DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, frames, total, hipMemcpyHostToDevice, h->stream));
        if (acc) DIPS_HIP(h, hipMemcpyAsync(h->stage_series.p, state, state_bytes, hipMemcpyHostToDevice, h->stream));
        const uint8_t* ref_dev = acc ? nullptr : h->stage_frames.as<uint8_t>();
        if (ref) {
            DIPS_HIP(h, h->stage_ref.ensure(fb));
            DIPS_HIP(h, hipMemcpyAsync(h->stage_ref.p, ref, fb, hipMemcpyHostToDevice, h->stream));
            ref_dev = h->stage_ref.as<uint8_t>();
        }
        st = run_sigma_delta_device(h, width, height, total ? h->stage_frames.as<uint8_t>() : nullptr, n_frames, ref_dev,
                                    g, n_amp, v_min, v_max, acc, h->stage_series.as<uint16_t>(),
                                    mask_bytes ? h->stage_map.as<uint8_t>() : nullptr, h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(state, h->stage_series.p, state_bytes, hipMemcpyDeviceToHost, h->stream));
        if (mask_bytes) DIPS_HIP(h, hipMemcpyAsync(mask, h->stage_map.p, mask_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_components(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w,
                                 uint32_t roi_h, uint32_t connectivity, uint32_t min_area, uint32_t max_boxes,
                                 uint32_t chunk_frames, uint32_t* counts, uint32_t* boxes, uint32_t* labels) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts || (!boxes && max_boxes != 0u))
            return fail(h, DIPS_ERR_INVALID, "mask_components: null argument");
        if (connectivity != 4u && connectivity != 8u)
            return fail(h, DIPS_ERR_INVALID, "mask_components: connectivity must be 4 or 8");
        if (roi_w == 0 || roi_h == 0 || roi_w >= (1u << 24) || roi_h >= (1u << 24))
            return fail(h, DIPS_ERR_INVALID, "mask_components: roi_w and roi_h must be 1 .. 2^24 - 1");
        const uint64_t n_px = (uint64_t)roi_w * roi_h;
        if (n_px >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_components: the region must stay below 2^30 pixels");
        if ((uint64_t)n_frames * max_boxes * DIPS_BOX_WORDS >= (1ull << 32))
            return fail(h, DIPS_ERR_INVALID, "mask_components: n_frames * max_boxes * 8 must stay below 2^32");
        if (max_boxes == 0u) boxes = nullptr;
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            if ((((uintptr_t)mask | (uintptr_t)counts | (uintptr_t)boxes | (uintptr_t)labels) & 3u) != 0)
                return fail(h, DIPS_ERR_INVALID, "mask_components: the device pointers must be 4-byte aligned");
            return run_components_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes,
                                         chunk_frames, counts, boxes, labels, h->stream);
        }
        // host pointers: stage through HBM (synchronous call); counts and
        // boxes share one buffer
        const size_t mask_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h) * n_frames;
        const size_t counts_bytes = sizeof(uint32_t) * (size_t)n_frames;
        const size_t boxes_bytes = sizeof(uint32_t) * DIPS_BOX_WORDS * (size_t)n_frames * max_boxes;
        const size_t labels_bytes = labels ? sizeof(uint32_t) * (size_t)n_px * n_frames : 0u;
        DIPS_HIP(h, h->stage_frames.ensure(mask_bytes));
        DIPS_HIP(h, h->stage_series.ensure(counts_bytes + boxes_bytes));
        if (labels) DIPS_HIP(h, h->stage_map.ensure(labels_bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, mask, mask_bytes, hipMemcpyHostToDevice, h->stream));
        uint32_t* counts_dev = h->stage_series.as<uint32_t>();
        uint32_t* boxes_dev = max_boxes != 0u ? counts_dev + n_frames : nullptr;
        st = run_components_device(h, h->stage_frames.as<uint8_t>(), n_frames, roi_w, roi_h, connectivity, min_area,
                                   max_boxes, chunk_frames, counts_dev, boxes_dev,
                                   labels ? h->stage_map.as<uint32_t>() : nullptr, h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(counts, counts_dev, counts_bytes, hipMemcpyDeviceToHost, h->stream));
        if (max_boxes != 0u)
            DIPS_HIP(h, hipMemcpyAsync(boxes, boxes_dev, boxes_bytes, hipMemcpyDeviceToHost, h->stream));
        if (labels) DIPS_HIP(h, hipMemcpyAsync(labels, h->stage_map.p, labels_bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_tracks(dips_handle* h, const uint8_t* mask, uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                             uint32_t connectivity, uint32_t min_area, uint32_t max_boxes, uint32_t chunk_frames,
                             const uint8_t* prev_mask, uint32_t* state, uint32_t* counts, uint32_t* boxes,
                             uint32_t* links) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!mask || !counts || !boxes || !links) return fail(h, DIPS_ERR_INVALID, "mask_tracks: null argument");
        if (max_boxes == 0u || max_boxes > DIPS_TRACK_MAX_BOXES)
            return fail(h, DIPS_ERR_INVALID, "mask_tracks: max_boxes must be 1 .. 256");
        if (prev_mask && !state) return fail(h, DIPS_ERR_INVALID, "mask_tracks: prev_mask needs state");
        if (connectivity != 4u && connectivity != 8u)
            return fail(h, DIPS_ERR_INVALID, "mask_tracks: connectivity must be 4 or 8");
        if (roi_w == 0 || roi_h == 0 || roi_w >= (1u << 24) || roi_h >= (1u << 24))
            return fail(h, DIPS_ERR_INVALID, "mask_tracks: roi_w and roi_h must be 1 .. 2^24 - 1");
        const uint64_t n_px = (uint64_t)roi_w * roi_h;
        if (n_px >= (1ull << 30)) return fail(h, DIPS_ERR_INVALID, "mask_tracks: the region must stay below 2^30 pixels");
        if ((uint64_t)n_frames * max_boxes * DIPS_BOX_WORDS >= (1ull << 32))
            return fail(h, DIPS_ERR_INVALID, "mask_tracks: n_frames * max_boxes * 8 must stay below 2^32");
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            if ((((uintptr_t)mask | (uintptr_t)prev_mask | (uintptr_t)state | (uintptr_t)counts | (uintptr_t)boxes |
                  (uintptr_t)links) & 3u) != 0)
                return fail(h, DIPS_ERR_INVALID, "mask_tracks: the device pointers must be 4-byte aligned");
            return run_tracks_device(h, mask, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes, chunk_frames,
                                     prev_mask, state, counts, boxes, links, h->stream);
        }
        // host pointers: stage through HBM (synchronous call); the frame
        // before the clip behind the mask, the outputs and the state in one buffer
        const size_t frame_bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h);
        const size_t mask_bytes = frame_bytes * n_frames;
        const size_t counts_words = (size_t)n_frames;
        const size_t boxes_words = DIPS_BOX_WORDS * (size_t)n_frames * max_boxes;
        const size_t links_words = DIPS_LINK_WORDS * (size_t)n_frames * max_boxes;
        const size_t state_words = 1u + 2u * (size_t)max_boxes;
        DIPS_HIP(h, h->stage_frames.ensure(mask_bytes + frame_bytes));
        DIPS_HIP(h, h->stage_series.ensure(sizeof(uint32_t) * (counts_words + boxes_words + links_words + state_words)));
        uint8_t* mask_dev = h->stage_frames.as<uint8_t>();
        uint8_t* prev_dev = prev_mask ? mask_dev + mask_bytes : nullptr;
        uint32_t* counts_dev = h->stage_series.as<uint32_t>();
        uint32_t* boxes_dev = counts_dev + counts_words;
        uint32_t* links_dev = boxes_dev + boxes_words;
        uint32_t* state_dev = state ? links_dev + links_words : nullptr;
        DIPS_HIP(h, hipMemcpyAsync(mask_dev, mask, mask_bytes, hipMemcpyHostToDevice, h->stream));
        if (prev_mask) DIPS_HIP(h, hipMemcpyAsync(prev_dev, prev_mask, frame_bytes, hipMemcpyHostToDevice, h->stream));
        if (state)
            DIPS_HIP(h, hipMemcpyAsync(state_dev, state, sizeof(uint32_t) * state_words, hipMemcpyHostToDevice, h->stream));
        st = run_tracks_device(h, mask_dev, n_frames, roi_w, roi_h, connectivity, min_area, max_boxes, chunk_frames,
                               prev_dev, state_dev, counts_dev, boxes_dev, links_dev, h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(counts, counts_dev, sizeof(uint32_t) * counts_words, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipMemcpyAsync(boxes, boxes_dev, sizeof(uint32_t) * boxes_words, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipMemcpyAsync(links, links_dev, sizeof(uint32_t) * links_words, hipMemcpyDeviceToHost, h->stream));
        if (state)
            DIPS_HIP(h, hipMemcpyAsync(state, state_dev, sizeof(uint32_t) * state_words, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_mask_morph(dips_handle* h, const uint8_t* mask_in, uint32_t n_frames, uint32_t roi_w,
                            uint32_t roi_h, uint32_t op, uint32_t shape, uint32_t rx, uint32_t ry,
                            uint8_t* mask_out) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!mask_in || !mask_out) return fail(h, DIPS_ERR_INVALID, "mask_morph: null argument");
        if (op > DIPS_MORPH_CLOSE) return fail(h, DIPS_ERR_INVALID, "mask_morph: op must be 0 .. 3");
        if (shape > DIPS_MORPH_DIAMOND) return fail(h, DIPS_ERR_INVALID, "mask_morph: shape must be 0 or 1");
        if (rx > DIPS_MORPH_MAX_RADIUS || ry > DIPS_MORPH_MAX_RADIUS)
            return fail(h, DIPS_ERR_INVALID, "mask_morph: rx and ry must be 0 .. 15");
        if (shape == DIPS_MORPH_DIAMOND && ry != rx)
            return fail(h, DIPS_ERR_INVALID, "mask_morph: a diamond needs ry == rx");
        if (roi_w == 0 || roi_h == 0) return fail(h, DIPS_ERR_INVALID, "mask_morph: roi_w and roi_h must not be 0");
        if ((uint64_t)roi_w * roi_h >= (1ull << 30))
            return fail(h, DIPS_ERR_INVALID, "mask_morph: the region must stay below 2^30 pixels");
        const size_t bytes = (size_t)(4u * mask_words_per_row(roi_w) * roi_h) * n_frames;
        const uintptr_t pi = (uintptr_t)mask_in, po = (uintptr_t)mask_out;
        if (pi < po + bytes && po < pi + bytes)
            return fail(h, DIPS_ERR_INVALID, "mask_morph: mask_in and mask_out must not overlap");
        if (h->p.flags & DIPS_FLAG_DEVICE_PTRS) {
            if (((pi | po) & 3u) != 0)
                return fail(h, DIPS_ERR_INVALID, "mask_morph: the device pointers must be 4-byte aligned");
            return run_morph_device(h, mask_in, n_frames, roi_w, roi_h, op, shape, rx, ry, mask_out, h->stream);
        }
        // host pointers: stage through HBM (synchronous call)
        DIPS_HIP(h, h->stage_frames.ensure(bytes));
        DIPS_HIP(h, h->stage_map.ensure(bytes));
        DIPS_HIP(h, hipMemcpyAsync(h->stage_frames.p, mask_in, bytes, hipMemcpyHostToDevice, h->stream));
        st = run_morph_device(h, h->stage_frames.as<uint8_t>(), n_frames, roi_w, roi_h, op, shape, rx, ry,
                              h->stage_map.as<uint8_t>(), h->stream);
        if (st != DIPS_OK) return st;
        DIPS_HIP(h, hipMemcpyAsync(mask_out, h->stage_map.p, bytes, hipMemcpyDeviceToHost, h->stream));
        DIPS_HIP(h, hipStreamSynchronize(h->stream));
        return DIPS_OK;
    });
}

dips_status dips_synth_frames(dips_handle* h, uint32_t width, uint32_t height, uint64_t seed, uint64_t t0,
                              uint32_t n_frames, uint8_t* dst) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (n_frames == 0) return DIPS_OK;
        if (!dst || width == 0 || height == 0)
            return fail(h, DIPS_ERR_INVALID, "synth_frames: null or empty argument");
        dips::SynthArgs a{};
        a.dst = dst;
        a.channels = h->p.format;
        a.width = width;
        a.height = height;
        a.frame_bytes = (uint64_t)width * height * a.channels;
        a.total_bytes = a.frame_bytes * n_frames;
        a.seed = seed;
        a.t0 = t0;
        a.radius = height / 8u > 0 ? height / 8u : 1u;
        DIPS_HIP(h, dips::launch_synth(a, h->stream));
        return DIPS_OK;
    });
}

dips_status dips_read_ceiling(dips_handle* h, const uint8_t* dev_bytes, uint64_t bytes, double* ms) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (!dev_bytes || !ms) return fail(h, DIPS_ERR_INVALID, "read_ceiling: null argument");
        return time_leg(h, ms, [&]() {
            return dips::launch_read_ceiling(dev_bytes, bytes, h->probe_out.as<uint32_t>(), h->stream);
        });
    });
}

dips_status dips_read_ceiling_walk(dips_handle* h, const uint8_t* dev_frames, uint32_t width, uint32_t height,
                                   uint32_t n_frames, double* ms) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        if (!dev_frames || !ms) return fail(h, DIPS_ERR_INVALID, "read_ceiling_walk: null argument");
        const int C = (int)h->p.format;
        if (C != 3 && C != 4) return fail(h, DIPS_ERR_INVALID, "read_ceiling_walk: RGB8 / RGBA8 only");
        // the geometry and schedule an aligned batch of this shape runs with
        // (part-major for batches of >= 256 frames, either mode)
        FastGeom g = fast_geometry(h, width, height, n_frames, C, h->p.mode == DIPS_MODE_PER_FRAME, false, false,
                                   series_isi_form(h));
        if (!g.ok) return fail(h, DIPS_ERR_INVALID, "read_ceiling_walk: shape not eligible for the series kernel");
        dips::SeriesArgs a{};
        a.frames = dev_frames;
        a.items = g.items;
        a.frame_bytes = (uint32_t)((uint64_t)width * height * (uint64_t)C);
        a.vec_bytes = (uint32_t)g.vec_bytes;
        a.n_frames = n_frames;
        a.n_tiles = (uint32_t)g.n_tiles;
        a.n_waves = (uint32_t)g.n_waves;
        a.part_frames = g.part_frames;
        return time_leg(h, ms, [&]() {
            return dips::launch_read_walk(a, C == 3 ? 12 : 16, (uint32_t)g.blocks, h->probe_out.as<uint32_t>(),
                                          h->stream);
        });
    });
}

dips_status dips_series_geometry(dips_handle* h, uint32_t width, uint32_t height, uint32_t n_frames,
                                 uint64_t* waves, uint64_t* tiles, uint64_t* partial_bytes) {
    return guard(h, [&]() -> dips_status {
        dips_status st = bind(h);
        if (st != DIPS_OK) return st;
        const int C = (int)h->p.format;
        // the kernel an aligned batch of this shape runs (its occupancy sets
        // the wave slots)
        FastGeom g = C == 1 && gray_lut_enabled(h)
                         ? gray_lut_geometry(h, width, height, n_frames)
                         : fast_geometry(h, width, height, n_frames, C, h->p.mode == DIPS_MODE_PER_FRAME, false,
                                         false, series_isi_form(h));
        if (waves) *waves = g.ok ? g.n_waves : 0;
        if (tiles) *tiles = g.ok ? g.n_tiles : 0;
        if (partial_bytes) *partial_bytes = g.ok ? g.n_tiles * 16u : 0;
        return g.ok ? DIPS_OK : fail(h, DIPS_ERR_INVALID, "shape not eligible for the fast kernel");
    });
}

}  // extern "C"
