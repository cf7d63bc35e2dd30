/*
 * dips_hip.h -- C ABI of the MI355X-native DiPs frame-difference path.
 *
 * This is the drop-in boundary.  The reference crate (RubenMovsesyan/DiPs,
 * Rust) reaches its GPU operator only through
 *     type CallbackFunction = fn(u32, u32, &[u8], &mut ComputeState) -> Vec<u8>
 * (dips/src/lib.rs:23) and the three ComputeState methods new / add_texture /
 * dispatch (dips/src/gpu/mod.rs:59, :170, :306; identical copies in
 * dips_opencv/src/gpu/mod.rs:59, :172, :308).  Each entry point below names
 * the reference item it replaces.  Everything is plain C: pointers, sizes,
 * status codes.  No exception or panic crosses this boundary.
 *
 * Threading: a handle is not internally synchronised (the reference uses
 * ComputeState under an RwLock write guard, dips/src/frame_extractor.rs:232);
 * a handle may move between threads.  The caller owns every buffer.  Every
 * entry point leaves the calling thread's current HIP device as it found it
 * (work runs on the handle's device).
 */
#ifndef DIPS_HIP_H
#define DIPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIPS_ABI_VERSION 3

typedef enum dips_status {
    DIPS_OK = 0,
    DIPS_ERR_INVALID = -1,  /* bad argument / shape / parameter */
    DIPS_ERR_HIP = -2,      /* HIP runtime error (see dips_last_error) */
    DIPS_ERR_STATE = -3,    /* call not valid in the handle's state */
    DIPS_ERR_NOMEM = -4,    /* device or host allocation failed */
    DIPS_ERR_CAPACITY = -5, /* caller's output buffer too small */
    DIPS_ERR_NODEVICE = -6, /* no HIP device / device index out of range */
    DIPS_ERR_INTERNAL = -7, /* a C++ exception inside the library, caught at the
                               boundary (see dips_last_error); the handle may
                               be left mid-call and should be destroyed */
    DIPS_ERR_COMM = -8      /* a communicator's transport failed (RCCL error,
                               a loopback rank that never arrived, a host
                               transport callback's non-zero return) */
} dips_status;

/* DiPsFilter -> override id 3 (dips/src/lib.rs:25-41, dips_shader.wgsl:20). */
#define DIPS_FILTER_SIGMOID 0u
#define DIPS_FILTER_INVERSE_SIGMOID 1u
#define DIPS_FILTER_UNFILTERED 255u
/* ChromaFilter -> override id 4 (dips/src/lib.rs:43-61, dips_shader.wgsl:21). */
#define DIPS_CHROMA_NONE 0u
#define DIPS_CHROMA_RED 1u
#define DIPS_CHROMA_GREEN 2u
#define DIPS_CHROMA_BLUE 3u

/* Pixel formats of the series path (the compat path is RGBA8 only, like the
 * reference's appsink caps, dips/src/frame_extractor.rs:141-148). */
#define DIPS_FMT_GRAY8 1u
#define DIPS_FMT_RGB8 3u
#define DIPS_FMT_RGBA8 4u

/* Reference choice of the series path (README.md:7-11). */
#define DIPS_MODE_OVERALL 0u   /* against frame 0 (or the given reference) */
#define DIPS_MODE_PER_FRAME 1u /* against the previous frame */

/* dips_params.flags */
#define DIPS_FLAG_DEVICE_PTRS 0x1u /* series pointers are device (HBM) pointers */
#define DIPS_FLAG_TIME_KERNEL 0x2u /* record hipEvents around the series kernel */
#define DIPS_FLAG_FORCE_GENERIC 0x4u /* use the generic (any-shape) series kernel */
/* Cross-check forms: the same results through the plain kernels instead of
 * the specialised ones -- GRAY8 series: the f32 kernel, not the table kernel;
 * RGB8 / RGBA8 series: the exact f64 intensity sum at every tau, not the
 * integer sum of tau >= 2^-5; dips-compat / dips_alt batches: the per-pixel
 * arithmetic epilogue, not the epilogue table; the per-frame calls: whole
 * RGBA8 frames through the DMA staging (add_texture + dispatch), not the
 * striped zero-copy pipeline with compact transfers.  For tests and
 * A/B checks; slower. */
#define DIPS_FLAG_CROSSCHECK 0x8u
/* GRAY8 series: pin the table kernel's layout instead of its per-workgroup
 * choice from the content it walks (series_gray.hip layout 4) -- the table
 * keyed by (a ^ b, a) with the band clamp (BAND: fastest on consecutive video
 * frames) or by (a, b) (PAIR: fastest on flat or i.i.d. random content).
 * Same results either way; both set = BAND. */
#define DIPS_FLAG_GRAY_BAND_TABLE 0x10u
#define DIPS_FLAG_GRAY_PAIR_TABLE 0x20u

/* Operator parameters.  The first five mirror ComputeState::new's arguments
 * (dips/src/gpu/mod.rs:59-65) and DiPsProperties (dips/src/lib.rs:63-86);
 * the rest configure the batch series path. */
typedef struct dips_params {
    uint8_t colorize;            /* override id 0; default 0 (lib.rs:80) */
    int32_t spatial_window_size; /* override id 1; 1..11; default 1 (lib.rs:81) */
    float sensitivity;           /* override id 2; default 5.0 (lib.rs:82) */
    uint32_t filter_type;        /* DIPS_FILTER_*; default UNFILTERED (lib.rs:83) */
    uint32_t chroma_filter;      /* DIPS_CHROMA_*; default NONE (lib.rs:84) */
    uint32_t mode;               /* DIPS_MODE_*; default OVERALL */
    uint32_t format;             /* DIPS_FMT_*; default RGB8 */
    float tau;                   /* intensity threshold, >= 0; default 0 */
    uint32_t flags;              /* DIPS_FLAG_* */
} dips_params;

/* One entry of the per-frame difference series.
 *   sad      = sum over pixels and channels of |F_t - R|          (exact)
 *   sj       = sum over pixels of |J_t - J_R|, J = max+min bytes   (exact)
 *   count    = number of pixels with dI > tau
 *   si_fixed = sum of dI over those pixels, scaled by 2^32         (exact)
 * dI = |I_t - I_R| in f32 with I = get_intensity (dips_shader.wgsl:64-82).
 * The f64 intensity sum is si_fixed * 2^-32 (dips_series_si). */
typedef struct dips_series_entry {
    uint64_t sad;
    uint64_t sj;
    uint64_t count;
    uint64_t si_fixed;
} dips_series_entry;

typedef struct dips_handle dips_handle;

/* Layouts pinned for foreign bindings: the Rust crate rust/dips-hip
 * (src/ffi.rs) asserts the same sizes and offsets on its #[repr(C)] twins. */
#ifdef __cplusplus
#define DIPS_LAYOUT_ASSERT(cond, msg) static_assert(cond, msg)
#else
#define DIPS_LAYOUT_ASSERT(cond, msg) _Static_assert(cond, msg)
#endif
DIPS_LAYOUT_ASSERT(sizeof(dips_params) == 36, "dips_params size");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, colorize) == 0, "dips_params.colorize");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, spatial_window_size) == 4, "dips_params.spatial_window_size");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, sensitivity) == 8, "dips_params.sensitivity");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, filter_type) == 12, "dips_params.filter_type");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, chroma_filter) == 16, "dips_params.chroma_filter");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, mode) == 20, "dips_params.mode");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, format) == 24, "dips_params.format");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, tau) == 28, "dips_params.tau");
DIPS_LAYOUT_ASSERT(offsetof(dips_params, flags) == 32, "dips_params.flags");
DIPS_LAYOUT_ASSERT(sizeof(dips_series_entry) == 32, "dips_series_entry size");
DIPS_LAYOUT_ASSERT(offsetof(dips_series_entry, sad) == 0, "dips_series_entry.sad");
DIPS_LAYOUT_ASSERT(offsetof(dips_series_entry, sj) == 8, "dips_series_entry.sj");
DIPS_LAYOUT_ASSERT(offsetof(dips_series_entry, count) == 16, "dips_series_entry.count");
DIPS_LAYOUT_ASSERT(offsetof(dips_series_entry, si_fixed) == 24, "dips_series_entry.si_fixed");

/* Fill `p` with DiPsProperties::new() defaults (dips/src/lib.rs:74-86). */
dips_status dips_params_default(dips_params *p);

/* Replaces ComputeState::new (dips/src/gpu/mod.rs:59-165): binds HIP device
 * `device`, validates the parameters, creates the stream and tables. */
dips_status dips_create(const dips_params *params, int device, dips_handle **out);

/* Replaces Drop of ComputeState. */
void dips_destroy(dips_handle *h);

/* Last error message for `h` (or the last creation failure if h == NULL). */
const char *dips_last_error(const dips_handle *h);

/* Run subsequent work on `stream` (a hipStream_t; NULL = the handle's own).
 * The handle's own stream is a blocking stream: its work is ordered with the
 * legacy default stream (stream 0) both ways, so a caller whose work runs on
 * stream 0 -- torch's default stream reports cuda_stream 0, which the Python
 * wrappers pass as NULL -- needs no extra synchronisation.  Switching streams orders the new stream after all work already issued on
 * the previous one (the handle's device scratch serves both), so the previous
 * stream must still exist at the switch; setting the current stream again is
 * free.  A caller that binds an external stream and may destroy it should
 * switch back to NULL before doing so (the Python wrappers do this after
 * every call: dips_amd._lib.on_stream). */
dips_status dips_set_stream(dips_handle *h, void *stream);

/* Block until all work issued through `h` has finished. */
dips_status dips_synchronize(dips_handle *h);

/* Replaces ComputeState::add_texture (dips/src/gpu/mod.rs:170-216): queue an
 * RGBA8 host frame (len = width*height*4, stride = width*4 as at
 * bind_groups.rs:264); the 4th frame builds the start texture and the
 * temporal ring, later frames replace the ring slot.  The frame is read
 * before the call returns (borrowed, as in the reference).  In steady state
 * (window 1, host pointers) the call also starts the compute of the
 * dispatch that normally follows on the staged frame; that dispatch then
 * only collects it, and any other call first lets it finish, keeping the
 * reference's state (DIPS_FLAG_CROSSCHECK turns this off). */
dips_status dips_add_texture(dips_handle *h, uint32_t width, uint32_t height,
                             const uint8_t *frame_rgba, size_t len);

/* Replaces ComputeState::dispatch (dips/src/gpu/mod.rs:306-397): returns 1
 * and writes width*height*4 RGBA8 bytes to `out` (Some), 0 while fewer than
 * four frames were added (None), or a negative dips_status. */
int dips_dispatch(dips_handle *h, uint8_t *out_rgba, size_t cap);

/* Replaces frame_callback (dips/src/lib.rs:233-246): add_texture, then
 * dispatch; if dispatch gives None the input is copied to `out`.  Returns 1
 * when `out` holds the visualisation, 0 when it holds the passthrough copy,
 * negative on error. */
int dips_frame_callback(dips_handle *h, uint32_t width, uint32_t height,
                        const uint8_t *frame_rgba, size_t len, uint8_t *out, size_t cap);

/* `n_frames` consecutive frame_callback calls (dips/src/lib.rs:233-246) in
 * one pass: frames and out are n_frames x width*height*4 RGBA8; out[t] is
 * the visualisation, or the passthrough copy for the stream's first three
 * frames.  The first frames of a stream (start texture, unquantised ring)
 * and spatial windows W > 1 run frame by frame; the steady state (W = 1,
 * from the stream's 8th frame) runs as one HBM-streaming kernel.  With
 * DIPS_FLAG_DEVICE_PTRS both are device pointers and the call is
 * asynchronous on the handle's stream; otherwise host pointers. */
dips_status dips_frame_callback_batch(dips_handle *h, uint32_t width, uint32_t height, const uint8_t *frames,
                                      uint32_t n_frames, uint8_t *out);

/* Where the last dips_frame_callback call that took the zero-copy striped
 * path (steady state, window 1, host pointers) spent its time -- the
 * per-phase record of the per-frame call pattern (dips/src/frame_extractor.rs:
 * 206-276 -> lib.rs:233-246 -> gpu/mod.rs:170-397, whose per-frame cost is
 * what this path replaces).  Writes up to `cap` values to `us`, *n = the
 * number available (DIPS_CALLBACK_PHASES), in this order:
 *   0 sync     us from the call's start to the end of its stream syncs
 *   1 staged   .. to the last input piece packed into pinned memory
 *   2 launched .. to the last stripe's kernel launch
 *   3 kernels  .. to the last output task past its wait for its stripe's
 *              kernel (output tasks start once every input piece is taken,
 *              so this is max(kernel done, output task start))
 *   4 wall     .. to the call's return
 *   5 pack_cpu, 6 expand_cpu, 7 wait_cpu: thread-time sums (us) of the copy
 *     pool's staging tasks, output tasks and their waits for the kernels
 *   8 threads  copy-pool threads (workers + the calling thread)
 *   9 stripes  row stripes the frame was cut into
 *  10 expand   us from the call's start to the first output task's start
 * DIPS_ERR_STATE if no such call has completed on `h`. */
#define DIPS_CALLBACK_PHASES 11u
dips_status dips_callback_phases(const dips_handle *h, double *us, uint32_t cap, uint32_t *n);

/* Copy the start texture (RGBA8 gray, pre_compute_shader.wgsl:92-132) built
 * at the 4th frame.  Returns 1 if available, 0 if not yet built. */
int dips_start_texture(dips_handle *h, uint8_t *out_rgba, size_t cap);

/* Frame-range sharding of the dips-compat path ("dips-compat
 * T=4 needs a 3-frame halo"): put the handle in the state ComputeState has
 * after frame_callback of global frames 0..t0-1 (dips/src/lib.rs:233-246;
 * ring and start texture of dips/src/gpu/mod.rs:170-216, bind_groups.rs:
 * 407-427), rebuilt from the start texture S (dips_start_texture of the
 * handle that saw frames 0..3) and the raw RGBA8 frames t0-3, t0-2, t0-1
 * (`halo`, 3 contiguous frames in that order; for spatial_window_size > 1
 * they are filtered into the ring as compute_main would have).  Requires
 * t0 >= 7.  Device pointers with DIPS_FLAG_DEVICE_PTRS
 * (asynchronous), host pointers otherwise. */
dips_status dips_compat_resume(dips_handle *h, uint32_t width, uint32_t height,
                               const uint8_t *start_rgba, const uint8_t *halo, uint64_t t0);

/* North-star batch path: the per-frame difference series of `n_frames`
 * contiguous frames (each width*height*C bytes, C from params.format).
 *   ref: overall mode -> the reference frame (NULL = frames[0]);
 *        per-frame mode -> the frame preceding frames[0] (NULL = frames[0]).
 *   series: n_frames entries (required).
 *   absdiff_map: optional n_frames*width*height*C bytes, |F_t - R| per byte.
 * With DIPS_FLAG_DEVICE_PTRS all four pointers are device pointers and the
 * call is asynchronous on the handle's stream; otherwise they are host
 * pointers and the call returns when the results are in host memory. */
dips_status dips_diff_series(dips_handle *h, uint32_t width, uint32_t height,
                             const uint8_t *frames, uint32_t n_frames,
                             const uint8_t *ref, dips_series_entry *series,
                             uint8_t *absdiff_map);

/* f64 intensity sum of one entry: si_fixed * 2^-32. */
double dips_series_si(const dips_series_entry *e);

/* Streaming front-end feed (next-1 of SURVEY.md s8f): frames in pageable or
 * pinned HOST memory are staged through pinned buffers and copied to HBM
 * with hipMemcpyAsync on a side stream, overlapping the series kernel of the
 * previous chunk.  Same semantics as dips_diff_series with host pointers;
 * `chunk_frames` = frames per DMA chunk (0 = automatic). */
dips_status dips_diff_series_streamed(dips_handle *h, uint32_t width, uint32_t height,
                                      const uint8_t *host_frames, uint32_t n_frames,
                                      const uint8_t *host_ref, dips_series_entry *series,
                                      uint32_t chunk_frames);

/* The series resolved in space: a rows x cols grid over a region of interest.
 *
 * rect[4] = {x, y, w, h} of cell (row, col) of a rows x cols grid over roi
 * (roi[4] = {x, y, w, h}; NULL = the whole width x height frame).
 * Columns split [x, x+w) as dips_shard_range splits frames: column c covers
 * [x + c*w/cols, x + (c+1)*w/cols); rows likewise.  Host only, no device.
 * DIPS_ERR_INVALID for a null rect, rows or cols of 0 or beyond the roi's
 * extent, an roi of zero extent or one that leaves the frame, row >= rows or
 * col >= cols. */
dips_status dips_grid_cell(uint32_t width, uint32_t height, const uint32_t *roi,
                           uint32_t rows, uint32_t cols, uint32_t row, uint32_t col, uint32_t *rect);

/* dips_diff_series per cell: cells[(t*rows + r)*cols + c] is exactly the entry
 * dips_diff_series gives for the frames and ref cropped to that cell
 * (n_frames*rows*cols entries, one read of the batch).  ref, the mode, the
 * format, tau, chroma_filter and DIPS_FLAG_DEVICE_PTRS keep the meaning they
 * have in dips_diff_series (device pointers: asynchronous on the handle's
 * stream; host pointers: staged through HBM, synchronous; roi is always a
 * host pointer, read before the call returns).  n_frames == 0 returns OK and
 * writes nothing.  DIPS_ERR_INVALID for a null argument, the grid and roi
 * errors of dips_grid_cell, and n_frames*rows*cols >= 2^30. */
dips_status dips_diff_series_grid(dips_handle *h, uint32_t width, uint32_t height,
                                  const uint8_t *frames, uint32_t n_frames, const uint8_t *ref,
                                  const uint32_t *roi, uint32_t rows, uint32_t cols,
                                  dips_series_entry *cells);

/* The series summed over time per pixel of a region of interest (the
 * activity map of a clip): sums[(py - y)*w + (px - x)] is the sum over t of
 * the entry dips_diff_series gives for frame t when frames and reference are
 * cropped to the single pixel (px, py) -- equivalently the sum over t of
 * dips_diff_series_grid's cells with rows = h, cols = w.  roi_w * roi_h
 * entries; every field an exact u64 sum.  Mode, format, tau, chroma_filter,
 * ref and DIPS_FLAG_DEVICE_PTRS as in dips_diff_series (device pointers:
 * asynchronous on the handle's stream; host pointers: staged through HBM,
 * synchronous; roi is always a host pointer, read before the call returns).
 * accumulate == 0: sums is overwritten (zero-filled when n_frames == 0);
 * accumulate != 0: the batch's sums are added to what sums holds (nothing is
 * written when n_frames == 0) -- a clip longer than memory goes chunk by
 * chunk, with the previous chunk's last frame as ref in 'per-frame' mode or
 * the same reference in 'overall' mode, and per-rank maps of a sharded clip
 * are combined the same way.  DIPS_ERR_INVALID for null frames with
 * n_frames > 0, null sums, the roi errors of dips_grid_cell (at rows = cols
 * = 1) and a region of 2^30 pixels or more. */
dips_status dips_diff_pixel_sums(dips_handle *h, uint32_t width, uint32_t height,
                                 const uint8_t *frames, uint32_t n_frames, const uint8_t *ref,
                                 const uint32_t *roi, uint32_t accumulate,
                                 dips_series_entry *sums);

/* Bytes of one row of a change mask of a region roi_w pixels wide:
 * 4 * ((roi_w + 31) / 32).  Host only, no device. */
uint32_t dips_mask_row_bytes(uint32_t roi_w);

/* The per-frame change mask of a region of interest, one bit per pixel (the
 * "difference pixels" themselves): for roi = {x, y, w, h} (NULL = the whole
 * frame), frame t and region pixel (i, j),
 *   bit(t, j, i) = the count field of the entry dips_diff_series gives for
 *                  frame t when frames and reference are cropped to the
 *                  single pixel (x + i, y + j)
 * -- 0 or 1, equal to dips_diff_series_grid's cells[t] with rows = h and
 * cols = w.  The compare is strict (an unchanged pixel is 0 even at tau = 0),
 * and in 'per-frame' mode with ref == NULL frame 0 is all zero.  The
 * reference has no counterpart: it keeps |dI| per pixel only inside its
 * shader (dips_shader.wgsl:64-82) and returns the coloured visualisation.
 * Layout of mask: a row is dips_mask_row_bytes(w) bytes, a frame h rows,
 * frames contiguous (n_frames * h * row_bytes bytes); bit i of a row is bit
 * (i & 7) of byte (i >> 3), i.e. bit (i & 31) of the little-endian u32 word
 * (i >> 5).  The pad bits of a row's last word are written as 0 and the call
 * writes every byte of the mask: the caller need not clear it.
 * Mode, format, tau, chroma_filter, ref and DIPS_FLAG_DEVICE_PTRS as in
 * dips_diff_series (device pointers: asynchronous on the handle's stream,
 * mask 4-byte aligned, frames and ref at any byte alignment; host pointers:
 * staged through HBM, synchronous, any alignment; roi is always a host
 * pointer, read before the call returns).  n_frames == 0 returns OK and
 * writes nothing.  A clip longer than memory goes chunk by chunk with no
 * further machinery: in 'per-frame' mode pass the previous chunk's last
 * frame as ref, in 'overall' mode the same reference each time.
 * DIPS_ERR_INVALID for null frames or mask with n_frames > 0, a device mask
 * that is not 4-byte aligned, the roi errors of dips_grid_cell (at rows =
 * cols = 1) and a region of 2^30 pixels or more. */
dips_status dips_diff_change_mask(dips_handle *h, uint32_t width, uint32_t height,
                                  const uint8_t *frames, uint32_t n_frames, const uint8_t *ref,
                                  const uint32_t *roi, uint8_t *mask);

/* The change times per pixel of a region of interest: when each pixel first
 * and last changed and for how long it changed without a break.  With
 * bit(t, j, i) exactly dips_diff_change_mask's bit of frame t and region pixel
 * (i, j) (strict compare; 'per-frame' mode with ref == NULL: frame 0 all
 * zero) and g = t0 + t the global index of frames[t], the state of a pixel is
 * four u32, initially {NONE, NONE, 0, 0}, and the fold of one frame is
 *   bit = 1: first = (first == NONE ? g : first), last = g, run_cur += 1,
 *            run_max = max(run_max, run_cur)
 *   bit = 0: run_cur = 0
 * so after frames g = t0 .. t0 + n_frames - 1 in order: first / last the
 * smallest / largest g with bit 1 (DIPS_TIME_NONE if none yet: the arrival
 * map and the motion-history image), run_max the longest run of consecutive
 * frames with bit 1 (dwell), run_cur the run that ends at the newest frame (0
 * if its bit is 0; carried so that a run across two calls is counted whole).
 * Layout of times: four planes of w * h u32, times[k*w*h + j*w + i] with k =
 * DIPS_TIMES_FIRST, _LAST, _RUN_MAX, _RUN_CUR; each plane is an image.
 * accumulate == 0: the call starts from the initial state and overwrites
 * times (with n_frames == 0 it writes the initial state); accumulate != 0:
 * the batch is folded onto the state times holds (nothing is written when
 * n_frames == 0); the caller promises that the batch follows the frames
 * folded before without a gap -- a clip longer than memory goes chunk by
 * chunk with t0 = the frames folded so far and the previous chunk's last
 * frame as ref in 'per-frame' mode, the same reference in 'overall' mode.
 * Mode, format, tau, chroma_filter, ref and DIPS_FLAG_DEVICE_PTRS as in
 * dips_diff_pixel_sums (device pointers: asynchronous on the handle's stream,
 * times 4-byte aligned; host pointers: staged through HBM, synchronous, the
 * state uploaded first when accumulating; roi is always a host pointer, read
 * before the call returns).  DIPS_ERR_INVALID for null frames with n_frames
 * > 0, null times, a device times that is not 4-byte aligned, the roi errors
 * of dips_grid_cell (at rows = cols = 1), a region of 2^30 pixels or more and
 * t0 + n_frames > 0xFFFFFFFF (index 0xFFFFFFFF is DIPS_TIME_NONE); times is
 * then untouched. */
#define DIPS_TIME_NONE 0xFFFFFFFFu
#define DIPS_TIMES_FIRST 0u
#define DIPS_TIMES_LAST 1u
#define DIPS_TIMES_RUN_MAX 2u
#define DIPS_TIMES_RUN_CUR 3u
#define DIPS_TIMES_PLANES 4u
dips_status dips_diff_pixel_times(dips_handle *h, uint32_t width, uint32_t height,
                                  const uint8_t *frames, uint32_t n_frames, const uint8_t *ref,
                                  const uint32_t *roi, uint32_t t0, uint32_t accumulate,
                                  uint32_t *times);

/* The running-average background model of a region of interest and the
 * change mask taken against it: a reference that adapts, where 'overall'
 * breaks under drifting light and 'per-frame' sees only the edges of a moving
 * object.  The reference has no counterpart.  Exact and integer.
 * State: per region pixel and channel c < C (RGBA8's alpha is tracked like
 * any channel) a u16 B in 8.8 fixed point, 0 <= B <= 65280.  rate_shift k in
 * 0 .. 8 gives the update rate 2^-k.  For frame t, in order, per pixel:
 *   R[c]  = (B[c] + 128) >> 8                  the reference bytes (<= 255)
 *   bit(t, j, i) = dips_diff_change_mask's bit of the single frame F_t in
 *                  'overall' mode with reference R: strict compare, the same
 *                  tau and chroma_filter; params.mode is not consulted
 *   B'[c] = B[c] - ((B[c] + h) >> k) + (F[c] << (8 - k)),  h = (1 << k) >> 1
 * the update skipped for the whole pixel when bg_flags has DIPS_BG_SELECTIVE
 * and bit = 1 (foreground is not absorbed).  B = 256 F is a fixed point, for
 * a static input R settles on F exactly, and k = 0 gives B' = 256 F: the mask
 * is then dips_diff_change_mask's in 'per-frame' mode with the same ref.
 * accumulate == 0: the initial state is B = 256 ref (ref == NULL: 256
 * frames[0], so frame 0 is all zero); with n_frames == 0 the call writes the
 * initial state (ref is then required).  accumulate != 0: the state
 * background holds is continued and ref must be NULL; nothing is written when
 * n_frames == 0.  A clip longer than memory goes chunk by chunk.
 * Layout of background: C planes of w * h u16, background[c*w*h + j*w + i],
 * each plane an image; required, 2-byte aligned, written in full.  mask:
 * exactly dips_diff_change_mask's layout (pad bits 0, every byte written), or
 * NULL to estimate the background alone.
 * roi, format, tau, chroma_filter, DIPS_FLAG_DEVICE_PTRS (asynchronous on the
 * handle's stream; mask 4-byte aligned) and host pointers (staged through
 * HBM, synchronous, the state uploaded first when accumulating) as in
 * dips_diff_pixel_times.  DIPS_ERR_INVALID, the outputs untouched, for
 * rate_shift > 8, unknown bg_flags bits, null frames with n_frames > 0, null
 * background, ref given with accumulate, no ref and no frames without
 * accumulate, a misaligned device background or mask, the roi errors of
 * dips_grid_cell (at rows = cols = 1) and a region of 2^30 pixels or more. */
#define DIPS_BG_SELECTIVE 1u
#define DIPS_BG_MAX_RATE_SHIFT 8u
dips_status dips_diff_background_mask(dips_handle *h, uint32_t width, uint32_t height,
                                      const uint8_t *frames, uint32_t n_frames, const uint8_t *ref,
                                      const uint32_t *roi, uint32_t rate_shift, uint32_t bg_flags,
                                      uint32_t accumulate, uint16_t *background, uint8_t *mask);

/* The Sigma-Delta background model of a region of interest and its change
 * mask: a threshold that adapts per pixel, where every other mask compares
 * with one global tau (Manzanera & Richefeu, 2007).  The reference has no
 * counterpart.  Exact and integer: no f32, no rate multiply, no tau.
 * It works in the integer intensity J of a pixel, 0 <= J <= 510: max + min of
 * the R, G, B bytes with no chroma filter, 2 * channel with
 * DIPS_CHROMA_R / G / B, 2 * g for GRAY8; RGBA8's alpha never enters.
 * State: per region pixel two u16, a running median M of J (0 <= M <= 510)
 * and a running estimate V of the pixel's own temporal activity (v_min <= V
 * <= v_max).  Parameters: n_amp N in 1 .. 15, 0 <= v_min <= v_max <= 510.
 * For frame t, in order, per pixel (update, then decide):
 *   M' = M + sgn(J_t - M)
 *   D  = |J_t - M'|
 *   V' = clamp(V + sgn(N * D - V), v_min, v_max)   if D != 0, else V' = V
 *   bit(t, j, i) = D > V'                          strict, like every mask
 * M cannot leave [0, 510], since it moves toward a J inside it; N * D <= 7650
 * and every difference above fits a signed 16-bit lane (the kernels rely on
 * it).  params.tau and params.mode are not consulted; chroma_filter is.
 * accumulate == 0: the initial state is M = J(ref) (ref == NULL: J(frames[0]),
 * so frame 0 is all zero) and V = v_min; with n_frames == 0 the call writes
 * that initial state (ref is then required).  accumulate != 0: the state the
 * buffer holds is continued and ref must be NULL; nothing is written when
 * n_frames == 0; the caller promises that the held V lies in [v_min, v_max]
 * and M in [0, 510].  A clip of any length goes chunk by chunk, bit for bit.
 * Layout of state: DIPS_SD_PLANES planes of w * h u16, state[p*w*h + j*w + i]
 * with plane 0 = M and plane 1 = V, each plane an image; required, 2-byte
 * aligned, written in full.  mask: exactly dips_diff_change_mask's layout
 * (pad bits 0, every byte written), or NULL for the state alone.
 * roi, format, DIPS_FLAG_DEVICE_PTRS (asynchronous on the handle's stream;
 * mask 4-byte aligned) and host pointers (staged through HBM, synchronous,
 * the state uploaded first when accumulating) as in
 * dips_diff_background_mask.  DIPS_ERR_INVALID, the outputs untouched, for
 * n_amp of 0 or > 15, v_min > v_max, v_max > 510, null frames with n_frames
 * > 0, null state, ref given with accumulate, no ref and no frames without
 * accumulate, a misaligned device state or mask, the roi errors of
 * dips_grid_cell (at rows = cols = 1) and a region of 2^30 pixels or more. */
#define DIPS_SD_MAX_AMP 15u
#define DIPS_SD_MAX_V 510u
#define DIPS_SD_PLANES 2u
dips_status dips_diff_sigma_delta_mask(dips_handle *h, uint32_t width, uint32_t height,
                                       const uint8_t *frames, uint32_t n_frames, const uint8_t *ref,
                                       const uint32_t *roi, uint32_t n_amp, uint32_t v_min,
                                       uint32_t v_max, uint32_t accumulate, uint16_t *state,
                                       uint8_t *mask);

/* The connected components of a change mask, frame by frame: the blobs and
 * bounding boxes the README promises the mask "feeds" (difference ->
 * threshold -> components -> boxes).  The reference has no counterpart.  A
 * second stage behind dips_diff_change_mask: it reads the mask, not the
 * frames, so it serves every pixel format, and the answer is combinatorial,
 * hence exact.
 * Input: mask in exactly dips_diff_change_mask's layout -- n_frames frames of
 * roi_h rows of dips_mask_row_bytes(roi_w) bytes, bit i of a row = bit
 * (i & 31) of little-endian word i >> 5.  The pad bits of a row's last word
 * are ignored, whatever they hold.  Frames are independent: nothing connects
 * the last row of frame t to frame t + 1, or a row's end to the next row.
 * Components: the set pixels of frame t partitioned under connectivity 4
 * (edge neighbours) or 8 (edge and corner neighbours).  The anchor of a
 * component is j*roi_w + i of its first pixel in row-major order; a
 * component is kept if its area is >= min_area (0 and 1 keep all); the kept
 * components of a frame are ordered by ascending anchor.
 * Outputs: counts[t] = the kept components of frame t, not capped by
 * max_boxes (truncation is visible).  boxes[(t*max_boxes + k)*DIPS_BOX_WORDS
 * + f] is the k-th kept component for k < min(counts[t], max_boxes); every
 * other record is zeros and every word of boxes is written.  Fields: X0, Y0
 * the smallest i, j (region-relative), X1, Y1 the largest i, j plus 1 (the
 * box is [X0, X1) x [Y0, Y1)), AREA the pixels, ANCHOR as above, CX256 /
 * CY256 the centroid in 1/256 pixel: (S / area)*256 + ((S % area)*256) / area
 * with S the exact 64-bit sum of i (of j), both divisions floor.  labels
 * (NULL: not produced) is labels[(t*roi_h + j)*roi_w + i]: 0 for a clear bit
 * or a dropped component, else 1 + the component's rank among the frame's
 * kept ones (not capped by max_boxes: label k + 1 is record k where both
 * exist).
 * chunk_frames: frames labelled per round in handle-owned scratch (grown on
 * demand, freed with the handle); 0 = as many as keep it within 1 GiB, at
 * least one.  The result does not depend on it; DIPS_ERR_NOMEM if the scratch
 * cannot be allocated.  The time depends on the bits.
 * DIPS_FLAG_DEVICE_PTRS: all four pointers are device pointers, 4-byte
 * aligned, the call asynchronous on the handle's stream; else host pointers
 * of any alignment, staged through HBM, synchronous.  DIPS_FLAG_TIME_KERNEL:
 * one entry for all launches of the call.  n_frames == 0: DIPS_OK, nothing
 * written.  DIPS_ERR_INVALID, outputs untouched: null mask or counts, null
 * boxes with max_boxes > 0, a misaligned device pointer, connectivity not 4
 * or 8, roi_w or roi_h of 0 or >= 2^24 (CX256 stays in 32 bits), a region of
 * 2^30 pixels or more, n_frames*max_boxes*DIPS_BOX_WORDS >= 2^32. */
#define DIPS_BOX_X0 0u
#define DIPS_BOX_Y0 1u
#define DIPS_BOX_X1 2u
#define DIPS_BOX_Y1 3u
#define DIPS_BOX_AREA 4u
#define DIPS_BOX_ANCHOR 5u
#define DIPS_BOX_CX256 6u
#define DIPS_BOX_CY256 7u
#define DIPS_BOX_WORDS 8u
dips_status dips_mask_components(dips_handle *h, const uint8_t *mask, uint32_t n_frames,
                                 uint32_t roi_w, uint32_t roi_h,
                                 uint32_t connectivity, uint32_t min_area, uint32_t max_boxes,
                                 uint32_t chunk_frames,
                                 uint32_t *counts, uint32_t *boxes, uint32_t *labels);

/* The components of a change mask linked across frames: tracks.  The step
 * from "boxes per frame" to the identity of a moving object, how long it has
 * been visible, where it came from when one blob splits and where it went
 * when two merge (difference -> threshold -> morphology -> components ->
 * tracks).  The reference has no counterpart.  It reads masks only, so it
 * serves every pixel format and both mask sources, and it is exact.
 * mask, roi_w, roi_h, connectivity, min_area, max_boxes (K), chunk_frames,
 * counts and boxes mean exactly what they mean in dips_mask_components, and
 * counts and boxes of this call equal that call's, word for word, on the same
 * arguments.  The records of frame t are its first m_t = min(counts[t], K)
 * kept components.  K must be 1 .. DIPS_TRACK_MAX_BOXES: the link stage keeps
 * a K x K overlap table per frame.
 * Overlap: for record a of frame t and record b of frame t - 1, ov(t, a, b)
 * is the number of pixels (j, i) that lie in component a in frame t and in
 * component b in frame t - 1.  Components beyond K and components dropped by
 * min_area take no part.  Frame -1 is prev_mask (one frame in the mask
 * layout, pad bits ignored), labelled with the same arguments; if prev_mask
 * is NULL, frame 0 has no predecessor and all its ov are 0.
 * links[(t*K + k)*DIPS_LINK_WORDS + f], for k < m_t:
 *   PREV     the b with the largest ov(t, k, b) > 0, the smallest such b on a
 *            tie, DIPS_LINK_NONE if every ov is 0;
 *   OVERLAP  that ov (0 with NONE);
 *   TRACK, AGE  with NEXT(t - 1, b) the a with the largest ov(t, a, b) > 0,
 *            the smallest a on a tie: record k continues b when PREV = b and
 *            NEXT(t - 1, b) = k, a mutual best match.  Then TRACK = TRACK of
 *            (t - 1, b) and AGE = its AGE + 1.  Otherwise the record is a
 *            head: AGE = 0 and TRACK is the next unused id.  Ids are handed
 *            out to heads in ascending (t, k) order, starting at state[0] (0
 *            when state is NULL); arithmetic on ids and ages is modulo 2^32.
 * For k >= m_t the record is {NONE, 0, NONE, 0}.  Every word of links is
 * written.  Consequences: a blob that splits keeps its track in the child
 * that shares the most pixels with it, and the other child is a head whose
 * PREV still names the parent; of two blobs that merge, the one contributing
 * more pixels continues; an object that vanishes for a frame returns under a
 * new id.
 * state (NULL: no carry) is 1 + 2K words, read before and written after:
 * [0] the next unused id, [1 + k] TRACK of record k of the predecessor frame,
 * [1 + K + k] its AGE ({NONE, 0} for k beyond its records).  On return it
 * describes the call's last frame; it is unchanged when n_frames = 0.  It is
 * read for tracks and ages only when prev_mask is given, and prev_mask
 * without state is DIPS_ERR_INVALID.  A clip of any length goes call by call:
 * pass the previous call's last mask frame as prev_mask and the same state
 * buffer, and the result equals the one call over the whole clip, bit for
 * bit.  roi_w, roi_h, connectivity, min_area and max_boxes must be the same
 * from call to call: prev_mask is labelled with this call's, and state is
 * indexed by its records.  state given without prev_mask is a scene cut: the
 * ids go on, every record of frame 0 is a head.
 * chunk_frames, DIPS_FLAG_TIME_KERNEL and n_frames == 0 as in
 * dips_mask_components; the scratch of a round includes its overlap tables,
 * and a round holds at most 256 frames.
 * DIPS_FLAG_DEVICE_PTRS: all six pointers are device pointers, 4-byte
 * aligned, the call asynchronous on the handle's stream with no host
 * synchronisation (the carried id stays on the device); else host pointers of
 * any alignment, staged through HBM, synchronous.  DIPS_ERR_INVALID, outputs
 * untouched: that call's cases, and K = 0 or K > DIPS_TRACK_MAX_BOXES, null
 * boxes or links, prev_mask without state.  DIPS_ERR_NOMEM if the scratch
 * cannot be allocated. */
#define DIPS_LINK_PREV 0u
#define DIPS_LINK_OVERLAP 1u
#define DIPS_LINK_TRACK 2u
#define DIPS_LINK_AGE 3u
#define DIPS_LINK_WORDS 4u
#define DIPS_LINK_NONE 0xFFFFFFFFu
#define DIPS_TRACK_MAX_BOXES 256u
dips_status dips_mask_tracks(dips_handle *h, const uint8_t *mask, uint32_t n_frames,
                             uint32_t roi_w, uint32_t roi_h,
                             uint32_t connectivity, uint32_t min_area, uint32_t max_boxes,
                             uint32_t chunk_frames,
                             const uint8_t *prev_mask, uint32_t *state,
                             uint32_t *counts, uint32_t *boxes, uint32_t *links);

/* The shape of every component of a change mask: exact second-order moments
 * (elongation, orientation), the crack perimeter (compactness), the Euler
 * number (holes) and the sum and peak of a per-pixel weight (how strongly it
 * changed): what a box cannot say.  The reference has no counterpart.  Every
 * field is an integer sum over the set bits of a component, hence exact.
 * mask, roi_w, roi_h, connectivity, min_area, max_boxes (K), chunk_frames,
 * counts and boxes mean exactly what they mean in dips_mask_components, and
 * counts and boxes of this call equal that call's, word for word, on the same
 * arguments; so do dips_mask_tracks', so shapes record k of frame t describes
 * the component of link record k.
 * weights: NULL (no weights) or n_frames*roi_h*roi_w bytes, one u8 per pixel
 * of the region, row stride roi_w, at any byte alignment.  Nothing produces
 * it inside this call: the abs-diff map of a whole-frame GRAY8 series, or any
 * saliency plane of the caller's.
 * shapes[(t*K + k)*DIPS_SHAPE_WORDS + f] for k < min(counts[t], K); every
 * other record is zeros and every word of shapes is written.  With C the set
 * of pixels (i, j) of the component, region-relative; the 64-bit fields are
 * stored as (low word, high word) at even word offsets:
 *   SX, SY, SXX, SYY, SXY  the sums over C of i, j, i*i, j*j, i*j (64 bits);
 *   WSUM   the sum over C of weight(i, j) (64 bits); 0 without weights;
 *   WMAX   the largest weight(i, j) over C; 0 without weights;
 *   CRACKS_V  the number of pairs (p in C, horizontal neighbour q = (i-1, j)
 *          or (i+1, j)) with q clear or outside the region;
 *   CRACKS_H  the same for the vertical neighbours (i, j-1) and (i, j+1);
 *   EULER  int32 in two's complement: 1 minus the number of holes of C taken
 *          alone.  The holes are the bounded connected components of the
 *          complement of C in the plane under the dual connectivity (4 when
 *          connectivity is 8, 8 when it is 4); everything outside the region
 *          is background.  A component that lies inside a hole of C does not
 *          fill it.
 * A set horizontal or vertical neighbour of a pixel of C is in C under both
 * connectivities, so the crack fields depend on the bits alone; CRACKS_V +
 * CRACKS_H is the crack perimeter, CRACKS_V / 2 the number of maximal row
 * runs of C.  The area is boxes' AREA.
 * chunk_frames, the scratch, DIPS_FLAG_TIME_KERNEL (one entry for all
 * launches of the call) and n_frames == 0 as in dips_mask_components; the
 * result does not depend on chunk_frames.  DIPS_FLAG_DEVICE_PTRS: device
 * pointers, the call asynchronous on the handle's stream; shapes must be
 * 8-byte aligned, mask, counts and boxes 4-byte aligned, weights may have any
 * alignment; else host pointers of any alignment, staged through HBM,
 * synchronous.  DIPS_ERR_INVALID, outputs untouched: that call's cases, and
 * roi_w or roi_h above 65536 (every sum stays below 2^62),
 * n_frames*max_boxes*DIPS_SHAPE_WORDS >= 2^32, null shapes with max_boxes >
 * 0, a misaligned shapes.  DIPS_ERR_NOMEM if the scratch cannot be allocated. */
#define DIPS_SHAPE_SX 0u
#define DIPS_SHAPE_SY 2u
#define DIPS_SHAPE_SXX 4u
#define DIPS_SHAPE_SYY 6u
#define DIPS_SHAPE_SXY 8u
#define DIPS_SHAPE_WSUM 10u
#define DIPS_SHAPE_WMAX 12u
#define DIPS_SHAPE_CRACKS_V 13u
#define DIPS_SHAPE_CRACKS_H 14u
#define DIPS_SHAPE_EULER 15u
#define DIPS_SHAPE_WORDS 16u
dips_status dips_mask_shapes(dips_handle *h, const uint8_t *mask, const uint8_t *weights,
                             uint32_t n_frames, uint32_t roi_w, uint32_t roi_h,
                             uint32_t connectivity, uint32_t min_area, uint32_t max_boxes,
                             uint32_t chunk_frames,
                             uint32_t *counts, uint32_t *boxes, uint32_t *shapes);

/* The binary morphology of a change mask, frame by frame: the cleanup
 * between threshold and components (difference -> threshold -> morphology ->
 * components -> boxes).  The reference has no counterpart.  A second stage
 * like dips_mask_components: it reads a mask and writes a mask, so it serves
 * every pixel format, and the answer is exact.
 * Input and output: both in exactly dips_diff_change_mask's layout --
 * n_frames frames of roi_h rows of dips_mask_row_bytes(roi_w) bytes, bit i of
 * a row = bit (i & 31) of little-endian word i >> 5.  The pad bits of the
 * input are ignored, whatever they hold; those of the output are written as
 * 0, and every byte of mask_out is written.  Frames are independent, and so
 * are rows' ends: nothing reaches from the last row of frame t into frame
 * t + 1, or from a row's end into the next row.
 * Structuring element B (symmetric): DIPS_MORPH_BOX {(dx, dy): |dx| <= rx,
 * |dy| <= ry}; DIPS_MORPH_DIAMOND {(dx, dy): |dx| + |dy| <= rx}, ry must
 * equal rx.  With X the set pixels of one frame inside the region D =
 * [0, roi_w) x [0, roi_h):
 *   dilate(X) = {p in D: some b in B has p + b in X}   (outside D is clear)
 *   erode(X)  = {p in D: every b in B with p + b in D has p + b in X}
 *               (outside D counts as set: B is clipped to the region)
 *   open = erode, then dilate;  close = dilate, then erode.
 * This is OpenCV's default border (scipy: binary_dilation(border_value=0),
 * binary_erosion(border_value=1)).  It makes the two an adjunction on the
 * subsets of D: erode(X) = D \ dilate(D \ X), open(X) <= X <= close(X), open
 * and close are idempotent, a frame of all ones erodes to all ones.  The
 * diamond of radius r equals r applications of the diamond of radius 1.
 * rx = ry = 0 copies the mask with the pad bits zeroed; a radius larger than
 * the region is legal.  DIPS_MORPH_MAX_RADIUS is 15 so that open and close
 * reach 2 * 15 = 30 < 32 bits sideways and a word depends on its two
 * neighbour words only; larger boxes compose from two calls.
 * One kernel launch per call, no scratch; the time does not
 * depend on the bits.
 * DIPS_FLAG_DEVICE_PTRS: both pointers are device pointers, 4-byte aligned,
 * the call asynchronous on the handle's stream; else host pointers of any
 * alignment, staged through HBM, synchronous.  DIPS_FLAG_TIME_KERNEL: one
 * entry for all launches of the call.  n_frames == 0: DIPS_OK, nothing
 * written.  DIPS_ERR_INVALID, mask_out untouched: a null pointer with
 * n_frames > 0, a misaligned device pointer, op > 3, shape > 1, rx or ry >
 * DIPS_MORPH_MAX_RADIUS, a diamond with ry != rx, roi_w or roi_h of 0, a
 * region of 2^30 pixels or more, and input and output byte ranges that
 * overlap at all (in place is refused, not silently wrong). */
#define DIPS_MORPH_ERODE 0u
#define DIPS_MORPH_DILATE 1u
#define DIPS_MORPH_OPEN 2u    /* erode, then dilate */
#define DIPS_MORPH_CLOSE 3u   /* dilate, then erode */
#define DIPS_MORPH_BOX 0u     /* B = {(dx, dy): |dx| <= rx, |dy| <= ry} */
#define DIPS_MORPH_DIAMOND 1u /* B = {(dx, dy): |dx| + |dy| <= rx}; ry must equal rx */
#define DIPS_MORPH_MAX_RADIUS 15u
dips_status dips_mask_morph(dips_handle *h, const uint8_t *mask_in, uint32_t n_frames,
                            uint32_t roi_w, uint32_t roi_h,
                            uint32_t op, uint32_t shape, uint32_t rx, uint32_t ry,
                            uint8_t *mask_out);

/* The temporal m-of-k vote on a change mask: the cleanup in time, where
 * dips_mask_morph cleans in space (difference -> threshold -> vote ->
 * morphology -> components).  The reference has no counterpart.  It reads a
 * mask and writes a mask, so it serves every pixel format and every mask
 * source, and the answer is exact.
 * Input and output: both in exactly dips_diff_change_mask's layout.  With
 * k = window, m = votes and X_t the input frame t, 0 <= t < n_frames:
 *   out(t, j, i) = 1  iff  #{s: t - k + 1 <= s <= t, X_s(j, i) = 1} >= m.
 * The vote is causal: output frame t belongs to input frame t and looks at
 * it and the k - 1 frames before it.  The frames before the clip, X_{-(k-1)}
 * .. X_{-1}, are the k - 1 frames of history_in, oldest first, in the same
 * layout; history_in = NULL means that every frame before the clip is clear
 * (with m = k the first k - 1 output frames are then all clear).
 *   m = 1            temporal dilation (OR of the window): bridges dropouts
 *   m = k            temporal erosion (AND); k = 2 on a 'per-frame' mask is
 *                    the three-frame difference D_{t-1} AND D_t
 *   m = k / 2 + 1    temporal median: removes flicker and fills dropouts
 *                    shorter than k / 2 without touching shape
 * The pad bits of mask_in and history_in are ignored, whatever they hold;
 * those of mask_out and history_out are written as 0, and every byte of both
 * outputs is written.
 * history_out may be NULL.  When given it receives the last k - 1 frames of
 * the sequence history ++ input: for n_frames >= k - 1 the last k - 1 input
 * frames, otherwise the newest k - 1 - n_frames history frames (clear ones
 * for NULL history) followed by the n_frames input frames.  It is written
 * also when n_frames == 0 (the history with its pad bits zeroed, or all
 * clear).  So a clip fed call by call, one call's history_out as the next
 * call's history_in, gives byte for byte the output and the history of one
 * call over the whole clip, for any chunking, one frame per call included.
 * window = 1: votes must be 1, the call copies the mask with the pad bits
 * zeroed, both history pointers are ignored and history_out is not written.
 * window <= DIPS_VOTE_MAX_WINDOW = 31: the count of a pixel fits 5 bits.
 * One launch per call and one more for history_out, no scratch;
 * the time does not depend on the bits.
 * DIPS_FLAG_DEVICE_PTRS: all pointers are device pointers, 4-byte aligned,
 * the call asynchronous on the handle's stream; else host pointers of any
 * alignment, staged through HBM, synchronous.  DIPS_FLAG_TIME_KERNEL: one
 * entry for all launches of the call.  n_frames == 0: DIPS_OK, mask_out
 * untouched, history_out written as above.  DIPS_ERR_INVALID, the outputs
 * untouched: a null mask_in or mask_out with n_frames > 0, window of 0 or
 * above DIPS_VOTE_MAX_WINDOW, votes of 0 or above window, roi_w or roi_h of
 * 0, a region of 2^30 pixels or more, n_frames of 2^31 or more, a
 * misaligned device pointer, and any
 * overlap between the byte range of an output (mask_out: n_frames frames,
 * history_out: window - 1 frames) and that of an input or of the other
 * output (in place is refused, not silently wrong). */
#define DIPS_VOTE_MAX_WINDOW 31u
dips_status dips_mask_vote(dips_handle *h, const uint8_t *mask_in, uint32_t n_frames,
                           uint32_t roi_w, uint32_t roi_h,
                           uint32_t window, uint32_t votes,
                           const uint8_t *history_in, uint8_t *history_out,
                           uint8_t *mask_out);

/* The selection of components of a change mask: the labelling's knowledge of
 * which pixels belong to which object, given back as a mask (difference ->
 * threshold -> vote -> morphology -> selection -> components / statistics).
 * Area opening (drop the components below A pixels, leave the rest bit for
 * bit), reconstruction by marker (keep the components that hold a set bit of
 * another mask: hysteresis thresholding, zone queries, opening by
 * reconstruction), border clearing and, with dips_mask_logic, hole filling.
 * The reference has no counterpart.  It reads masks and writes a mask, so it
 * serves every pixel format and every mask source, and the answer is exact.
 * Input and output: mask, marker and mask_out in exactly
 * dips_diff_change_mask's layout for a region roi_w x roi_h.  Frames are
 * independent.  The components of frame t are those of dips_mask_components
 * under the same connectivity (4 or 8).  A component C of frame t is kept iff
 *   area(C) >= min_area  (0 and 1 keep all),
 *   max_area == 0 or area(C) <= max_area,
 *   marker == NULL or C contains a pixel whose marker bit is set,
 *   DIPS_SELECT_CLEAR_BORDER is not set or C has no pixel in row 0, row
 *   roi_h - 1, column 0 or column roi_w - 1.
 * marker_frames is 1 or n_frames (0 with marker == NULL): with 1 the one
 * marker frame serves every t, with n_frames frame t of the marker serves
 * frame t of the mask.  A marker bit on a clear mask pixel has no effect.
 * mask_out(t) is the union of the kept components of frame t; with
 * DIPS_SELECT_DROPPED it is the mask minus that union, so the two outputs
 * partition the mask.  The pad bits of mask and marker are ignored, whatever
 * they hold; those of mask_out are written as 0, and every byte of mask_out
 * is written.  counts (NULL: not produced): counts[t] = the kept components
 * of frame t, with or without DIPS_SELECT_DROPPED.  With marker == NULL,
 * select == 0 and max_area == 0, counts equals dips_mask_components' counts
 * and mask_out the packing of that call's labels != 0.
 * chunk_frames and the scratch as in dips_mask_components; the result does
 * not depend on chunk_frames.  The labelling's three launches and one or two
 * more; the time depends on the bits.
 * DIPS_FLAG_DEVICE_PTRS: all pointers are device pointers, 4-byte aligned,
 * the call asynchronous on the handle's stream; else host pointers of any
 * alignment, staged through HBM, synchronous.  DIPS_FLAG_TIME_KERNEL: one
 * entry for all launches of the call.  n_frames == 0: DIPS_OK, nothing
 * written.  DIPS_ERR_INVALID, outputs untouched: connectivity not 4 or 8,
 * roi_w or roi_h of 0 or >= 2^24, a region of 2^30 pixels or more, a null
 * mask or mask_out, bits of select other than the two above, max_area != 0
 * and max_area < min_area, a marker with marker_frames not 1 or n_frames, no
 * marker with marker_frames != 0, a misaligned device pointer, and any
 * overlap between the byte range of an output (mask_out: n_frames frames,
 * counts: n_frames words) and that of an input or of the other output.
 * DIPS_ERR_NOMEM if the scratch cannot be allocated. */
#define DIPS_SELECT_CLEAR_BORDER 0x1u /* drop components with a pixel in row 0, row roi_h-1, column 0 or column roi_w-1 */
#define DIPS_SELECT_DROPPED 0x2u      /* write mask \ kept instead of kept */
dips_status dips_mask_select(dips_handle *h, const uint8_t *mask, uint32_t n_frames,
                             uint32_t roi_w, uint32_t roi_h, uint32_t connectivity,
                             uint32_t min_area, uint32_t max_area, uint32_t select,
                             const uint8_t *marker, uint32_t marker_frames,
                             uint32_t chunk_frames, uint8_t *mask_out, uint32_t *counts);

/* Word-wise logic of masks: mask_out(t) = a(t) op b(t) inside the region, for
 * the composites of the mask toolkit (a static zone mask ANDed onto every
 * frame, the complement for hole filling, the union of a mask and its filled
 * holes).  a, b and mask_out in exactly dips_diff_change_mask's layout for a
 * region roi_w x roi_h; b_frames is 1 (the one frame of b serves every t) or
 * n_frames; DIPS_LOGIC_NOT takes no b (b NULL, b_frames 0).  The pad bits of
 * the inputs are ignored, whatever they hold; those of mask_out are written
 * as 0 (DIPS_LOGIC_NOT of a clear frame has exactly roi_w bits per row), and
 * every byte of mask_out is written.  One launch, no scratch; the time does
 * not depend on the bits.  Pointer kinds, DIPS_FLAG_TIME_KERNEL and n_frames
 * == 0 as in dips_mask_select.  DIPS_ERR_INVALID, mask_out untouched: a null
 * a or mask_out, op > 4, DIPS_LOGIC_NOT with b or b_frames != 0, another op
 * without b, b_frames not 1 or n_frames, roi_w or roi_h of 0, a region of
 * 2^30 pixels or more, a misaligned device pointer, mask_out overlapping a or
 * b. */
#define DIPS_LOGIC_AND 0u
#define DIPS_LOGIC_OR 1u
#define DIPS_LOGIC_XOR 2u
#define DIPS_LOGIC_ANDNOT 3u /* a & ~b */
#define DIPS_LOGIC_NOT 4u    /* ~a inside the region; b must be NULL */
dips_status dips_mask_logic(dips_handle *h, const uint8_t *a, uint32_t n_frames,
                            uint32_t roi_w, uint32_t roi_h,
                            uint32_t op, const uint8_t *b, uint32_t b_frames, uint8_t *mask_out);

/* The statistics of a change mask: what dips_diff_series_grid,
 * dips_diff_pixel_sums and dips_diff_pixel_times give for the raw decision
 * |dI| > tau, for any mask -- one taken against a background model, or
 * cleaned by dips_mask_vote or dips_mask_morph.  The reference has no
 * counterpart.  Both calls read a mask in exactly dips_diff_change_mask's
 * layout for a region roi_w x roi_h, so they serve every pixel format and
 * every mask source; the pad bits of the input are ignored, whatever they
 * hold; the answers are exact.
 *
 * dips_mask_counts: counts[(t*rows + r)*cols + c] is the number of set bits
 * of frame t inside dips_grid_cell(roi_w, roi_h, NULL, rows, cols, r, c).
 * rows = cols = 1 is the count series of the mask, rows = roi_h and cols =
 * roi_w the mask unpacked to u32.  Every entry is written.  n_frames == 0
 * returns OK and writes nothing.  DIPS_ERR_INVALID, counts untouched: the
 * grid errors of dips_grid_cell, roi_w or roi_h of 0, a region of 2^30 pixels
 * or more, n_frames * rows * cols >= 2^30, a null pointer with n_frames > 0,
 * a misaligned device pointer, counts overlapping mask.
 *
 * dips_mask_pixel_times: times (four planes of roi_w * roi_h u32 in exactly
 * dips_diff_pixel_times' layout, the same fold with bit(t, j, i) the mask's
 * bit and g = t0 + t, the same DIPS_TIMES_* and DIPS_TIME_NONE) and sums
 * (sums[j*roi_w + i] = the number of frames whose bit is set, modulo 2^32)
 * from one read of the mask.  Either output may be NULL, not both.
 * accumulate == 0: the call starts from the initial state ({NONE, NONE, 0,
 * 0}, sums 0) and overwrites (with n_frames == 0 it writes the initial
 * state); accumulate != 0: the batch is folded onto what the outputs hold
 * (nothing is written when n_frames == 0).  Any chunking of a clip gives,
 * byte for byte, what one call gives, one frame per call and empty calls
 * included; a run across a call boundary is counted whole.  DIPS_ERR_INVALID,
 * the outputs untouched: both outputs null, a null mask with n_frames > 0,
 * roi_w or roi_h of 0, a region of 2^30 pixels or more, times given and t0 +
 * n_frames > 0xFFFFFFFF, a misaligned device pointer, an output overlapping
 * the mask or the other output.
 *
 * Both: DIPS_FLAG_DEVICE_PTRS: the pointers are device pointers, 4-byte
 * aligned, the call asynchronous on the handle's stream; else host pointers
 * of any alignment, staged through HBM, synchronous, the state uploaded first
 * when accumulating.  DIPS_FLAG_TIME_KERNEL: one entry for all launches of a
 * call.  No scratch beyond the per-part summaries of a clip whose frames are
 * cut into parts. */
dips_status dips_mask_counts(dips_handle *h, const uint8_t *mask, uint32_t n_frames,
                             uint32_t roi_w, uint32_t roi_h, uint32_t rows, uint32_t cols,
                             uint32_t *counts);
dips_status dips_mask_pixel_times(dips_handle *h, const uint8_t *mask, uint32_t n_frames,
                                  uint32_t roi_w, uint32_t roi_h, uint32_t t0, uint32_t accumulate,
                                  uint32_t *times, uint32_t *sums);

/* Synthetic frames (shared integer generator, bit-identical to the oracle),
 * global frame indices t0 .. t0+n_frames-1, written to DEVICE memory `dst`. */
dips_status dips_synth_frames(dips_handle *h, uint32_t width, uint32_t height,
                              uint64_t seed, uint64_t t0, uint32_t n_frames, uint8_t *dst);

/* Kernel timing (DIPS_FLAG_TIME_KERNEL): total milliseconds and launch count
 * of the series kernel since the last reset, from hipEvents recorded on the
 * launch stream.  Synchronises the handle's stream. */
dips_status dips_kernel_time(dips_handle *h, double *total_ms, uint64_t *launches);
dips_status dips_kernel_time_reset(dips_handle *h);
/* The same launches one by one: up to `cap` per-launch milliseconds (oldest
 * first) into ms_each, the number of launches held into *launches.  The
 * handle holds the launches since the last reset, at most the most recent
 * 65,536 (beyond that the older half is dropped; dips_kernel_time still
 * counts every launch). */
dips_status dips_kernel_time_each(dips_handle *h, double *ms_each, uint64_t cap, uint64_t *launches);

/* Geometry of the series kernel for a frame shape (for roofline accounting):
 * waves launched, tiles per frame, bytes of partial records per frame. */
dips_status dips_series_geometry(dips_handle *h, uint32_t width, uint32_t height,
                                 uint32_t n_frames, uint64_t *waves, uint64_t *tiles,
                                 uint64_t *partial_bytes);

/* Measured read ceiling: one read-only stream (non-temporal 16-byte loads,
 * grid-stride) over `bytes` of DEVICE memory, synchronous; *ms = its
 * hipEvent duration.  bench.py divides the series kernel's rate by it
 * ("% of a measured read-only-stream ceiling"). */
dips_status dips_read_ceiling(dips_handle *h, const uint8_t *dev_bytes, uint64_t bytes, double *ms);

/* The same with the RGB8 / RGBA8 series kernel's own access shape: its
 * persistent (tile, frame) schedule over n_frames DEVICE frames of
 * width x height (the handle's format and mode; the part-major schedule where
 * the series kernel runs it), 12- / 16-byte vecs, two frames of loads in
 * flight, no compute; *ms = the hipEvent duration. */
dips_status dips_read_ceiling_walk(dips_handle *h, const uint8_t *dev_frames, uint32_t width, uint32_t height,
                                   uint32_t n_frames, double *ms);

/* Library ABI version (DIPS_ABI_VERSION). */
int dips_abi_version(void);

/* ------------------------------------------------------------------------
 * Frame-range sharding of the difference series over one rank per GPU
 * (BASELINE.json north_star: "sharded by frame-range across
 * the 8 GPUs of one node with a single RCCL gather").  The reference is
 * single-device -- one wgpu adapter and queue (dips/src/gpu/mod.rs:66-98,
 * chosen at :71-78) driving frames strictly in order -- so these entry
 * points have no reference counterpart; they let a Rust (or C) host that
 * replaces dips/src/gpu/mod.rs:39-398 with this library use every GPU of a
 * node without any other runtime.
 *
 * Rank r of G owns the contiguous global frames [r*N/G, (r+1)*N/G)
 * (dips_shard_range).  The exchanges are:
 *   'overall':   the reference frame, broadcast from rank 0;
 *   'per-frame': the halo frame r*N/G - 1, sent by rank r-1 to rank r,
 *                overlapped with the series launch over the rank's own frames
 *                1..n-1 (which need no halo);
 *   both:        the per-frame series entries (32 B each), reassembled on
 *                rank 0 by ONE gather (ncclGather, rccl.h:745).
 * No collective touches the frame batch itself.
 *
 * A communicator is one of three transports behind one internal table:
 *   DIPS_COMM_RCCL      RCCL over xGMI (librccl), one process per GPU;
 *   DIPS_COMM_LOOPBACK  ranks as threads of one process on one device,
 *                       stream-ordered hipMemcpyAsync + events (tests, and a
 *                       host that shards one GPU between decoders);
 *   DIPS_COMM_HOST      the caller's own transport (MPI, a torch process
 *                       group, ...) through host-memory callbacks,
 *                       synchronous.
 * Collective contract (as RCCL's): every rank makes the same sequence of
 * sharded calls with the same n_total, mode and shard_flags; an argument
 * error one rank alone detects returns on that rank before any collective
 * and leaves the others waiting in theirs.
 * ------------------------------------------------------------------------ */
typedef struct dips_comm dips_comm;

#define DIPS_COMM_ID_BYTES 128u /* NCCL_UNIQUE_ID_BYTES (rccl.h:40) */
#define DIPS_COMM_RCCL 1
#define DIPS_COMM_LOOPBACK 2
#define DIPS_COMM_HOST 3

/* Caller-supplied transport of DIPS_COMM_HOST: every buffer is HOST memory
 * owned by the library for the call; each function returns 0 on success and
 * any other value on failure.  broadcast: `bytes` from rank `root` into
 * `buf` on every rank (in place).  sendrecv: send `bytes` of `send` to rank
 * `to` and receive `bytes` from rank `from` into `recv`, concurrently (either
 * side < 0: none).  gather: `bytes` of `send` from every rank into `recv` at
 * offset rank*bytes on rank `root` (`recv` NULL elsewhere). */
typedef struct dips_comm_ops {
    int (*broadcast)(void *ctx, void *buf, size_t bytes, int root);
    int (*sendrecv)(void *ctx, const void *send, int to, void *recv, int from, size_t bytes);
    int (*gather)(void *ctx, const void *send, void *recv, size_t bytes, int root);
} dips_comm_ops;

/* A new RCCL unique id (ncclGetUniqueId) into id[DIPS_COMM_ID_BYTES]; rank 0
 * makes it and the caller hands it to every rank out of band. */
dips_status dips_comm_unique_id(uint8_t *id);

/* Join the RCCL communicator `id` as `rank` of `nranks` on HIP device
 * `device` (ncclCommInitRank; blocks until every rank has joined). */
dips_status dips_comm_create(const uint8_t *id, int nranks, int rank, int device, dips_comm **out);

/* All `nranks` RCCL communicators of ONE process (ncclCommInitAll): rank r
 * on HIP device devices[r] (NULL: device r), comms[r] = rank r.  The host
 * that drives every GPU from one process -- the reference's single decoder
 * feeding a node -- runs each rank's calls on its own thread. */
dips_status dips_comm_create_all(int nranks, const int *devices, dips_comm **comms);

/* `nranks` loopback communicators on `device`; comms[r] = rank r; each must
 * be driven by its own thread (the collectives meet on the host). */
dips_status dips_comm_create_loopback(int nranks, int device, dips_comm **comms);

/* A communicator over the caller's transport `ops` (context `ctx`). */
dips_status dips_comm_create_host(const dips_comm_ops *ops, void *ctx, int nranks, int rank, int device,
                                  dips_comm **out);

/* Leave and free a communicator (ncclCommDestroy for RCCL). */
void dips_comm_destroy(dips_comm *comm);

/* Last error message of `comm` (or of the last failed creation if NULL). */
const char *dips_comm_last_error(const dips_comm *comm);

/* Transport (DIPS_COMM_*), size and rank of `comm`. */
dips_status dips_comm_info(const dips_comm *comm, int *kind, int *nranks, int *rank);

/* The frame range of `rank` of `nranks` over `n_total` frames: global
 * frames [*first, *first + *count), balanced to within one frame. */
dips_status dips_shard_range(uint64_t n_total, int nranks, int rank, uint64_t *first, uint32_t *count);

/* DIPS_SHARD_REF_RESIDENT: 'overall' mode, every rank passes in `ref`
 * its own copy of the reference (e.g. from dips_shard_broadcast), so the
 * call skips the broadcast. */
#define DIPS_SHARD_REF_RESIDENT 0x1u

/* Broadcast one frame (width*height*C bytes) from rank 0's `frame` into
 * `out` on every rank (on rank 0 `out` may equal `frame`).  Device pointers
 * with DIPS_FLAG_DEVICE_PTRS (asynchronous on the handle's stream), host
 * pointers otherwise. */
dips_status dips_shard_broadcast(dips_handle *h, dips_comm *comm, uint32_t width, uint32_t height,
                                 const uint8_t *frame, uint8_t *out);

/* The sharded series: this rank's `n_local` frames (its dips_shard_range of
 * n_total; every rank needs >= 1 frame, so n_total >= nranks), the same
 * semantics as one dips_diff_series over all n_total frames.
 *   ref:          'overall': on rank 0 the reference (NULL = its frames[0]),
 *                 broadcast to every rank; with DIPS_SHARD_REF_RESIDENT every
 *                 rank's own copy.  'per-frame': on rank 0 the frame before
 *                 global frame 0 (NULL = frame 0 itself); ignored elsewhere
 *                 (the halo comes from rank r-1).
 *   series_local: n_local entries, this rank's slice (required).
 *   series_all:   rank 0: n_total entries, the gathered series (required;
 *                 may begin at series_local); other ranks: ignored.
 * With DIPS_FLAG_DEVICE_PTRS every pointer is a device pointer and the call
 * is asynchronous on the handle's stream (RCCL / loopback); otherwise host
 * pointers: the exchange runs first, then the rank's frames go through the
 * pinned side-stream feed of dips_diff_series_streamed (no batch-sized HBM
 * staging), and the call returns with the results in host memory.  h's
 * device must be the communicator's. */
dips_status dips_diff_series_sharded(dips_handle *h, dips_comm *comm, uint32_t width, uint32_t height,
                                     const uint8_t *frames, uint32_t n_local, uint64_t n_total,
                                     const uint8_t *ref, uint32_t shard_flags, dips_series_entry *series_local,
                                     dips_series_entry *series_all);

/* The plan of that call on this rank, without running it: its frame range
 * and the waves of its main series launch (the one the halo transfer
 * overlaps: frames 1..n-1 on ranks > 0 in 'per-frame' mode, all frames
 * otherwise), with the DIPS_SERIES_WAVES_PER_SIMD deployment cap applied
 * (`waves`) and without it (`waves_uncapped`).  The launch itself runs the
 * full persistent grid: the halo's kernels are posted before it. */
dips_status dips_shard_plan(dips_handle *h, const dips_comm *comm, uint32_t width, uint32_t height,
                            uint64_t n_total, uint64_t *first, uint32_t *count, uint64_t *waves,
                            uint64_t *waves_uncapped);

/* The dips-compat ComputeState over frame ranges ("dips-compat
 * T=4 needs a 3-frame halo"): consecutive frame_callback calls of global
 * frames [first, first + n_local) (this rank's dips_shard_range of n_total)
 * on a FRESH handle of every rank, the outputs those frames get from one
 * ComputeState that saw every frame (dips/src/lib.rs:233-246,
 * dips/src/gpu/mod.rs:170-397).  Rank 0 runs frames 0..3 (passthrough, then
 * the start texture) and broadcasts the start texture; rank r sends its last
 * three frames to rank r+1 and resumes (dips_compat_resume) from the start
 * texture and the three frames it receives.  Every rank after the first must
 * start at global frame >= 7 and every rank but the last own >= 3 frames
 * (n_total >= 7 * nranks suffices); the check is the same on every rank.
 * out: n_local RGBA8 frames on this rank (no gather: the outputs are frames,
 * each rank's muxer takes its own).  Pointers as dips_frame_callback_batch. */
dips_status dips_frame_callback_batch_sharded(dips_handle *h, dips_comm *comm, uint32_t width, uint32_t height,
                                              const uint8_t *frames, uint32_t n_local, uint64_t n_total,
                                              uint8_t *out);

/* Copy the reference the last sharded call used for this rank's first frame
 * (the received halo, the broadcast reference, or rank 0's own) into `out`
 * (width*height*C bytes; device pointer with DIPS_FLAG_DEVICE_PTRS).
 * Returns 1 if copied, 0 before any sharded call. */
int dips_shard_reference(dips_handle *h, uint8_t *out, size_t cap);

/* ------------------------------------------------------------------------
 * dips_alt operator.  The dips_alt crate's GPU
 * operator is DiPsCompute (dips_alt/src/dips_compute/mod.rs:243-647):
 * new(num_textures, textures_width, textures_height, window, device, queue,
 * properties) and send_frame(frame, snapshot, surface) -> Vec<u8>, driven by
 * the frame loop of run_dips_on_file (dips_alt/src/lib.rs:554-690).  The
 * reference's constructor takes (rows, cols) in that order (lib.rs:596-603);
 * this ABI takes width = columns, height = rows.  Frames are RGBA8, stride
 * width*4 (mod.rs:510-521).
 * ------------------------------------------------------------------------ */

/* DiPsProperties of dips_alt (dips_alt/src/dips_compute/mod.rs:167-186) plus
 * the operator's texture count. */
typedef struct dips_alt_params {
    uint8_t colorize;                /* COLORIZE; default 1 (mod.rs:179) */
    int32_t window_size;             /* WINDOW_SIZE; 1..11; default 1 (mod.rs:180) */
    float sigmoid_horizontal_scalar; /* SIGMOID_HORIZONTAL_SCALAR; default 5.0 (mod.rs:181) */
    uint32_t filter_type;            /* DIPS_FILTER_SIGMOID (default) / _INVERSE_SIGMOID;
                                        any other code: no filter (shader default branch) */
    uint32_t chroma_filter;          /* DIPS_CHROMA_*: All = NONE (default), Red, Green, Blue */
    uint32_t num_textures;           /* NUM_TEXTURES, 1..16; default FRAME_COUNT = 2 (lib.rs:36) */
    uint32_t flags;                  /* DIPS_FLAG_DEVICE_PTRS, _TIME_KERNEL, _FORCE_GENERIC */
} dips_alt_params;

typedef struct dips_alt_handle dips_alt_handle;

DIPS_LAYOUT_ASSERT(sizeof(dips_alt_params) == 28, "dips_alt_params size");
DIPS_LAYOUT_ASSERT(offsetof(dips_alt_params, colorize) == 0, "dips_alt_params.colorize");
DIPS_LAYOUT_ASSERT(offsetof(dips_alt_params, window_size) == 4, "dips_alt_params.window_size");
DIPS_LAYOUT_ASSERT(offsetof(dips_alt_params, sigmoid_horizontal_scalar) == 8,
                   "dips_alt_params.sigmoid_horizontal_scalar");
DIPS_LAYOUT_ASSERT(offsetof(dips_alt_params, filter_type) == 12, "dips_alt_params.filter_type");
DIPS_LAYOUT_ASSERT(offsetof(dips_alt_params, chroma_filter) == 16, "dips_alt_params.chroma_filter");
DIPS_LAYOUT_ASSERT(offsetof(dips_alt_params, num_textures) == 20, "dips_alt_params.num_textures");
DIPS_LAYOUT_ASSERT(offsetof(dips_alt_params, flags) == 24, "dips_alt_params.flags");

/* Fill `p` with DiPsProperties::default() (mod.rs:176-186), num_textures 2. */
dips_status dips_alt_params_default(dips_alt_params *p);

/* Replaces DiPsCompute::new (dips_alt/src/dips_compute/mod.rs:270-496):
 * texture slots, snapshot texture and output, all zero-initialised. */
dips_status dips_alt_create(const dips_alt_params *params, uint32_t width, uint32_t height, int device,
                            dips_alt_handle **out);

/* Replaces Drop of DiPsCompute. */
void dips_alt_destroy(dips_alt_handle *h);

/* Last error message for `h` (or the last creation failure if h == NULL). */
const char *dips_alt_last_error(const dips_alt_handle *h);

/* Run subsequent work on `stream` (a hipStream_t; NULL = the handle's own);
 * ordered after the previous stream's work as dips_set_stream. */
dips_status dips_alt_set_stream(dips_alt_handle *h, void *stream);
dips_status dips_alt_synchronize(dips_alt_handle *h);

/* Replaces DiPsCompute::send_frame (mod.rs:498-646): writes the frame into
 * texture slot texture_index, advances it, runs pre_compute_main with the
 * snapshot uniform = (snapshot != 0) and copies the RGBA8 output texture
 * (width*height*4 bytes) to `out_rgba`.  Host pointers always. */
dips_status dips_alt_send_frame(dips_alt_handle *h, const uint8_t *frame_rgba, size_t len, int snapshot,
                                uint8_t *out_rgba, size_t cap);

/* `n_frames` consecutive send_frame calls in one pass: frames n_frames x
 * width*height*4, snapshot_flags (host, n_frames bytes, NULL = none) the
 * per-frame snapshot argument, out n_frames x width*height*4.  With
 * DIPS_FLAG_DEVICE_PTRS frames/out are device pointers and the call is
 * asynchronous on the handle's stream. */
dips_status dips_alt_send_frames(dips_alt_handle *h, const uint8_t *frames, uint32_t n_frames,
                                 const uint8_t *snapshot_flags, uint8_t *out);

/* The frame loop of run_dips_on_file (lib.rs:588-683) minus OpenCV decode /
 * encode: snapshot while index == FRAME_COUNT, index saturating, a refresh
 * marker equal to the running 1-based frame count resets index to 0.  The
 * loop state persists across calls, so a video may be fed in pieces. */
dips_status dips_alt_run(dips_alt_handle *h, const uint8_t *frames, uint32_t n_frames,
                         const uint64_t *refresh_markers, uint32_t n_markers, uint8_t *out);

/* The dips_alt run loop over frame ranges: this rank's frames [first,
 * first + n_local) of an n_total-frame video (its dips_shard_range), on a
 * FRESH handle of every rank, with the outputs one run_dips_on_file loop over
 * every frame gives them (the same refresh markers on every rank).  Rank r
 * replays, outputs discarded, the source frames of the last snapshot before
 * its first frame and the num_textures frames before it (fewer, after zero
 * frames, near the start), fetched point to point from the ranks that own
 * them, then runs its own frames; any split, ranks with no frame included.
 * Pointers as dips_alt_send_frames; synchronous. */
dips_status dips_alt_run_sharded(dips_alt_handle *h, dips_comm *comm, const uint8_t *frames, uint32_t n_local,
                                 uint64_t n_total, const uint64_t *refresh_markers, uint32_t n_markers, uint8_t *out);

/* Copy the snapshot texture's .r channel (width*height bytes, host). */
dips_status dips_alt_snapshot_texture(dips_alt_handle *h, uint8_t *out_gray, size_t cap);

/* Kernel timing of the batch kernel (DIPS_FLAG_TIME_KERNEL), as dips_kernel_time. */
dips_status dips_alt_kernel_time(dips_alt_handle *h, double *total_ms, uint64_t *launches);
dips_status dips_alt_kernel_time_reset(dips_alt_handle *h);

/* Self-check of the batch kernel's epilogue table (alt_lut.h) for the
 * handle's properties: every snapshot byte against every (max, min) byte
 * pair -- all pixel intensities of every chroma mode -- through the table and
 * through the specification's epilogue; *mismatches = the count of texels
 * that differ (0 expected).  Synchronous; for tests. */
dips_status dips_alt_lut_selfcheck(dips_alt_handle *h, uint64_t *mismatches);

/* The host-built index of that table (alt_lut.h), no device needed: the
 * level-1 entries {x, sh} of the 1,021 clusters (l1_cap >= 2042 words), the
 * distinct diff values and their level-2 slots (cap >= *n_diffs), and the
 * level-2 size.  Any output pointer may be NULL.  For tests. */
dips_status dips_alt_lut_index(uint32_t *l1, uint32_t l1_cap, float *diffs, uint16_t *slots, uint32_t cap,
                               uint32_t *n_diffs, uint32_t *l2_entries);

#ifdef __cplusplus
}
#endif
#endif /* DIPS_HIP_H */
