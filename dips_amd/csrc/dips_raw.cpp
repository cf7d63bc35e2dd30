// dips_raw.cpp -- native host program over the C ABI (include/dips_hip.h),
// the stand-in for the Rust host side (cargo is absent in this image).
//
// It mirrors dips' perform_dips loop (dips/src/frame_extractor.rs:206-276:
// appsink delivers RGBA8 frames, frame_callback (dips/src/lib.rs:233-246)
// turns each into the output frame, the muxer writes it) with the GStreamer
// decode / encode replaced by raw files, and exposes the north-star series:
//
//   dips_raw callback IN.rgba W H OUT.rgba [--colorize] [--window N]
//            [--sensitivity K] [--filter sigmoid|inverse|none]
//            [--chroma none|red|green|blue] [--batch N]
//            [--ranks N [--transport loopback|rccl]]
//                                         -> with --ranks, N ranks (one thread
//            and one fresh handle each) run their frame ranges through
//            dips_frame_callback_batch_sharded
//   dips_raw alt IN.rgba W H OUT.rgba [--markers M1,M2,...] [--window N]
//            [--textures N] [--ranks N [--transport loopback|rccl]]
//                                         -> the dips_alt run_dips_on_file
//            loop (dips_alt/src/lib.rs:588-683) with its refresh markers;
//            with --ranks, dips_alt_run_sharded
//   dips_raw series IN.raw W H rgb8|rgba8|gray8 [--mode overall|per-frame]
//            [--tau T] [--chunk N]        -> CSV frame,sad,sj,count,si
//            [--grid RxC [--roi x,y,w,h]] -> the series per cell of an R x C
//            grid over the region (default: the whole frame) with
//            dips_diff_series_grid: CSV t,row,col,sad,sj,count,si_fixed
//            [--pixel-sums FILE [--roi x,y,w,h]] -> the series summed over
//            time per pixel of the region with dips_diff_pixel_sums: FILE gets
//            roi_h x roi_w x {sad, sj, count, si_fixed} little-endian u64,
//            stdout one line with the region, the frames and the four totals
//            [--mask FILE [--roi x,y,w,h]] -> the per-frame change mask of the
//            region with dips_diff_change_mask: FILE gets frames x roi_h x
//            row_bytes bytes (one bit per pixel, LSB first, rows padded to
//            32 bits), stdout one line with the region, the frames, the row
//            bytes and the number of set bits
//            [--pixel-times FILE [--roi x,y,w,h]] -> the change times per pixel
//            of the region with dips_diff_pixel_times: FILE gets the four
//            planes first, last, run_max, run_cur of roi_h x roi_w
//            little-endian u32 each, stdout one line with the region, the
//            frames, the pixels that never changed, the smallest first, the
//            largest last (-1 when no pixel changed) and the largest run_max
//            [--boxes FILE [--connectivity 4|8] [--min-area A] [--max-boxes K]
//            [--roi x,y,w,h]] -> the connected components of the region's
//            change mask with dips_diff_change_mask and dips_mask_components
//            (defaults 8, 1, 64): FILE gets the CSV frame,k,x0,y0,x1,y1,area,
//            anchor,cx256,cy256, one row per stored record, and a line
//            "# frame,count" per frame (count is not capped by K); stdout one
//            line with the region, the frames, the components and the records
//            [--tracks FILE [--connectivity 4|8] [--min-area A] [--max-boxes K]
//            [--roi x,y,w,h]] -> the same components linked across frames with
//            dips_mask_tracks (K 1 .. 256): FILE is --boxes' file with the
//            columns prev,overlap,track,age behind every record (4294967295:
//            none); the stdout line begins with "tracks" and ends with
//            tracks=<ids handed out>
//            [--shapes [--shape-weights FILE.raw]] -> with --boxes or --tracks:
//            the shape record of every component with dips_mask_shapes
//            (--boxes: instead of dips_mask_components; --tracks: in addition
//            to dips_mask_tracks): the columns sx,sy,sxx,syy,sxy,wsum,wmax,
//            cracks_v,cracks_h,euler behind every record; FILE.raw is the
//            weight of every pixel, frames x roi_h x roi_w raw u8 planes of the
//            region (without it wsum and wmax are 0); the stdout line ends
//            with shapes=1
//            [--morph erode|dilate|open|close:box|diamond:RXxRY]... -> with
//            --mask, --boxes or --tracks: the binary morphology of the change mask with
//            dips_mask_morph (radii 0 .. 15, a diamond needs RX = RY), the steps
//            applied in the order given; --mask then writes the cleaned mask
//            and --boxes / --tracks take the components of the cleaned mask, and the
//            stdout line ends with morph=<steps>
//            [--vote K[,M]] -> with --mask, --boxes or --tracks: the temporal
//            M-of-K vote on the change mask with dips_mask_vote (K 1 .. 31, M
//            1 .. K, default the majority K / 2 + 1), over the whole clip in
//            one call with clear frames before it, applied before --morph;
//            the stdout line has vote=K,M; a bad value exits with status 2
//            [--select [min-area=A][,max-area=B][,clear-border][,dropped]
//            [,connectivity=4|8]] -> with what takes a mask: the components of
//            the change mask that pass the predicate, with dips_mask_select
//            (defaults 1, 0 = no upper bound, 8), applied after --vote and
//            --morph; the stdout line has select=A,B,<flags>,<connectivity>
//            [--hysteresis TAU_HIGH] -> likewise, only with the plain change
//            mask (not with --background or --sigma-delta): of those
//            components only the ones that hold a pixel of the change mask at
//            TAU_HIGH >= --tau (a second handle), in the same
//            dips_mask_select call; the stdout line has hysteresis=TAU_HIGH
//            [--fill-holes [MAX]] -> likewise: after --select the holes of the
//            mask (of at most MAX pixels; default 0: all) are filled with
//            dips_mask_logic and dips_mask_select, under --select's
//            connectivity; the stdout line has fill_holes=MAX
//            [--background K[,selective] [--background-out FILE]] -> with
//            --mask, --boxes or --tracks: the mask is taken against the running-average
//            background with dips_diff_background_mask (rate_shift K in
//            0 .. 8, starting at frame 0) instead of --mode's reference;
//            --background-out gets the final state, channel planes of roi_h x
//            roi_w little-endian u16, and the stdout line ends with
//            background=K[,selective]
//            [--sigma-delta N[,VMIN[,VMAX]] [--sigma-delta-out FILE]] -> with
//            --mask, --boxes or --tracks, and not with --background: the mask
//            is taken under the Sigma-Delta model's per-pixel threshold with
//            dips_diff_sigma_delta_mask (n_amp N in 1 .. 15, v_min 2 and v_max
//            510 unless given, starting at frame 0); --sigma-delta-out gets
//            the final state, the planes M and V of roi_h x roi_w
//            little-endian u16, and the stdout line ends with
//            sigma_delta=N,VMIN,VMAX
//            [--mask-counts FILE [--mask-grid RxC]] [--mask-times FILE]
//            [--mask-sums FILE] -> the statistics of the final mask (behind
//            --background / --sigma-delta, --vote, --morph, --select and
//            --fill-holes; --roi as for
//            --mask) with dips_mask_counts and dips_mask_pixel_times, with
//            --mask, --boxes or --tracks or on their own (the stdout line then
//            begins with "mask-stats" and no mask is written): the counts as
//            the CSV t,row,col,count over an R x C grid of the region (default
//            1x1: the set bits per frame), the times as --pixel-times writes
//            them, the sums as one plane of roi_h x roi_w little-endian u32;
//            the stdout line ends with mask_stats=<what was written>
//   dips_raw sharded IN.raw W H rgb8|rgba8|gray8 --ranks N [--mode ...]
//            [--tau T] [--transport loopback|rccl]
//                                         -> the same CSV, computed by N
//            ranks (one thread and one handle each) with
//            dips_diff_series_sharded: each rank hands its frame range of the
//            file to the library, rank 0 prints the gathered series.
//            loopback: every rank on device 0; rccl: rank r on device r, all
//            ranks of this process from dips_comm_create_all -- one process
//            that decodes once and feeds every GPU of a node
//
// Input files are memory-mapped and handed over as host pointers: the
// library stages them through pinned memory and overlaps the PCIe transfers
// with the kernels.  Exit status 0 on success, 1 on a usage error, 2 on a
// library error (message from dips_last_error on stderr).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dips_hip.h"

namespace {

struct Mapped {
    const uint8_t* p = nullptr;
    size_t n = 0;
    bool open(const char* path) {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st {};
        if (fstat(fd, &st) != 0 || st.st_size <= 0) {
            ::close(fd);
            return false;
        }
        n = (size_t)st.st_size;
        void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (m == MAP_FAILED) return false;
        p = static_cast<const uint8_t*>(m);
        return true;
    }
    ~Mapped() {
        if (p) munmap(const_cast<uint8_t*>(p), n);
    }
};

int usage() {
    std::fprintf(stderr,
                 "usage: dips_raw callback IN.rgba W H OUT.rgba [--colorize] [--window N] [--sensitivity K]\n"
                 "                [--filter sigmoid|inverse|none] [--chroma none|red|green|blue] [--batch N]\n"
                 "                [--ranks N [--transport loopback|rccl]]\n"
                 "       dips_raw alt IN.rgba W H OUT.rgba [--markers M1,M2,...] [--window N] [--textures N]\n"
                 "                [--ranks N [--transport loopback|rccl]]\n"
                 "       dips_raw series IN.raw W H rgb8|rgba8|gray8 [--mode overall|per-frame] [--tau T]\n"
                 "                [--chunk N] [--grid RxC [--roi x,y,w,h]] [--pixel-sums FILE [--roi x,y,w,h]]\n"
                 "                [--mask FILE [--roi x,y,w,h]] [--pixel-times FILE [--roi x,y,w,h]]\n"
                 "                [--boxes FILE [--connectivity 4|8] [--min-area A] [--max-boxes K] [--roi x,y,w,h]]\n"
                 "                [--tracks FILE [--connectivity 4|8] [--min-area A] [--max-boxes K] [--roi x,y,w,h]]\n"
                 "                [--shapes [--shape-weights FILE.raw]] (with --boxes or --tracks)\n"
                 "                [--vote K[,M]] (with --mask, --boxes or --tracks; before --morph)\n"
                 "                [--morph erode|dilate|open|close:box|diamond:RXxRY]... (with --mask, --boxes or --tracks)\n"
                 "                [--select [min-area=A][,max-area=B][,clear-border][,dropped][,connectivity=4|8]]\n"
                 "                [--hysteresis TAU_HIGH] [--fill-holes [MAX]] (with what takes a mask, after --morph: select,\n"
                 "                then fill-holes; the last two not with --background or --sigma-delta)\n"
                 "                [--background K[,selective] [--background-out FILE]] (with --mask, --boxes or --tracks)\n"
                 "                [--sigma-delta N[,VMIN[,VMAX]] [--sigma-delta-out FILE]] (likewise; not with --background)\n"
                 "                [--mask-counts FILE [--mask-grid RxC]] [--mask-times FILE] [--mask-sums FILE]\n"
                 "                (of the final mask; alone or with --mask, --boxes or --tracks; take --roi, --vote,\n"
                 "                --morph, --select, --hysteresis, --fill-holes, --background and --sigma-delta as --mask does)\n"
                 "       dips_raw sharded IN.raw W H rgb8|rgba8|gray8 --ranks N [--mode overall|per-frame]\n"
                 "                [--tau T] [--transport loopback|rccl]\n");
    return 1;
}

int lib_error(dips_handle* h, const char* what, int st) {
    std::fprintf(stderr, "dips_raw: %s failed (%d): %s\n", what, st, dips_last_error(h));
    return 2;
}

bool parse_u32(const char* s, uint32_t* v) {
    char* end = nullptr;
    const unsigned long x = std::strtoul(s, &end, 10);
    if (!s[0] || *end || x == 0 || x > 0xFFFFFFFFul) return false;
    *v = (uint32_t)x;
    return true;
}

// as parse_u32, 0 allowed (--min-area, --max-boxes)
bool parse_u32_or_zero(const char* s, uint32_t* v) {
    if (s[0] == '0' && !s[1]) {
        *v = 0;
        return true;
    }
    return parse_u32(s, v);
}

// "RxC" -> rows, cols (both >= 1)
bool parse_grid(const std::string& s, uint32_t* rows, uint32_t* cols) {
    const size_t x = s.find('x');
    if (x == std::string::npos) return false;
    return parse_u32(s.substr(0, x).c_str(), rows) && parse_u32(s.substr(x + 1).c_str(), cols);
}

// One step of --morph: the arguments of dips_mask_morph.
struct MorphStep {
    uint32_t op, shape, rx, ry;
};

// "OP:SHAPE:RXxRY" -> a step (radii 0 .. DIPS_MORPH_MAX_RADIUS, a diamond with RX = RY)
bool parse_morph(const std::string& s, MorphStep* m) {
    const size_t c1 = s.find(':'), c2 = c1 == std::string::npos ? c1 : s.find(':', c1 + 1);
    if (c2 == std::string::npos) return false;
    const std::string op = s.substr(0, c1), shape = s.substr(c1 + 1, c2 - c1 - 1), radii = s.substr(c2 + 1);
    const size_t x = radii.find('x');
    if (x == std::string::npos) return false;
    m->op = op == "erode" ? DIPS_MORPH_ERODE : op == "dilate" ? DIPS_MORPH_DILATE : op == "open" ? DIPS_MORPH_OPEN
                                                                                                  : DIPS_MORPH_CLOSE;
    if (m->op == DIPS_MORPH_CLOSE && op != "close") return false;
    if (shape != "box" && shape != "diamond") return false;
    m->shape = shape == "box" ? DIPS_MORPH_BOX : DIPS_MORPH_DIAMOND;
    if (!parse_u32_or_zero(radii.substr(0, x).c_str(), &m->rx) || !parse_u32_or_zero(radii.substr(x + 1).c_str(), &m->ry))
        return false;
    if (m->rx > DIPS_MORPH_MAX_RADIUS || m->ry > DIPS_MORPH_MAX_RADIUS) return false;
    return m->shape == DIPS_MORPH_BOX || m->rx == m->ry;
}

// --background: rate_shift and flags of dips_diff_background_mask.
struct BackgroundOpt {
    bool on = false;
    uint32_t rate_shift = 0, flags = 0;
    const char* out_path = nullptr;
};

bool parse_background(const std::string& s, BackgroundOpt* b) {
    const size_t comma = s.find(',');
    if (comma != std::string::npos && s.substr(comma + 1) != "selective") return false;
    if (!parse_u32_or_zero(s.substr(0, comma).c_str(), &b->rate_shift) || b->rate_shift > DIPS_BG_MAX_RATE_SHIFT)
        return false;
    b->flags = comma != std::string::npos ? DIPS_BG_SELECTIVE : 0u;
    b->on = true;
    return true;
}

// --sigma-delta: n_amp, v_min and v_max of dips_diff_sigma_delta_mask.
struct SigmaDeltaOpt {
    bool on = false;
    uint32_t n_amp = 0, v_min = 2, v_max = DIPS_SD_MAX_V;
    const char* out_path = nullptr;
};

// N[,VMIN[,VMAX]]
bool parse_sigma_delta(const std::string& s, SigmaDeltaOpt* d) {
    uint32_t* fields[3] = {&d->n_amp, &d->v_min, &d->v_max};
    size_t pos = 0;
    for (int k = 0; k < 3; ++k) {
        const size_t comma = s.find(',', pos);
        if (!parse_u32_or_zero(s.substr(pos, comma == std::string::npos ? comma : comma - pos).c_str(), fields[k])) return false;
        if (comma == std::string::npos) {
            pos = comma;
            break;
        }
        pos = comma + 1;
    }
    if (pos != std::string::npos) return false;  // a fourth field
    if (d->n_amp == 0 || d->n_amp > DIPS_SD_MAX_AMP || d->v_min > d->v_max || d->v_max > DIPS_SD_MAX_V) return false;
    d->on = true;
    return true;
}

// The u16 values of the state --background or --sigma-delta keeps for a
// region of rw x rh pixels (1: neither is on, or the library will refuse).
size_t state_values(bool sane, const BackgroundOpt& bg, const SigmaDeltaOpt& sd, uint32_t format, uint32_t rw, uint32_t rh) {
    if (!sane || (!bg.on && !sd.on)) return 1u;
    return (size_t)(sd.on ? DIPS_SD_PLANES : format) * rw * rh;
}

// The region's mask for --mask and --boxes: dips_diff_change_mask, or with
// --background dips_diff_background_mask, or with --sigma-delta
// dips_diff_sigma_delta_mask, whose final state goes to `state`.
int region_mask(dips_handle* hd, uint32_t w, uint32_t h, const uint8_t* frames, uint32_t n, const uint32_t* roi,
                const BackgroundOpt& bg, const SigmaDeltaOpt& sd, std::vector<uint16_t>& state, uint8_t* mask,
                const char** what) {
    if (sd.on) {
        *what = "dips_diff_sigma_delta_mask";
        return dips_diff_sigma_delta_mask(hd, w, h, frames, n, nullptr, roi, sd.n_amp, sd.v_min, sd.v_max, 0u, state.data(),
                                          mask);
    }
    if (!bg.on) {
        *what = "dips_diff_change_mask";
        return dips_diff_change_mask(hd, w, h, frames, n, nullptr, roi, mask);
    }
    *what = "dips_diff_background_mask";
    return dips_diff_background_mask(hd, w, h, frames, n, nullptr, roi, bg.rate_shift, bg.flags, 0u, state.data(), mask);
}

// The final background or Sigma-Delta state as raw u16 planes (0: written or
// not asked for).
int write_background(const BackgroundOpt& bg, const SigmaDeltaOpt& sd, const std::vector<uint16_t>& state) {
    const char* path = sd.on ? sd.out_path : bg.out_path;
    if (!path) return 0;
    std::FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(state.data(), sizeof(uint16_t), state.size(), f) != state.size() || std::fclose(f) != 0) {
        std::fprintf(stderr, "dips_raw: cannot write %s\n", path);
        return 1;
    }
    return 0;
}

void print_background(const BackgroundOpt& bg, const SigmaDeltaOpt& sd) {
    if (bg.on) std::printf(" background=%u%s", bg.rate_shift, bg.flags ? ",selective" : "");
    if (sd.on) std::printf(" sigma_delta=%u,%u,%u", sd.n_amp, sd.v_min, sd.v_max);
}

// --vote: window and votes of dips_mask_vote (window 0: no vote).
struct VoteOpt {
    uint32_t window = 0, votes = 0;
};

// "K[,M]" -> the option (K 1 .. DIPS_VOTE_MAX_WINDOW, M 1 .. K, default K / 2 + 1)
bool parse_vote(const std::string& s, VoteOpt* v) {
    const size_t comma = s.find(',');
    if (!parse_u32(s.substr(0, comma).c_str(), &v->window)) return false;
    v->votes = v->window / 2u + 1u;
    if (comma != std::string::npos && !parse_u32(s.substr(comma + 1).c_str(), &v->votes)) return false;
    return v->window >= 1u && v->window <= DIPS_VOTE_MAX_WINDOW && v->votes >= 1u && v->votes <= v->window;
}

// The vote over the whole host mask of n frames of rw x rh pixels, clear
// frames before it; the result is in `mask` again.
int apply_vote(dips_handle* hd, std::vector<uint8_t>& mask, uint32_t n, uint32_t rw, uint32_t rh, const VoteOpt& v) {
    if (v.window == 0u) return DIPS_OK;
    std::vector<uint8_t> other(mask.size());
    const int st = dips_mask_vote(hd, mask.data(), n, rw, rh, v.window, v.votes, nullptr, nullptr, other.data());
    if (st == DIPS_OK) mask.swap(other);
    return st;
}

// The steps in order on the host mask of n frames of rw x rh pixels; the
// result is in `mask` again.
int apply_morph(dips_handle* hd, std::vector<uint8_t>& mask, uint32_t n, uint32_t rw, uint32_t rh,
                const std::vector<MorphStep>& steps) {
    std::vector<uint8_t> other(steps.empty() ? 0u : mask.size());
    for (const MorphStep& m : steps) {
        const int st = dips_mask_morph(hd, mask.data(), n, rw, rh, m.op, m.shape, m.rx, m.ry, other.data());
        if (st != DIPS_OK) return st;
        mask.swap(other);
    }
    return DIPS_OK;
}

// --select, --hysteresis, --fill-holes: the selection of components of the
// final mask (dips_mask_select, dips_mask_logic).
struct SelectOpt {
    bool on = false;  // --select
    uint32_t min_area = 1, max_area = 0, flags = 0, connectivity = 8;
    bool hysteresis = false;
    float tau_high = 0.0f;
    bool fill = false;
    uint32_t max_hole = 0;
    bool any() const { return on || hysteresis || fill; }
};

// "[min-area=A][,max-area=B][,clear-border][,dropped][,connectivity=4|8]" -> the option
bool parse_select(const std::string& s, SelectOpt* o) {
    size_t at = 0;
    while (at <= s.size()) {
        const size_t comma = std::min(s.find(',', at), s.size());
        const std::string item = s.substr(at, comma - at);
        const size_t eq = item.find('=');
        const std::string key = item.substr(0, eq), val = eq == std::string::npos ? "" : item.substr(eq + 1);
        if (key == "min-area" && eq != std::string::npos) {
            if (!parse_u32_or_zero(val.c_str(), &o->min_area)) return false;
        } else if (key == "max-area" && eq != std::string::npos) {
            if (!parse_u32_or_zero(val.c_str(), &o->max_area)) return false;
        } else if (key == "connectivity" && eq != std::string::npos) {
            if (!parse_u32(val.c_str(), &o->connectivity) || (o->connectivity != 4u && o->connectivity != 8u)) return false;
        } else if (item == "clear-border") {
            o->flags |= DIPS_SELECT_CLEAR_BORDER;
        } else if (item == "dropped") {
            o->flags |= DIPS_SELECT_DROPPED;
        } else {
            return false;
        }
        at = comma + 1;
    }
    o->on = true;
    return o->max_area == 0u || o->max_area >= o->min_area;
}

// The selection, then the hole filling, on the host mask of n frames of rw x
// rh pixels; the result is in `mask` again.  --hysteresis takes its marker,
// the change mask of the same frames at tau_high, from a handle of its own;
// a failure there is reported here and *what set to NULL.
int apply_select(dips_handle* hd, const dips_params& p, uint32_t w, uint32_t h, const uint8_t* frames, uint32_t n,
                 const uint32_t* roi, std::vector<uint8_t>& mask, uint32_t rw, uint32_t rh, const SelectOpt& o,
                 const char** what) {
    if (!o.any() || n == 0) return DIPS_OK;
    std::vector<uint8_t> other(mask.size());
    if (o.on || o.hysteresis) {
        std::vector<uint8_t> strong;
        if (o.hysteresis) {
            dips_params ph = p;
            ph.tau = o.tau_high;
            dips_handle* hs = nullptr;
            int st = dips_create(&ph, 0, &hs);
            if (st == DIPS_OK) {
                strong.resize(mask.size());
                st = dips_diff_change_mask(hs, w, h, frames, n, nullptr, roi, strong.data());
            }
            if (st != DIPS_OK) {
                lib_error(hs, hs ? "dips_diff_change_mask (--hysteresis)" : "dips_create (--hysteresis)", st);
                *what = nullptr;
            }
            if (hs) dips_destroy(hs);
            if (st != DIPS_OK) return st;
        }
        *what = "dips_mask_select";
        const int st = dips_mask_select(hd, mask.data(), n, rw, rh, o.connectivity, o.min_area, o.max_area, o.flags,
                                        o.hysteresis ? strong.data() : nullptr, o.hysteresis ? n : 0u, 0u, other.data(),
                                        nullptr);
        if (st != DIPS_OK) return st;
        mask.swap(other);
    }
    if (o.fill) {
        // the holes: the components of the complement, under the dual
        // connectivity, that do not touch the border
        std::vector<uint8_t> holes(mask.size());
        *what = "dips_mask_logic";
        int st = dips_mask_logic(hd, mask.data(), n, rw, rh, DIPS_LOGIC_NOT, nullptr, 0u, other.data());
        if (st != DIPS_OK) return st;
        *what = "dips_mask_select";
        st = dips_mask_select(hd, other.data(), n, rw, rh, 12u - o.connectivity, 1u, o.max_hole, DIPS_SELECT_CLEAR_BORDER,
                              nullptr, 0u, 0u, holes.data(), nullptr);
        if (st != DIPS_OK) return st;
        *what = "dips_mask_logic";
        st = dips_mask_logic(hd, mask.data(), n, rw, rh, DIPS_LOGIC_OR, holes.data(), n, other.data());
        if (st != DIPS_OK) return st;
        mask.swap(other);
    }
    return DIPS_OK;
}

void print_select(const SelectOpt& o) {
    if (o.on) std::printf(" select=%u,%u,%u,%u", o.min_area, o.max_area, o.flags, o.connectivity);
    if (o.hysteresis) std::printf(" hysteresis=%g", (double)o.tau_high);
    if (o.fill) std::printf(" fill_holes=%u", o.max_hole);
}

// --mask-counts [--mask-grid], --mask-times, --mask-sums: the statistics of
// the final mask (dips_mask_counts, dips_mask_pixel_times).
struct StatsOpt {
    const char* counts_path = nullptr;
    const char* times_path = nullptr;
    const char* sums_path = nullptr;
    uint32_t rows = 1, cols = 1;
    bool has_grid = false;
    bool on() const { return counts_path || times_path || sums_path; }
};

struct StatsOut {
    std::vector<uint32_t> counts, times, sums;
};

// The statistics asked for of the host mask of n frames of rw x rh pixels
// into `out`; the status of the first call that fails, named in *what.
int mask_stats(dips_handle* hd, const std::vector<uint8_t>& mask, uint32_t n, uint32_t rw, uint32_t rh,
               const StatsOpt& so, StatsOut* out, const char** what) {
    const size_t npx = (size_t)rw * rh;
    if (so.counts_path) {
        // a grid the library will refuse gets one entry: nothing is written to it
        const bool sane = so.rows <= rh && so.cols <= rw && (uint64_t)n * so.rows * so.cols < (1ull << 30);
        out->counts.assign(sane ? (size_t)n * so.rows * so.cols : 1u, 0u);
        *what = "dips_mask_counts";
        const int st = dips_mask_counts(hd, mask.data(), n, rw, rh, so.rows, so.cols, out->counts.data());
        if (st != DIPS_OK) return st;
        if (n == 0) out->counts.clear();
    }
    if (so.times_path || so.sums_path) {
        if (so.times_path) out->times.assign(DIPS_TIMES_PLANES * npx, 0u);
        if (so.sums_path) out->sums.assign(npx, 0u);
        *what = "dips_mask_pixel_times";
        return dips_mask_pixel_times(hd, n ? mask.data() : nullptr, n, rw, rh, 0u, 0u,
                                     so.times_path ? out->times.data() : nullptr,
                                     so.sums_path ? out->sums.data() : nullptr);
    }
    return DIPS_OK;
}

bool write_u32_file(const char* path, const std::vector<uint32_t>& v) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(uint32_t), v.size(), f) != v.size() || std::fclose(f) != 0) {
        std::fprintf(stderr, "dips_raw: cannot write %s\n", path);
        return false;
    }
    return true;
}

// The files of the statistics: the counts as the CSV t,row,col,count, the
// times as --pixel-times writes them, the sums as one plane of roi_h x roi_w
// little-endian u32 (0: written or not asked for).
int write_mask_stats(const StatsOpt& so, const StatsOut& out) {
    if (so.counts_path) {
        std::FILE* f = std::fopen(so.counts_path, "w");
        if (!f) {
            std::fprintf(stderr, "dips_raw: cannot write %s\n", so.counts_path);
            return 1;
        }
        std::fprintf(f, "t,row,col,count\n");
        const size_t cells = (size_t)so.rows * so.cols;
        for (size_t i = 0; i < out.counts.size(); ++i)
            std::fprintf(f, "%zu,%zu,%zu,%u\n", i / cells, (i % cells) / so.cols, i % so.cols, out.counts[i]);
        if (std::ferror(f) != 0 || std::fclose(f) != 0) {
            std::fprintf(stderr, "dips_raw: cannot write %s\n", so.counts_path);
            return 1;
        }
    }
    if (so.times_path && !write_u32_file(so.times_path, out.times)) return 1;
    if (so.sums_path && !write_u32_file(so.sums_path, out.sums)) return 1;
    return 0;
}

void print_mask_stats(const StatsOpt& so) {
    if (!so.on()) return;
    std::printf(" mask_stats=");
    const char* sep = "";
    if (so.counts_path) {
        std::printf("counts:%ux%u", so.rows, so.cols);
        sep = ",";
    }
    if (so.times_path) {
        std::printf("%stimes", sep);
        sep = ",";
    }
    if (so.sums_path) std::printf("%ssums", sep);
}

// "x,y,w,h" -> roi[4] (decimal, zero allowed; the library checks the extent)
bool parse_roi(const std::string& s, uint32_t* roi) {
    size_t at = 0;
    for (int k = 0; k < 4; ++k) {
        const size_t comma = k < 3 ? s.find(',', at) : s.size();
        if (comma == std::string::npos || comma == at) return false;
        const std::string tok = s.substr(at, comma - at);
        char* end = nullptr;
        const unsigned long v = std::strtoul(tok.c_str(), &end, 10);
        if (tok[0] < '0' || tok[0] > '9' || *end || v > 0xFFFFFFFFul) return false;
        roi[k] = (uint32_t)v;
        at = comma + 1;
    }
    return true;
}

// `ranks` communicators, loopback on device 0 or RCCL with rank r on device
// r (dips_comm_create_all); 0 or the exit status of the failure
int make_comms(const std::string& transport, uint32_t ranks, std::vector<dips_comm*>& comms) {
    const bool rccl = transport == "rccl";
    comms.assign(ranks, nullptr);
    // RCCL prints its version banner to stdout when a communicator is made:
    // send it to stderr, stdout carries the program's own output only
    std::fflush(stdout);
    const int saved_stdout = dup(1);
    dup2(2, 1);
    const int st = rccl ? dips_comm_create_all((int)ranks, nullptr, comms.data())
                        : dips_comm_create_loopback((int)ranks, 0, comms.data());
    std::fflush(stdout);
    dup2(saved_stdout, 1);
    close(saved_stdout);
    if (st != DIPS_OK) {
        std::fprintf(stderr, "dips_raw: %s failed (%d): %s\n", rccl ? "dips_comm_create_all" : "dips_comm_create_loopback",
                     st, dips_comm_last_error(nullptr));
        return 2;
    }
    return 0;
}

// Run `body(rank, first, count, why)` on one thread per rank; 0, or 2 after
// printing the first failing rank's message
template <typename Body>
int on_ranks(uint32_t ranks, uint64_t n_total, const char* what, Body&& body) {
    std::vector<int> rc(ranks, 0);
    std::vector<std::string> why(ranks);
    std::vector<std::thread> threads;
    for (uint32_t r = 0; r < ranks; ++r)
        threads.emplace_back([&, r]() {
            uint64_t first = 0;
            uint32_t count = 0;
            if (dips_shard_range(n_total, (int)ranks, (int)r, &first, &count) != DIPS_OK) {
                rc[r] = 1;
                why[r] = "bad shard range";
                return;
            }
            rc[r] = body(r, first, count, why[r]);
        });
    for (auto& t : threads) t.join();
    for (uint32_t r = 0; r < ranks; ++r)
        if (rc[r] != 0) {
            std::fprintf(stderr, "dips_raw: rank %u: %s failed (%d): %s\n", r, what, rc[r], why[r].c_str());
            return 2;
        }
    return 0;
}

bool write_all(const char* path, const uint8_t* p, size_t n) {
    FILE* f = std::fopen(path, "wb");
    if (!f) {
        std::fprintf(stderr, "dips_raw: cannot create %s\n", path);
        return false;
    }
    const bool ok = std::fwrite(p, 1, n, f) == n;
    if (std::fclose(f) != 0 || !ok) {
        std::fprintf(stderr, "dips_raw: short write to %s\n", path);
        return false;
    }
    return true;
}

int run_callback(int argc, char** argv) {
    if (argc < 6) return usage();
    uint32_t w = 0, h = 0, batch = 1, ranks = 0;
    std::string transport = "loopback";
    if (!parse_u32(argv[3], &w) || !parse_u32(argv[4], &h)) return usage();
    dips_params p;
    dips_params_default(&p);  // DiPsProperties defaults (dips/src/lib.rs:71-90)
    for (int i = 6; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has = i + 1 < argc;
        if (a == "--colorize") {
            p.colorize = 1;
        } else if (a == "--window" && has) {
            p.spatial_window_size = std::atoi(argv[++i]);
        } else if (a == "--sensitivity" && has) {
            p.sensitivity = std::strtof(argv[++i], nullptr);
        } else if (a == "--filter" && has) {
            const std::string f = argv[++i];
            p.filter_type = f == "sigmoid" ? DIPS_FILTER_SIGMOID
                            : f == "inverse" ? DIPS_FILTER_INVERSE_SIGMOID
                                             : DIPS_FILTER_UNFILTERED;
        } else if (a == "--chroma" && has) {
            const std::string c = argv[++i];
            p.chroma_filter = c == "red" ? DIPS_CHROMA_RED
                              : c == "green" ? DIPS_CHROMA_GREEN
                              : c == "blue" ? DIPS_CHROMA_BLUE
                                            : DIPS_CHROMA_NONE;
        } else if (a == "--batch" && has) {
            if (!parse_u32(argv[++i], &batch)) return usage();
        } else if (a == "--ranks" && has) {
            if (!parse_u32(argv[++i], &ranks) || ranks > 64) return usage();
        } else if (a == "--transport" && has) {
            transport = argv[++i];
            if (transport != "loopback" && transport != "rccl") return usage();
        } else {
            return usage();
        }
    }
    Mapped in;
    if (!in.open(argv[2])) {
        std::fprintf(stderr, "dips_raw: cannot map %s\n", argv[2]);
        return 1;
    }
    const size_t fb = (size_t)w * h * 4u;
    if (in.n % fb != 0) {
        std::fprintf(stderr, "dips_raw: %s is not a whole number of %ux%u RGBA8 frames\n", argv[2], w, h);
        return 1;
    }
    const uint64_t n = in.n / fb;
    if (ranks > 0) {
        // one fresh ComputeState per rank; every output frame is the one
        // ComputeState over the whole file gives
        std::vector<dips_comm*> comms;
        int rc = make_comms(transport, ranks, comms);
        if (rc != 0) return rc;
        std::vector<uint8_t> outbuf(in.n);
        rc = on_ranks(ranks, n, "dips_frame_callback_batch_sharded",
                      [&](uint32_t r, uint64_t first, uint32_t count, std::string& why) {
                          dips_handle* hd = nullptr;
                          int s2 = dips_create(&p, transport == "rccl" ? (int)r : 0, &hd);
                          if (s2 != DIPS_OK) {
                              why = dips_last_error(nullptr);
                              return s2;
                          }
                          s2 = dips_frame_callback_batch_sharded(hd, comms[r], w, h, in.p + first * fb, count, n,
                                                                 outbuf.data() + first * fb);
                          if (s2 != DIPS_OK) why = dips_last_error(hd);
                          dips_destroy(hd);
                          return s2;
                      });
        for (auto* c : comms) dips_comm_destroy(c);
        if (rc != 0) return rc;
        return write_all(argv[5], outbuf.data(), outbuf.size()) ? 0 : 1;
    }
    FILE* out = std::fopen(argv[5], "wb");
    if (!out) {
        std::fprintf(stderr, "dips_raw: cannot create %s\n", argv[5]);
        return 1;
    }
    dips_handle* hd = nullptr;
    int st = dips_create(&p, 0, &hd);
    if (st != DIPS_OK) {
        std::fclose(out);
        return lib_error(nullptr, "dips_create", st);
    }
    std::vector<uint8_t> buf(fb * batch);
    int rc = 0;
    for (uint64_t t = 0; t < n && rc == 0;) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(batch, n - t);
        const uint8_t* src = in.p + t * fb;
        if (batch == 1) {
            // frame_callback: frames 0..2 come back unchanged (lib.rs:241-245)
            st = dips_frame_callback(hd, w, h, src, fb, buf.data(), buf.size());
            if (st < 0) rc = lib_error(hd, "dips_frame_callback", st);
        } else {
            st = dips_frame_callback_batch(hd, w, h, src, m, buf.data());
            if (st != DIPS_OK) rc = lib_error(hd, "dips_frame_callback_batch", st);
        }
        if (rc == 0 && std::fwrite(buf.data(), fb, m, out) != m) {
            std::fprintf(stderr, "dips_raw: short write\n");
            rc = 1;
        }
        t += m;
    }
    dips_destroy(hd);
    if (std::fclose(out) != 0 && rc == 0) rc = 1;
    return rc;
}

void print_series(const dips_series_entry* series, uint64_t n) {
    std::printf("frame,sad,sj,count,si\n");
    for (uint64_t t = 0; t < n; ++t)
        std::printf("%llu,%llu,%llu,%llu,%.17g\n", (unsigned long long)t, (unsigned long long)series[t].sad,
                    (unsigned long long)series[t].sj, (unsigned long long)series[t].count,
                    dips_series_si(&series[t]));
}

int run_sharded(int argc, char** argv) {
    if (argc < 6) return usage();
    uint32_t w = 0, h = 0, ranks = 0;
    std::string transport = "loopback";
    if (!parse_u32(argv[3], &w) || !parse_u32(argv[4], &h)) return usage();
    dips_params p;
    dips_params_default(&p);
    const std::string fmt = argv[5];
    p.format = fmt == "rgb8" ? DIPS_FMT_RGB8 : fmt == "rgba8" ? DIPS_FMT_RGBA8 : fmt == "gray8" ? DIPS_FMT_GRAY8 : 0u;
    if (!p.format) return usage();
    for (int i = 6; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has = i + 1 < argc;
        if (a == "--mode" && has) {
            const std::string m = argv[++i];
            if (m != "overall" && m != "per-frame") return usage();
            p.mode = m == "overall" ? DIPS_MODE_OVERALL : DIPS_MODE_PER_FRAME;
        } else if (a == "--tau" && has) {
            p.tau = std::strtof(argv[++i], nullptr);
        } else if (a == "--ranks" && has) {
            if (!parse_u32(argv[++i], &ranks) || ranks > 64) return usage();
        } else if (a == "--transport" && has) {
            transport = argv[++i];
            if (transport != "loopback" && transport != "rccl") return usage();
        } else {
            return usage();
        }
    }
    if (ranks == 0) return usage();
    Mapped in;
    if (!in.open(argv[2])) {
        std::fprintf(stderr, "dips_raw: cannot map %s\n", argv[2]);
        return 1;
    }
    const size_t fb = (size_t)w * h * p.format;
    if (in.n % fb != 0) {
        std::fprintf(stderr, "dips_raw: %s is not a whole number of %ux%u %s frames\n", argv[2], w, h, fmt.c_str());
        return 1;
    }
    const uint64_t n_total = in.n / fb;
    const bool rccl = transport == "rccl";
    std::vector<dips_comm*> comms;
    int rc = make_comms(transport, ranks, comms);
    if (rc != 0) return rc;
    std::vector<dips_series_entry> all(n_total);
    rc = on_ranks(ranks, n_total, "dips_diff_series_sharded",
                  [&](uint32_t r, uint64_t first, uint32_t count, std::string& why) {
                      dips_handle* hd = nullptr;
                      int s2 = dips_create(&p, rccl ? (int)r : 0, &hd);
                      if (s2 != DIPS_OK) {
                          why = dips_last_error(nullptr);
                          return s2;
                      }
                      std::vector<dips_series_entry> local(count);
                      // host pointers: the rank's frames straight from the mapped file
                      s2 = dips_diff_series_sharded(hd, comms[r], w, h, in.p + first * fb, count, n_total, nullptr, 0,
                                                    local.data(), r == 0 ? all.data() : nullptr);
                      if (s2 != DIPS_OK) why = dips_last_error(hd);
                      dips_destroy(hd);
                      return s2;
                  });
    for (auto* c : comms) dips_comm_destroy(c);
    if (rc != 0) return rc;
    print_series(all.data(), n_total);
    return 0;
}

int run_series(int argc, char** argv) {
    if (argc < 6) return usage();
    uint32_t w = 0, h = 0, chunk = 0, rows = 0, cols = 0;
    uint32_t roi[4] = {0, 0, 0, 0};
    bool has_roi = false;
    const char* pix_path = nullptr;
    const char* mask_path = nullptr;
    const char* times_path = nullptr;
    const char* boxes_path = nullptr;
    const char* tracks_path = nullptr;
    uint32_t connectivity = 8, min_area = 1, max_boxes = 64;
    bool has_box_opt = false;
    bool shapes = false;
    const char* shape_weights_path = nullptr;
    std::vector<MorphStep> morph;
    VoteOpt vote;
    SelectOpt sel;
    BackgroundOpt bg;
    SigmaDeltaOpt sd;
    StatsOpt stats;
    if (!parse_u32(argv[3], &w) || !parse_u32(argv[4], &h)) return usage();
    dips_params p;
    dips_params_default(&p);
    const std::string fmt = argv[5];
    p.format = fmt == "rgb8" ? DIPS_FMT_RGB8 : fmt == "rgba8" ? DIPS_FMT_RGBA8 : fmt == "gray8" ? DIPS_FMT_GRAY8 : 0u;
    if (!p.format) return usage();
    for (int i = 6; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has = i + 1 < argc;
        if (a == "--mode" && has) {
            const std::string m = argv[++i];
            if (m != "overall" && m != "per-frame") return usage();
            p.mode = m == "overall" ? DIPS_MODE_OVERALL : DIPS_MODE_PER_FRAME;
        } else if (a == "--tau" && has) {
            p.tau = std::strtof(argv[++i], nullptr);
        } else if (a == "--chunk" && has) {
            if (!parse_u32(argv[++i], &chunk)) return usage();
        } else if (a == "--grid" && has) {
            if (!parse_grid(argv[++i], &rows, &cols)) return usage();
        } else if (a == "--pixel-sums" && has) {
            pix_path = argv[++i];
        } else if (a == "--mask" && has) {
            mask_path = argv[++i];
        } else if (a == "--pixel-times" && has) {
            times_path = argv[++i];
        } else if (a == "--boxes" && has) {
            boxes_path = argv[++i];
        } else if (a == "--tracks" && has) {
            tracks_path = argv[++i];
        } else if ((a == "--connectivity" || a == "--min-area" || a == "--max-boxes") && has) {
            uint32_t* v = a == "--connectivity" ? &connectivity : a == "--min-area" ? &min_area : &max_boxes;
            if (!parse_u32_or_zero(argv[++i], v)) return usage();
            has_box_opt = true;
        } else if (a == "--shapes") {
            shapes = true;
        } else if (a == "--shape-weights" && has) {
            shape_weights_path = argv[++i];
        } else if (a == "--morph" && has) {
            MorphStep m{};
            if (!parse_morph(argv[++i], &m)) return usage();
            morph.push_back(m);
        } else if (a == "--vote" && has) {
            if (!parse_vote(argv[++i], &vote)) {  // a bad value: the status of a call the library refuses
                usage();
                return 2;
            }
        } else if (a == "--select" && has) {
            if (!parse_select(argv[++i], &sel)) return usage();
        } else if (a == "--hysteresis" && has) {
            char* end = nullptr;
            sel.tau_high = std::strtof(argv[++i], &end);
            if (end == argv[i] || *end) return usage();
            sel.hysteresis = true;
        } else if (a == "--fill-holes") {
            sel.fill = true;
            if (has && parse_u32_or_zero(argv[i + 1], &sel.max_hole)) ++i;  // MAX is optional
        } else if (a == "--background" && has) {
            if (!parse_background(argv[++i], &bg)) return usage();
        } else if (a == "--background-out" && has) {
            bg.out_path = argv[++i];
        } else if (a == "--sigma-delta" && has) {
            if (!parse_sigma_delta(argv[++i], &sd)) return usage();
        } else if (a == "--sigma-delta-out" && has) {
            sd.out_path = argv[++i];
        } else if (a == "--mask-counts" && has) {
            stats.counts_path = argv[++i];
        } else if (a == "--mask-grid" && has) {
            if (!parse_grid(argv[++i], &stats.rows, &stats.cols)) return usage();
            stats.has_grid = true;
        } else if (a == "--mask-times" && has) {
            stats.times_path = argv[++i];
        } else if (a == "--mask-sums" && has) {
            stats.sums_path = argv[++i];
        } else if (a == "--roi" && has) {
            if (!parse_roi(argv[++i], roi)) return usage();
            has_roi = true;
        } else {
            return usage();
        }
    }
    // --mask-grid belongs to --mask-counts; the statistics are the mask's, not --grid's, --pixel-sums' or --pixel-times'
    if ((stats.has_grid && !stats.counts_path) || (stats.on() && (rows != 0 || pix_path || times_path))) return usage();
    // what takes a mask: --mask, --boxes, --tracks or a statistic of the mask
    const bool masked = mask_path || boxes_path || tracks_path || stats.on();
    // --morph belongs to those
    if (!morph.empty() && !masked) return usage();
    // so does --vote
    if (vote.window != 0u && !masked) return usage();
    // so do --select, --hysteresis and --fill-holes; the last two take the plain change mask only
    if (sel.any() && !masked) return usage();
    if ((sel.hysteresis || sel.fill) && (bg.on || sd.on)) return usage();
    if (sel.hysteresis && !(sel.tau_high >= p.tau)) return usage();
    // --background too, --background-out to --background
    if ((bg.on && !masked) || (bg.out_path && !bg.on)) return usage();
    // so does --sigma-delta, --sigma-delta-out to --sigma-delta; the two models exclude each other
    if ((sd.on && !masked) || (sd.out_path && !sd.on) || (sd.on && bg.on)) return usage();
    // --roi belongs to --grid, --pixel-sums, --pixel-times or what takes a mask
    if (has_roi && rows == 0 && !pix_path && !times_path && !masked) return usage();
    if ((rows != 0) + (pix_path != nullptr) + (mask_path != nullptr) + (times_path != nullptr) +
            (boxes_path != nullptr) + (tracks_path != nullptr) > 1)
        return usage();
    if (has_box_opt && !boxes_path && !tracks_path) return usage();
    // --shapes belongs to --boxes or --tracks, --shape-weights to --shapes
    if ((shapes && !boxes_path && !tracks_path) || (shape_weights_path && !shapes)) return usage();
    if (connectivity != 4u && connectivity != 8u) return usage();
    Mapped in;
    if (!in.open(argv[2])) {
        std::fprintf(stderr, "dips_raw: cannot map %s\n", argv[2]);
        return 1;
    }
    const size_t fb = (size_t)w * h * p.format;
    if (in.n % fb != 0 || in.n / fb > 0xFFFFFFFFull) {
        std::fprintf(stderr, "dips_raw: %s is not a whole number of %ux%u %s frames\n", argv[2], w, h, fmt.c_str());
        return 1;
    }
    const uint32_t n = (uint32_t)(in.n / fb);
    dips_handle* hd = nullptr;
    int st = dips_create(&p, 0, &hd);
    if (st != DIPS_OK) return lib_error(nullptr, "dips_create", st);
    if (rows != 0) {
        std::vector<dips_series_entry> cells((size_t)n * rows * cols);
        st = dips_diff_series_grid(hd, w, h, in.p, n, nullptr, has_roi ? roi : nullptr, rows, cols, cells.data());
        if (st != DIPS_OK) {
            const int rc = lib_error(hd, "dips_diff_series_grid", st);
            dips_destroy(hd);
            return rc;
        }
        std::printf("t,row,col,sad,sj,count,si_fixed\n");
        for (size_t i = 0; i < cells.size(); ++i) {
            const size_t cell = i % ((size_t)rows * cols);
            std::printf("%zu,%zu,%zu,%llu,%llu,%llu,%llu\n", i / ((size_t)rows * cols), cell / cols, cell % cols,
                        (unsigned long long)cells[i].sad, (unsigned long long)cells[i].sj,
                        (unsigned long long)cells[i].count, (unsigned long long)cells[i].si_fixed);
        }
        dips_destroy(hd);
        return 0;
    }
    if (pix_path) {
        const uint32_t rw = has_roi ? roi[2] : w, rh = has_roi ? roi[3] : h;
        // a region the library will refuse gets one entry: nothing is written to it
        uint32_t rect[4];
        const bool sane = dips_grid_cell(w, h, has_roi ? roi : nullptr, 1u, 1u, 0u, 0u, rect) == DIPS_OK &&
                          (uint64_t)rw * rh < (1ull << 30);
        std::vector<dips_series_entry> sums(sane ? (size_t)rw * rh : 1u);
        st = dips_diff_pixel_sums(hd, w, h, in.p, n, nullptr, has_roi ? roi : nullptr, 0u, sums.data());
        if (st != DIPS_OK) {
            const int rc = lib_error(hd, "dips_diff_pixel_sums", st);
            dips_destroy(hd);
            return rc;
        }
        dips_destroy(hd);
        // roi_h x roi_w x {sad, sj, count, si_fixed}, little-endian u64 (the host's own order on every target)
        std::FILE* f = std::fopen(pix_path, "wb");
        if (!f || std::fwrite(sums.data(), sizeof(dips_series_entry), sums.size(), f) != sums.size() ||
            std::fclose(f) != 0) {
            std::fprintf(stderr, "dips_raw: cannot write %s\n", pix_path);
            return 1;
        }
        unsigned long long tot[4] = {0, 0, 0, 0};
        for (const dips_series_entry& e : sums) {
            tot[0] += e.sad;
            tot[1] += e.sj;
            tot[2] += e.count;
            tot[3] += e.si_fixed;
        }
        std::printf("pixel-sums roi=%u,%u,%u,%u frames=%u sad=%llu sj=%llu count=%llu si_fixed=%llu\n",
                    has_roi ? roi[0] : 0u, has_roi ? roi[1] : 0u, rw, rh, n, tot[0], tot[1], tot[2], tot[3]);
        return 0;
    }
    if (mask_path || (stats.on() && !boxes_path && !tracks_path)) {  // the statistics alone: the mask is not written
        const uint32_t rw = has_roi ? roi[2] : w, rh = has_roi ? roi[3] : h;
        // a region the library will refuse gets one byte: nothing is written to it
        uint32_t rect[4];
        const bool sane = dips_grid_cell(w, h, has_roi ? roi : nullptr, 1u, 1u, 0u, 0u, rect) == DIPS_OK &&
                          (uint64_t)rw * rh < (1ull << 30);
        const uint32_t row_bytes = dips_mask_row_bytes(rw);
        std::vector<uint8_t> mask(sane ? (size_t)n * rh * row_bytes : 1u);
        std::vector<uint16_t> state(state_values(sane, bg, sd, p.format, rw, rh));
        const char* what = nullptr;
        st = region_mask(hd, w, h, in.p, n, has_roi ? roi : nullptr, bg, sd, state, mask.data(), &what);
        if (st == DIPS_OK && vote.window != 0u) {
            what = "dips_mask_vote";
            st = apply_vote(hd, mask, n, rw, rh, vote);
        }
        if (st == DIPS_OK && !morph.empty()) {
            what = "dips_mask_morph";
            st = apply_morph(hd, mask, n, rw, rh, morph);
        }
        if (st == DIPS_OK) st = apply_select(hd, p, w, h, in.p, n, has_roi ? roi : nullptr, mask, rw, rh, sel, &what);
        StatsOut stats_out;
        if (st == DIPS_OK) st = mask_stats(hd, mask, n, rw, rh, stats, &stats_out, &what);
        if (st != DIPS_OK) {
            const int rc = what ? lib_error(hd, what, st) : 2;  // NULL: reported already
            dips_destroy(hd);
            return rc;
        }
        dips_destroy(hd);
        if (n == 0) mask.clear();
        if (write_background(bg, sd, state) != 0 || write_mask_stats(stats, stats_out) != 0) return 1;
        if (mask_path) {
            // frames x roi_h x row_bytes, bit i of a row = bit (i & 7) of byte (i >> 3)
            std::FILE* f = std::fopen(mask_path, "wb");
            if (!f || std::fwrite(mask.data(), 1, mask.size(), f) != mask.size() || std::fclose(f) != 0) {
                std::fprintf(stderr, "dips_raw: cannot write %s\n", mask_path);
                return 1;
            }
        }
        unsigned long long set = 0;
        for (const uint8_t b : mask) set += (unsigned long long)__builtin_popcount(b);
        std::printf("%s roi=%u,%u,%u,%u frames=%u row_bytes=%u set=%llu", mask_path ? "mask" : "mask-stats",
                    has_roi ? roi[0] : 0u, has_roi ? roi[1] : 0u, rw, rh, n, row_bytes, set);
        if (vote.window != 0u) std::printf(" vote=%u,%u", vote.window, vote.votes);
        if (!morph.empty()) std::printf(" morph=%zu", morph.size());
        print_select(sel);
        print_background(bg, sd);
        print_mask_stats(stats);
        std::printf("\n");
        return 0;
    }
    if (boxes_path || tracks_path) {
        // --tracks: the same file with the four link words behind every record
        const bool tracks = tracks_path != nullptr;
        const char* out_path = tracks ? tracks_path : boxes_path;
        const uint32_t rw = has_roi ? roi[2] : w, rh = has_roi ? roi[3] : h;
        // a region or a record count the library will refuse gets one element: nothing is written to it
        uint32_t rect[4];
        const bool sane = dips_grid_cell(w, h, has_roi ? roi : nullptr, 1u, 1u, 0u, 0u, rect) == DIPS_OK &&
                          (uint64_t)rw * rh < (1ull << 30) && rw < (1u << 24) && rh < (1u << 24) &&
                          (uint64_t)n * max_boxes * DIPS_BOX_WORDS < (1ull << 32) &&
                          (!tracks || max_boxes <= DIPS_TRACK_MAX_BOXES) &&
                          (!shapes || (rw <= 65536u && rh <= 65536u &&
                                       (uint64_t)n * max_boxes * DIPS_SHAPE_WORDS < (1ull << 32)));
        Mapped weights;
        if (shape_weights_path && (!weights.open(shape_weights_path) || weights.n != (size_t)n * rw * rh)) {
            std::fprintf(stderr, "dips_raw: %s is not %u planes of %ux%u bytes\n", shape_weights_path, n, rw, rh);
            dips_destroy(hd);
            return 1;
        }
        std::vector<uint8_t> mask(sane ? (size_t)n * rh * dips_mask_row_bytes(rw) : 1u);
        std::vector<uint32_t> counts(sane ? (size_t)n : 1u), recs(sane ? (size_t)n * max_boxes * DIPS_BOX_WORDS : 1u);
        std::vector<uint32_t> links(sane && tracks ? (size_t)n * max_boxes * DIPS_LINK_WORDS : 1u);
        std::vector<uint32_t> shape_recs(sane && shapes ? (size_t)n * max_boxes * DIPS_SHAPE_WORDS : 1u);
        std::vector<uint32_t> ids(sane && tracks ? 1u + 2u * (size_t)max_boxes : 1u);  // the state: [0] counts the tracks
        std::vector<uint16_t> state(state_values(sane, bg, sd, p.format, rw, rh));
        const char* what = nullptr;
        st = region_mask(hd, w, h, in.p, n, has_roi ? roi : nullptr, bg, sd, state, mask.data(), &what);
        if (st == DIPS_OK && vote.window != 0u) {
            what = "dips_mask_vote";
            st = apply_vote(hd, mask, n, rw, rh, vote);
        }
        if (st == DIPS_OK && !morph.empty()) {
            what = "dips_mask_morph";
            st = apply_morph(hd, mask, n, rw, rh, morph);
        }
        if (st == DIPS_OK) st = apply_select(hd, p, w, h, in.p, n, has_roi ? roi : nullptr, mask, rw, rh, sel, &what);
        if (st == DIPS_OK && tracks) {
            what = "dips_mask_tracks";
            st = dips_mask_tracks(hd, mask.data(), n, rw, rh, connectivity, min_area, max_boxes, 0u, nullptr, ids.data(),
                                  counts.data(), recs.data(), links.data());
        } else if (st == DIPS_OK && !shapes) {
            what = "dips_mask_components";
            st = dips_mask_components(hd, mask.data(), n, rw, rh, connectivity, min_area, max_boxes, 0u, counts.data(),
                                      max_boxes ? recs.data() : nullptr, nullptr);
        }
        if (st == DIPS_OK && shapes) {  // the same counts and records once more, and their shapes
            what = "dips_mask_shapes";
            st = dips_mask_shapes(hd, mask.data(), weights.p, n, rw, rh, connectivity, min_area, max_boxes, 0u,
                                  counts.data(), max_boxes ? recs.data() : nullptr,
                                  max_boxes ? shape_recs.data() : nullptr);
        }
        StatsOut stats_out;
        if (st == DIPS_OK) st = mask_stats(hd, mask, n, rw, rh, stats, &stats_out, &what);
        if (st != DIPS_OK) {
            const int rc = what ? lib_error(hd, what, st) : 2;  // NULL: reported already
            dips_destroy(hd);
            return rc;
        }
        dips_destroy(hd);
        if (write_background(bg, sd, state) != 0 || write_mask_stats(stats, stats_out) != 0) return 1;
        std::FILE* f = std::fopen(out_path, "w");
        if (!f) {
            std::fprintf(stderr, "dips_raw: cannot write %s\n", out_path);
            return 1;
        }
        std::fprintf(f, "frame,k,x0,y0,x1,y1,area,anchor,cx256,cy256%s%s\n", tracks ? ",prev,overlap,track,age" : "",
                     shapes ? ",sx,sy,sxx,syy,sxy,wsum,wmax,cracks_v,cracks_h,euler" : "");
        unsigned long long total = 0, stored = 0;
        for (uint32_t t = 0; t < n; ++t) {
            std::fprintf(f, "# %u,%u\n", t, counts[t]);
            total += counts[t];
            for (uint32_t k = 0; k < std::min(counts[t], max_boxes); ++k, ++stored) {
                const uint32_t* r = &recs[((size_t)t * max_boxes + k) * DIPS_BOX_WORDS];
                std::fprintf(f, "%u,%u,%u,%u,%u,%u,%u,%u,%u,%u", t, k, r[DIPS_BOX_X0], r[DIPS_BOX_Y0], r[DIPS_BOX_X1],
                             r[DIPS_BOX_Y1], r[DIPS_BOX_AREA], r[DIPS_BOX_ANCHOR], r[DIPS_BOX_CX256], r[DIPS_BOX_CY256]);
                if (tracks) {
                    const uint32_t* l = &links[((size_t)t * max_boxes + k) * DIPS_LINK_WORDS];
                    std::fprintf(f, ",%u,%u,%u,%u", l[DIPS_LINK_PREV], l[DIPS_LINK_OVERLAP], l[DIPS_LINK_TRACK],
                                 l[DIPS_LINK_AGE]);
                }
                if (shapes) {
                    const uint32_t* q = &shape_recs[((size_t)t * max_boxes + k) * DIPS_SHAPE_WORDS];
                    for (uint32_t fld = DIPS_SHAPE_SX; fld <= DIPS_SHAPE_WSUM; fld += 2u)
                        std::fprintf(f, ",%llu", (unsigned long long)q[fld] | ((unsigned long long)q[fld + 1u] << 32));
                    std::fprintf(f, ",%u,%u,%u,%d", q[DIPS_SHAPE_WMAX], q[DIPS_SHAPE_CRACKS_V], q[DIPS_SHAPE_CRACKS_H],
                                 (int32_t)q[DIPS_SHAPE_EULER]);
                }
                std::fprintf(f, "\n");
            }
        }
        if (std::ferror(f) != 0 || std::fclose(f) != 0) {
            std::fprintf(stderr, "dips_raw: cannot write %s\n", out_path);
            return 1;
        }
        std::printf("%s roi=%u,%u,%u,%u frames=%u connectivity=%u min_area=%u max_boxes=%u components=%llu records=%llu",
                    tracks ? "tracks" : "boxes", has_roi ? roi[0] : 0u, has_roi ? roi[1] : 0u, rw, rh, n, connectivity,
                    min_area, max_boxes, total, stored);
        if (tracks) std::printf(" tracks=%u", ids[0]);
        if (vote.window != 0u) std::printf(" vote=%u,%u", vote.window, vote.votes);
        if (!morph.empty()) std::printf(" morph=%zu", morph.size());
        print_select(sel);
        print_background(bg, sd);
        print_mask_stats(stats);
        if (shapes) std::printf(" shapes=1");
        std::printf("\n");
        return 0;
    }
    if (times_path) {
        const uint32_t rw = has_roi ? roi[2] : w, rh = has_roi ? roi[3] : h;
        // a region the library will refuse gets one value: nothing is written to it
        uint32_t rect[4];
        const bool sane = dips_grid_cell(w, h, has_roi ? roi : nullptr, 1u, 1u, 0u, 0u, rect) == DIPS_OK &&
                          (uint64_t)rw * rh < (1ull << 30);
        const size_t npx = sane ? (size_t)rw * rh : 0u;
        std::vector<uint32_t> times(sane ? DIPS_TIMES_PLANES * npx : 1u);
        st = dips_diff_pixel_times(hd, w, h, in.p, n, nullptr, has_roi ? roi : nullptr, 0u, 0u, times.data());
        if (st != DIPS_OK) {
            const int rc = lib_error(hd, "dips_diff_pixel_times", st);
            dips_destroy(hd);
            return rc;
        }
        dips_destroy(hd);
        // four planes of roi_h x roi_w little-endian u32 (the host's own order on every target)
        std::FILE* f = std::fopen(times_path, "wb");
        if (!f || std::fwrite(times.data(), sizeof(uint32_t), times.size(), f) != times.size() || std::fclose(f) != 0) {
            std::fprintf(stderr, "dips_raw: cannot write %s\n", times_path);
            return 1;
        }
        unsigned long long never = 0;
        long long min_first = -1, max_last = -1;
        uint32_t max_run = 0;
        for (size_t i = 0; i < npx; ++i) {
            const uint32_t fi = times[DIPS_TIMES_FIRST * npx + i], la = times[DIPS_TIMES_LAST * npx + i];
            max_run = std::max(max_run, times[DIPS_TIMES_RUN_MAX * npx + i]);
            if (fi == DIPS_TIME_NONE) {
                never += 1;
                continue;
            }
            min_first = min_first < 0 ? (long long)fi : std::min(min_first, (long long)fi);
            max_last = std::max(max_last, (long long)la);
        }
        std::printf("pixel-times roi=%u,%u,%u,%u frames=%u never=%llu min_first=%lld max_last=%lld max_run=%u\n",
                    has_roi ? roi[0] : 0u, has_roi ? roi[1] : 0u, rw, rh, n, never, min_first, max_last, max_run);
        return 0;
    }
    std::vector<dips_series_entry> series(n);
    st = dips_diff_series_streamed(hd, w, h, in.p, n, nullptr, series.data(), chunk);
    if (st != DIPS_OK) {
        const int rc = lib_error(hd, "dips_diff_series_streamed", st);
        dips_destroy(hd);
        return rc;
    }
    print_series(series.data(), n);
    dips_destroy(hd);
    return 0;
}

int alt_error(dips_alt_handle* h, const char* what, int st) {
    std::fprintf(stderr, "dips_raw: %s failed (%d): %s\n", what, st, dips_alt_last_error(h));
    return 2;
}

int run_alt(int argc, char** argv) {
    if (argc < 6) return usage();
    uint32_t w = 0, h = 0, ranks = 0;
    std::string transport = "loopback";
    std::vector<uint64_t> markers;
    if (!parse_u32(argv[3], &w) || !parse_u32(argv[4], &h)) return usage();
    dips_alt_params p;
    dips_alt_params_default(&p);  // DiPsProperties::default() (dips_alt/src/dips_compute/mod.rs:176-186)
    for (int i = 6; i < argc; ++i) {
        const std::string a = argv[i];
        const bool has = i + 1 < argc;
        if (a == "--markers" && has) {
            // comma-separated 1-based frame positions (lib.rs:668-670)
            const std::string list = argv[++i];
            size_t at = 0;
            while (at <= list.size()) {
                const size_t comma = std::min(list.find(',', at), list.size());
                uint32_t m = 0;
                if (!parse_u32(list.substr(at, comma - at).c_str(), &m)) return usage();
                markers.push_back(m);
                at = comma + 1;
            }
        } else if (a == "--window" && has) {
            p.window_size = std::atoi(argv[++i]);
        } else if (a == "--textures" && has) {
            if (!parse_u32(argv[++i], &p.num_textures)) return usage();
        } else if (a == "--ranks" && has) {
            if (!parse_u32(argv[++i], &ranks) || ranks > 64) return usage();
        } else if (a == "--transport" && has) {
            transport = argv[++i];
            if (transport != "loopback" && transport != "rccl") return usage();
        } else {
            return usage();
        }
    }
    Mapped in;
    if (!in.open(argv[2])) {
        std::fprintf(stderr, "dips_raw: cannot map %s\n", argv[2]);
        return 1;
    }
    const size_t fb = (size_t)w * h * 4u;
    if (in.n % fb != 0 || in.n / fb > 0xFFFFFFFFull) {
        std::fprintf(stderr, "dips_raw: %s is not a whole number of %ux%u RGBA8 frames\n", argv[2], w, h);
        return 1;
    }
    const uint64_t n = in.n / fb;
    const uint64_t* mk = markers.empty() ? nullptr : markers.data();
    std::vector<uint8_t> outbuf(in.n);
    if (ranks == 0) {
        dips_alt_handle* hd = nullptr;
        int st = dips_alt_create(&p, w, h, 0, &hd);
        if (st != DIPS_OK) return alt_error(nullptr, "dips_alt_create", st);
        st = dips_alt_run(hd, in.p, (uint32_t)n, mk, (uint32_t)markers.size(), outbuf.data());
        const int rc = st != DIPS_OK ? alt_error(hd, "dips_alt_run", st) : 0;
        dips_alt_destroy(hd);
        if (rc != 0) return rc;
    } else {
        std::vector<dips_comm*> comms;
        int rc = make_comms(transport, ranks, comms);
        if (rc != 0) return rc;
        rc = on_ranks(ranks, n, "dips_alt_run_sharded",
                      [&](uint32_t r, uint64_t first, uint32_t count, std::string& why) {
                          dips_alt_handle* hd = nullptr;
                          int s2 = dips_alt_create(&p, w, h, transport == "rccl" ? (int)r : 0, &hd);
                          if (s2 != DIPS_OK) {
                              why = dips_alt_last_error(nullptr);
                              return s2;
                          }
                          s2 = dips_alt_run_sharded(hd, comms[r], in.p + first * fb, count, n, mk,
                                                    (uint32_t)markers.size(), outbuf.data() + first * fb);
                          if (s2 != DIPS_OK) why = dips_alt_last_error(hd);
                          dips_alt_destroy(hd);
                          return s2;
                      });
        for (auto* c : comms) dips_comm_destroy(c);
        if (rc != 0) return rc;
    }
    return write_all(argv[5], outbuf.data(), outbuf.size()) ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    if (cmd == "callback") return run_callback(argc, argv);
    if (cmd == "series") return run_series(argc, argv);
    if (cmd == "sharded") return run_sharded(argc, argv);
    if (cmd == "alt") return run_alt(argc, argv);
    return usage();
}
