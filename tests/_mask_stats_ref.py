"""The specification of dips_mask_counts and dips_mask_pixel_times in plain
numpy, written from the definitions in include/dips_hip.h: the mask unpacked
with bitorder "little" and cropped to the width, a per-cell sum over the
rectangles of dips_grid_cell, and the fold of dips_diff_pixel_times frame by
frame."""
import numpy as np

NONE = 0xFFFFFFFF  # DIPS_TIME_NONE


def unpack(mask_bytes, w):
    """mask bytes [n, h, row_bytes] -> bool [n, h, w]; the pad bits are dropped."""
    return np.unpackbits(np.asarray(mask_bytes, dtype=np.uint8), axis=-1, bitorder="little")[..., :w].astype(bool)


def grid_cell(w, h, rows, cols, r, c):
    """(x, y, cw, ch) of cell (r, c): column c covers [c*w//cols, (c+1)*w//cols), rows likewise."""
    x0, x1 = c * w // cols, (c + 1) * w // cols
    y0, y1 = r * h // rows, (r + 1) * h // rows
    return x0, y0, x1 - x0, y1 - y0


def counts_bits(bits, rows=1, cols=1):
    """bits bool [n, h, w] -> uint32 [n, rows, cols]: the set bits per frame and cell."""
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    assert 1 <= rows <= h and 1 <= cols <= w
    out = np.zeros((n, rows, cols), dtype=np.uint32)
    for r in range(rows):
        for c in range(cols):
            x, y, cw, ch = grid_cell(w, h, rows, cols, r, c)
            out[:, r, c] = bits[:, y:y + ch, x:x + cw].sum(axis=(1, 2), dtype=np.uint32)
    return out


def counts(mask_bytes, w, rows=1, cols=1):
    return counts_bits(unpack(mask_bytes, w), rows, cols)


def initial_times(h, w):
    t = np.zeros((4, h, w), dtype=np.uint32)
    t[:2] = NONE
    return t


def times_bits(bits, t0=0, state=None):
    """bits bool [n, h, w] -> uint32 [4, h, w] (first, last, run_max, run_cur):
    the fold of the header, frame by frame, from `state` or the initial state."""
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    first, last, rmax, rcur = (initial_times(h, w) if state is None else np.array(state, dtype=np.uint32))
    for t in range(n):
        b, g = bits[t], np.uint32(t0 + t)
        first = np.where(b & (first == NONE), g, first)
        last = np.where(b, g, last)
        rcur = np.where(b, rcur + np.uint32(1), np.uint32(0))
        rmax = np.maximum(rmax, rcur)
    return np.stack([first, last, rmax, rcur]).astype(np.uint32)


def sums_bits(bits, state=None):
    """bits bool [n, h, w] -> uint32 [h, w]: the frames whose bit is set, modulo 2^32."""
    bits = np.asarray(bits, dtype=bool)
    s = bits.sum(axis=0, dtype=np.uint64)
    if state is not None:
        s = s + np.asarray(state, dtype=np.uint64)
    return (s & 0xFFFFFFFF).astype(np.uint32)


def times(mask_bytes, w, t0=0, state=None):
    return times_bits(unpack(mask_bytes, w), t0, state)


def sums(mask_bytes, w, state=None):
    return sums_bits(unpack(mask_bytes, w), state)


def times_naive(bits, t0=0):
    """times_bits from the initial state by a loop over pixels and frames."""
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    out = initial_times(h, w)
    for j in range(h):
        for i in range(w):
            first, last, rmax, rcur = NONE, NONE, 0, 0
            for t in range(n):
                if bits[t, j, i]:
                    first = t0 + t if first == NONE else first
                    last = t0 + t
                    rcur += 1
                    rmax = max(rmax, rcur)
                else:
                    rcur = 0
            out[:, j, i] = (first, last, rmax, rcur)
    return out


# The schedule harness: tests compile dips_amd/csrc/series_sched.h alone with
# g++ and read the schedules of the mask statistics from it.
# stdin rows: "T frame_slots n_frames summary_bytes parts_bytes resident" or
# "C roi_w roi_h rows cols n_frames chunk_cells min_band_words resident_blocks";
# stdout rows: T: ok part_frames parts n_tiles n_waves blocks; C: ok col_chunks
# bands band_rows items blocks
GEOMETRY_PROGRAM = r'''
#include "series_sched.h"
#include <cstdio>
using namespace dips_sched;
int main() {
    char kind;
    long long v[8];
    while (std::scanf(" %c", &kind) == 1) {
        const int nv = kind == 'T' ? 5 : 8;
        for (int i = 0; i < nv; ++i)
            if (std::scanf("%lld", &v[i]) != 1) return 1;
        if (kind == 'T') {
            const Geom q = mask_times_geometry((uint64_t)v[0], (uint32_t)v[1], (uint64_t)v[2], (uint64_t)v[3], (uint64_t)v[4]);
            std::printf("%d %u %u %llu %llu %llu\n", (int)q.ok, q.part_frames, q.parts, (unsigned long long)q.n_tiles,
                        (unsigned long long)q.n_waves, (unsigned long long)q.blocks);
        } else {
            const CountsGeom q = mask_counts_geometry((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3],
                                                      (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6], (uint64_t)v[7]);
            std::printf("%d %u %u %u %llu %llu\n", (int)q.ok, q.col_chunks, q.bands, q.band_rows,
                        (unsigned long long)q.items, (unsigned long long)q.blocks);
        }
    }
    return 0;
}
'''

PARTS_BYTES = 1 << 30  # kMaskTimesPartsBytes of mask_abi.hip


def build_geometry(directory, csrc):
    import subprocess
    src = directory / "mask_stats_sched.cpp"
    src.write_text(GEOMETRY_PROGRAM)
    exe = directory / "mask_stats_sched"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    return exe


def _run(exe, kind, rows, names):
    import subprocess
    txt = "".join(kind + " " + " ".join(str(int(x)) for x in r) + "\n" for r in rows)
    r = subprocess.run([str(exe)], input=txt, capture_output=True, text=True, timeout=60, check=True)
    out = [dict(zip(names, (int(x) for x in line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(rows)
    return out


def times_geometry(exe, rows):
    """dicts ok, part_frames, parts, n_tiles, n_waves, blocks for rows
    (frame_slots, n_frames, summary_bytes, parts_bytes, resident)."""
    return _run(exe, "T", rows, "ok part_frames parts n_tiles n_waves blocks".split())


def counts_geometry(exe, rows):
    """dicts ok, col_chunks, bands, band_rows, items, blocks for rows (roi_w,
    roi_h, rows, cols, n_frames, chunk_cells, min_band_words, resident_blocks)."""
    return _run(exe, "C", rows, "ok col_chunks bands band_rows items blocks".split())


def kernel_constants(csrc):
    """(pixels per lane, chunk cells, min band words) of dips_kernels.h."""
    import os
    import re
    with open(os.path.join(csrc, "dips_kernels.h")) as f:
        txt = f.read()
    return (int(re.search(r"#define DIPS_MASK_TIMES_PX (\d+)", txt).group(1)),
            int(re.search(r"kCountsChunkCells = (\d+);", txt).group(1)),
            int(re.search(r"kCountsMinBandWords = (\d+);", txt).group(1)))


def frame_slots(w, h, px):
    """Lane slots of a frame: its bytes times the slots of a byte."""
    return 4 * ((w + 31) // 32) * h * (8 // px)


def summary_bytes(w, h, times=True, sums=True):
    return 4 * ((5 if times else 0) + (1 if sums else 0)) * w * h
