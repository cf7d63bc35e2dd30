"""CPU checks of the mask statistics (dips_mask_counts, dips_mask_pixel_times):
the numpy specification tests/_mask_stats_ref.py against hand-worked cases and
its own naive loop, chunked equals whole on the specification, the schedules
(series_sched.h mask_times_geometry and mask_counts_geometry, compiled alone
with g++): every (part, tile) and every (row, column) covered exactly once,
the Python argument checks that need no device, and the exported names."""
import os

import numpy as np
import pytest

import _components_ref as cref
import _mask_stats_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")
N = sref.NONE


def bits_of(n, h, w, density, seed=0):
    return np.random.default_rng([103, seed, n, h, w]).random((n, h, w)) < density


# -- the reference ------------------------------------------------------------------------

def test_counts_hand_worked():
    # 2 frames of 2 x 5: frame 0 = rows 11100 / 00011, frame 1 all set
    bits = np.array([[[1, 1, 1, 0, 0], [0, 0, 0, 1, 1]], [[1] * 5, [1] * 5]], dtype=bool)
    assert sref.counts_bits(bits).tolist() == [[[5]], [[10]]]
    # cols = 2: columns [0, 2) and [2, 5)
    assert sref.counts_bits(bits, 1, 2).tolist() == [[[2, 3]], [[4, 6]]]
    assert sref.counts_bits(bits, 2, 2).tolist() == [[[2, 1], [0, 2]], [[2, 3], [2, 3]]]
    # rows = h, cols = w: the mask itself
    assert np.array_equal(sref.counts_bits(bits, 2, 5), bits.astype(np.uint32))
    # the packed form drops the pad bits
    assert np.array_equal(sref.counts(cref.pack(bits, 1), 5, 2, 2), sref.counts_bits(bits, 2, 2))
    assert [sref.grid_cell(100, 17, 3, 7, 2, c)[::2] for c in range(7)] == [
        (0, 14), (14, 14), (28, 14), (42, 15), (57, 14), (71, 14), (85, 15)]
    assert [sref.grid_cell(100, 17, 3, 7, r, 0)[1::2] for r in range(3)] == [(0, 5), (5, 6), (11, 6)]


def test_times_hand_worked():
    # one row of 4 pixels over 6 frames, t0 = 10
    #            never  always  0 1 1 0 1 0   0 0 0 1 1 1
    cols = [[0] * 6, [1] * 6, [0, 1, 1, 0, 1, 0], [0, 0, 0, 1, 1, 1]]
    bits = np.array(cols, dtype=bool).T.reshape(6, 1, 4)
    got = sref.times_bits(bits, t0=10)
    assert got[:, 0].T.tolist() == [[N, N, 0, 0], [10, 15, 6, 6], [11, 14, 2, 0], [13, 15, 3, 3]]
    assert sref.sums_bits(bits)[0].tolist() == [0, 6, 3, 3]
    assert np.array_equal(got, sref.times_naive(bits, t0=10))
    # no frames: the initial state, or the state given
    empty = np.zeros((0, 1, 4), dtype=bool)
    assert sref.times_bits(empty)[:, 0, 0].tolist() == [N, N, 0, 0]
    assert np.array_equal(sref.times_bits(empty, state=got), got)
    # a run across a chunk boundary is counted whole
    head = sref.times_bits(bits[:2], t0=10)
    assert head[:, 0, 2].tolist() == [11, 11, 1, 1]
    assert np.array_equal(sref.times_bits(bits[2:], t0=12, state=head), got)
    # sums wrap modulo 2^32
    assert sref.sums_bits(bits, state=np.full((1, 4), 0xFFFFFFFE, dtype=np.uint32))[0].tolist() == [0xFFFFFFFE, 4, 1, 1]


@pytest.mark.parametrize("density", [0.0, 0.05, 0.5, 1.0])
def test_reference_equals_the_naive_loop_and_its_chunks(density):
    bits = bits_of(23, 3, 37, density, seed=int(density * 100))
    whole = sref.times_bits(bits, t0=5)
    assert np.array_equal(whole, sref.times_naive(bits, t0=5))
    state, s, t = None, None, 5
    for k in (1, 7, 0, 15):
        state = sref.times_bits(bits[t - 5:t - 5 + k], t0=t, state=state)
        s = sref.sums_bits(bits[t - 5:t - 5 + k], state=s)
        t += k
    assert np.array_equal(state, whole) and np.array_equal(s, sref.sums_bits(bits))
    assert np.array_equal(sref.times(cref.pack(bits, 1), 37, 5), whole)
    assert np.array_equal(sref.sums(cref.pack(bits, 1), 37), bits.sum(axis=0))
    # the 1 x 1 grid is the count series, and the cells of any grid add up to it
    assert np.array_equal(sref.counts_bits(bits)[:, 0, 0], bits.sum(axis=(1, 2)))
    assert np.array_equal(sref.counts_bits(bits, 2, 5).sum(axis=(1, 2)), bits.sum(axis=(1, 2)))


# -- the schedules ------------------------------------------------------------------------

RESIDENTS = [256, 1024, 4096, 6144, 8192, 16384]
# (w, h, n) of the GPU test's shapes and degenerate ones
TIMES_SHAPES = [(1, 1, 1), (1, 1, 40), (33, 2, 600), (33, 2, 15), (33, 2, 16), (33, 2, 31), (33, 2, 32), (257, 17, 40),
                (100, 3, 7), (67, 19, 12), (3840, 2160, 8), (3840, 2160, 500), (640, 480, 5000), (1, 1, 100000)]


@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    return sref.build_geometry(tmp_path_factory.mktemp("mask_stats_sched"), CSRC)


def test_times_geometry_covers_every_part_and_tile_once(sched):
    px, _, _ = sref.kernel_constants(CSRC)
    assert px in (4, 8)
    rows = [(sref.frame_slots(w, h, px), n, sref.summary_bytes(w, h), sref.PARTS_BYTES, res)
            for (w, h, n) in TIMES_SHAPES for res in RESIDENTS]
    several = 0
    for (slots, n, summary, _, res), q in zip(rows, sref.times_geometry(sched, rows)):
        assert q["ok"] == 1 and q["n_tiles"] == -(-slots // 64)
        L, parts = q["part_frames"], q["parts"]
        # the parts [p L, min(n, (p + 1) L)) tile [0, n): none is empty, the last ends at n
        assert L >= 1 and parts == -(-n // L) and (parts - 1) * L < n <= parts * L
        frames = np.zeros(n, dtype=np.int64)
        for p in range(parts):
            frames[p * L:min(n, (p + 1) * L)] += 1
        assert (frames == 1).all()
        # the tiles of 64 slots tile the frame's slots: the last may be partial, none is empty
        assert (q["n_tiles"] - 1) * 64 < slots <= q["n_tiles"] * 64
        # the waves take items wave, wave + n_waves, ...: every item has exactly one wave
        items = parts * q["n_tiles"]
        assert 1 <= q["n_waves"] <= min(res, items) and q["blocks"] == -(-q["n_waves"] // 4)
        if items <= 1 << 16:
            seen = np.zeros(items, dtype=np.int64)
            for wv in range(q["n_waves"]):
                seen[wv::q["n_waves"]] += 1
            assert (seen == 1).all()
        # parts only where the tiles leave wave slots empty, of 16 frames or more, their summaries within the cap
        assert parts == 1 or (q["n_tiles"] * 100 < res * 98 and L >= 16)
        assert parts * summary <= max(summary, sref.PARTS_BYTES)
        several += parts >= 2
    assert several >= 3 * len(RESIDENTS)


def test_times_geometry_of_the_part_seam_shape_does_not_depend_on_the_device(sched):
    """tests/test_gpu_mask_stats.py reads the cut of its 33 x 2 region over 600
    frames from the same harness: one tile, so 600 // 16 = 37 parts are asked
    for, which gives 36 parts of 17 frames for every realistic slot count."""
    px, _, _ = sref.kernel_constants(CSRC)
    for times, sums in ((True, True), (True, False), (False, True)):
        got = sref.times_geometry(sched, [(sref.frame_slots(33, 2, px), 600, sref.summary_bytes(33, 2, times, sums),
                                           sref.PARTS_BYTES, res) for res in RESIDENTS])
        assert {(q["parts"], q["part_frames"]) for q in got} == {(36, 17)}


def test_times_geometry_refusals_and_the_summary_cap(sched):
    got = sref.times_geometry(sched, [(16, 0, 24, 1 << 30, 4096), (16, 10, 24, 1 << 30, 0), (0, 10, 24, 1 << 30, 4096),
                                      (16, 10, 0, 1 << 30, 4096)])
    assert [q["ok"] for q in got] == [0, 0, 0, 0]
    # the summaries of a part outweigh the cap: one part, whatever the slots
    one = sref.times_geometry(sched, [(16, 600, 1 << 20, 1 << 19, 4096), (16, 600, 1 << 20, 0, 4096)])
    assert [(q["ok"], q["parts"], q["part_frames"]) for q in one] == [(1, 1, 600)] * 2
    # ... and three parts where three fit
    three = sref.times_geometry(sched, [(16, 600, 1 << 20, 3 << 20, 4096)])[0]
    assert (three["parts"], three["part_frames"]) == (3, 200)
    # the largest region: 2^30 - 1 rows of one word
    px, _, _ = sref.kernel_constants(CSRC)
    big = sref.times_geometry(sched, [(sref.frame_slots(1, 2 ** 30 - 1, px), 5, 24 * (2 ** 30 - 1), 1 << 30, 8192)])[0]
    assert big["ok"] == 1 and big["parts"] == 1 and big["n_waves"] == 8192


# (w, h, rows, cols, n) of the GPU test's grids and degenerate ones
COUNTS_SHAPES = [(1, 1, 1, 1, 1), (37, 5, 5, 37, 3), (100, 17, 3, 7, 7), (200, 17, 1, 2, 7), (200, 17, 4, 2, 2),
                 (257, 17, 17, 257, 2), (3840, 2160, 1, 1, 8), (3840, 2160, 1, 1, 500), (3840, 2160, 9, 16, 500),
                 (3840, 2160, 2160, 3840, 1), (5000, 3, 1, 5000, 2), (2049, 1, 1, 2049, 1), (64, 4000, 7, 1, 3)]
RESIDENT_BLOCKS = [1, 64, 2048, 4096]


def test_counts_geometry_covers_every_row_and_column_once(sched):
    _, chunk_cells, min_words = sref.kernel_constants(CSRC)
    rows_in = [(w, h, r, c, n, chunk_cells, min_words, res) for (w, h, r, c, n) in COUNTS_SHAPES
               for res in RESIDENT_BLOCKS]
    banded = 0
    for (w, h, rows, cols, n, _, _, res), q in zip(rows_in, sref.counts_geometry(sched, rows_in)):
        assert q["ok"] == 1
        chunks, bands, band_rows = q["col_chunks"], q["bands"], q["band_rows"]
        assert chunks == -(-cols // chunk_cells) and q["items"] == n * rows * chunks * bands
        assert 1 <= q["blocks"] <= min(q["items"], 2 * res)
        # every grid column lies in exactly one chunk
        col_seen = np.zeros(cols, dtype=np.int64)
        for k in range(chunks):
            col_seen[k * chunk_cells:min(cols, (k + 1) * chunk_cells)] += 1
        assert (col_seen == 1).all()
        # every mask row lies in exactly one band of exactly one grid row
        row_seen = np.zeros(h, dtype=np.int64)
        for r in range(rows):
            y_lo, y_hi = r * h // rows, (r + 1) * h // rows
            for b in range(bands):
                y0 = y_lo + b * band_rows
                row_seen[y0:max(y0, min(y_hi, y0 + band_rows))] += 1
        assert (row_seen == 1).all()
        # no band is cut thinner than the minimum unless the grid row is
        words = -(-((w + 31) // 32) // chunks)
        assert bands == 1 or band_rows * words >= min_words or band_rows == 1
        banded += bands >= 2
    assert banded >= 4
    bad = sref.counts_geometry(sched, [(0, 5, 1, 1, 1, chunk_cells, min_words, 64), (5, 5, 6, 1, 1, chunk_cells, min_words, 64),
                                       (5, 5, 1, 6, 1, chunk_cells, min_words, 64), (5, 5, 0, 1, 1, chunk_cells, min_words, 64),
                                       (5, 5, 1, 1, 0, chunk_cells, min_words, 64), (5, 5, 1, 1, 1, chunk_cells, min_words, 0)])
    assert [q["ok"] for q in bad] == [0] * 6


# -- the Python surface -------------------------------------------------------------------

def test_python_argument_checks_that_need_no_device():
    from dips_amd import ChangeMask
    from dips_amd.api import _mask_grid_args, _mask_host_args
    bits = cref.pack(bits_of(3, 5, 37, 0.5))
    got = _mask_host_args(ChangeMask(bits, 37))
    assert got[1:] == (37, 5, 3) and np.array_equal(got[0], bits)
    for bad in (bits, ChangeMask(bits, 0), ChangeMask(bits, 65), ChangeMask(bits[0], 37), ChangeMask(bits[:, :0], 37)):
        with pytest.raises(ValueError):
            _mask_host_args(bad)
    with pytest.raises(ValueError):  # 2^30 pixels
        _mask_host_args(ChangeMask(np.broadcast_to(np.zeros((1, 1, 4096), dtype=np.uint8), (0, 1 << 15, 4096)), 1 << 15))
    assert _mask_grid_args(1, 1, 37, 5, 3) == (1, 1) and _mask_grid_args(5, 37, 37, 5, 3) == (5, 37)
    for bad in ((0, 1), (1, 0), (6, 1), (1, 38), (-1, 1)):
        with pytest.raises(ValueError):
            _mask_grid_args(bad[0], bad[1], 37, 5, 3)
    with pytest.raises(ValueError):
        _mask_grid_args(1024, 1024, 1024, 1024, 1024)  # n * rows * cols = 2^30


def test_python_surface():
    import inspect

    import dips_amd
    op = dips_amd.DiffSeriesOperator
    params = lambda f: list(inspect.signature(f).parameters)[1:]  # noqa: E731
    assert params(op.mask_counts) == ["mask", "rows", "cols"]
    assert params(op.run_mask_counts_device) == ["mask", "width", "counts_out", "rows", "cols", "stream"]
    assert params(op.mask_times) == ["mask", "t0", "into"]
    assert params(op.mask_sums) == ["mask", "into"]
    assert params(op.run_mask_times_device) == ["mask", "width", "times_out", "sums_out", "t0", "accumulate", "stream"]
    assert params(op.change_activity) == ["frames", "roi", "ref", "rows", "cols", "morph", "background", "sigma_delta",
                                          "vote"]
    sig = inspect.signature(op.change_activity)
    assert [sig.parameters[k].default for k in ("rows", "cols", "morph", "vote")] == [1, 1, None, None]


def test_the_functions_are_exported_and_declared():
    import ctypes
    import re

    from dips_amd import _lib
    names = _lib.header_functions()
    assert "dips_mask_counts" in names and "dips_mask_pixel_times" in names
    with open(os.path.join(ROOT, "include", "dips_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"^#define DIPS_ABI_VERSION 3$", hdr, flags=re.M)  # no new struct: the version stays
    with open(os.path.join(ROOT, "rust", "dips-hip", "src", "ffi.rs")) as f:
        rs = f.read()
    assert "pub fn dips_mask_counts(" in rs and "pub fn dips_mask_pixel_times(" in rs
    lib = _lib.load()
    assert lib.dips_mask_counts.restype is ctypes.c_int and len(lib.dips_mask_counts.argtypes) == 8
    assert lib.dips_mask_pixel_times.restype is ctypes.c_int and len(lib.dips_mask_pixel_times.argtypes) == 9
