"""dips_diff_series_grid on the GPU: every cell of the grid is exactly the
series the CPU oracle gives for the frames (and the reference) cropped to
that cell.  The cell rectangles come from the pure-Python restatement of the
split in tests/test_grid_cpu.py, not from the library.  Frames are
independent random bytes (small-noise video has count 0 at tau = 8/255 and
would hide a broken threshold path); every tau > 0 case asserts that some
cell has 0 < count < w * h.  All comparisons are np.array_equal."""
import functools

import numpy as np
import pytest

from oracle import oracle
from test_grid_cpu import py_cell

pytestmark = pytest.mark.gpu

TAUS = {0: 0.0, 4: 4 / 255, 8: 8 / 255}  # f64 sum, f64 sum with a threshold, integer sum (8/255 >= 2^-5)


def _fmt(c):
    from dips_amd import PixelFormat
    return {1: PixelFormat.Gray8, 3: PixelFormat.RGB8, 4: PixelFormat.RGBA8}[c]


@functools.lru_cache(maxsize=None)
def frames_of(c, w, h, n, seed=0):
    shape = (n, h, w) if c == 1 else (n, h, w, c)
    a = np.random.default_rng([seed, c, w, h, n]).integers(0, 256, shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ref_of(c, w, h):
    shape = (h, w) if c == 1 else (h, w, c)
    a = np.random.default_rng([77, c, w, h]).integers(0, 256, shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


def oracle_grid(frames, rows, cols, roi, mode, tau, chroma=0, ref=None):
    """want[t, r, c] = the oracle's series of the crop to cell (r, c)."""
    n, h, w = frames.shape[:3]
    want = np.zeros((n, rows, cols, 4), dtype=np.uint64)
    area = np.zeros((rows, cols), dtype=np.uint64)
    for r in range(rows):
        for c in range(cols):
            x, y, cw, ch = py_cell(w, h, rows, cols, r, c, roi)
            crop_ref = None if ref is None else np.ascontiguousarray(ref[y:y + ch, x:x + cw])
            want[:, r, c] = oracle.series(np.ascontiguousarray(frames[:, y:y + ch, x:x + cw]), mode=mode, tau=tau,
                                          chroma=chroma, ref=crop_ref)[0]
            area[r, c] = cw * ch
    return want, area


@functools.lru_cache(maxsize=None)
def want_of(c, w, h, n, rows, cols, roi, mode, tau_k, chroma=0, with_ref=False):
    ref = ref_of(c, w, h) if with_ref else None
    return oracle_grid(frames_of(c, w, h, n), rows, cols, roi, mode, TAUS[tau_k], chroma, ref)


def run_grid(c, frames, rows, cols, roi, mode, tau, chroma=0, ref=None, **kw):
    from dips_amd import ChromaFilter, DiffSeriesOperator, Mode
    op = DiffSeriesOperator(_fmt(c), Mode(mode), tau, ChromaFilter(chroma), **kw)
    try:
        return op.grid(frames, rows, cols, roi=roi, ref=ref).as_array()
    finally:
        op.close()


def check_threshold_bites(got, area, tau_k):
    if tau_k:
        cnt = got[..., 2]
        assert ((cnt > 0) & (cnt < area[None])).any(), "no cell has 0 < count < w*h: the threshold path is untested"


# chroma: none for every tau, one channel at the two ends
CONFIGS = [(0, 0), (4, 0), (8, 0), (0, 1), (8, 2)]


@pytest.mark.parametrize("tau_k,chroma", CONFIGS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_formats_modes_taus(c, mode, tau_k, chroma):
    """37x29 on a 4x3 grid: odd row pitch for RGB8, cell widths 12/12/13."""
    if c == 1 and chroma:
        chroma = 0  # GRAY8 has no channels to pick; the case still runs its tau
    w, h, n, rows, cols = 37, 29, 9, 4, 3
    want, area = want_of(c, w, h, n, rows, cols, None, mode, tau_k, chroma)
    got = run_grid(c, frames_of(c, w, h, n), rows, cols, None, mode, TAUS[tau_k], chroma)
    assert got.shape == (n, rows, cols, 4)
    check_threshold_bites(got, area, tau_k)
    assert np.array_equal(got, want)


GEOMETRY = [
    (37, 29, 4, 3, None),           # widths 12/12/13, the last vec of the frame is partial
    (8, 8, 8, 8, None),             # 1-pixel cells
    (23, 5, 2, 23, None),           # cols = width
    (37, 29, 2, 5, (3, 2, 21, 17)),  # x not a multiple of 4, widths 4/4/4/4/5
    (37, 29, 1, 1, (1, 0, 3, 29)),  # narrower than a vec
    (96, 64, 1, 2, None),           # 3072-pixel cells: several tiles per cell
    (40, 33, 3, 2, (20, 9, 20, 24)),  # a region ending at the frame's corner, widths of 10 (two px in the last vec)
    (37, 29, 2, 3, (10, 9, 26, 20)),  # a region ending one pixel short of the corner: widths 8/9/9
]


@pytest.mark.parametrize("w,h,rows,cols,roi", GEOMETRY)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_geometry(c, mode, w, h, rows, cols, roi):
    n, tau_k = 5, 8
    want, area = want_of(c, w, h, n, rows, cols, roi, mode, tau_k)
    got = run_grid(c, frames_of(c, w, h, n), rows, cols, roi, mode, TAUS[tau_k])
    if min(area.flat) > 16:
        check_threshold_bites(got, area, tau_k)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_one_cell_equals_diff_series(c, mode):
    from dips_amd import DiffSeriesOperator, Mode
    frames = frames_of(c, 37, 29, 9)
    op = DiffSeriesOperator(_fmt(c), Mode(mode), 8 / 255)
    try:
        whole = op(frames)[0].as_array()
        got = op.grid(frames, 1, 1)
    finally:
        op.close()
    assert got.sad.shape == (9, 1, 1) and got.si.shape == (9, 1, 1)
    assert np.array_equal(got.as_array()[:, 0, 0], whole)
    assert np.array_equal(whole, oracle.series(frames, mode=mode, tau=8 / 255)[0])


@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 5, 9, 37])
@pytest.mark.parametrize("c", [3, 4])
def test_frame_counts_and_reference(c, n, mode, with_ref):
    """Ring (4 frames per turn), tail (1-3) and, at 37 frames, two frame
    parts; an explicit reference in both modes and none."""
    w, h, rows, cols, tau_k = 37, 29, 4, 3, 4
    want, area = want_of(c, w, h, n, rows, cols, None, mode, tau_k, 0, with_ref)
    got = run_grid(c, frames_of(c, w, h, n), rows, cols, None, mode, TAUS[tau_k],
                   ref=ref_of(c, w, h) if with_ref else None)
    if n > 1 or with_ref:
        check_threshold_bites(got, area, tau_k)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_device_path_equals_host_path(c, mode):
    import torch
    from dips_amd import DiffSeriesOperator, Mode
    w, h, n, rows, cols, roi = 37, 29, 9, 2, 5, (3, 2, 21, 17)
    frames, ref = frames_of(c, w, h, n), ref_of(c, w, h)
    op = DiffSeriesOperator(_fmt(c), Mode(mode), 8 / 255)
    try:
        host = op.grid(frames, rows, cols, roi=roi, ref=ref).as_array()
        out = torch.full((n, rows, cols, 4), -1, dtype=torch.int64, device="cuda")
        op.run_grid_device(torch.from_numpy(frames.copy()).cuda(), out, rows, cols, roi=roi,
                           ref=torch.from_numpy(ref.copy()).cuda())
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            op.run_grid_device(torch.from_numpy(frames.copy()).cuda(), out, rows + 1, cols)
    finally:
        op.close()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), host)
    assert np.array_equal(host, want_of(c, w, h, n, rows, cols, roi, mode, 8, 0, True)[0])


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_unaligned_device_base(c, mode):
    """Frames taken from a tensor offset by 1 byte: every RGB8 / RGBA8 vec
    load is off its natural alignment."""
    import torch
    from dips_amd import DiffSeriesOperator, Mode
    w, h, n, rows, cols = 37, 29, 9, 4, 3
    frames = frames_of(c, w, h, n)
    buf = torch.zeros(frames.nbytes + 16, dtype=torch.uint8, device="cuda")
    dev = buf[1:1 + frames.nbytes].view(frames.shape)
    dev.copy_(torch.from_numpy(frames.copy()))
    assert dev.data_ptr() % 4 == 1
    out = torch.zeros((n, rows, cols, 4), dtype=torch.int64, device="cuda")
    op = DiffSeriesOperator(_fmt(c), Mode(mode), 8 / 255)
    try:
        op.run_grid_device(dev, out, rows, cols)
        torch.cuda.synchronize()
    finally:
        op.close()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want_of(c, w, h, n, rows, cols, None, mode, 8)[0])


@pytest.mark.parametrize("tau_k", [0, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_cells_sum_to_the_whole_frame_series(c, mode, tau_k):
    from dips_amd import DiffSeriesOperator, Mode
    frames = frames_of(c, 96, 64, 5)
    op = DiffSeriesOperator(_fmt(c), Mode(mode), TAUS[tau_k])
    try:
        whole = op(frames)[0].as_array()
        cells = op.grid(frames, 5, 7).as_array()
    finally:
        op.close()
    assert np.array_equal(cells.sum(axis=(1, 2)), whole)


@pytest.mark.parametrize("tau_k", [0, 4, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_fast_generic_and_crosscheck_paths_agree(c, mode, tau_k):
    w, h, n, rows, cols, roi = 96, 64, 9, 3, 4, (5, 3, 90, 61)
    frames = frames_of(c, w, h, n)
    fast = run_grid(c, frames, rows, cols, roi, mode, TAUS[tau_k])
    generic = run_grid(c, frames, rows, cols, roi, mode, TAUS[tau_k], force_generic=True)
    cross = run_grid(c, frames, rows, cols, roi, mode, TAUS[tau_k], crosscheck=True)
    assert np.array_equal(fast, generic)
    assert np.array_equal(fast, cross)
    assert np.array_equal(fast, want_of(c, w, h, n, rows, cols, roi, mode, tau_k)[0])


def test_errors_leave_the_operator_usable():
    from dips_amd import DiffSeriesOperator, DipsError, Mode, PixelFormat
    frames = frames_of(3, 37, 29, 5)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    try:
        for kw in (dict(rows=30, cols=1), dict(rows=1, cols=0), dict(rows=1, cols=1, roi=(30, 0, 8, 5)),
                   dict(rows=18, cols=1, roi=(3, 2, 21, 17))):
            with pytest.raises(DipsError) as e:
                op.grid(frames, **kw)
            assert e.value.status == -1 and "diff_series_grid:" in str(e.value)
        empty = op.grid(frames[:0], 4, 3)
        assert empty.sad.shape == (0, 4, 3)
        got = op.grid(frames, 4, 3).as_array()
    finally:
        op.close()
    assert np.array_equal(got, want_of(3, 37, 29, 5, 4, 3, None, 1, 8)[0])


def test_kernel_time_records_the_grid_launch():
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    frames = torch.from_numpy(frames_of(3, 96, 64, 5).copy()).cuda()
    out = torch.zeros((5, 2, 2, 4), dtype=torch.int64, device="cuda")
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255, time_kernel=True)
    try:
        op.run_grid_device(frames, out, 2, 2)
        op.run_grid_device(frames, out, 2, 2)
        ms, launches = op.kernel_time()
    finally:
        op.close()
    assert launches == 2 and ms > 0.0


def test_full_hd_heat_map():
    """1920x1080 RGB8, 16x9 cells of 120x120, 12 frames, per-frame, tau =
    8/255: every cell against the oracle."""
    c, w, h, n, rows, cols = 3, 1920, 1080, 12, 9, 16
    frames = frames_of(c, w, h, n)
    want, area = oracle_grid(frames, rows, cols, None, 1, 8 / 255)
    got = run_grid(c, frames, rows, cols, None, 1, 8 / 255)
    check_threshold_bites(got, area, 8)
    assert np.array_equal(got, want)
