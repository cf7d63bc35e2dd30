"""dips_diff_pixel_sums on the GPU: every pixel's entry is exactly the sum over
the frames of the series the CPU oracle gives for the frames (and the
reference) cropped to that pixel (oracle_pixel_sums, tests/test_pixel_sums_cpu.py;
the 1280x720 case uses the vectorised py_pixel_sums that file proves equal).
Frames are independent random bytes unless stated (small-noise video has count
0 at tau = 8/255 and would hide a broken threshold path); every tau > 0 case on
random frames asserts that the threshold bites.  All comparisons are
np.array_equal.

Schedules (series_sched.h pix_geometry; 4 waves per SIMD x 4 SIMDs x the CUs
wave slots, far more than the tiles of any shape here): one part -- plain
stores, or load-add-store when accumulating -- for fewer than 32 frames (9
and 5 frames: every 37x29, 96x64x9 and 1280x720 case); frames in parts added
with u64 atomics from 32 frames on: 37x29x37 (2 parts), 8x8x300 and 37x29x300
(18 parts of 17 frames)."""
import functools

import numpy as np
import pytest

from oracle import oracle
from test_pixel_sums_cpu import oracle_pixel_sums, py_pixel_sums

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


@functools.lru_cache(maxsize=None)
def flicker_of(c, w, h, n):
    """Frames alternating all-0 and all-255: every pixel adds the per-frame
    maximum of every field on every differing frame."""
    a = np.zeros((n, h, w, c), dtype=np.uint8)
    a[1::2] = 255
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_of(c, w, h, n, roi, mode, tau_k, chroma=0, with_ref=False, flicker=False):
    frames = flicker_of(c, w, h, n) if flicker else frames_of(c, w, h, n)
    ref = ref_of(c, w, h) if with_ref else None
    a = oracle_pixel_sums(frames, mode, TAUS[tau_k], chroma, ref, roi)
    a.setflags(write=False)
    return a


def make_op(c, mode, tau, chroma=0, **kw):
    from dips_amd import ChromaFilter, DiffSeriesOperator, Mode
    return DiffSeriesOperator(_fmt(c), Mode(mode), tau, ChromaFilter(chroma), **kw)


def run_pix(c, frames, roi, mode, tau, chroma=0, ref=None, **kw):
    op = make_op(c, mode, tau, chroma, **kw)
    try:
        return op.pixel_sums(frames, roi=roi, ref=ref).as_array()
    finally:
        op.close()


def check_threshold_bites(got, c, w, h, n, roi, mode, tau_k, chroma=0, with_ref=False):
    """count is below the tau = 0 oracle count at some pixel, and not the same everywhere."""
    if tau_k:
        cnt = got[..., 2]
        cnt0 = want_of(c, w, h, n, roi, mode, 0, chroma, with_ref)[..., 2]
        assert (cnt < cnt0).any(), "the threshold removes nothing: its path is untested"
        assert cnt.min() < cnt.max()


# chroma: none for every tau, one channel at the two ends
CONFIGS = [(0, 0), (4, 0), (8, 0), (0, 1), (8, 2)]


@pytest.mark.parametrize("tau_k,chroma", CONFIGS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_formats_modes_taus(c, mode, tau_k, chroma):
    if c == 1 and chroma:
        chroma = 0  # GRAY8 has no channels to pick; the case still runs its tau
    w, h, n = 37, 29, 9
    got = run_pix(c, frames_of(c, w, h, n), None, mode, TAUS[tau_k], chroma)
    assert got.shape == (h, w, 4) and got.dtype == np.uint64
    check_threshold_bites(got, c, w, h, n, None, mode, tau_k, chroma)
    assert np.array_equal(got, want_of(c, w, h, n, None, mode, tau_k, chroma))


GEOMETRY = [
    (37, 29, None),             # the last vec of the frame is partial
    (37, 29, (3, 2, 21, 17)),   # x not a multiple of 4
    (37, 29, (1, 0, 3, 29)),    # narrower than a vec
    (40, 33, (20, 9, 20, 24)),  # ends at the frame's corner
    (37, 29, (10, 9, 26, 20)),  # ends one pixel short of the corner
    (96, 64, None),             # several tiles
    (8, 8, None),
]


@pytest.mark.parametrize("w,h,roi", GEOMETRY)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_geometry(c, mode, w, h, roi):
    n, tau_k = 5, 8
    got = run_pix(c, frames_of(c, w, h, n), roi, mode, TAUS[tau_k])
    assert got.shape == ((h, w, 4) if roi is None else (roi[3], roi[2], 4))
    check_threshold_bites(got, c, w, h, n, roi, mode, tau_k)
    assert np.array_equal(got, want_of(c, w, h, n, roi, mode, tau_k))


NARROW = [
    (1, 8, None),          # every vec is partial; rows 5, 6 and 7 would read past the frame's end
    (2, 8, None),          # rows 6 and 7
    (2, 8, (1, 0, 1, 8)),  # a one-pixel column at x = 1: rows 6 and 7
    (2, 8, (0, 0, 1, 8)),  # at x = 0: row 7 only
    (1, 3, None),          # every row
]


@pytest.mark.parametrize("n", [9, 37])
@pytest.mark.parametrize("w,h,roi", NARROW)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_narrow_frames(c, mode, w, h, roi, n):
    """Frames narrower than 3 pixels: partial vecs of several rows would read
    past the frame's end; the fast kernel leaves each of them out and the
    generic kernel adds it.  9 frames run one part (plain stores into a map
    pre-filled with -1 on the device path), 37 frames two parts (atomics)."""
    import torch
    tau_k = 8
    frames = frames_of(c, w, h, n)
    got = run_pix(c, frames, roi, mode, TAUS[tau_k])
    check_threshold_bites(got, c, w, h, n, roi, mode, tau_k)
    want = want_of(c, w, h, n, roi, mode, tau_k)
    assert np.array_equal(got, want)
    out = torch.full(want.shape, -1, dtype=torch.int64, device="cuda")
    op = make_op(c, mode, TAUS[tau_k])
    try:
        op.run_pixel_sums_device(torch.from_numpy(frames.copy()).cuda(), out, roi=roi)
        torch.cuda.synchronize()
    finally:
        op.close()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)


@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 5, 9, 37])
@pytest.mark.parametrize("c", [3, 4])
def test_frame_counts_and_reference(c, n, mode, with_ref):
    """Ring (4 frames per turn), tail (1-3) and, at 37 frames, two frame
    parts added with atomics; an explicit reference in both modes and none.
    With one frame and no reference the frame meets itself and every entry is
    zero: there is no threshold to see, so that case skips the bite check."""
    w, h, tau_k = 37, 29, 4
    got = run_pix(c, frames_of(c, w, h, n), None, mode, TAUS[tau_k], ref=ref_of(c, w, h) if with_ref else None)
    if n > 1 or with_ref:
        check_threshold_bites(got, c, w, h, n, None, mode, tau_k, 0, with_ref)
    else:
        assert not got.any()
    assert np.array_equal(got, want_of(c, w, h, n, None, mode, tau_k, 0, with_ref))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_few_tiles_many_frames(c, mode):
    """8x8 x 300 frames: one tile, so the frames are cut into 18 parts of 17
    (the frames-in-parts schedule: a memset launch, then u64 atomic adds)."""
    w, h, n, tau_k = 8, 8, 300, 8
    got = run_pix(c, frames_of(c, w, h, n), None, mode, TAUS[tau_k])
    check_threshold_bites(got, c, w, h, n, None, mode, tau_k)
    assert np.array_equal(got, want_of(c, w, h, n, None, mode, tau_k))


@pytest.mark.parametrize("tau_k", [0, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_saturating_clip(c, mode, tau_k):
    """37x29 x 300 frames alternating all-0 and all-255: SAD 765 / 1020, SJ
    510 and SI 2^32 per pixel on every differing frame (every frame but the
    first per-frame, every second one overall)."""
    w, h, n = 37, 29, 300
    want = want_of(c, w, h, n, None, mode, tau_k, flicker=True)
    differing = n - 1 if mode == 1 else n // 2
    assert np.array_equal(want[0, 0], np.array([255 * c * differing, 510 * differing, differing, differing << 32],
                                               dtype=np.uint64))
    got = run_pix(c, flicker_of(c, w, h, n), None, mode, TAUS[tau_k])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("tau_k", [0, 8])
@pytest.mark.parametrize("c", [3, 4])
def test_saturating_clip_at_the_part_cap(c, tau_k, monkeypatch):
    """The in-register accumulators at their stated limit: parts of 2048
    frames (DIPS_PIXEL_PART_FRAMES; the geometry would cut this small frame
    into parts of 17), every pixel at the per-frame maximum of every field:
    SJ 510 * 2048 in 20 bits beside a count of 2048 in 12.  2050 frames: one
    full part and a part of 2."""
    monkeypatch.setenv("DIPS_PIXEL_PART_FRAMES", "2048")
    w, h, n = 13, 5, 2050
    want = want_of(c, w, h, n, None, 1, tau_k, flicker=True)
    assert want[0, 0, 1] == 510 * (n - 1) and want[0, 0, 3] == (n - 1) << 32
    got = run_pix(c, flicker_of(c, w, h, n), None, 1, TAUS[tau_k])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("k", [1, 4, 5])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_accumulate_in_chunks(c, mode, k, device):
    """pixel_sums(frames[:k]) then pixel_sums(frames[k:], ref, into) equals
    pixel_sums(frames); an accumulating call without frames changes nothing,
    an overwriting one without frames leaves zeros."""
    from dips_amd import PixelSums
    w, h, n, tau_k = 37, 29, 9, 8
    frames = frames_of(c, w, h, n)
    ref2 = frames[k - 1] if mode == 1 else frames[0]
    want = want_of(c, w, h, n, None, mode, tau_k)
    op = make_op(c, mode, TAUS[tau_k])
    try:
        if device:
            import torch
            dev = torch.from_numpy(frames.copy()).cuda()
            out = torch.full((h, w, 4), -1, dtype=torch.int64, device="cuda")
            op.run_pixel_sums_device(dev[:k], out)
            op.run_pixel_sums_device(dev[k:], out, ref=torch.from_numpy(ref2.copy()).cuda(), accumulate=True)
            op.run_pixel_sums_device(dev[:0], out, accumulate=True)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint64)
            out.fill_(-1)
            op.run_pixel_sums_device(dev[:0], out)
            torch.cuda.synchronize()
            empty = out.cpu().numpy().view(np.uint64)
        else:
            first = op.pixel_sums(frames[:k])
            both = op.pixel_sums(frames[k:], ref=ref2, into=first)
            got = op.pixel_sums(frames[:0], into=both).as_array()
            assert np.array_equal(first.as_array(), oracle_pixel_sums(frames[:k], mode, TAUS[tau_k]))
            empty = op.pixel_sums(frames[:0]).as_array()
            assert isinstance(both, PixelSums)
    finally:
        op.close()
    check_threshold_bites(got, c, w, h, n, None, mode, tau_k)
    assert np.array_equal(got, want)
    assert empty.shape == (h, w, 4) and not empty.any()


def test_accumulate_onto_the_parts_schedule():
    """37 frames run in two parts with atomics; accumulating them onto an
    earlier map adds to it without the zeroing launch."""
    c, w, h, n, mode, tau_k = 3, 37, 29, 37, 1, 8
    frames = frames_of(c, w, h, n)
    op = make_op(c, mode, TAUS[tau_k])
    try:
        first = op.pixel_sums(frames)
        twice = op.pixel_sums(frames, ref=frames[0], into=first).as_array()
    finally:
        op.close()
    check_threshold_bites(twice // 2, c, w, h, n, None, mode, tau_k)
    assert np.array_equal(twice, 2 * want_of(c, w, h, n, None, mode, tau_k))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_sums_equal_the_series_and_the_one_cell_grid(c, mode):
    w, h, n, roi = 37, 29, 9, (3, 2, 21, 17)
    frames = frames_of(c, w, h, n)
    op = make_op(c, mode, 8 / 255)
    try:
        whole = op(frames)[0].as_array().sum(axis=0, dtype=np.uint64)
        pix = op.pixel_sums(frames).as_array()
        cell = op.grid(frames, 1, 1, roi=roi).as_array().sum(axis=0, dtype=np.uint64)[0, 0]
        pix_roi = op.pixel_sums(frames, roi=roi).as_array()
    finally:
        op.close()
    check_threshold_bites(pix, c, w, h, n, None, mode, 8)
    check_threshold_bites(pix_roi, c, w, h, n, roi, mode, 8)
    assert np.array_equal(pix.sum(axis=(0, 1), dtype=np.uint64), whole)
    assert np.array_equal(pix_roi.sum(axis=(0, 1), dtype=np.uint64), cell)
    assert np.array_equal(pix_roi, pix[2:19, 3:24])


@pytest.mark.parametrize("tau_k", [0, 4, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_fast_generic_and_crosscheck_paths_agree(c, mode, tau_k):
    w, h, n, roi = 96, 64, 9, (5, 3, 90, 61)
    frames = frames_of(c, w, h, n)
    fast = run_pix(c, frames, roi, mode, TAUS[tau_k])
    generic = run_pix(c, frames, roi, mode, TAUS[tau_k], force_generic=True)
    cross = run_pix(c, frames, roi, mode, TAUS[tau_k], crosscheck=True)
    check_threshold_bites(fast, c, w, h, n, roi, mode, tau_k)
    assert np.array_equal(fast, generic)
    assert np.array_equal(fast, cross)
    assert np.array_equal(fast, want_of(c, w, h, n, roi, mode, tau_k))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_device_path_equals_host_path(c, mode):
    import torch
    w, h, n, roi = 37, 29, 9, (3, 2, 21, 17)
    frames, ref = frames_of(c, w, h, n), ref_of(c, w, h)
    op = make_op(c, mode, 8 / 255)
    try:
        host = op.pixel_sums(frames, roi=roi, ref=ref).as_array()
        out = torch.full((roi[3], roi[2], 4), -1, dtype=torch.int64, device="cuda")
        op.run_pixel_sums_device(torch.from_numpy(frames.copy()).cuda(), out, roi=roi,
                                 ref=torch.from_numpy(ref.copy()).cuda())
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            op.run_pixel_sums_device(torch.from_numpy(frames.copy()).cuda(), out)  # the whole frame's shape is asked
    finally:
        op.close()
    check_threshold_bites(host, c, w, h, n, roi, mode, 8, 0, True)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), host)
    assert np.array_equal(host, want_of(c, w, h, n, roi, mode, 8, 0, True))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_unaligned_device_base(c, mode):
    """Frames taken from a tensor offset by 1 byte: every RGB8 / RGBA8 vec
    load is off its natural alignment; the output starts as -1."""
    import torch
    w, h, n = 37, 29, 9
    frames = frames_of(c, w, h, n)
    buf = torch.zeros(frames.nbytes + 16, dtype=torch.uint8, device="cuda")
    dev = buf[1:1 + frames.nbytes].view(frames.shape)
    dev.copy_(torch.from_numpy(frames.copy()))
    assert dev.data_ptr() % 4 == 1
    out = torch.full((h, w, 4), -1, dtype=torch.int64, device="cuda")
    op = make_op(c, mode, 8 / 255)
    try:
        op.run_pixel_sums_device(dev, out)
        torch.cuda.synchronize()
    finally:
        op.close()
    got = out.cpu().numpy().view(np.uint64)
    check_threshold_bites(got, c, w, h, n, None, mode, 8)
    assert np.array_equal(got, want_of(c, w, h, n, None, mode, 8))


def test_errors_leave_the_operator_usable():
    import torch
    from dips_amd import DipsError
    frames = frames_of(3, 37, 29, 5)
    op = make_op(3, 1, 8 / 255)
    try:
        for roi in ((30, 0, 8, 5), (0, 25, 8, 5), (3, 2, 0, 17), (3, 2, 21, 0)):
            with pytest.raises(DipsError) as e:
                op.pixel_sums(frames, roi=roi)
            assert e.value.status == -1 and "diff_pixel_sums:" in str(e.value)
        dev = torch.from_numpy(frames.copy()).cuda()
        for shape in ((29, 37), (29, 37, 3), (28, 37, 4)):
            with pytest.raises(ValueError):
                op.run_pixel_sums_device(dev, torch.zeros(shape, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError):
            op.run_pixel_sums_device(dev, torch.zeros((29, 37, 4), dtype=torch.int32, device="cuda"))
        got = op.pixel_sums(frames).as_array()
    finally:
        op.close()
    check_threshold_bites(got, 3, 37, 29, 5, None, 1, 8)
    assert np.array_equal(got, want_of(3, 37, 29, 5, None, 1, 8))


def test_kernel_time_records_the_launch():
    import torch
    frames = torch.from_numpy(frames_of(3, 96, 64, 5).copy()).cuda()
    out = torch.zeros((64, 96, 4), dtype=torch.int64, device="cuda")
    op = make_op(3, 1, 8 / 255, time_kernel=True)
    try:
        op.run_pixel_sums_device(frames, out)
        op.run_pixel_sums_device(frames, out)
        ms, launches = op.kernel_time()
    finally:
        op.close()
    assert launches == 2 and ms > 0.0


def test_hd_activity_map():
    """1280x720 RGB8, 5 frames, per-frame, tau = 8/255, against py_pixel_sums
    (7,200 tiles: more than the wave slots, several items per wave)."""
    c, w, h, n = 3, 1280, 720, 5
    frames = frames_of(c, w, h, n)
    want = py_pixel_sums(frames, 1, 8 / 255)
    got = run_pix(c, frames, None, 1, 8 / 255)
    cnt0 = py_pixel_sums(frames, 1, 0.0)[..., 2]
    assert (got[..., 2] < cnt0).any() and got[..., 2].min() < got[..., 2].max()
    assert np.array_equal(got, want)
    assert np.array_equal(got.sum(axis=(0, 1), dtype=np.uint64),
                          oracle.series(frames, mode=1, tau=8 / 255)[0].sum(axis=0, dtype=np.uint64))
