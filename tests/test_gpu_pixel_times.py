"""dips_diff_pixel_times on the GPU: the four planes are, bit for bit, the fold
of the bits the CPU oracle gives for the frames (and the reference) cropped to
each pixel (oracle_pixel_times, tests/test_pixel_times_cpu.py; the 1920x1080
case uses the vectorised py_pixel_times that file proves equal).  Frames are
event_frames: a pixel equals its base value outside a window of its own and
carries noise in [-40, 40] inside, so first, last and the runs differ from
pixel to pixel; every case asserts check_informative on the oracle's planes
and the part cases that at least 10 % of the pixels have a run that crosses a
part boundary.  Every comparison is np.array_equal on all four planes.

Schedule (series_sched.h times_geometry): a tile is 64 * kUnrollTimes vecs of
the region; tiles that fill less than 98 % of the wave slots are cut into
parts of >= 16 frames (one part below 32 frames, parts of 19 and 18 at 37
frames, of 17 at 300 frames); DIPS_PIXEL_PART_FRAMES pins the part length.
Parts write summaries that times_combine_kernel folds in order."""
import functools

import numpy as np
import pytest

from test_change_mask_cpu import TAUS, py_change_mask, unpack_mask
from test_gpu_change_mask import CONFIGS, GEOMETRY
from test_pixel_times_cpu import (NONE, check_informative, crossing_share, event_frames, event_ref, fold_times,
                                  initial_state, oracle_pixel_times, py_pixel_times)

pytestmark = pytest.mark.gpu


def _fmt(c):
    from dips_amd import PixelFormat
    return {1: PixelFormat.Gray8, 3: PixelFormat.RGB8, 4: PixelFormat.RGBA8}[c]


@functools.lru_cache(maxsize=None)
def want_of(c, w, h, n, roi, mode, tau_k, chroma=0, with_ref=False, t0=0):
    ref = event_ref(c, w, h) if with_ref else None
    a = oracle_pixel_times(event_frames(c, w, h, n), mode, TAUS[tau_k], chroma, ref, roi, t0)
    a.setflags(write=False)
    return a


def checked_want(c, w, h, n, roi, mode, tau_k, chroma=0, with_ref=False, t0=0):
    want = want_of(c, w, h, n, roi, mode, tau_k, chroma, with_ref, t0)
    if n > 1 or with_ref:
        check_informative(want, n)
    return want


def make_op(c, mode, tau, chroma=0, **kw):
    from dips_amd import ChromaFilter, DiffSeriesOperator, Mode
    return DiffSeriesOperator(_fmt(c), Mode(mode), tau, ChromaFilter(chroma), **kw)


def run_times(c, frames, roi, mode, tau, chroma=0, ref=None, t0=0, **kw):
    op = make_op(c, mode, tau, chroma, **kw)
    try:
        t = op.pixel_times(frames, roi=roi, ref=ref, t0=t0)
    finally:
        op.close()
    for plane in (t.first, t.last, t.run_max, t.run_cur):
        assert plane.dtype == np.uint32
    return t.as_array()


@pytest.mark.parametrize("tau_k,chroma", CONFIGS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_formats_modes_taus(c, mode, tau_k, chroma):
    """c = 1 runs the generic kernel."""
    if c == 1 and chroma:
        chroma = 0  # GRAY8 has no channels to pick; the case still runs its tau
    w, h, n = 37, 29, 9
    got = run_times(c, event_frames(c, w, h, n), None, mode, TAUS[tau_k], chroma)
    assert got.shape == (4, h, w)
    assert np.array_equal(got, checked_want(c, w, h, n, None, mode, tau_k, chroma))


@pytest.mark.parametrize("w,h,roi", GEOMETRY)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_geometry(c, mode, w, h, roi):
    n, tau_k = 5, 8
    got = run_times(c, event_frames(c, w, h, n), roi, mode, TAUS[tau_k])
    rw, rh = (w, h) if roi is None else roi[2:]
    assert got.shape == (4, rh, rw)
    assert np.array_equal(got, checked_want(c, w, h, n, roi, mode, tau_k))


@pytest.mark.parametrize("w,h", [(1, 8), (2, 8), (1, 3)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_narrow_frames(c, mode, w, h):
    """Frames narrower than 3 pixels: the partial vecs of several rows would
    read past the frame's end; the generic kernel writes their pixels."""
    n, tau_k = 9, 4
    want = checked_want(c, w, h, n, None, mode, tau_k)
    assert np.array_equal(run_times(c, event_frames(c, w, h, n), None, mode, TAUS[tau_k]), want)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_ring_prologue_and_tail(c, mode, n):
    w, h, tau_k = 37, 29, 4
    got = run_times(c, event_frames(c, w, h, n), None, mode, TAUS[tau_k])
    if n == 1:
        assert np.array_equal(got, initial_state(h, w))  # frame 0 meets itself
    assert np.array_equal(got, checked_want(c, w, h, n, None, mode, tau_k))


PARTS = [(8, 8, 300, 17), (8, 8, 300, 19), (37, 29, 37, 17), (37, 29, 37, 19), (37, 29, 24, 17)]


def _bits(c, w, h, n, mode, tau_k):
    return unpack_mask(py_change_mask(event_frames(c, w, h, n), mode, TAUS[tau_k]), w)


@pytest.mark.parametrize("w,h,n,plen", PARTS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_frame_parts(c, mode, w, h, n, plen, monkeypatch):
    """Parts of `plen` frames: runs that cross a part boundary are counted
    whole, and in per-frame mode a part's first reference is the frame before
    it."""
    tau_k = 8
    want = checked_want(c, w, h, n, None, mode, tau_k)
    assert crossing_share(_bits(c, w, h, n, mode, tau_k), plen) >= 0.10
    monkeypatch.setenv("DIPS_PIXEL_PART_FRAMES", str(plen))
    got = run_times(c, event_frames(c, w, h, n), None, mode, TAUS[tau_k])
    for k, name in enumerate(("first", "last", "run_max", "run_cur")):
        assert np.array_equal(got[k], want[k]), name


@pytest.mark.parametrize("w,h,n", [(8, 8, 300), (37, 29, 37), (37, 29, 24)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_default_geometry_equals_pinned_parts(c, mode, w, h, n, monkeypatch):
    """The same clips with the hook unset (the geometry's own parts), with one
    part and with parts of 17: the result does not depend on the part count."""
    tau_k = 8
    frames = event_frames(c, w, h, n)
    monkeypatch.delenv("DIPS_PIXEL_PART_FRAMES", raising=False)
    default = run_times(c, frames, None, mode, TAUS[tau_k])
    monkeypatch.setenv("DIPS_PIXEL_PART_FRAMES", str(n))
    one = run_times(c, frames, None, mode, TAUS[tau_k])
    monkeypatch.setenv("DIPS_PIXEL_PART_FRAMES", "17")
    pinned = run_times(c, frames, None, mode, TAUS[tau_k])
    want = checked_want(c, w, h, n, None, mode, tau_k)
    assert np.array_equal(default, want)
    assert np.array_equal(one, want)
    assert np.array_equal(pinned, want)


@pytest.mark.parametrize("plen", [17, 300])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_saturated_and_constant_clips(c, mode, plen, monkeypatch):
    """Every bit 1 from frame 0 on: overall against an all-zero reference with
    all-255 frames, per-frame with alternating 255 / 0 frames after a zero
    reference.  Constant frames: nothing ever changes."""
    monkeypatch.setenv("DIPS_PIXEL_PART_FRAMES", str(plen))
    w, h, n, t0 = 8, 8, 300, 1000
    shape = (n, h, w, c)
    frames = np.full(shape, 255, dtype=np.uint8)
    if mode == 1:
        frames[1::2] = 0
    ref = np.zeros(shape[1:], dtype=np.uint8)
    got = run_times(c, frames, None, mode, 8 / 255, ref=ref, t0=t0)
    assert (got[0] == t0).all() and (got[1] == t0 + n - 1).all()
    assert (got[2] == n).all() and (got[3] == n).all()
    const = np.full(shape, 77, dtype=np.uint8)
    assert np.array_equal(run_times(c, const, None, mode, 8 / 255, t0=t0), initial_state(h, w))


@pytest.mark.parametrize("c", [1, 3, 4])
def test_t0_and_the_index_limit(c):
    from dips_amd import DipsError
    w, h, n, mode, tau_k = 37, 29, 9, 1, 8
    frames = event_frames(c, w, h, n)
    t0 = 0xFFFFFFFF - n
    want = checked_want(c, w, h, n, None, mode, tau_k, t0=t0)
    assert want[1][want[1] != NONE].max() == 0xFFFFFFFE
    op = make_op(c, mode, TAUS[tau_k])
    try:
        got = op.pixel_times(frames, t0=t0).as_array()
        lib, hp = op._host._lib, op._host.ptr
        buf = np.full((4, h, w), 0xA5A5A5A5, dtype=np.uint32)
        for acc in (0, 1):
            st = lib.dips_diff_pixel_times(hp, w, h, frames.ctypes.data, n, None, None, t0 + 1, acc, buf.ctypes.data)
            assert st == -1
        assert (buf == 0xA5A5A5A5).all()
        with pytest.raises(DipsError) as e:
            op.pixel_times(frames, t0=t0 + 1)
        assert e.value.status == -1 and "t0 + n_frames" in str(e.value)
        again = op.pixel_times(frames, t0=t0).as_array()
    finally:
        op.close()
    assert np.array_equal(got, want) and np.array_equal(again, want)


@pytest.mark.parametrize("k", [1, 4, 5])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_clip_in_two_chunks_host(c, mode, k):
    """pixel_times(frames[:k]) then pixel_times(frames[k:], into=...) with t0
    = k -- ref the previous chunk's last frame in per-frame mode, the same
    reference in overall mode -- is the clip in one call; a run that spans the
    cut is counted whole."""
    w, h, n, tau_k, t0 = 37, 29, 9, 8, 50
    frames = event_frames(c, w, h, n)
    bits = unpack_mask(py_change_mask(frames, mode, TAUS[tau_k]), w)
    if k > 1:  # frame 0 meets itself: no run can span a cut at 1
        assert (bits[k - 1] & bits[k]).mean() > 0.02  # runs that span the cut
    op = make_op(c, mode, TAUS[tau_k])
    try:
        a = op.pixel_times(frames[:k], t0=t0)
        b = op.pixel_times(frames[k:], ref=frames[k - 1] if mode == 1 else frames[0], t0=t0 + k, into=a)
        whole = op.pixel_times(frames, t0=t0)
    finally:
        op.close()
    want = checked_want(c, w, h, n, None, mode, tau_k, t0=t0)
    assert np.array_equal(a.as_array(), fold_times(bits[:k], t0))
    assert np.array_equal(whole.as_array(), want)
    assert np.array_equal(b.as_array(), want)


@pytest.mark.parametrize("plen", [0, 17])
@pytest.mark.parametrize("k", [1, 4, 5])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_clip_in_two_chunks_device(c, mode, k, plen, monkeypatch):
    """The same on device pointers with an roi at an odd x; plen = 17: the
    second chunk (37 - k frames) runs in parts and the combine folds them onto
    the accumulated state."""
    import torch
    if plen:
        monkeypatch.setenv("DIPS_PIXEL_PART_FRAMES", str(plen))
    else:
        monkeypatch.delenv("DIPS_PIXEL_PART_FRAMES", raising=False)
    w, h, n, tau_k, roi = 37, 29, 37 if plen else 9, 8, (3, 2, 34, 27)
    frames = event_frames(c, w, h, n)
    want = checked_want(c, w, h, n, roi, mode, tau_k)
    dev = torch.from_numpy(frames.copy()).cuda()
    out = torch.full((4, roi[3], roi[2]), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    op = make_op(c, mode, TAUS[tau_k])
    try:
        op.run_pixel_times_device(dev[:k], out, roi=roi)
        op.run_pixel_times_device(dev[k:], out, roi=roi, ref=dev[k - 1] if mode == 1 else dev[0], t0=k,
                                  accumulate=True)
        torch.cuda.synchronize()
    finally:
        op.close()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


def test_no_frames():
    """n_frames = 0: an overwriting call writes the initial state, an
    accumulating one leaves a poisoned buffer alone (host and device)."""
    import torch
    c, w, h = 3, 37, 29
    frames = event_frames(c, w, h, 5)
    op = make_op(c, 1, 8 / 255)
    try:
        assert np.array_equal(op.pixel_times(frames[:0]).as_array(), initial_state(h, w))
        lib, hp = op._host._lib, op._host.ptr
        buf = np.full((4, h, w), 0xA5A5A5A5, dtype=np.uint32)
        assert lib.dips_diff_pixel_times(hp, w, h, None, 0, None, None, 0, 1, buf.ctypes.data) == 0
        assert (buf == 0xA5A5A5A5).all()
        assert lib.dips_diff_pixel_times(hp, w, h, None, 0, None, None, 0, 0, buf.ctypes.data) == 0
        assert np.array_equal(buf, initial_state(h, w))
        dev = torch.from_numpy(frames.copy()).cuda()
        out = torch.full((4, h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        op.run_pixel_times_device(dev[:0], out, accumulate=True)
        torch.cuda.synchronize()
        assert bool((out == 0x5A5A5A5A).all())
        op.run_pixel_times_device(dev[:0], out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), initial_state(h, w))
    finally:
        op.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_explicit_reference(c, mode):
    w, h, n, tau_k = 37, 29, 9, 8
    got = run_times(c, event_frames(c, w, h, n), None, mode, TAUS[tau_k], ref=event_ref(c, w, h))
    assert (got[0] == 0).any()  # against the reference frame 0 changes too
    assert np.array_equal(got, checked_want(c, w, h, n, None, mode, tau_k, 0, True))


@pytest.mark.parametrize("tau_k", [0, 4, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_fast_generic_and_crosscheck_paths_agree(c, mode, tau_k):
    w, h, n, roi = 37, 29, 9, (3, 2, 33, 27)
    frames = event_frames(c, w, h, n)
    fast = run_times(c, frames, roi, mode, TAUS[tau_k], t0=7)
    generic = run_times(c, frames, roi, mode, TAUS[tau_k], t0=7, force_generic=True)
    cross = run_times(c, frames, roi, mode, TAUS[tau_k], t0=7, crosscheck=True)
    want = checked_want(c, w, h, n, roi, mode, tau_k, t0=7)
    assert np.array_equal(generic, fast)
    assert np.array_equal(cross, fast)
    assert np.array_equal(fast, want)


@pytest.mark.parametrize("plen", [0, 17])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_device_path_writes_exactly_its_bytes(c, mode, plen, monkeypatch):
    """times_out is poisoned and sits between two guard bands; the roi has an
    odd x and touches the frame's last pixel (a partial vec that would cross
    the frame's end); the frames tensor starts 1 byte off every natural
    alignment.  Every u32 of the four planes is written, no guard byte is."""
    import torch
    if plen:
        monkeypatch.setenv("DIPS_PIXEL_PART_FRAMES", str(plen))
    else:
        monkeypatch.delenv("DIPS_PIXEL_PART_FRAMES", raising=False)
    w, h, n, tau_k, roi = 37, 29, 24 if plen else 9, 8, (3, 2, 34, 27)
    frames, ref = event_frames(c, w, h, n), event_ref(c, w, h)
    want = checked_want(c, w, h, n, roi, mode, tau_k, 0, True)
    buf = torch.zeros(frames.nbytes + 16, dtype=torch.uint8, device="cuda")
    dev = buf[1:1 + frames.nbytes].view(frames.shape)
    dev.copy_(torch.from_numpy(frames.copy()))
    assert dev.data_ptr() % 4 == 1
    words, guard = 4 * roi[3] * roi[2], 64
    poison = 0x5A5A5A5A  # not a value of any plane: no index or run of these clips is that large
    store = torch.full((guard + words + guard,), poison, dtype=torch.int32, device="cuda")
    out = store[guard:guard + words].view(4, roi[3], roi[2])
    op = make_op(c, mode, TAUS[tau_k])
    try:
        op.run_pixel_times_device(dev, out, roi=roi, ref=torch.from_numpy(ref.copy()).cuda())
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            op.run_pixel_times_device(dev, out)  # the whole frame's shape is asked
    finally:
        op.close()
    got = store.cpu().numpy()
    assert (got[:guard] == poison).all() and (got[guard + words:] == poison).all()
    assert (want != poison).all()
    assert np.array_equal(got[guard:guard + words].view(np.uint32).reshape(want.shape), want)


def test_device_times_must_be_word_aligned():
    import torch
    from dips_amd import DipsError
    c, w, h, n = 3, 37, 29, 5
    dev = torch.from_numpy(event_frames(c, w, h, n).copy()).cuda()
    nbytes = 4 * h * w * 4
    buf = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    op = make_op(c, 1, 8 / 255)
    try:
        lib, hp = op._dev._lib, op._dev.ptr
        st = lib.dips_diff_pixel_times(hp, w, h, dev.data_ptr(), n, None, None, 0, 0, buf.data_ptr() + 2)
        torch.cuda.synchronize()
        assert st == -1
        with pytest.raises(DipsError) as e:
            op._dev.check(st)
        assert "4-byte aligned" in str(e.value)
        assert bool((buf == 0xFF).all())
        good = buf[:nbytes].view(torch.int32).view(4, h, w)
        op.run_pixel_times_device(dev, good)
        torch.cuda.synchronize()
    finally:
        op.close()
    assert np.array_equal(good.cpu().numpy().view(np.uint32), want_of(c, w, h, n, None, 1, 8))


def test_consistency_with_the_other_products_full_hd():
    """1920x1080 RGB8, 8 frames, per-frame, tau = 8/255, against
    py_pixel_times and the library's own change mask and region form."""
    c, w, h, n, roi = 3, 1920, 1080, 8, (161, 90, 641, 360)
    frames = event_frames(c, w, h, n)
    want = py_pixel_times(frames, 1, 8 / 255)
    check_informative(want, n)
    op = make_op(c, 1, 8 / 255)
    try:
        t = op.pixel_times(frames)
        bits = op.change_mask(frames).unpack()
        part = op.pixel_times(frames, roi=roi)
    finally:
        op.close()
    assert np.array_equal(t.as_array(), want)
    assert np.array_equal(t.first != NONE, bits.any(axis=0))
    last_t = (n - 1 - np.argmax(bits[::-1], axis=0)).astype(np.uint32)
    assert np.array_equal(t.last, np.where(bits.any(axis=0), last_t, np.uint32(NONE)))
    assert np.array_equal(part.as_array(), t.as_array()[:, 90:450, 161:802])


def test_errors_leave_the_operator_usable():
    import torch
    from dips_amd import DipsError, PixelTimes, _lib
    c, w, h, n = 3, 37, 29, 5
    frames = event_frames(c, w, h, n)
    op = make_op(c, 1, 8 / 255)
    try:
        for roi in ((30, 0, 8, 5), (0, 25, 8, 5), (3, 2, 0, 17), (3, 2, 21, 0)):
            with pytest.raises(DipsError) as e:
                op.pixel_times(frames, roi=roi)
            assert e.value.status == -1 and "diff_pixel_times:" in str(e.value)
        lib, hp = op._host._lib, op._host.ptr
        buf = np.full((4, h, w), 0xA5A5A5A5, dtype=np.uint32)
        f = frames.ctypes.data
        assert lib.dips_diff_pixel_times(hp, w, h, None, n, None, None, 0, 0, buf.ctypes.data) == _lib.DIPS_ERR_INVALID
        assert lib.dips_diff_pixel_times(hp, w, h, f, n, None, None, 0, 0, None) == _lib.DIPS_ERR_INVALID
        assert lib.dips_diff_pixel_times(hp, w, h, None, 0, None, None, 0, 0, None) == _lib.DIPS_ERR_INVALID
        assert lib.dips_diff_pixel_times(None, w, h, f, n, None, None, 0, 0, buf.ctypes.data) == _lib.DIPS_ERR_INVALID
        assert (buf == 0xA5A5A5A5).all()
        with pytest.raises(ValueError):
            op.pixel_times(frames, into=PixelTimes.from_array(np.zeros((4, h, w - 1), dtype=np.uint32)))
        with pytest.raises(ValueError):
            op.pixel_times(frames, t0=-1)
        dev = torch.from_numpy(frames.copy()).cuda()
        for shape in ((4, h, w - 1), (3, h, w), (h, w, 4)):
            with pytest.raises(ValueError):
                op.run_pixel_times_device(dev, torch.zeros(shape, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError):
            op.run_pixel_times_device(dev, torch.zeros((4, h, w), dtype=torch.int64, device="cuda"))
        got = op.pixel_times(frames).as_array()
    finally:
        op.close()
    assert np.array_equal(got, checked_want(c, w, h, n, None, 1, 8))


def test_kernel_time_records_the_launch():
    import torch
    frames = torch.from_numpy(event_frames(3, 96, 64, 5).copy()).cuda()
    out = torch.zeros((4, 64, 96), dtype=torch.int32, device="cuda")
    op = make_op(3, 1, 8 / 255, time_kernel=True)
    try:
        op.run_pixel_times_device(frames, out)
        op.run_pixel_times_device(frames, out, t0=5, accumulate=True, ref=frames[4])
        ms, launches = op.kernel_time()
    finally:
        op.close()
    assert launches == 2 and ms > 0.0
