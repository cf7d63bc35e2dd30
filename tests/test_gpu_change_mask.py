"""dips_diff_change_mask on the GPU: every bit is exactly the count field of the
series the CPU oracle gives for the frames (and the reference) cropped to that
pixel (oracle_change_mask, tests/test_change_mask_cpu.py; the 1280x720 case
uses the vectorised py_change_mask that file proves equal).  Frames are a
random base frame plus uniform integer noise in [-12, 12] per frame; every
tau > 0 case asserts that the oracle's mask has 20-80 % of its bits set, every
tau = 0 case that it has zeros and ones.  Every comparison is np.array_equal
on the whole mask, pad bits included.

Schedule (series_sched.h mask_geometry): a tile is 64 * kUnrollMask vecs of
the region rows padded to whole mask words; the frames are cut into as many
parts of >= 16 frames as give every wave slot (4 waves per SIMD x 4 SIMDs x
the CUs, far more than the tiles of any small shape here) an item: one part
below 32 frames, two parts of 19 and 18 at 37 frames, 18 parts of 17 frames
at 300 frames."""
import functools

import numpy as np
import pytest

from test_change_mask_cpu import TAUS, check_share, noise_frames, noise_ref, oracle_change_mask, py_change_mask

pytestmark = pytest.mark.gpu


def _fmt(c):
    from dips_amd import PixelFormat
    return {1: PixelFormat.Gray8, 3: PixelFormat.RGB8, 4: PixelFormat.RGBA8}[c]


@functools.lru_cache(maxsize=None)
def want_of(c, w, h, n, roi, mode, tau_k, chroma=0, with_ref=False):
    ref = noise_ref(c, w, h) if with_ref else None
    a = oracle_change_mask(noise_frames(c, w, h, n), mode, TAUS[tau_k], chroma, ref, roi)
    a.setflags(write=False)
    return a


def checked_want(c, w, h, n, roi, mode, tau_k, chroma=0, with_ref=False):
    """The oracle's mask, shown informative (frame 0 of a call without a
    reference meets itself and is left out of the share)."""
    want = want_of(c, w, h, n, roi, mode, tau_k, chroma, with_ref)
    rw = w if roi is None else roi[2]
    if n > 1 or with_ref:
        check_share(want, rw, tau_k, first=0 if with_ref else 1)
    return want


def make_op(c, mode, tau, chroma=0, **kw):
    from dips_amd import ChromaFilter, DiffSeriesOperator, Mode
    return DiffSeriesOperator(_fmt(c), Mode(mode), tau, ChromaFilter(chroma), **kw)


def run_mask(c, frames, roi, mode, tau, chroma=0, ref=None, **kw):
    op = make_op(c, mode, tau, chroma, **kw)
    try:
        m = op.change_mask(frames, roi=roi, ref=ref)
    finally:
        op.close()
    assert m.width == (frames.shape[2] if roi is None else roi[2])
    return m.bits


# chroma: none for every tau (4/255 < 2^-5 <= 8/255), one channel at the two ends
CONFIGS = [(0, 0), (4, 0), (8, 0), (0, 1), (8, 2)]


@pytest.mark.parametrize("tau_k,chroma", CONFIGS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_formats_modes_taus(c, mode, tau_k, chroma):
    """c = 1 runs the generic kernel."""
    if c == 1 and chroma:
        chroma = 0  # GRAY8 has no channels to pick; the case still runs its tau
    w, h, n = 37, 29, 9
    got = run_mask(c, noise_frames(c, w, h, n), None, mode, TAUS[tau_k], chroma)
    assert got.shape == (n, h, 8) and got.dtype == np.uint8
    assert np.array_equal(got, checked_want(c, w, h, n, None, mode, tau_k, chroma))


GEOMETRY = [
    (37, 29, None),             # the last vec of the frame is partial and would cross the frame's end
    (37, 29, (3, 2, 21, 17)),   # an odd x
    (37, 29, (33, 0, 4, 29)),   # touching the right edge
    (32, 5, None),              # a word-exact row
    (33, 5, None),              # one pad-heavy word
    (64, 5, None),              # two words
    (40, 70, None),             # 1120 padded vecs: several tiles, the last partly empty
    (96, 64, None),
]


@pytest.mark.parametrize("w,h,roi", GEOMETRY)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_geometry(c, mode, w, h, roi):
    n, tau_k = 5, 8
    got = run_mask(c, noise_frames(c, w, h, n), roi, mode, TAUS[tau_k])
    rw, rh = (w, h) if roi is None else roi[2:]
    assert got.shape == (n, rh, 4 * ((rw + 31) // 32))
    assert np.array_equal(got, checked_want(c, w, h, n, roi, mode, tau_k))


@pytest.mark.parametrize("w,h", [(1, 8), (2, 8), (1, 3)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_narrow_frames(c, mode, w, h):
    """Frames narrower than 3 pixels: the partial vecs of several rows would
    read past the frame's end; the generic kernel rewrites their words."""
    n, tau_k = 9, 4
    want = checked_want(c, w, h, n, None, mode, tau_k)
    assert np.array_equal(run_mask(c, noise_frames(c, w, h, n), None, mode, TAUS[tau_k]), want)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_ring_prologue_and_tail(c, mode, n):
    w, h, tau_k = 37, 29, 4
    got = run_mask(c, noise_frames(c, w, h, n), None, mode, TAUS[tau_k])
    assert not got[0].any()  # frame 0 meets itself
    assert np.array_equal(got, checked_want(c, w, h, n, None, mode, tau_k))


@pytest.mark.parametrize("w,h,n,plen", [(37, 29, 37, 19), (8, 8, 300, 17)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_frame_parts(c, mode, w, h, n, plen):
    """Several frame parts (the part rule is in this file's docstring: parts
    of `plen` frames here; the library exposes no geometry of the mask to
    assert it through).  In per-frame mode a part's first reference is the
    frame before it: every part boundary is compared on its own."""
    tau_k = 8
    got = run_mask(c, noise_frames(c, w, h, n), None, mode, TAUS[tau_k])
    want = checked_want(c, w, h, n, None, mode, tau_k)
    for t in range(plen, n, plen):
        assert np.array_equal(got[t], want[t]), f"first frame of the part at {t}"
        assert np.array_equal(got[t - 1], want[t - 1]), f"last frame of the part before {t}"
    assert np.array_equal(got, want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_explicit_reference(c, mode):
    w, h, n, tau_k = 37, 29, 9, 8
    got = run_mask(c, noise_frames(c, w, h, n), None, mode, TAUS[tau_k], ref=noise_ref(c, w, h))
    assert got[0].any()
    assert np.array_equal(got, checked_want(c, w, h, n, None, mode, tau_k, 0, True))


@pytest.mark.parametrize("tau_k", [0, 4, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_fast_generic_and_crosscheck_paths_agree(c, mode, tau_k):
    w, h, n, roi = 37, 29, 9, (3, 2, 33, 27)
    frames = noise_frames(c, w, h, n)
    fast = run_mask(c, frames, roi, mode, TAUS[tau_k])
    generic = run_mask(c, frames, roi, mode, TAUS[tau_k], force_generic=True)
    cross = run_mask(c, frames, roi, mode, TAUS[tau_k], crosscheck=True)
    want = checked_want(c, w, h, n, roi, mode, tau_k)
    assert np.array_equal(generic, fast)
    assert np.array_equal(cross, fast)
    assert np.array_equal(fast, want)


@pytest.mark.parametrize("roi", [None, (3, 2, 21, 17)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_device_path_writes_every_byte(c, mode, roi):
    """mask_out starts as 0xFF everywhere: every byte is written, pad bits 0;
    the frames tensor starts 1 byte off every natural alignment."""
    import torch
    w, h, n, tau_k = 37, 29, 9, 8
    frames, ref = noise_frames(c, w, h, n), noise_ref(c, w, h)
    want = checked_want(c, w, h, n, roi, mode, tau_k, 0, True)
    buf = torch.zeros(frames.nbytes + 16, dtype=torch.uint8, device="cuda")
    dev = buf[1:1 + frames.nbytes].view(frames.shape)
    dev.copy_(torch.from_numpy(frames.copy()))
    assert dev.data_ptr() % 4 == 1
    out = torch.full(want.shape, 0xFF, dtype=torch.uint8, device="cuda")
    op = make_op(c, mode, TAUS[tau_k])
    try:
        op.run_change_mask_device(dev, out, roi=roi, ref=torch.from_numpy(ref.copy()).cuda())
        torch.cuda.synchronize()
        if roi is not None:
            with pytest.raises(ValueError):
                op.run_change_mask_device(dev, out)  # the whole frame's shape is asked
    finally:
        op.close()
    assert np.array_equal(out.cpu().numpy(), want)


def test_device_mask_must_be_word_aligned():
    import torch
    from dips_amd import DipsError
    c, w, h, n = 3, 37, 29, 5
    dev = torch.from_numpy(noise_frames(c, w, h, n).copy()).cuda()
    buf = torch.full((n * h * 8 + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    out = buf[2:2 + n * h * 8].view(n, h, 8)
    assert out.data_ptr() % 4 == 2
    op = make_op(c, 1, 8 / 255)
    try:
        with pytest.raises(DipsError) as e:
            op.run_change_mask_device(dev, out)
        torch.cuda.synchronize()
        assert e.value.status == -1 and "4-byte aligned" in str(e.value)
        assert bool((buf == 0xFF).all())
        good = buf[4:4 + n * h * 8].view(n, h, 8)
        op.run_change_mask_device(dev, good)
        torch.cuda.synchronize()
    finally:
        op.close()
    assert np.array_equal(good.cpu().numpy(), want_of(c, w, h, n, None, 1, 8))


def test_consistency_with_the_other_products_hd():
    """1280x720 RGB8, 5 frames, per-frame, tau = 8/255, against py_change_mask
    and the library's own per-pixel sums, one-cell grid and region form."""
    c, w, h, n, roi = 3, 1280, 720, 5, (161, 90, 641, 360)
    frames = noise_frames(c, w, h, n)
    want = py_change_mask(frames, 1, 8 / 255)
    check_share(want, w, 8, first=1)
    op = make_op(c, 1, 8 / 255)
    try:
        m = op.change_mask(frames)
        sums = op.pixel_sums(frames).count
        cell = op.grid(frames, 1, 1).count[:, 0, 0]
        part = op.change_mask(frames, roi=roi)
    finally:
        op.close()
    assert np.array_equal(m.bits, want)
    assert np.array_equal(m.unpack().sum(axis=0, dtype=np.uint64), sums)
    assert np.array_equal(m.counts(), cell)
    assert np.array_equal(part.unpack(), m.unpack()[:, 90:450, 161:802])
    assert np.array_equal(part.bits, py_change_mask(frames, 1, 8 / 255, roi=roi))


def test_errors_leave_the_operator_usable():
    import torch
    from dips_amd import DipsError, _lib
    c, w, h, n = 3, 37, 29, 5
    frames = noise_frames(c, w, h, n)
    op = make_op(c, 1, 8 / 255)
    try:
        for roi in ((30, 0, 8, 5), (0, 25, 8, 5), (3, 2, 0, 17), (3, 2, 21, 0)):
            with pytest.raises(DipsError) as e:
                op.change_mask(frames, roi=roi)
            assert e.value.status == -1 and "diff_change_mask:" in str(e.value)
        lib, hp = op._host._lib, op._host.ptr
        buf = np.full((n, h, 8), 0xFF, dtype=np.uint8)
        assert lib.dips_diff_change_mask(hp, w, h, None, n, None, None, buf.ctypes.data) == _lib.DIPS_ERR_INVALID
        assert lib.dips_diff_change_mask(hp, w, h, frames.ctypes.data, n, None, None, None) == _lib.DIPS_ERR_INVALID
        assert lib.dips_diff_change_mask(None, w, h, frames.ctypes.data, n, None, None,
                                         buf.ctypes.data) == _lib.DIPS_ERR_INVALID
        # no frames: OK, and nothing is written
        assert lib.dips_diff_change_mask(hp, w, h, frames.ctypes.data, 0, None, None, buf.ctypes.data) == 0
        assert lib.dips_diff_change_mask(hp, w, h, None, 0, None, None, None) == 0
        assert (buf == 0xFF).all()
        assert op.change_mask(frames[:0]).bits.shape == (0, h, 8)
        dev = torch.from_numpy(frames.copy()).cuda()
        for shape in ((n, h, 4), (n, h - 1, 8), (n, h * 8)):
            with pytest.raises(ValueError):
                op.run_change_mask_device(dev, torch.zeros(shape, dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            op.run_change_mask_device(dev, torch.zeros((n, h, 8), dtype=torch.int8, device="cuda"))
        got = op.change_mask(frames).bits
    finally:
        op.close()
    assert np.array_equal(got, checked_want(c, w, h, n, None, 1, 8))


@pytest.mark.parametrize("k", [1, 4, 5])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 4])
def test_clip_in_two_chunks(c, mode, k):
    """change_mask(frames[:k]) and change_mask(frames[k:], ref) -- ref the
    previous chunk's last frame in per-frame mode, the same reference in
    overall mode -- are the mask of the clip in one call."""
    w, h, n, tau_k = 37, 29, 9, 8
    frames = noise_frames(c, w, h, n)
    op = make_op(c, mode, TAUS[tau_k])
    try:
        a = op.change_mask(frames[:k]).bits
        b = op.change_mask(frames[k:], ref=frames[k - 1] if mode == 1 else frames[0]).bits
        whole = op.change_mask(frames).bits
    finally:
        op.close()
    assert np.array_equal(np.concatenate([a, b]), whole)
    assert np.array_equal(whole, checked_want(c, w, h, n, None, mode, tau_k))


def test_kernel_time_records_the_launch():
    import torch
    frames = torch.from_numpy(noise_frames(3, 96, 64, 5).copy()).cuda()
    out = torch.zeros((5, 64, 12), dtype=torch.uint8, device="cuda")
    op = make_op(3, 1, 8 / 255, time_kernel=True)
    try:
        op.run_change_mask_device(frames, out)
        op.run_change_mask_device(frames, out)
        ms, launches = op.kernel_time()
    finally:
        op.close()
    assert launches == 2 and ms > 0.0
