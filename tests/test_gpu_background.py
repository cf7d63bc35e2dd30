"""dips_diff_background_mask on the GPU: the mask (pad bits included) and the
state are exactly those of the definition in tests/_background_ref.py -- the
fold over py_change_mask, which tests/test_background_cpu.py proves equal to
the fold over the C oracle's per-pixel crops.  Content: noise_frames (a random
base frame plus uniform noise in [-12, 12] per frame) and the
drift-and-moving-square clip.  Informative-input conditions are asserted on
the reference alone: at tau > 0 its mask from frame 1 on has 5-95 % of its
bits set; on the drift clip at k = 1 .. 3 it differs from both the
'per-frame' and the 'overall' oracle mask in at least 5 % of the bits.

Schedule (series_sched.h background_geometry): one part always; a tile is 64
* kUnrollBackground vecs of the region rows padded to whole mask words, 64
vecs when the larger tiles would fill under half of the wave slots (every
small shape here; test_large_tiles reaches the larger tiles)."""
import functools

import numpy as np
import pytest

import _components_ref as cref
from _background_ref import background_fold, drift_clip
from test_change_mask_cpu import TAUS, noise_frames, noise_ref, py_change_mask, unpack_mask
from test_gpu_change_mask import CONFIGS, GEOMETRY, make_op

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def want_of(c, w, h, n, roi, k, selective, tau_k, chroma=0, with_ref=False, clip="noise"):
    frames = noise_frames(c, w, h, n) if clip == "noise" else drift_clip(c, w, h, n)
    ref = noise_ref(c, w, h) if with_ref else None
    mask, state = background_fold(frames, k, selective, TAUS[tau_k], chroma, ref, roi)
    mask.setflags(write=False)
    state.setflags(write=False)
    return mask, state


def checked_want(c, w, h, n, roi, k, selective, tau_k, chroma=0, with_ref=False, clip="noise"):
    mask, state = want_of(c, w, h, n, roi, k, selective, tau_k, chroma, with_ref, clip)
    rw = w if roi is None else roi[2]
    if tau_k and n > 1:
        share = unpack_mask(mask, rw)[1:].mean()
        assert 0.05 < share < 0.95, share
    return mask, state


def run_bg(c, frames, roi=None, tau=8 / 255, chroma=0, ref=None, k=3, selective=False, state=None, mode=1, **kw):
    op = make_op(c, mode, tau, chroma, **kw)
    try:
        m, b = op.background_mask(frames, roi=roi, ref=ref, rate_shift=k, selective=selective, state=state)
    finally:
        op.close()
    assert m.width == (frames.shape[2] if roi is None else roi[2])
    return m.bits, b.state


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("tau_k,chroma", CONFIGS)
@pytest.mark.parametrize("k", [0, 1, 3, 8])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_formats_and_parameters(c, k, tau_k, chroma):
    """c = 1 runs the generic kernel.  Selective on and off, with and without ref."""
    from dips_amd import Background
    if c == 1 and chroma:
        chroma = 0
    w, h, n = 37, 29, 9
    frames = noise_frames(c, w, h, n)
    op = make_op(c, 1, TAUS[tau_k], chroma)
    try:
        for selective in (False, True):
            for with_ref in (False, True):
                want = checked_want(c, w, h, n, None, k, selective, tau_k, chroma, with_ref)
                m, b = op.background_mask(frames, ref=noise_ref(c, w, h) if with_ref else None, rate_shift=k,
                                          selective=selective)
                assert isinstance(b, Background) and b.state.shape == (c, h, w) and b.state.dtype == np.uint16
                assert m.bits.shape == (n, h, 8) and m.width == w
                assert same((m.bits, b.state), want), (selective, with_ref)
                if not with_ref:
                    assert not m.bits[0].any()  # frame 0 meets itself
    finally:
        op.close()


@pytest.mark.parametrize("w,h,roi", GEOMETRY)
@pytest.mark.parametrize("c", [3, 4])
def test_geometry(c, w, h, roi):
    n, tau_k = 5, 8
    got = run_bg(c, noise_frames(c, w, h, n), roi, TAUS[tau_k], k=2, selective=True)
    rw, rh = (w, h) if roi is None else roi[2:]
    assert got[0].shape == (n, rh, 4 * ((rw + 31) // 32)) and got[1].shape == (c, rh, rw)
    assert same(got, checked_want(c, w, h, n, roi, 2, True, tau_k))


@pytest.mark.parametrize("w,h", [(1, 8), (2, 8), (1, 3)])
@pytest.mark.parametrize("selective", [False, True])
@pytest.mark.parametrize("c", [3, 4])
def test_narrow_frames(c, selective, w, h):
    """Frames narrower than 3 pixels: the partial vecs of several rows would
    read past the frame's end; the generic kernel owns their words and state."""
    n, tau_k = 9, 4
    want = checked_want(c, w, h, n, None, 2, selective, tau_k)
    assert same(run_bg(c, noise_frames(c, w, h, n), None, TAUS[tau_k], k=2, selective=selective), want)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7])
@pytest.mark.parametrize("c", [3, 4])
def test_ring_prologue_and_tail(c, n):
    w, h, tau_k = 37, 29, 4
    assert same(run_bg(c, noise_frames(c, w, h, n), None, TAUS[tau_k], k=1), checked_want(c, w, h, n, None, 1, False, tau_k))


@pytest.mark.parametrize("selective", [False, True])
@pytest.mark.parametrize("c", [3, 4])
def test_one_wave_carries_a_long_state(c, selective):
    w, h, n, tau_k = 8, 8, 300, 8
    assert same(run_bg(c, noise_frames(c, w, h, n), None, TAUS[tau_k], k=3, selective=selective),
                checked_want(c, w, h, n, None, 3, selective, tau_k))


@pytest.mark.parametrize("selective", [False, True])
@pytest.mark.parametrize("c", [3, 4])
def test_large_tiles(c, selective, monkeypatch):
    """The tiles of 64 * kUnrollBackground vecs: taken when they fill at least
    half of the wave slots.  With DIPS_SERIES_WAVES_PER_SIMD = 1 the slots
    are 4 per CU (1024 on 256 CUs), and 1021 x 400 pixels are 800 such tiles.
    The ragged last vec of the frame is left to the generic kernel."""
    monkeypatch.setenv("DIPS_SERIES_WAVES_PER_SIMD", "1")
    w, h, n, tau_k = 1021, 400, 5, 8
    want = checked_want(c, w, h, n, None, 3, selective, tau_k)
    assert same(run_bg(c, noise_frames(c, w, h, n), None, TAUS[tau_k], k=3, selective=selective), want)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("selective", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_drift_clip(c, k, selective):
    """The clip the feature is for: the adaptive reference decides unlike
    both fixed ones, and the library follows it bit for bit."""
    w, h, n, tau_k = 37, 29, 24, 8
    clip = drift_clip(c, w, h, n)
    want = checked_want(c, w, h, n, None, k, selective, tau_k, clip="drift")
    bits = unpack_mask(want[0], w)[1:]
    for mode in (0, 1):
        other = unpack_mask(py_change_mask(clip, mode, TAUS[tau_k]), w)[1:]
        assert (bits != other).mean() >= 0.05, (mode, (bits != other).mean())
    assert same(run_bg(c, clip, None, TAUS[tau_k], k=k, selective=selective), want)


@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_rate_shift_zero_is_the_per_frame_mask_on_the_device(c, with_ref):
    w, h, n, tau_k = 37, 29, 9, 8
    frames = noise_frames(c, w, h, n)
    ref = noise_ref(c, w, h) if with_ref else None
    op = make_op(c, 1, TAUS[tau_k])
    try:
        per_frame = op.change_mask(frames, ref=ref).bits
        m, b = op.background_mask(frames, ref=ref, rate_shift=0)
    finally:
        op.close()
    assert 0.05 < unpack_mask(per_frame, w)[1:].mean() < 0.95
    assert np.array_equal(m.bits, per_frame)
    last = frames[-1][None] if c == 1 else np.moveaxis(frames[-1], -1, 0)
    assert np.array_equal(b.state, 256 * last.astype(np.uint16))


@pytest.mark.parametrize("selective", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_chunks_continue_the_state(c, selective):
    """9 + 1 + 7 frames with state= equal one call of 17, mask and state."""
    w, h, n, tau_k = 37, 29, 17, 8
    frames = noise_frames(c, w, h, n)
    op = make_op(c, 1, TAUS[tau_k])
    try:
        whole = op.background_mask(frames, selective=selective)
        bits, state = [], None
        for lo, hi in ((0, 9), (9, 10), (10, 17)):
            m, state = op.background_mask(frames[lo:hi], selective=selective, state=state)
            bits.append(m.bits)
        kept = state.state.copy()
        m, again = op.background_mask(frames[:0], state=state)  # no frames: the state comes back as it is
    finally:
        op.close()
    want = checked_want(c, w, h, n, None, 3, selective, tau_k)
    assert same((whole[0].bits, whole[1].state), want)
    assert same((np.concatenate(bits), state.state), want)
    assert m.bits.shape == (0, h, 8) and np.array_equal(again.state, kept)


@pytest.mark.parametrize("roi", [None, (3, 2, 33, 27)])
@pytest.mark.parametrize("c", [3, 4])
def test_kernel_paths_agree(c, roi):
    """fast = generic = crosscheck = definition; params.mode is not consulted."""
    w, h, n, tau_k = 37, 29, 9, 4
    frames = noise_frames(c, w, h, n)
    want = checked_want(c, w, h, n, roi, 2, True, tau_k)
    fast = run_bg(c, frames, roi, TAUS[tau_k], k=2, selective=True)
    assert same(fast, want)
    assert same(run_bg(c, frames, roi, TAUS[tau_k], k=2, selective=True, force_generic=True), want)
    assert same(run_bg(c, frames, roi, TAUS[tau_k], k=2, selective=True, crosscheck=True), want)
    assert same(run_bg(c, frames, roi, TAUS[tau_k], k=2, selective=True, mode=0), want)


@pytest.mark.parametrize("roi", [None, (3, 2, 21, 17)])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_device_path_writes_every_byte(c, accumulate, roi):
    """The outputs start as 0xFF everywhere; the frames tensor starts 1 byte
    off every natural alignment; mask None gives the same state."""
    import torch
    w, h, n, tau_k = 37, 29, 9, 8
    frames = noise_frames(c, w, h, n)
    rw, rh = (w, h) if roi is None else roi[2:]
    want = checked_want(c, w, h, n, roi, 3, True, tau_k)
    buf = torch.zeros(frames.nbytes + 16, dtype=torch.uint8, device="cuda")
    dev = buf[1:1 + frames.nbytes].view(frames.shape)
    dev.copy_(torch.from_numpy(frames.copy()))
    assert dev.data_ptr() % 4 == 1
    split = 4 if accumulate else 0
    op = make_op(c, 1, TAUS[tau_k])
    try:
        out = torch.full(want[0].shape, 0xFF, dtype=torch.uint8, device="cuda")
        bg = torch.full((c, rh, rw), -1, dtype=torch.int16, device="cuda")
        alone = torch.full((c, rh, rw), -1, dtype=torch.int16, device="cuda")
        if accumulate:
            op.run_background_mask_device(dev[:split], bg, out[:split], roi=roi, selective=True)
            op.run_background_mask_device(dev[:split], alone, None, roi=roi, selective=True)
        op.run_background_mask_device(dev[split:], bg, out[split:], roi=roi, selective=True, accumulate=accumulate)
        op.run_background_mask_device(dev[split:], alone, None, roi=roi, selective=True, accumulate=accumulate)
        torch.cuda.synchronize()
        if roi is not None:
            with pytest.raises(ValueError):
                op.run_background_mask_device(dev, bg, out)  # the whole frame's shapes are asked
    finally:
        op.close()
    assert np.array_equal(out.cpu().numpy(), want[0])
    assert np.array_equal(bg.cpu().numpy().view(np.uint16), want[1])
    assert np.array_equal(alone.cpu().numpy().view(np.uint16), want[1])


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_saturation(c, k):
    """Content alternating 0 / 255 per frame, channel and column: B at both
    ends of its range."""
    w, h, n = 37, 29, 9
    t, x, ch = np.meshgrid(np.arange(n), np.arange(w), np.arange(c), indexing="ij")
    frames = np.broadcast_to((255 * ((t + x + ch) & 1)).astype(np.uint8)[:, None], (n, h, w, c))
    frames = np.ascontiguousarray(frames[..., 0] if c == 1 else frames)
    # with every channel in (max + min is 255 in every RGB pixel) the intensity
    # never moves and only the state is at stake; the red channel alone flips
    chroma = 0 if c == 1 else 1
    assert unpack_mask(background_fold(frames, k, False, 8 / 255, chroma)[0], w)[1:].mean() > 0.3
    for selective, ch in ((False, 0), (True, 0), (False, chroma), (True, chroma)):
        want = background_fold(frames, k, selective, 8 / 255, ch)
        assert same(run_bg(c, frames, None, 8 / 255, ch, k=k, selective=selective), want)
    ends = background_fold(frames[:1], k, False, 8 / 255)[1]
    assert ends.min() == 0 and ends.max() == 65280


def test_initial_state_alone():
    """n_frames = 0 without accumulate writes 256 * ref of the region."""
    import torch
    c, w, h, roi = 3, 37, 29, (3, 2, 21, 17)
    frames, ref = noise_frames(c, w, h, 9), noise_ref(c, w, h)
    want = 256 * np.moveaxis(ref[2:19, 3:24], -1, 0).astype(np.uint16)
    op = make_op(c, 1, 8 / 255)
    try:
        m, b = op.background_mask(frames[:0], roi=roi, ref=ref)
        bg = torch.full((c, 17, 21), -1, dtype=torch.int16, device="cuda")
        op.run_background_mask_device(torch.from_numpy(frames[:0].copy()).cuda(), bg, None, roi=roi,
                                      ref=torch.from_numpy(ref.copy()).cuda())
        torch.cuda.synchronize()
    finally:
        op.close()
    assert m.bits.shape == (0, 17, 4) and np.array_equal(b.state, want)
    assert np.array_equal(bg.cpu().numpy().view(np.uint16), want)


def test_errors_leave_the_outputs_untouched():
    import torch
    from dips_amd import DipsError, _lib
    c, w, h, n = 3, 37, 29, 5
    frames, ref = noise_frames(c, w, h, n), noise_ref(c, w, h)
    op = make_op(c, 1, 8 / 255)
    try:
        for roi in ((30, 0, 8, 5), (0, 25, 8, 5), (3, 2, 0, 17), (3, 2, 21, 0)):
            with pytest.raises(DipsError) as e:
                op.background_mask(frames, roi=roi)
            assert e.value.status == -1 and "diff_background_mask:" in str(e.value)
        lib, hp = op._host._lib, op._host.ptr
        mask = np.full((n, h, 8), 0xFF, dtype=np.uint8)
        bg = np.full((c, h, w), 0xFFFF, dtype=np.uint16)
        fp, rp, mp, bp = frames.ctypes.data, ref.ctypes.data, mask.ctypes.data, bg.ctypes.data
        call = lib.dips_diff_background_mask
        bad = [
            (hp, w, h, fp, n, None, None, 9, 0, 0, bp, mp),       # rate_shift
            (hp, w, h, fp, n, None, None, 3, 2, 0, bp, mp),       # unknown flag bit
            (hp, w, h, fp, n, None, None, 3, 3, 0, bp, mp),
            (hp, w, h, None, n, None, None, 3, 0, 0, bp, mp),     # null frames
            (hp, w, h, fp, n, None, None, 3, 0, 0, None, mp),     # null background
            (hp, w, h, fp, n, rp, None, 3, 0, 1, bp, mp),         # ref while accumulating
            (hp, w, h, None, 0, None, None, 3, 0, 0, bp, mp),     # nothing to start from
            (hp, 32768, 32768, fp, n, None, None, 3, 0, 0, bp, mp),  # 2^30 pixels
            (None, w, h, fp, n, None, None, 3, 0, 0, bp, mp),
        ]
        for args in bad:
            assert call(*args) == _lib.DIPS_ERR_INVALID, args[7:10]
        # accumulate without frames: OK, nothing is written
        assert call(hp, w, h, None, 0, None, None, 3, 0, 1, bp, mp) == 0
        assert (mask == 0xFF).all() and (bg == 0xFFFF).all()
        dev = torch.from_numpy(frames.copy()).cuda()
        mbuf = torch.full((n * h * 8 + 16,), 0xFF, dtype=torch.uint8, device="cuda")
        bbuf = torch.full((c * h * w * 2 + 16,), 0xFF, dtype=torch.uint8, device="cuda")
        good_m, good_b = mbuf[4:4 + n * h * 8].view(n, h, 8), bbuf[4:4 + c * h * w * 2].view(torch.int16).view(c, h, w)
        dl, dp = op._dev._lib, op._dev.ptr
        for b_off, m_off, word in ((1, 4, "2-byte aligned"), (4, 2, "4-byte aligned")):
            st = dl.dips_diff_background_mask(dp, w, h, dev.data_ptr(), n, None, None, 3, 0, 0,
                                              bbuf.data_ptr() + b_off, mbuf.data_ptr() + m_off)
            assert st == _lib.DIPS_ERR_INVALID and word in dl.dips_last_error(dp).decode()
        torch.cuda.synchronize()
        assert bool((mbuf == 0xFF).all()) and bool((bbuf == 0xFF).all())
        for shape in ((c, h, w - 1), (c + 1, h, w), (c * h, w)):
            with pytest.raises(ValueError):
                op.run_background_mask_device(dev, torch.zeros(shape, dtype=torch.int16, device="cuda"), good_m)
        with pytest.raises(ValueError):
            op.run_background_mask_device(dev, torch.zeros((c, h, w), dtype=torch.int32, device="cuda"), good_m)
        with pytest.raises(ValueError):
            op.run_background_mask_device(dev, good_b, torch.zeros((n, h, 4), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            op.run_background_mask_device(dev, good_b, good_m, ref=torch.from_numpy(ref.copy()).cuda(), accumulate=True)
        op.run_background_mask_device(dev, good_b, good_m)
        torch.cuda.synchronize()
        got = op.background_mask(frames)
    finally:
        op.close()
    want = checked_want(c, w, h, n, None, 3, False, 8)
    assert same((got[0].bits, got[1].state), want)
    assert same((good_m.cpu().numpy(), good_b.cpu().numpy().view(np.uint16)), want)


@pytest.mark.parametrize("background", [3, (2, True)])
@pytest.mark.parametrize("c", [3, 1])
def test_change_boxes_on_the_background_mask(c, background):
    w, h, n, tau_k, roi = 37, 29, 24, 8, (2, 1, 34, 27)
    clip = drift_clip(c, w, h, n).copy()
    k, selective = background if isinstance(background, tuple) else (background, False)
    op = make_op(c, 0, TAUS[tau_k])
    try:
        for r in (None, roi):
            mask = checked_want(c, w, h, n, r, k, selective, tau_k, clip="drift")[0]
            rw = w if r is None else r[2]
            got = op.change_boxes(clip, roi=r, connectivity=8, min_area=4, max_boxes=16, labels=True, background=background)
            ref = cref.components(mask, rw, 8, 4, 16)
            assert ref[0].any()
            assert all(np.array_equal(g, x) for g, x in zip((got.counts, got.boxes, got.labels), ref))
        with pytest.raises(ValueError):
            op.change_boxes(clip, background=9)
    finally:
        op.close()


def test_kernel_time_records_the_launch():
    import torch
    frames = torch.from_numpy(noise_frames(3, 96, 64, 5).copy()).cuda()
    out = torch.zeros((5, 64, 12), dtype=torch.uint8, device="cuda")
    bg = torch.zeros((3, 64, 96), dtype=torch.int16, device="cuda")
    op = make_op(3, 1, 8 / 255, time_kernel=True)
    try:
        op.run_background_mask_device(frames, bg, out)
        op.run_background_mask_device(frames, bg, out, accumulate=True)
        ms, launches = op.kernel_time()
    finally:
        op.close()
    assert launches == 2 and ms > 0.0
