"""dips_diff_sigma_delta_mask on the GPU: the mask (pad bits included) and the
state are exactly those of the definition in tests/_sigma_delta_ref.py, which
tests/test_sigma_delta_cpu.py proves equal to a scalar per-pixel loop.
Content: noise_frames (a random base frame plus uniform noise in [-12, 12]
per frame) and the drift-and-moving-square clip.  Informative-input conditions
are asserted on the reference alone: its mask from frame 1 on has 5-95 % of
its bits set, and where stated V takes at least 3 distinct values.

Schedule (series_sched.h background_geometry with the Sigma-Delta kernels):
one part always; a tile is 64 * kUnrollSigmaDelta vecs of the region rows
padded to whole mask words, 64 vecs when the larger tiles would fill under
half of the wave slots (every small shape here; test_large_tiles reaches the
larger tiles)."""
import functools

import numpy as np
import pytest

import _components_ref as cref
from _background_ref import drift_clip
from _sigma_delta_ref import PARAMS, sigma_delta_fold
from test_change_mask_cpu import noise_frames, noise_ref, unpack_mask
from test_gpu_change_mask import GEOMETRY, make_op

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def want_of(c, w, h, n, roi, params, chroma=0, with_ref=False, clip="noise"):
    frames = noise_frames(c, w, h, n) if clip == "noise" else drift_clip(c, w, h, n)
    ref = noise_ref(c, w, h) if with_ref else None
    mask, state = sigma_delta_fold(frames, *params, chroma, ref, roi)
    mask.setflags(write=False)
    state.setflags(write=False)
    return mask, state


def checked_want(c, w, h, n, roi, params, chroma=0, with_ref=False, clip="noise", values=0):
    mask, state = want_of(c, w, h, n, roi, params, chroma, with_ref, clip)
    rw = w if roi is None else roi[2]
    if n > 1:
        share = unpack_mask(mask, rw)[1:].mean()
        assert 0.05 < share < 0.95, share
    assert len(np.unique(state[1])) >= values
    return mask, state


def run_sd(c, frames, roi=None, chroma=0, ref=None, params=(2, 2, 510), state=None, mode=1, tau=8 / 255, **kw):
    op = make_op(c, mode, tau, chroma, **kw)
    try:
        m, s = op.sigma_delta_mask(frames, roi=roi, ref=ref, n_amp=params[0], v_min=params[1], v_max=params[2], state=state)
    finally:
        op.close()
    assert m.width == (frames.shape[2] if roi is None else roi[2])
    return m.bits, s.state


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("chroma", [0, 1, 2, 3])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_formats_and_parameters(c, chroma):
    """c = 1 runs the generic kernel.  Every parameter set, with and without ref."""
    from dips_amd import SigmaDelta
    w, h, n = 37, 29, 9
    frames = noise_frames(c, w, h, n)
    op = make_op(c, 1, 8 / 255, 0 if c == 1 else chroma)
    try:
        for params in PARAMS:
            for with_ref in (False, True):
                want = checked_want(c, w, h, n, None, params, chroma, with_ref)
                m, s = op.sigma_delta_mask(frames, ref=noise_ref(c, w, h) if with_ref else None, n_amp=params[0],
                                           v_min=params[1], v_max=params[2])
                assert isinstance(s, SigmaDelta) and s.state.shape == (2, h, w) and s.state.dtype == np.uint16
                assert m.bits.shape == (n, h, 8) and m.width == w
                assert same((m.bits, s.state), want), (params, with_ref)
                if not with_ref:
                    assert not m.bits[0].any()  # frame 0 meets itself
    finally:
        op.close()


@pytest.mark.parametrize("w,h,roi", GEOMETRY)
@pytest.mark.parametrize("c", [3, 4])
def test_geometry(c, w, h, roi):
    n = 5
    got = run_sd(c, noise_frames(c, w, h, n), roi)
    rw, rh = (w, h) if roi is None else roi[2:]
    assert got[0].shape == (n, rh, 4 * ((rw + 31) // 32)) and got[1].shape == (2, rh, rw)
    assert same(got, checked_want(c, w, h, n, roi, (2, 2, 510)))


@pytest.mark.parametrize("w,h", [(1, 8), (2, 8), (1, 3)])
@pytest.mark.parametrize("params", [(2, 2, 510), (4, 1, 6)])
@pytest.mark.parametrize("c", [3, 4])
def test_narrow_frames(c, params, w, h):
    """Frames narrower than 3 pixels: the partial vecs of several rows would
    read past the frame's end; the generic kernel owns their words and state."""
    n = 9
    assert same(run_sd(c, noise_frames(c, w, h, n), params=params), checked_want(c, w, h, n, None, params))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7])
@pytest.mark.parametrize("c", [3, 4])
def test_ring_prologue_and_tail(c, n):
    w, h = 37, 29
    assert same(run_sd(c, noise_frames(c, w, h, n)), checked_want(c, w, h, n, None, (2, 2, 510)))


@pytest.mark.parametrize("params", [(2, 2, 510), (4, 1, 6)])
@pytest.mark.parametrize("c", [3, 4])
def test_one_wave_carries_a_long_state(c, params):
    w, h, n = 8, 8, 300
    want = checked_want(c, w, h, n, None, params, values=3)
    if params == (4, 1, 6):
        assert want[1][1].max() == 6  # V reaches v_max
    assert same(run_sd(c, noise_frames(c, w, h, n), params=params), want)


@pytest.mark.parametrize("c", [3, 4])
def test_large_tiles(c, monkeypatch):
    """The tiles of 64 * kUnrollSigmaDelta (4) vecs: taken when they fill at
    least half of the wave slots.  With DIPS_SERIES_WAVES_PER_SIMD = 1 the
    slots are 4 per CU (1024 on 256 CUs); a padded row of 1021 pixels is one
    such tile of 256 vecs, so 400 rows are under half of the slots and 520
    are not.  The ragged last vec of the frame is left to the generic
    kernel."""
    monkeypatch.setenv("DIPS_SERIES_WAVES_PER_SIMD", "1")
    w, h, n = 1021, 520, 5
    want = checked_want(c, w, h, n, None, (2, 2, 510), values=3)
    assert same(run_sd(c, noise_frames(c, w, h, n)), want)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_drift_clip(c):
    w, h, n = 37, 29, 24
    want = checked_want(c, w, h, n, None, (2, 2, 510), clip="drift", values=3)
    assert same(run_sd(c, drift_clip(c, w, h, n)), want)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_chunks_continue_the_state(c):
    """9 + 1 + 7 frames with state= equal one call of 17, mask and state."""
    w, h, n = 37, 29, 17
    frames = noise_frames(c, w, h, n)
    op = make_op(c, 1, 8 / 255)
    try:
        whole = op.sigma_delta_mask(frames)
        bits, state = [], None
        for lo, hi in ((0, 9), (9, 10), (10, 17)):
            m, state = op.sigma_delta_mask(frames[lo:hi], state=state)
            bits.append(m.bits)
        kept = state.state.copy()
        m, again = op.sigma_delta_mask(frames[:0], state=state)  # no frames: the state comes back as it is
    finally:
        op.close()
    want = checked_want(c, w, h, n, None, (2, 2, 510), values=3)
    assert same((whole[0].bits, whole[1].state), want)
    assert same((np.concatenate(bits), state.state), want)
    assert m.bits.shape == (0, h, 8) and np.array_equal(again.state, kept)


@pytest.mark.parametrize("roi", [None, (3, 2, 33, 27)])
@pytest.mark.parametrize("c", [3, 4])
def test_kernel_paths_agree(c, roi):
    """fast = generic = crosscheck = definition; params.mode and params.tau
    are not consulted."""
    w, h, n, params = 37, 29, 9, (4, 1, 6)
    frames = noise_frames(c, w, h, n)
    want = checked_want(c, w, h, n, roi, params)
    assert same(run_sd(c, frames, roi, params=params), want)
    assert same(run_sd(c, frames, roi, params=params, force_generic=True), want)
    assert same(run_sd(c, frames, roi, params=params, crosscheck=True), want)
    assert same(run_sd(c, frames, roi, params=params, mode=0), want)
    assert same(run_sd(c, frames, roi, params=params, tau=0.0), want)
    assert same(run_sd(c, frames, roi, params=params, tau=0.5, force_generic=True), want)


@pytest.mark.parametrize("roi", [None, (3, 2, 21, 17)])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_device_path_writes_every_byte(c, accumulate, roi):
    """The outputs start as 0xFF everywhere; the frames tensor starts 1 byte
    off every natural alignment; mask None gives the same state."""
    import torch
    w, h, n = 37, 29, 9
    frames = noise_frames(c, w, h, n)
    rw, rh = (w, h) if roi is None else roi[2:]
    want = checked_want(c, w, h, n, roi, (2, 2, 510))
    buf = torch.zeros(frames.nbytes + 16, dtype=torch.uint8, device="cuda")
    dev = buf[1:1 + frames.nbytes].view(frames.shape)
    dev.copy_(torch.from_numpy(frames.copy()))
    assert dev.data_ptr() % 4 == 1
    split = 4 if accumulate else 0
    op = make_op(c, 1, 8 / 255)
    try:
        out = torch.full(want[0].shape, 0xFF, dtype=torch.uint8, device="cuda")
        sd = torch.full((2, rh, rw), -1, dtype=torch.int16, device="cuda")
        alone = torch.full((2, rh, rw), -1, dtype=torch.int16, device="cuda")
        if accumulate:
            op.run_sigma_delta_mask_device(dev[:split], sd, out[:split], roi=roi)
            op.run_sigma_delta_mask_device(dev[:split], alone, None, roi=roi)
        op.run_sigma_delta_mask_device(dev[split:], sd, out[split:], roi=roi, accumulate=accumulate)
        op.run_sigma_delta_mask_device(dev[split:], alone, None, roi=roi, accumulate=accumulate)
        torch.cuda.synchronize()
        if roi is not None:
            with pytest.raises(ValueError):
                op.run_sigma_delta_mask_device(dev, sd, out)  # the whole frame's shapes are asked
    finally:
        op.close()
    assert np.array_equal(out.cpu().numpy(), want[0])
    assert np.array_equal(sd.cpu().numpy().view(np.uint16), want[1])
    assert np.array_equal(alone.cpu().numpy().view(np.uint16), want[1])


@pytest.mark.parametrize("params", [(2, 2, 510), (4, 1, 6), (15, 0, 510)])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_state_ends(c, params):
    """A continued state holding M in {0, 1, 509, 510} and V in {v_min,
    v_max} under pixels alternating 0 / 255 per frame and column: with every
    channel in, max + min of an alternating RGB pixel never moves, so the
    colour formats take the red channel alone."""
    w, h, n = 37, 29, 9
    t, x, ch = np.meshgrid(np.arange(n), np.arange(w), np.arange(c), indexing="ij")
    frames = np.broadcast_to((255 * ((t + x + ch) & 1)).astype(np.uint8)[:, None], (n, h, w, c))
    frames = np.ascontiguousarray(frames[..., 0] if c == 1 else frames)
    chroma = 0 if c == 1 else 1
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    held = np.stack([np.array([0, 1, 509, 510])[(x + y) % 4], np.where((x // 4 + y) & 1, params[1], params[2])]).astype(np.uint16)
    from dips_amd import SigmaDelta
    for st in (None, held):
        want = sigma_delta_fold(frames, *params, chroma, state=st)
        bits = unpack_mask(want[0], w)
        # M steps away from and back to its start, so a swing of 510 fires every
        # other frame; a held V of 510 is never exceeded
        assert bits[1:].mean() > 0.05 and (st is None or bits[1:].mean() < 0.95)
        got = run_sd(c, frames, chroma=chroma, params=params, state=None if st is None else SigmaDelta(st))
        assert same(got, want)
    first = sigma_delta_fold(frames[:1], *params, chroma, state=held)[1]
    assert first[0].min() <= 1 and first[0].max() >= 509


def test_initial_state_alone():
    """n_frames = 0 without accumulate writes M = J(ref), V = v_min of the region."""
    import torch
    from oracle.np_restatement import jtwin
    c, w, h, roi = 3, 37, 29, (3, 2, 21, 17)
    frames, ref = noise_frames(c, w, h, 9), noise_ref(c, w, h)
    want = np.stack([jtwin(ref[None], 0)[0][2:19, 3:24], np.full((17, 21), 5)]).astype(np.uint16)
    op = make_op(c, 1, 8 / 255)
    try:
        m, s = op.sigma_delta_mask(frames[:0], roi=roi, ref=ref, v_min=5)
        sd = torch.full((2, 17, 21), -1, dtype=torch.int16, device="cuda")
        op.run_sigma_delta_mask_device(torch.from_numpy(frames[:0].copy()).cuda(), sd, None, roi=roi,
                                       ref=torch.from_numpy(ref.copy()).cuda(), v_min=5)
        torch.cuda.synchronize()
    finally:
        op.close()
    assert m.bits.shape == (0, 17, 4) and np.array_equal(s.state, want)
    assert np.array_equal(sd.cpu().numpy().view(np.uint16), want)


def test_errors_leave_the_outputs_untouched():
    import torch
    from dips_amd import DipsError, _lib
    c, w, h, n = 3, 37, 29, 5
    frames, ref = noise_frames(c, w, h, n), noise_ref(c, w, h)
    op = make_op(c, 1, 8 / 255)
    try:
        for roi in ((30, 0, 8, 5), (0, 25, 8, 5), (3, 2, 0, 17), (3, 2, 21, 0)):
            with pytest.raises(DipsError) as e:
                op.sigma_delta_mask(frames, roi=roi)
            assert e.value.status == -1 and "diff_sigma_delta_mask:" in str(e.value)
        lib, hp = op._host._lib, op._host.ptr
        mask = np.full((n, h, 8), 0xFF, dtype=np.uint8)
        sd = np.full((2, h, w), 0xFFFF, dtype=np.uint16)
        fp, rp, mp, sp = frames.ctypes.data, ref.ctypes.data, mask.ctypes.data, sd.ctypes.data
        call = lib.dips_diff_sigma_delta_mask
        bad = [
            (hp, w, h, fp, n, None, None, 0, 2, 510, 0, sp, mp),      # n_amp
            (hp, w, h, fp, n, None, None, 16, 2, 510, 0, sp, mp),
            (hp, w, h, fp, n, None, None, 2, 3, 2, 0, sp, mp),        # v_min > v_max
            (hp, w, h, fp, n, None, None, 2, 2, 511, 0, sp, mp),      # v_max
            (hp, w, h, None, n, None, None, 2, 2, 510, 0, sp, mp),    # null frames
            (hp, w, h, fp, n, None, None, 2, 2, 510, 0, None, mp),    # null state
            (hp, w, h, fp, n, rp, None, 2, 2, 510, 1, sp, mp),        # ref while accumulating
            (hp, w, h, None, 0, None, None, 2, 2, 510, 0, sp, mp),    # nothing to start from
            (hp, 32768, 32768, fp, n, None, None, 2, 2, 510, 0, sp, mp),  # 2^30 pixels
            (None, w, h, fp, n, None, None, 2, 2, 510, 0, sp, mp),
        ]
        for args in bad:
            assert call(*args) == _lib.DIPS_ERR_INVALID, args[7:11]
        # accumulate without frames: OK, nothing is written
        assert call(hp, w, h, None, 0, None, None, 2, 2, 510, 1, sp, mp) == 0
        assert (mask == 0xFF).all() and (sd == 0xFFFF).all()
        dev = torch.from_numpy(frames.copy()).cuda()
        mbuf = torch.full((n * h * 8 + 16,), 0xFF, dtype=torch.uint8, device="cuda")
        sbuf = torch.full((2 * h * w * 2 + 16,), 0xFF, dtype=torch.uint8, device="cuda")
        good_m, good_s = mbuf[4:4 + n * h * 8].view(n, h, 8), sbuf[4:4 + 2 * h * w * 2].view(torch.int16).view(2, h, w)
        dl, dp = op._dev._lib, op._dev.ptr
        for s_off, m_off, word in ((1, 4, "2-byte aligned"), (4, 2, "4-byte aligned")):
            st = dl.dips_diff_sigma_delta_mask(dp, w, h, dev.data_ptr(), n, None, None, 2, 2, 510, 0,
                                               sbuf.data_ptr() + s_off, mbuf.data_ptr() + m_off)
            assert st == _lib.DIPS_ERR_INVALID and word in dl.dips_last_error(dp).decode()
        torch.cuda.synchronize()
        assert bool((mbuf == 0xFF).all()) and bool((sbuf == 0xFF).all())
        for shape in ((2, h, w - 1), (3, h, w), (2 * h, w)):
            with pytest.raises(ValueError):
                op.run_sigma_delta_mask_device(dev, torch.zeros(shape, dtype=torch.int16, device="cuda"), good_m)
        with pytest.raises(ValueError):
            op.run_sigma_delta_mask_device(dev, torch.zeros((2, h, w), dtype=torch.int32, device="cuda"), good_m)
        with pytest.raises(ValueError):
            op.run_sigma_delta_mask_device(dev, good_s, torch.zeros((n, h, 4), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            op.run_sigma_delta_mask_device(dev, good_s, good_m, ref=torch.from_numpy(ref.copy()).cuda(), accumulate=True)
        op.run_sigma_delta_mask_device(dev, good_s, good_m)
        torch.cuda.synchronize()
        got = op.sigma_delta_mask(frames)
    finally:
        op.close()
    want = checked_want(c, w, h, n, None, (2, 2, 510))
    assert same((got[0].bits, got[1].state), want)
    assert same((good_m.cpu().numpy(), good_s.cpu().numpy().view(np.uint16)), want)


@pytest.mark.parametrize("sigma_delta", [True, (4, 1, 6)])
@pytest.mark.parametrize("c", [3, 1])
def test_change_boxes_and_tracks_on_the_sigma_delta_mask(c, sigma_delta):
    """change_boxes / change_tracks with sigma_delta= equal sigma_delta_mask
    followed by mask_components / mask_tracks."""
    w, h, n, roi = 37, 29, 24, (2, 1, 34, 27)
    clip = drift_clip(c, w, h, n).copy()
    params = (2, 2, 510) if sigma_delta is True else sigma_delta
    op = make_op(c, 0, 8 / 255)
    try:
        for r in (None, roi):
            mask = checked_want(c, w, h, n, r, params, clip="drift")[0]
            rw = w if r is None else r[2]
            m, _ = op.sigma_delta_mask(clip, roi=r, n_amp=params[0], v_min=params[1], v_max=params[2])
            assert np.array_equal(m.bits, mask)
            got = op.change_boxes(clip, roi=r, connectivity=8, min_area=4, max_boxes=16, labels=True, sigma_delta=sigma_delta)
            ref = cref.components(mask, rw, 8, 4, 16)
            assert ref[0].any()
            assert all(np.array_equal(g, x) for g, x in zip((got.counts, got.boxes, got.labels), ref))
            two = op.mask_components(m, connectivity=8, min_area=4, max_boxes=16, labels=True)
            assert all(np.array_equal(g, x) for g, x in zip((two.counts, two.boxes, two.labels), ref))
            tracks = op.change_tracks(clip, roi=r, connectivity=8, min_area=4, max_boxes=16, sigma_delta=sigma_delta)
            staged = op.mask_tracks(m, connectivity=8, min_area=4, max_boxes=16)
            for f in ("counts", "boxes", "links"):
                assert np.array_equal(getattr(tracks, f), getattr(staged, f)), f
            assert np.array_equal(tracks.counts, ref[0])
        with pytest.raises(ValueError):
            op.change_boxes(clip, sigma_delta=(0, 2, 510))
        with pytest.raises(ValueError):
            op.change_tracks(clip, sigma_delta=True, background=3)
    finally:
        op.close()


def test_kernel_time_records_the_launch():
    import torch
    frames = torch.from_numpy(noise_frames(3, 96, 64, 5).copy()).cuda()
    out = torch.zeros((5, 64, 12), dtype=torch.uint8, device="cuda")
    sd = torch.zeros((2, 64, 96), dtype=torch.int16, device="cuda")
    op = make_op(3, 1, 8 / 255, time_kernel=True)
    try:
        op.run_sigma_delta_mask_device(frames, sd, out)
        op.run_sigma_delta_mask_device(frames, sd, out, accumulate=True)
        ms, launches = op.kernel_time()
    finally:
        op.close()
    assert launches == 2 and ms > 0.0
