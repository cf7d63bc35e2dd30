"""The expectation of dips_diff_sigma_delta_mask, without a GPU: the numpy
fold of tests/_sigma_delta_ref.py against a scalar per-pixel loop written
separately from it, the ranges of the state, chunks, and the exposure of the
call through every layer."""
import os
import re

import numpy as np
import pytest

from _background_ref import drift_clip
from _sigma_delta_ref import PARAMS, sigma_delta_fold, step
from test_change_mask_cpu import noise_frames, noise_ref, unpack_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scalar_fold(frames, n_amp, v_min, v_max, chroma=0, ref=None, state=None):
    """The definition pixel by pixel in plain Python integers."""
    n, h, w = frames.shape[:3]
    gray = frames.ndim == 3

    def J(px):
        if gray:
            return 2 * int(px)
        r, g, b = int(px[0]), int(px[1]), int(px[2])
        return 2 * (r, g, b)[chroma - 1] if chroma else max(r, g, b) + min(r, g, b)

    bits = np.zeros((n, h, w), dtype=bool)
    out = np.zeros((2, h, w), dtype=np.uint16)
    first = frames[0] if ref is None else ref
    for y in range(h):
        for x in range(w):
            if state is not None:
                M, V = int(state[0, y, x]), int(state[1, y, x])
            else:
                M, V = J(first[y, x]), v_min
            for t in range(n):
                j = J(frames[t, y, x])
                if j > M:
                    M += 1
                elif j < M:
                    M -= 1
                d = abs(j - M)
                if d:
                    if n_amp * d > V:
                        V += 1
                    elif n_amp * d < V:
                        V -= 1
                    V = min(max(V, v_min), v_max)
                bits[t, y, x] = d > V
            out[0, y, x], out[1, y, x] = M, V
    return bits, out


@pytest.mark.parametrize("chroma", [0, 1, 2, 3])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_numpy_fold_equals_the_scalar_loop(c, chroma):
    w, h, n = 8, 8, 24
    frames = noise_frames(c, w, h, n)
    for i, (n_amp, v_min, v_max) in enumerate(PARAMS):
        ref = noise_ref(c, w, h) if i & 1 else None
        mask, state = sigma_delta_fold(frames, n_amp, v_min, v_max, chroma, ref)
        bits, want_state = scalar_fold(frames, n_amp, v_min, v_max, 0 if c == 1 else chroma, ref)
        assert mask.shape == (n, h, 4) and state.shape == (2, h, w) and state.dtype == np.uint16
        assert np.array_equal(unpack_mask(mask, w), bits) and np.array_equal(state, want_state)
        assert not mask[:, :, 1:].any()  # pad bits
        if ref is None:
            assert not mask[0].any()  # frame 0 meets itself


@pytest.mark.parametrize("n_amp,v_min,v_max", PARAMS)
def test_state_stays_in_range(n_amp, v_min, v_max):
    """Every (M, J) pair, V at and next to both ends: M in [0, 510], V in
    [v_min, v_max]; a hand-made state at the ends under extreme frames."""
    M, J = np.meshgrid(np.arange(511), np.arange(0, 511), indexing="ij")
    for V0 in {v_min, min(v_min + 1, v_max), max(v_max - 1, v_min), v_max}:
        m, v, _ = step(M, np.full(M.shape, V0), J, n_amp, v_min, v_max)
        assert m.min() >= 0 and m.max() <= 510 and v.min() >= v_min and v.max() <= v_max
        assert np.abs(m - M).max() <= 1 and np.abs(v - V0).max() <= 1
    t, x = np.meshgrid(np.arange(6), np.arange(8), indexing="ij")
    frames = np.ascontiguousarray(np.broadcast_to((255 * ((t + x) & 1)).astype(np.uint8)[:, None, :, None], (6, 2, 8, 3)))
    held = np.stack([np.array([[0, 1, 509, 510] * 2] * 2), np.array([[v_min] * 4 + [v_max] * 4] * 2)]).astype(np.uint16)
    _, state = sigma_delta_fold(frames, n_amp, v_min, v_max, 1, state=held)
    assert state[0].max() <= 510 and v_min <= state[1].min() and state[1].max() <= v_max


@pytest.mark.parametrize("c", [1, 3, 4])
def test_chunks_continue_the_state(c):
    w, h, n = 8, 8, 24
    frames = noise_frames(c, w, h, n)
    whole = sigma_delta_fold(frames, 2, 2, 510)
    a_mask, a_state = sigma_delta_fold(frames[:7], 2, 2, 510)
    b_mask, b_state = sigma_delta_fold(frames[7:], 2, 2, 510, state=a_state)
    assert np.array_equal(np.concatenate([a_mask, b_mask]), whole[0]) and np.array_equal(b_state, whole[1])


def test_roi_is_the_crop():
    w, h, n, roi = 37, 29, 9, (3, 2, 21, 17)
    frames, ref = noise_frames(3, w, h, n), noise_ref(3, w, h)
    whole = sigma_delta_fold(frames, 2, 2, 510, 0, ref)
    part = sigma_delta_fold(frames, 2, 2, 510, 0, ref, roi)
    assert np.array_equal(unpack_mask(part[0], 21), unpack_mask(whole[0], w)[:, 2:19, 3:24])
    assert np.array_equal(part[1], whole[1][:, 2:19, 3:24])


def test_informative_inputs():
    """The shares the GPU tests rely on, on the definition alone."""
    for c in (1, 3, 4):
        for p in PARAMS:
            share = unpack_mask(sigma_delta_fold(noise_frames(c, 37, 29, 9), *p)[0], 37)[1:].mean()
            assert 0.05 < share < 0.95, (c, p, share)
        clip = drift_clip(c, 37, 29, 24)
        share = unpack_mask(sigma_delta_fold(clip, 2, 2, 510)[0], 37)[1:].mean()
        assert 0.05 < share < 0.95, (c, share)
    for p in ((2, 2, 510), (4, 1, 6)):
        mask, state = sigma_delta_fold(noise_frames(3, 8, 8, 300), *p)
        assert 0.05 < unpack_mask(mask, 8)[1:].mean() < 0.95
        assert len(np.unique(state[1])) >= 3
    assert sigma_delta_fold(noise_frames(3, 8, 8, 300), 4, 1, 6)[1][1].max() == 6


def test_every_layer_exposes_the_call():
    """Fails without the feature: the header's declaration, the binding and
    its argument types, the Rust extern block, the result type and the
    operator's methods."""
    import ctypes
    import inspect
    import dips_amd
    from dips_amd import _lib
    assert "dips_diff_sigma_delta_mask" in _lib.header_functions()
    hdr = open(os.path.join(ROOT, "include", "dips_hip.h")).read()
    for name, val in (("DIPS_SD_MAX_AMP", 15), ("DIPS_SD_MAX_V", 510), ("DIPS_SD_PLANES", 2)):
        assert re.search(rf"#define {name} {val}u\b", hdr)
    decl = re.search(r"dips_status dips_diff_sigma_delta_mask\(([^)]*)\);", hdr).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "width", "height", "frames", "n_frames", "ref", "roi", "n_amp", "v_min", "v_max", "accumulate", "state", "mask"]
    assert "uint16_t *state" in decl
    lib = _lib.load()
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    assert lib.dips_diff_sigma_delta_mask.argtypes == [vp, u32, u32, vp, u32, vp, ctypes.POINTER(u32), u32, u32, u32, u32, vp, vp]
    assert lib.dips_diff_sigma_delta_mask.restype == ctypes.c_int
    assert (_lib.SD_MAX_AMP, _lib.SD_MAX_V, _lib.SD_PLANES) == (15, 510, 2)
    ffi = open(os.path.join(ROOT, "rust", "dips-hip", "src", "ffi.rs")).read()
    assert re.search(r"pub fn dips_diff_sigma_delta_mask\(h: \*mut DipsHandle,[^;]*n_amp: u32, v_min: u32, v_max: u32,\s*"
                     r"accumulate: u32, state: \*mut u16, mask: \*mut u8\) -> DipsStatus;", ffi, flags=re.S)
    for line in ("pub const DIPS_SD_MAX_AMP: u32 = 15;", "pub const DIPS_SD_MAX_V: u32 = 510;", "pub const DIPS_SD_PLANES: u32 = 2;"):
        assert line in ffi
    state = np.arange(2 * 2 * 4, dtype=np.uint16).reshape(2, 2, 4) * 30 + 7
    sd = dips_amd.SigmaDelta.from_array(state)
    assert sd.state.dtype == np.uint16 and np.array_equal(sd.state, state)
    assert np.array_equal(sd.median, state[0]) and np.array_equal(sd.threshold, state[1])
    for bad in (np.zeros((2, 4), dtype=np.uint16), np.zeros((3, 2, 4), dtype=np.uint16)):
        with pytest.raises(ValueError):
            dips_amd.SigmaDelta.from_array(bad)
    op = dips_amd.DiffSeriesOperator
    sig = inspect.signature(op.sigma_delta_mask)
    assert list(sig.parameters)[1:] == ["frames", "roi", "ref", "n_amp", "v_min", "v_max", "state"]
    assert [sig.parameters[k].default for k in ("n_amp", "v_min", "v_max")] == [2, 2, 510]
    sig = inspect.signature(op.run_sigma_delta_mask_device)
    assert list(sig.parameters)[1:] == ["frames", "state", "mask_out", "roi", "ref", "n_amp", "v_min", "v_max", "accumulate", "stream"]
    for f in (op.change_boxes, op.change_tracks):
        assert inspect.signature(f).parameters["sigma_delta"].default is None


def test_python_side_argument_errors():
    """Refused before any library call (no device is touched)."""
    from dips_amd import PixelFormat
    from dips_amd.api import DiffSeriesOperator, SigmaDelta, _sigma_delta_args, _sigma_delta_option
    for bad in ((0, 2, 510), (16, 2, 510), (2, 3, 2), (2, 2, 511), (2, -1, 5), (2.5, 2, 510), (True, 2, 510), ("2", 2, 510)):
        with pytest.raises((ValueError, TypeError)):
            _sigma_delta_args(*bad)
    assert _sigma_delta_args(np.int64(15), 0, 510) == (15, 0, 510) and _sigma_delta_args(3, 7, 7) == (3, 7, 7)
    assert _sigma_delta_option(True) == (2, 2, 510) and _sigma_delta_option((4, 1, 6)) == (4, 1, 6)
    for bad in (False, 2, (2, 2), (0, 2, 510)):
        with pytest.raises(ValueError):
            _sigma_delta_option(bad)
    frames = noise_frames(3, 37, 29, 9)
    op = DiffSeriesOperator.__new__(DiffSeriesOperator)  # no handle: every check below comes first
    op.fmt = PixelFormat.RGB8
    good = SigmaDelta(np.zeros((2, 29, 37), dtype=np.uint16))
    for kw in (dict(n_amp=0), dict(n_amp=16), dict(v_min=5, v_max=4), dict(v_max=511), dict(state=good, ref=frames[0]),
               dict(state=SigmaDelta(np.zeros((2, 29, 36), dtype=np.uint16))),
               dict(state=SigmaDelta(np.zeros((3, 29, 37), dtype=np.uint16))), dict(state=np.zeros((2, 29, 37), dtype=np.uint16)),
               dict(ref=frames[0, :5]), dict(roi=(1, 2, 3))):
        with pytest.raises(ValueError):
            op.sigma_delta_mask(frames, **kw)
    with pytest.raises(ValueError):
        op.sigma_delta_mask(frames[:0])  # no frame and no ref: nothing to start from
    for f in (op.change_boxes, op.change_tracks):
        with pytest.raises(ValueError):
            f(frames, sigma_delta=True, background=3)
