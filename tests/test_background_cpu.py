"""The expectation of dips_diff_background_mask, without a GPU: the integer
recurrence's properties, the selective semantics, the vectorised fold
(tests/_background_ref.py with py_change_mask) against the fold over the C
oracle's per-pixel crops, and the exposure of the call through every layer."""
import os
import re

import numpy as np
import pytest

from _background_ref import background_fold, drift_clip, reference_bytes, update
from test_change_mask_cpu import TAUS, noise_frames, noise_ref, oracle_change_mask, py_change_mask, unpack_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", range(9))
def test_recurrence_range_and_fixed_point(k):
    F = np.arange(256, dtype=np.int64)[None, :]
    B = np.unique(np.concatenate([np.arange(0, 65281, 53), np.arange(0, 64), np.arange(65280 - 63, 65281)]))[:, None]
    nb = update(np.broadcast_to(B, (B.shape[0], 256)), np.broadcast_to(F, (B.shape[0], 256)), k)
    assert nb.min() >= 0 and nb.max() <= 65280
    assert np.array_equal(update(256 * F, F, k), 256 * F)  # B = 256 F stays
    if k == 0:
        assert np.array_equal(nb, np.broadcast_to(256 * F, nb.shape))


@pytest.mark.parametrize("k", range(9))
def test_static_input_settles_on_the_frame(k):
    """From both ends of the range B comes within 2^(k-1) of 256 F, so the
    reference bytes settle on F exactly."""
    F = np.arange(256, dtype=np.int64)
    for start in (0, 65280):
        B = np.full(256, start, dtype=np.int64)
        for _ in range(16 << k):
            B = update(B, F, k)
        assert np.abs(B - 256 * F).max() <= ((1 << k) >> 1)
        assert np.array_equal(reference_bytes(B), F)
        assert np.array_equal(update(B, F, k), B) or k > 0  # k = 0 reaches 256 F in one step


@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_rate_shift_zero_is_the_per_frame_mask(c, with_ref):
    w, h, n = 37, 29, 9
    frames = noise_frames(c, w, h, n)
    ref = noise_ref(c, w, h) if with_ref else None
    want = oracle_change_mask(frames, 1, 8 / 255, 0, ref)
    assert 0.05 < unpack_mask(want, w)[1:].mean() < 0.95
    mask, state = background_fold(frames, 0, False, 8 / 255, 0, ref)
    assert np.array_equal(mask, want)
    last = frames[-1][None] if c == 1 else np.moveaxis(frames[-1], -1, 0)
    assert np.array_equal(state, 256 * last.astype(np.uint16))


def test_selective_semantics_by_hand():
    """One RGB pixel, k = 1, tau = 8/255: background 100; a frame at 200 is
    foreground (kept out when selective, half absorbed otherwise); a frame at
    104 is not (absorbed either way)."""
    px = lambda v: np.full((1, 1, 3), v, dtype=np.uint8)  # noqa: E731
    frames = np.stack([px(200), px(104), px(104)])
    ref = px(100)
    mask, state = background_fold(frames, 1, True, 8 / 255, 0, ref)
    assert [int(m) for m in mask[:, 0, 0]] == [1, 0, 0]
    # 25600 kept; then 25600 -> 26112 (R = 102) -> 26368
    assert state.tolist() == [[[26368]]] * 3
    mask, state = background_fold(frames, 1, False, 8 / 255, 0, ref)
    # 25600 -> 38400 (R = 150: 104 is now foreground) -> 32512 (R = 127) -> 29568
    assert [int(m) for m in mask[:, 0, 0]] == [1, 1, 1]
    assert state.tolist() == [[[29568]]] * 3
    # selective keeps a changed pixel whole: every channel, although only one moved
    one = np.array([[[200, 100, 100]]], dtype=np.uint8)[None]
    mask, state = background_fold(one, 1, True, 8 / 255, 0, ref)
    assert mask[0, 0, 0] == 1 and state.reshape(-1).tolist() == [25600] * 3
    mask, state = background_fold(one, 1, False, 8 / 255, 0, ref)
    assert state.reshape(-1).tolist() == [38400, 25600, 25600]


@pytest.mark.parametrize("k,selective,tau_k,chroma", [(3, False, 8, 0), (1, True, 4, 0), (2, True, 8, 2), (8, False, 0, 0)])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_vectorised_fold_equals_oracle_crops(c, k, selective, tau_k, chroma):
    if c == 1:
        chroma = 0
    w, h, n = 37, 29, 9
    frames = noise_frames(c, w, h, n)
    want_mask, want_state = background_fold(frames, k, selective, TAUS[tau_k], chroma, mask_fn=oracle_change_mask)
    got_mask, got_state = background_fold(frames, k, selective, TAUS[tau_k], chroma, mask_fn=py_change_mask)
    assert want_state.shape == (c, h, w) and want_state.dtype == np.uint16
    assert want_mask.shape == (n, h, 8) and not want_mask[0].any()
    if tau_k:
        assert 0.05 < unpack_mask(want_mask, w)[1:].mean() < 0.95
    assert np.array_equal(got_mask, want_mask) and np.array_equal(got_state, want_state)


def test_fold_with_reference_roi_and_chunks():
    w, h, n, roi = 37, 29, 9, (3, 2, 21, 17)
    frames, ref = noise_frames(3, w, h, n), noise_ref(3, w, h)
    whole_mask, whole_state = background_fold(frames, 3, True, 8 / 255, 0, ref)
    part_mask, part_state = background_fold(frames, 3, True, 8 / 255, 0, ref, roi)
    assert np.array_equal(unpack_mask(part_mask, 21), unpack_mask(whole_mask, w)[:, 2:19, 3:24])
    assert np.array_equal(part_state, whole_state[:, 2:19, 3:24])
    a_mask, a_state = background_fold(frames[:4], 3, True, 8 / 255, 0, ref)
    b_mask, b_state = background_fold(frames[4:], 3, True, 8 / 255, 0, state=a_state)
    assert np.array_equal(np.concatenate([a_mask, b_mask]), whole_mask) and np.array_equal(b_state, whole_state)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_drift_clip_separates_the_three_references(k):
    """On the drift-and-moving-square clip the adaptive reference decides
    differently from both fixed ones in at least 5 % of the bits."""
    clip = drift_clip()
    w = clip.shape[2]
    bits = unpack_mask(background_fold(clip, k, False, 8 / 255)[0], w)[1:]
    assert 0.05 < bits.mean() < 0.95
    for mode in (0, 1):
        other = unpack_mask(py_change_mask(clip, mode, 8 / 255), w)[1:]
        assert (bits != other).mean() >= 0.05, (mode, (bits != other).mean())


def test_every_layer_exposes_the_call():
    """Fails without the feature: the header's declaration, the binding and
    its argument types, the Rust extern block, the result type and the
    operator's methods."""
    import ctypes
    import inspect
    import dips_amd
    from dips_amd import _lib
    assert "dips_diff_background_mask" in _lib.header_functions()
    hdr = open(os.path.join(ROOT, "include", "dips_hip.h")).read()
    assert re.search(r"#define DIPS_BG_SELECTIVE 1u\b", hdr) and "#define DIPS_ABI_VERSION 3" in hdr
    decl = re.search(r"dips_status dips_diff_background_mask\(([^)]*)\);", hdr).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "width", "height", "frames", "n_frames", "ref", "roi", "rate_shift", "bg_flags", "accumulate", "background",
        "mask"]
    assert "uint16_t *background" in decl
    lib = _lib.load()
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    assert lib.dips_diff_background_mask.argtypes == [vp, u32, u32, vp, u32, vp, ctypes.POINTER(u32), u32, u32, u32, vp, vp]
    assert lib.dips_diff_background_mask.restype == ctypes.c_int
    assert _lib.BG_SELECTIVE == 1 and _lib.BG_MAX_RATE_SHIFT == 8
    ffi = open(os.path.join(ROOT, "rust", "dips-hip", "src", "ffi.rs")).read()
    assert re.search(r"pub fn dips_diff_background_mask\(h: \*mut DipsHandle,[^;]*background: \*mut u16, mask: \*mut u8\) "
                     r"-> DipsStatus;", ffi, flags=re.S)
    assert "pub const DIPS_BG_SELECTIVE: u32 = 1;" in ffi
    state = np.arange(2 * 3 * 4, dtype=np.uint16).reshape(3, 2, 4) * 100 + 77
    bg = dips_amd.Background.from_array(state)
    assert bg.state.dtype == np.uint16 and np.array_equal(bg.state, state)
    img = bg.image()
    assert img.shape == (2, 4, 3) and img.dtype == np.uint8 and img.flags.c_contiguous
    assert np.array_equal(img, np.moveaxis((state.astype(np.uint32) + 128) >> 8, 0, -1))
    assert dips_amd.Background(np.full((1, 1, 1), 65280, dtype=np.uint16)).image()[0, 0, 0] == 255
    for bad in (np.zeros((2, 4), dtype=np.uint16), np.zeros((2, 2, 4), dtype=np.uint16)):
        with pytest.raises(ValueError):
            dips_amd.Background.from_array(bad)
    op = dips_amd.DiffSeriesOperator
    sig = inspect.signature(op.background_mask)
    assert list(sig.parameters)[1:] == ["frames", "roi", "ref", "rate_shift", "selective", "state"]
    assert sig.parameters["rate_shift"].default == 3 and sig.parameters["selective"].default is False
    assert hasattr(op, "run_background_mask_device")
    assert inspect.signature(op.change_boxes).parameters["background"].default is None


def test_python_side_argument_errors():
    """Refused before any library call (no device is touched)."""
    from dips_amd.api import Background, DiffSeriesOperator, _background_args
    for bad in (-1, 9, 2.5, True, "3"):
        with pytest.raises((ValueError, TypeError)):
            _background_args(bad, False)
    assert _background_args(0, False) == (0, 0) and _background_args(8, True) == (8, 1)
    assert _background_args(np.int64(3), 1) == (3, 1)
    frames = noise_frames(3, 37, 29, 9)
    op = DiffSeriesOperator.__new__(DiffSeriesOperator)  # no handle: every check below comes first
    from dips_amd import PixelFormat
    op.fmt = PixelFormat.RGB8
    good = Background(np.zeros((3, 29, 37), dtype=np.uint16))
    for kw in (dict(rate_shift=9), dict(rate_shift=-1), dict(state=good, ref=frames[0]),
               dict(state=Background(np.zeros((3, 29, 36), dtype=np.uint16))),
               dict(state=Background(np.zeros((4, 29, 37), dtype=np.uint16))), dict(state=np.zeros((3, 29, 37), dtype=np.uint16)),
               dict(ref=frames[0, :5]), dict(roi=(1, 2, 3))):
        with pytest.raises(ValueError):
            op.background_mask(frames, **kw)
    with pytest.raises(ValueError):
        op.background_mask(frames[:0])  # no frame and no ref: nothing to start from
