"""The expectation of dips_diff_change_mask, without a GPU.

The authoritative bit of frame t and pixel (x, y) is the count field of the C
oracle's series of the frames (and the reference) cropped to that single pixel
(oracle_change_mask): one call of the oracle per pixel.  The GPU tests with
more than a few thousand pixels use py_change_mask, the vectorised twin built
from oracle.np_restatement's intensity the way py_pixel_sums is.  This file
shows the two equal, and the mask consistent with the per-pixel sums.

Layout (include/dips_hip.h): a row is 4 * ceil(w / 32) bytes, bit i of a row
is bit (i & 7) of byte (i >> 3), pad bits 0.

Inputs: uniform random bytes set almost every bit at any tau and would hide a
broken layout or compare, so the frames are a random base frame plus per-frame
uniform integer noise in [-12, 12], clipped to bytes.  Every tau > 0 case
asserts that the oracle's mask has 20-80 % of its bits set, every tau = 0 case
that it has both zeros and ones."""
import functools

import numpy as np
import pytest

from oracle import np_restatement as npr
from oracle import oracle
from test_pixel_sums_cpu import oracle_pixel_sums

F32 = np.float32
TAUS = {0: 0.0, 4: 4 / 255, 8: 8 / 255}  # 4/255 < 2^-5 <= 8/255: both sides of the series' integer-sum switch


def pack_mask(bits):
    """bool [n, h, w] -> uint8 [n, h, 4 * ceil(w / 32)], LSB first, pad bits 0."""
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    padded = np.zeros((n, h, 32 * ((w + 31) // 32)), dtype=np.uint8)
    padded[..., :w] = bits
    return np.packbits(padded, axis=-1, bitorder="little")


def unpack_mask(mask, w):
    return np.unpackbits(mask, axis=-1, bitorder="little")[..., :w].astype(bool)


def oracle_change_mask(frames, mode=0, tau=0.0, chroma=0, ref=None, roi=None):
    """The definition: per pixel of roi the count column of the oracle's series of the 1x1 crop."""
    frames = np.asarray(frames, dtype=np.uint8)
    n, h, w = frames.shape[:3]
    x0, y0, rw, rh = roi if roi is not None else (0, 0, w, h)
    bits = np.zeros((n, rh, rw), dtype=bool)
    for y in range(rh):
        for x in range(rw):
            py, px = y0 + y, x0 + x
            crop_ref = None if ref is None else np.ascontiguousarray(ref[py:py + 1, px:px + 1])
            cnt = oracle.series(np.ascontiguousarray(frames[:, py:py + 1, px:px + 1]), mode=mode, tau=tau,
                                chroma=chroma, ref=crop_ref)[0][:, 2]
            assert cnt.max(initial=0) <= 1
            bits[:, y, x] = cnt != 0
    return pack_mask(bits)


def py_change_mask(frames, mode=0, tau=0.0, chroma=0, ref=None, roi=None):
    """The vectorised twin: |dI| > tau on np_restatement's intensity, packed."""
    frames = np.asarray(frames, dtype=np.uint8)
    n, h, w = frames.shape[:3]
    x0, y0, rw, rh = roi if roi is not None else (0, 0, w, h)
    if n == 0:
        return np.zeros((0, rh, 4 * ((rw + 31) // 32)), dtype=np.uint8)
    first = frames[0] if ref is None else np.asarray(ref, dtype=np.uint8).reshape(frames.shape[1:])
    if mode == 0:
        refs = np.broadcast_to(first[None], frames.shape)
    else:
        refs = np.concatenate([first[None], frames[:-1]], axis=0)
    dI = np.abs((npr.intensity(frames, chroma) - npr.intensity(refs, chroma)).astype(F32))
    return pack_mask((dI > F32(tau))[:, y0:y0 + rh, x0:x0 + rw])


def _base_frame(c, w, h):
    shape = (h, w) if c == 1 else (h, w, c)
    return np.random.default_rng([11, c, w, h]).integers(0, 256, shape, dtype=np.int16)


def _noisy(base, rng, n):
    a = np.clip(base[None] + rng.integers(-12, 13, (n,) + base.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def noise_frames(c, w, h, n):
    """A random base frame plus per-frame uniform integer noise in [-12, 12], clipped to bytes."""
    return _noisy(_base_frame(c, w, h), np.random.default_rng([12, c, w, h, n]), n)


@functools.lru_cache(maxsize=None)
def noise_ref(c, w, h):
    """A reference: the base frame of noise_frames(c, w, h, *) under noise of its own."""
    return _noisy(_base_frame(c, w, h), np.random.default_rng([13, c, w, h]), 1)[0]


def check_share(mask, w, tau_k, first=0):
    """The oracle's mask is informative: 20-80 % set at tau > 0, zeros and ones at tau = 0
    (frames from `first` on: frame 0 of a call without a reference meets itself)."""
    bits = unpack_mask(mask, w)[first:]
    if tau_k:
        assert 0.2 < bits.mean() < 0.8, bits.mean()
    else:
        assert bits.any() and not bits.all()


@pytest.mark.parametrize("tau_k", [0, 4, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_restatement_equals_oracle_crops(c, mode, tau_k):
    w, h, n = 37, 29, 9
    frames = noise_frames(c, w, h, n)
    want = oracle_change_mask(frames, mode, TAUS[tau_k])
    assert want.shape == (n, h, 8) and want.dtype == np.uint8
    check_share(want, w, tau_k, first=1)
    assert not want[0].any()  # frame 0 against itself: the compare is strict
    assert not unpack_mask(want, 64)[..., w:].any()  # pad bits
    assert np.array_equal(py_change_mask(frames, mode, TAUS[tau_k]), want)


@pytest.mark.parametrize("mode", [0, 1])
def test_restatement_with_reference_chroma_and_roi(mode):
    w, h, n = 37, 29, 9
    frames, ref = noise_frames(3, w, h, n), noise_ref(3, w, h)
    want = oracle_change_mask(frames, mode, 8 / 255, 0, ref)
    check_share(want, w, 8)
    assert np.array_equal(py_change_mask(frames, mode, 8 / 255, 0, ref), want)
    want = oracle_change_mask(frames, mode, 8 / 255, 2)
    check_share(want, w, 8, first=1)
    assert np.array_equal(py_change_mask(frames, mode, 8 / 255, 2), want)
    roi = (3, 2, 21, 17)
    want = oracle_change_mask(frames, mode, 4 / 255, 0, None, roi)
    check_share(want, roi[2], 4, first=1)
    assert np.array_equal(py_change_mask(frames, mode, 4 / 255, 0, None, roi), want)
    assert np.array_equal(unpack_mask(want, 21), unpack_mask(oracle_change_mask(frames, mode, 4 / 255), w)[:, 2:19, 3:24])


@pytest.mark.parametrize("tau_k", [0, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_mask_summed_over_time_is_the_pixel_sums_count(c, mode, tau_k):
    w, h, n = 37, 29, 9
    frames = noise_frames(c, w, h, n)
    bits = unpack_mask(oracle_change_mask(frames, mode, TAUS[tau_k]), w)
    assert np.array_equal(bits.sum(axis=0, dtype=np.uint64), oracle_pixel_sums(frames, mode, TAUS[tau_k])[..., 2])


def test_unchanged_pixels_stay_zero_at_tau_zero():
    frames = noise_frames(3, 37, 29, 9).copy()
    frames[:, 5, 7] = frames[0, 5, 7]
    bits = unpack_mask(oracle_change_mask(frames, 1, 0.0), 37)
    assert not bits[:, 5, 7].any() and bits[1:].mean() > 0.9


def test_library_and_package_expose_the_call():
    """Fails without the feature: the symbols, their bindings and the result type."""
    import dips_amd
    from dips_amd import _lib
    lib = _lib.load()
    assert len(lib.dips_diff_change_mask.argtypes) == 8
    assert {"dips_diff_change_mask", "dips_mask_row_bytes"} <= set(_lib.header_functions())
    for w, want in ((1, 4), (31, 4), (32, 4), (33, 8), (64, 8)):
        assert lib.dips_mask_row_bytes(w) == want == dips_amd.mask_row_bytes(w)
    bits = np.array([[True, False, True] + [False] * 30 + [True]])[None]  # [1, 1, 34]
    m = dips_amd.ChangeMask.from_array(pack_mask(bits), 34)
    assert m.bits.shape == (1, 1, 8) and m.bits[0, 0, 0] == 0b101 and m.bits[0, 0, 4] == 0b10
    assert np.array_equal(m.unpack(), bits) and m.unpack().dtype == bool
    assert np.array_equal(m.counts(), np.array([3], dtype=np.uint64))
    with pytest.raises(ValueError):
        dips_amd.ChangeMask.from_array(np.zeros((1, 1, 4), dtype=np.uint8), 34)
    assert hasattr(dips_amd.DiffSeriesOperator, "change_mask")
    assert hasattr(dips_amd.DiffSeriesOperator, "run_change_mask_device")
