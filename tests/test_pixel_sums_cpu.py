"""The expectation of dips_diff_pixel_sums, without a GPU.

The authoritative value of pixel (x, y) is the C oracle's series of the frames
(and the reference) cropped to that single pixel, summed over the frames
(oracle_pixel_sums).  That costs a call of the oracle per pixel, so the GPU
tests with more than a few thousand pixels use py_pixel_sums, a vectorised
restatement built from oracle.np_restatement's intensity and jtwin the way
np_restatement.series is built, summing over the frames instead of over the
pixels.  This file shows the two equal."""
import functools

import numpy as np
import pytest

from oracle import np_restatement as npr
from oracle import oracle

F32 = np.float32


def py_pixel_sums(frames, mode=0, tau=0.0, chroma=0, ref=None):
    """[H, W, 4] uint64: per pixel the sums over t of SAD, SJ, count, SI_fixed."""
    frames = np.asarray(frames, dtype=np.uint8)
    h, w = frames.shape[1:3]
    if frames.shape[0] == 0:
        return np.zeros((h, w, 4), dtype=np.uint64)
    first = frames[0] if ref is None else np.asarray(ref, dtype=np.uint8).reshape(frames.shape[1:])
    if mode == 0:
        refs = np.broadcast_to(first[None], frames.shape)
    else:
        refs = np.concatenate([first[None], frames[:-1]], axis=0)
    d = np.abs(frames.astype(np.int16) - refs.astype(np.int16)).astype(np.uint64)
    sad = (d if frames.ndim == 3 else d.sum(axis=3)).sum(axis=0)
    sj = np.abs(npr.jtwin(frames, chroma) - npr.jtwin(refs, chroma)).sum(axis=0)
    dI = np.abs((npr.intensity(frames, chroma) - npr.intensity(refs, chroma)).astype(F32))
    sel = dI > F32(tau)
    cnt = sel.sum(axis=0)
    sif = np.where(sel, np.ldexp(dI.astype(np.float64), 32), 0.0).astype(np.uint64).sum(axis=0, dtype=np.uint64)
    return np.stack([sad.astype(np.uint64), sj.astype(np.uint64), cnt.astype(np.uint64), sif], axis=-1)


def oracle_pixel_sums(frames, mode=0, tau=0.0, chroma=0, ref=None, roi=None):
    """The definition: per pixel of roi the oracle's series of the 1x1 crop, summed over t."""
    frames = np.asarray(frames, dtype=np.uint8)
    h, w = frames.shape[1:3]
    x0, y0, rw, rh = roi if roi is not None else (0, 0, w, h)
    want = np.zeros((rh, rw, 4), dtype=np.uint64)
    for y in range(rh):
        for x in range(rw):
            py, px = y0 + y, x0 + x
            crop_ref = None if ref is None else np.ascontiguousarray(ref[py:py + 1, px:px + 1])
            want[y, x] = oracle.series(np.ascontiguousarray(frames[:, py:py + 1, px:px + 1]), mode=mode, tau=tau,
                                       chroma=chroma, ref=crop_ref)[0].sum(axis=0, dtype=np.uint64)
    return want


@functools.lru_cache(maxsize=None)
def _frames(c, w=37, h=29, n=9):
    shape = (n, h, w) if c == 1 else (n, h, w, c)
    a = np.random.default_rng([5, c, w, h, n]).integers(0, 256, shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("tau", [0.0, 4 / 255, 8 / 255])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_restatement_equals_oracle_crops(c, mode, tau):
    frames = _frames(c)
    got = py_pixel_sums(frames, mode, tau)
    assert got.shape == (29, 37, 4) and got.dtype == np.uint64
    assert np.array_equal(got, oracle_pixel_sums(frames, mode, tau))


@pytest.mark.parametrize("mode", [0, 1])
def test_restatement_with_reference_and_chroma(mode):
    frames = _frames(3)
    ref = np.random.default_rng(9).integers(0, 256, frames.shape[1:], dtype=np.uint8)
    assert np.array_equal(py_pixel_sums(frames, mode, 8 / 255, 0, ref), oracle_pixel_sums(frames, mode, 8 / 255, 0, ref))
    assert np.array_equal(py_pixel_sums(frames, mode, 8 / 255, 2), oracle_pixel_sums(frames, mode, 8 / 255, 2))


@pytest.mark.parametrize("tau", [0.0, 8 / 255])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_sum_over_pixels_is_the_series_summed_over_frames(c, mode, tau):
    frames = _frames(c)
    whole = oracle.series(frames, mode=mode, tau=tau)[0].sum(axis=0, dtype=np.uint64)
    assert np.array_equal(py_pixel_sums(frames, mode, tau).sum(axis=(0, 1), dtype=np.uint64), whole)


def test_library_and_package_expose_the_call():
    """Fails without the feature: the symbol, its binding and the result type."""
    import dips_amd
    from dips_amd import _lib
    lib = _lib.load()
    assert lib.dips_diff_pixel_sums.argtypes is not None and len(lib.dips_diff_pixel_sums.argtypes) == 9
    assert "dips_diff_pixel_sums" in _lib.header_functions()
    a = np.arange(2 * 3 * 4, dtype=np.uint64).reshape(2, 3, 4)
    ps = dips_amd.PixelSums.from_array(a)
    assert ps.sad.shape == (2, 3) and np.array_equal(ps.as_array(), a)
    assert np.array_equal(ps.si, np.ldexp(a[..., 3].astype(np.float64), -32))
    with pytest.raises(ValueError):
        dips_amd.PixelSums.from_array(np.zeros((4, 4), dtype=np.uint64))
    assert hasattr(dips_amd.DiffSeriesOperator, "pixel_sums")
    assert hasattr(dips_amd.DiffSeriesOperator, "run_pixel_sums_device")
