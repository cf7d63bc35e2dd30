"""The expectation of dips_diff_pixel_times, without a GPU.

The state of a pixel is four uint32 -- first, last, run_max, run_cur -- and
the call folds the bits of dips_diff_change_mask over the frames in order
(fold_times below restates the fold of include/dips_hip.h in numpy).  The
authoritative bits are the C oracle's (oracle_change_mask of
tests/test_change_mask_cpu.py: the count of the series of the 1x1 crop), so
oracle_pixel_times = fold_times(unpack_mask(oracle_change_mask(...))) is the
definition; py_pixel_times folds py_change_mask, the vectorised twin, for the
shapes where one oracle call per pixel is too slow.  This file shows the two
equal, the fold consistent under chunking and with the per-pixel sums.

Inputs: noise on every frame (noise_frames) gives every pixel first ~ 1 and
last ~ n - 1 and would hide a broken index or run.  event_frames keeps a pixel
at its base value outside a window [a, b) of its own and puts uniform integer
noise in [-40, 40] on it inside: a ~ U{1..n-1}, b = min(n, a + U{0..n-1}), one
pixel in ten with an empty window, one in ten with [1, n).  check_informative
asserts on the oracle's result that such a clip exercises the planes: between
5 and 50 % of the pixels never change, first takes at least min(n - 1, 8)
values besides NONE and run_max at least 4.  These conditions need room: with
n < 5 frames run_max cannot take 4 values beside a share of unchanged pixels,
and a frame of a few pixels cannot show shares at all, so for n < 5 or fewer
than 256 pixels only what can hold is asserted (some pixel changed; at n >= 2
first takes a value).  The part tests add crossing_share >= 10 %: pixels whose
run crosses a part boundary."""
import functools

import numpy as np
import pytest

from test_change_mask_cpu import TAUS, _base_frame, oracle_change_mask, py_change_mask, unpack_mask
from test_pixel_sums_cpu import oracle_pixel_sums

NONE = 0xFFFFFFFF


def initial_state(h, w):
    s = np.zeros((4, h, w), dtype=np.uint32)
    s[:2] = NONE
    return s


def fold_times(bits, t0=0, state=None):
    """bool [n, h, w] folded in order onto state ([4, h, w] uint32; None: the
    initial state) -> [4, h, w] uint32: first, last, run_max, run_cur."""
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    assert 0 <= t0 and t0 + n <= NONE
    first, last, rmax, rcur = (initial_state(h, w) if state is None else np.array(state, dtype=np.uint32))
    for t in range(n):
        b, g = bits[t], np.uint32(t0 + t)
        first = np.where(b & (first == NONE), g, first)
        last = np.where(b, g, last)
        rcur = np.where(b, rcur + np.uint32(1), np.uint32(0))
        rmax = np.maximum(rmax, rcur)
    return np.stack([first, last, rmax, rcur]).astype(np.uint32)


def _region_w(frames, roi):
    return frames.shape[2] if roi is None else roi[2]


def oracle_pixel_times(frames, mode=0, tau=0.0, chroma=0, ref=None, roi=None, t0=0, state=None):
    """The definition: the fold over the C oracle's per-pixel counts."""
    m = oracle_change_mask(frames, mode, tau, chroma, ref, roi)
    return fold_times(unpack_mask(m, _region_w(frames, roi)), t0, state)


def py_pixel_times(frames, mode=0, tau=0.0, chroma=0, ref=None, roi=None, t0=0, state=None):
    """The vectorised twin: the fold over py_change_mask."""
    m = py_change_mask(frames, mode, tau, chroma, ref, roi)
    return fold_times(unpack_mask(m, _region_w(frames, roi)), t0, state)


@functools.lru_cache(maxsize=None)
def event_frames(c, w, h, n):
    """The base frame of noise_frames; per pixel a window [a, b) inside which
    uniform integer noise in [-40, 40] is added (clipped to bytes), outside
    which the pixel equals the base exactly."""
    base = _base_frame(c, w, h)
    rng = np.random.default_rng([21, c, w, h, n])
    if n >= 2:
        a = rng.integers(1, n, (h, w))
        b = np.minimum(n, a + rng.integers(0, n, (h, w)))
    else:
        a = np.ones((h, w), dtype=np.int64)
        b = np.ones((h, w), dtype=np.int64)
    kind = rng.integers(0, 10, (h, w))
    b = np.where(kind == 0, a, b)                 # one in ten: empty
    a = np.where(kind == 1, 1, a)                 # one in ten: [1, n)
    b = np.where(kind == 1, n, b)
    t = np.arange(n).reshape((n, 1, 1))
    inside = (t >= a[None]) & (t < b[None])       # [n, h, w]
    noise = rng.integers(-40, 41, (n,) + base.shape, dtype=np.int16)
    if c != 1:
        inside = inside[..., None]
    out = np.clip(base[None] + np.where(inside, noise, 0), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def event_ref(c, w, h):
    """A reference: the base frame under noise of its own on one pixel in two."""
    base = _base_frame(c, w, h)
    rng = np.random.default_rng([22, c, w, h])
    on = rng.integers(0, 2, (h, w)).astype(bool)
    noise = rng.integers(-40, 41, base.shape, dtype=np.int16)
    if c != 1:
        on = on[..., None]
    out = np.clip(base + np.where(on, noise, 0), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def check_informative(times, n):
    """The oracle's planes exercise the feature (the conditions of this file's docstring)."""
    first, last, rmax, rcur = times
    changed = first != NONE
    assert np.array_equal(changed, last != NONE) and np.array_equal(changed, rmax != 0)
    assert changed.any()
    if n >= 2:
        assert np.unique(first[changed]).size >= 1
    if n < 5 or first.size < 256:
        return
    never = 1.0 - changed.mean()
    assert 0.05 < never < 0.5, never
    assert np.unique(first[changed]).size >= min(n - 1, 8)
    assert np.unique(rmax).size >= 4


def crossing_share(bits, plen):
    """Share of pixels with a run that crosses a boundary of parts of plen frames."""
    bits = np.asarray(bits, dtype=bool)
    cross = np.zeros(bits.shape[1:], dtype=bool)
    for t in range(plen, bits.shape[0], plen):
        cross |= bits[t - 1] & bits[t]
    return cross.mean()


@pytest.mark.parametrize("tau_k", [4, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_restatement_equals_oracle_fold(c, mode, tau_k):
    w, h, n = 37, 29, 9
    frames = event_frames(c, w, h, n)
    want = oracle_pixel_times(frames, mode, TAUS[tau_k])
    assert want.shape == (4, h, w) and want.dtype == np.uint32
    check_informative(want, n)
    assert np.array_equal(py_pixel_times(frames, mode, TAUS[tau_k]), want)
    # frame 0 meets itself: nothing changes at index 0 without a reference
    assert want[0].min() >= 1


@pytest.mark.parametrize("mode", [0, 1])
def test_restatement_with_reference_chroma_roi_and_t0(mode):
    w, h, n = 37, 29, 9
    frames, ref = event_frames(3, w, h, n), event_ref(3, w, h)
    want = oracle_pixel_times(frames, mode, 8 / 255, 0, ref)
    assert (want[0] == 0).any()  # against the reference frame 0 changes too
    assert np.array_equal(py_pixel_times(frames, mode, 8 / 255, 0, ref), want)
    want = oracle_pixel_times(frames, mode, 8 / 255, 2)
    check_informative(want, n)
    assert np.array_equal(py_pixel_times(frames, mode, 8 / 255, 2), want)
    roi = (3, 2, 21, 17)
    whole = oracle_pixel_times(frames, mode, 4 / 255, t0=1000)
    want = oracle_pixel_times(frames, mode, 4 / 255, 0, None, roi, t0=1000)
    check_informative(want, n)
    assert np.array_equal(want, whole[:, 2:19, 3:24])
    assert np.array_equal(py_pixel_times(frames, mode, 4 / 255, 0, None, roi, t0=1000), want)
    # t0 shifts the indices of the changed pixels and nothing else
    base = oracle_pixel_times(frames, mode, 4 / 255)
    ch = base[0] != NONE
    assert np.array_equal(whole[:2][:, ch], base[:2][:, ch] + np.uint32(1000))
    assert (whole[:2][:, ~ch] == NONE).all() and np.array_equal(whole[2:], base[2:])


@pytest.mark.parametrize("w,h,n", [(37, 29, 9), (37, 29, 24), (8, 8, 300)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_event_frames_exercise_the_planes(c, mode, w, h, n):
    frames = event_frames(c, w, h, n)
    bits = unpack_mask(py_change_mask(frames, mode, 8 / 255), w)
    want = fold_times(bits)
    first, last, rmax, rcur = want
    changed = first != NONE
    never = 1.0 - changed.mean()
    assert 0.05 < never < 0.5, never
    assert np.unique(first[changed]).size >= min(n - 1, 8)
    assert np.unique(rmax).size >= 4
    if n >= 24:
        assert crossing_share(bits, 17) >= 0.10


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_fold_in_two_chunks_is_the_whole_fold(c, mode):
    w, h, n = 37, 29, 9
    bits = unpack_mask(py_change_mask(event_frames(c, w, h, n), mode, 8 / 255), w)
    whole = fold_times(bits, t0=7)
    spans = 0
    for k in (1, 4, 5, n - 1):
        a = fold_times(bits[:k], t0=7)
        assert np.array_equal(fold_times(bits[k:], t0=7 + k, state=a), whole)
        spans += int((bits[k - 1] & bits[k]).sum())
    assert spans > 0  # runs that span a cut exist and are counted whole


@pytest.mark.parametrize("tau_k", [4, 8])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_consistent_with_the_pixel_sums(c, mode, tau_k):
    w, h, n = 37, 29, 9
    frames = event_frames(c, w, h, n)
    bits = unpack_mask(oracle_change_mask(frames, mode, TAUS[tau_k]), w)
    count = oracle_pixel_sums(frames, mode, TAUS[tau_k])[..., 2]
    assert np.array_equal(bits.sum(axis=0, dtype=np.uint64), count)
    first, last, rmax, rcur = fold_times(bits)
    assert (rmax <= count).all() and (rcur <= rmax).all()
    ch = first != NONE
    assert np.array_equal(ch, count != 0)
    assert (first[ch] <= last[ch]).all()
    assert (last[ch] - first[ch] + 1 >= count[ch]).all()


def test_library_and_package_expose_the_call():
    """Fails without the feature: the symbol, its binding, the result type and the operator's methods."""
    import dips_amd
    from dips_amd import _lib
    lib = _lib.load()
    assert len(lib.dips_diff_pixel_times.argtypes) == 10
    assert "dips_diff_pixel_times" in _lib.header_functions()
    assert dips_amd.PixelTimes.NONE == NONE
    a = np.arange(4 * 3 * 5, dtype=np.uint32).reshape(4, 3, 5)
    a[0, 0, 0] = NONE
    t = dips_amd.PixelTimes.from_array(a)
    for k, plane in enumerate((t.first, t.last, t.run_max, t.run_cur)):
        assert plane.shape == (3, 5) and plane.dtype == np.uint32 and np.array_equal(plane, a[k])
    assert np.array_equal(t.as_array(), a) and t.as_array().dtype == np.uint32
    with pytest.raises(ValueError):
        dips_amd.PixelTimes.from_array(np.zeros((3, 5, 4), dtype=np.uint32))
    assert hasattr(dips_amd.DiffSeriesOperator, "pixel_times")
    assert hasattr(dips_amd.DiffSeriesOperator, "run_pixel_times_device")
