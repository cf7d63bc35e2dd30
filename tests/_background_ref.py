"""The definition of dips_diff_background_mask, once, in numpy.

State: per region pixel and channel a u16 B in 8.8 fixed point.  For frame t,
in order: R = (B + 128) >> 8; bit = the change mask of the single frame F_t in
'overall' mode with reference R (mask_fn: oracle_change_mask, one call of the C
oracle per pixel, or its vectorised twin py_change_mask, both from
tests/test_change_mask_cpu.py); B' = B - ((B + h) >> k) + (F << (8 - k)) with
h = (1 << k) >> 1, skipped for the whole pixel when selective and bit = 1.
The decision is per pixel, so the fold works on the frames cropped to roi."""
import numpy as np

from test_change_mask_cpu import py_change_mask, unpack_mask


def update(B, F, k):
    """One step of the integer recurrence on int64 arrays."""
    h = (1 << k) >> 1
    return B - ((B + h) >> k) + (F << (8 - k))


def reference_bytes(B):
    return (B + 128) >> 8


def background_fold(frames, rate_shift, selective=False, tau=0.0, chroma=0, ref=None, roi=None, state=None,
                    mask_fn=py_change_mask):
    """(mask uint8 [n, rh, 4 * ceil(rw / 32)], state uint16 [C, rh, rw]).
    state: the [C, rh, rw] state to continue (ref must be None), else the fold
    starts at 256 * ref (None: 256 * frames[0])."""
    frames = np.asarray(frames, dtype=np.uint8)
    n, h, w = frames.shape[:3]
    gray = frames.ndim == 3
    x0, y0, rw, rh = roi if roi is not None else (0, 0, w, h)
    crop = frames[:, y0:y0 + rh, x0:x0 + rw]
    if state is not None:
        assert ref is None
        B = np.moveaxis(np.asarray(state, dtype=np.int64), 0, -1)
        B = B[..., 0] if gray else B
    else:
        first = crop[0] if ref is None else np.asarray(ref, dtype=np.uint8).reshape(frames.shape[1:])[y0:y0 + rh, x0:x0 + rw]
        B = 256 * first.astype(np.int64)
    B = B.copy()
    assert B.shape == crop.shape[1:]
    masks = np.zeros((n, rh, 4 * ((rw + 31) // 32)), dtype=np.uint8)
    for t in range(n):
        R = reference_bytes(B)
        assert R.min(initial=0) >= 0 and R.max(initial=0) <= 255
        m = mask_fn(crop[t][None], 0, tau, chroma, ref=np.ascontiguousarray(R.astype(np.uint8)))
        masks[t] = m[0]
        nb = update(B, crop[t].astype(np.int64), rate_shift)
        if selective:
            bit = unpack_mask(m, rw)[0]
            nb = np.where(bit if gray else bit[..., None], B, nb)
        B = nb
        assert B.min(initial=0) >= 0 and B.max(initial=0) <= 65280
    planes = B[None] if gray else np.moveaxis(B, -1, 0)
    return masks, np.ascontiguousarray(planes.astype(np.uint16))


def drift_clip(c=3, w=37, h=29, n=24, seed=5):
    """A static-camera clip: a random base frame gaining 1 level per 2 frames
    (the light drifts), uniform noise in [-5, 5] per frame, and a 9 x 9 square
    90 levels brighter that moves 1 pixel per frame."""
    rng = np.random.default_rng([21, c, w, h, n, seed])
    shape = (h, w) if c == 1 else (h, w, c)
    base = rng.integers(40, 140, shape, dtype=np.int16)
    out = np.zeros((n,) + shape, dtype=np.uint8)
    for t in range(n):
        f = base + t // 2 + rng.integers(-5, 6, shape, dtype=np.int16)
        x, y = 2 + t, 4 + t // 2
        f[y:y + 9, x:x + 9] += 90
        out[t] = np.clip(f, 0, 255)
    out.setflags(write=False)
    return out
