"""The definition of dips_diff_sigma_delta_mask, once, in numpy.

J(F) per pixel is oracle.np_restatement.jtwin(F, chroma): max + min of R, G,
B, 2 * channel under a chroma filter, 2 * g for GRAY8 (0 .. 510).  State per
region pixel: M (0 .. 510) and V (v_min .. v_max).  For frame t, in order:
  M' = M + sgn(J_t - M)
  D  = |J_t - M'|
  V' = clamp(V + sgn(N * D - V), v_min, v_max)  if D != 0, else V' = V
  bit = D > V'
The decision is per pixel, so the fold works on the frames cropped to roi."""
import numpy as np

from oracle.np_restatement import jtwin
from test_change_mask_cpu import pack_mask

PARAMS = [(1, 0, 510), (2, 2, 510), (4, 1, 6), (15, 0, 510), (3, 7, 7)]


def step(M, V, J, n_amp, v_min, v_max):
    """One frame on int64 arrays: (M', V', bit)."""
    M = M + np.sign(J - M)
    D = np.abs(J - M)
    V = np.where(D != 0, np.clip(V + np.sign(n_amp * D - V), v_min, v_max), V)
    return M, V, D > V


def sigma_delta_fold(frames, n_amp=2, v_min=2, v_max=510, chroma=0, ref=None, roi=None, state=None):
    """(mask uint8 [n, rh, 4 * ceil(rw / 32)], state uint16 [2, rh, rw]).
    state: the [2, rh, rw] state to continue (ref must be None), else the fold
    starts at M = J(ref) (None: J(frames[0])), V = v_min."""
    assert 1 <= n_amp <= 15 and 0 <= v_min <= v_max <= 510
    frames = np.asarray(frames, dtype=np.uint8)
    n, h, w = frames.shape[:3]
    gray = frames.ndim == 3
    chroma = 0 if gray else chroma
    x0, y0, rw, rh = roi if roi is not None else (0, 0, w, h)
    crop = frames[:, y0:y0 + rh, x0:x0 + rw]
    if state is not None:
        assert ref is None
        M, V = (np.asarray(state, dtype=np.int64)[p].copy() for p in (0, 1))
    else:
        first = crop[0] if ref is None else np.asarray(ref, dtype=np.uint8).reshape(frames.shape[1:])[y0:y0 + rh, x0:x0 + rw]
        M = jtwin(first[None], chroma)[0].astype(np.int64)  # jtwin takes batches: [n, h, w] is GRAY8
        V = np.full(M.shape, v_min, dtype=np.int64)
    assert M.shape == (rh, rw) and V.shape == (rh, rw)
    J = jtwin(crop, chroma).astype(np.int64)
    bits = np.zeros((n, rh, rw), dtype=bool)
    for t in range(n):
        M, V, bits[t] = step(M, V, J[t], n_amp, v_min, v_max)
        assert M.min(initial=0) >= 0 and M.max(initial=0) <= 510
    return pack_mask(bits), np.ascontiguousarray(np.stack([M, V]).astype(np.uint16))
