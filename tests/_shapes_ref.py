"""The specification of dips_mask_shapes in plain numpy / Python, written
from the sentences of include/dips_hip.h on top of _components_ref: the sums
are taken pixel by pixel, the cracks are counted by looking at the four
neighbours on the zero-padded frame, and EULER is 1 minus the holes found by
labelling the padded complement of each component, taken alone, under the
dual connectivity.  Nothing here uses a local Euler formula."""
import numpy as np

import _components_ref as cref

WORDS = 16
SX, SY, SXX, SYY, SXY, WSUM, WMAX, CRACKS_V, CRACKS_H, EULER = 0, 2, 4, 6, 8, 10, 12, 13, 14, 15
COLUMNS = ("sx", "sy", "sxx", "syy", "sxy", "wsum", "wmax", "cracks_v", "cracks_h", "euler")


def holes(comp, connectivity):
    """The bounded components of the complement of `comp` (bool [h, w]) in
    the plane, under the dual of `connectivity`."""
    if not comp.any():
        return 0
    ys, xs = np.nonzero(comp)
    comp = comp[ys.min():ys.max() + 1, xs.min():xs.max() + 1]  # a hole is bounded by C: it lies inside C's box
    padded = np.pad(~comp, 1, constant_values=True)  # the ring around the box is background
    root = cref.label_frame(padded, 4 if connectivity == 8 else 8)
    return len(np.unique(root[padded])) - 1  # all but the one that holds the ring


def cracks(comp):
    """(CRACKS_V, CRACKS_H) of `comp` (bool [h, w]) by neighbour inspection."""
    p = np.pad(comp, 1, constant_values=False)
    c = p[1:-1, 1:-1]
    v = int((c & ~p[1:-1, :-2]).sum()) + int((c & ~p[1:-1, 2:]).sum())
    h = int((c & ~p[:-2, 1:-1]).sum()) + int((c & ~p[2:, 1:-1]).sum())
    return v, h


def put64(rec, f, v):
    assert 0 <= v < 1 << 64
    rec[f], rec[f + 1] = v & 0xFFFFFFFF, v >> 32


def get64(shapes, f):
    return shapes[..., f].astype(np.uint64) | (shapes[..., f + 1].astype(np.uint64) << np.uint64(32))


def shape_record(comp, connectivity, weights=None):
    """The 16 words of the component `comp` (bool [h, w]); weights uint8 [h, w] or None."""
    rec = np.zeros(WORDS, dtype=np.uint32)
    sx = sy = sxx = syy = sxy = wsum = wmax = 0
    ys, xs = np.nonzero(comp)
    for j, i in zip(ys.tolist(), xs.tolist()):
        sx, sy, sxx, syy, sxy = sx + i, sy + j, sxx + i * i, syy + j * j, sxy + i * j
        if weights is not None:
            wsum += int(weights[j, i])
            wmax = max(wmax, int(weights[j, i]))
    for f, v in ((SX, sx), (SY, sy), (SXX, sxx), (SYY, syy), (SXY, sxy), (WSUM, wsum)):
        put64(rec, f, v)
    rec[WMAX] = wmax
    rec[CRACKS_V], rec[CRACKS_H] = cracks(comp)
    rec[EULER] = (1 - holes(comp, connectivity)) & 0xFFFFFFFF
    return rec


def shapes(mask_bytes, w, weights=None, connectivity=8, min_area=1, max_boxes=64):
    """(counts uint32 [n], boxes uint32 [n, K, 8], shapes uint32 [n, K, 16])
    of the mask bytes [n, h, row_bytes(w)]; weights uint8 [n, h, w] or None."""
    counts, boxes, lab = cref.components(mask_bytes, w, connectivity, min_area, max_boxes, labels=True)
    n = counts.shape[0]
    out = np.zeros((n, max_boxes, WORDS), dtype=np.uint32)
    for t in range(n):
        for k in range(min(int(counts[t]), max_boxes)):
            out[t, k] = shape_record(lab[t] == k + 1, connectivity, None if weights is None else weights[t])
    return counts, boxes, out


def frame_euler(bits, connectivity):
    """The Euler number of a whole frame: its components minus its holes."""
    root = cref.label_frame(bits, connectivity)
    return len(np.unique(root[bits])) - holes(bits, connectivity)


def csv_columns(rec):
    """The ten CSV columns of a record, as integers (EULER signed)."""
    rec = np.asarray(rec, dtype=np.uint32)
    euler = int(rec[EULER]) - (1 << 32) if int(rec[EULER]) >> 31 else int(rec[EULER])
    return [int(get64(rec, f)) for f in (SX, SY, SXX, SYY, SXY, WSUM)] + [
        int(rec[WMAX]), int(rec[CRACKS_V]), int(rec[CRACKS_H]), euler]
