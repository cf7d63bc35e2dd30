"""The specification of dips_mask_select, dips_mask_logic and mask_fill_holes
in plain numpy / Python, written from the definitions in include/dips_hip.h:
the components are those of _components_ref.label_frame, and a component is
kept iff min_area <= area, (max_area == 0 or area <= max_area), (no marker or
it holds a marker pixel) and (not clear_border or it has no pixel on the
region's border).  Everything works on unpacked bool arrays [n, h, w]; the
packed forms (select_bytes, logic_bytes, fill_holes_bytes) ignore the pad
bits of their inputs and write those of their outputs as 0."""
import functools

import numpy as np

from _components_ref import label_frame, pack, unpack

AND, OR, XOR, ANDNOT, NOT = range(5)


@functools.lru_cache(maxsize=256)
def _roots(frame_bytes, h, w, connectivity):
    """label_frame of a frame given as its bool bytes: the tests ask for the
    same frame under many predicates."""
    root = label_frame(np.frombuffer(frame_bytes, dtype=bool).reshape(h, w), connectivity)
    root.setflags(write=False)
    return root


def select(bits, marker=None, connectivity=8, min_area=1, max_area=0, clear_border=False, dropped=False):
    """bits bool [n, h, w], marker None or bool [1 or n, h, w] ->
    (bool [n, h, w], counts uint32 [n])."""
    assert connectivity in (4, 8)
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    if marker is not None:
        marker = np.asarray(marker, dtype=bool)
        assert marker.shape in ((1, h, w), (n, h, w))
    out = np.zeros_like(bits)
    counts = np.zeros(n, dtype=np.uint32)
    edge = np.zeros((h, w), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    for t in range(n):
        root = _roots(bits[t].tobytes(), h, w, connectivity)
        flat = root[bits[t]]
        area = np.bincount(flat, minlength=h * w)
        keep = (area >= max(int(min_area), 1)) & (area > 0)
        if max_area:
            keep &= area <= int(max_area)
        if marker is not None:
            m = marker[t if marker.shape[0] == n else 0] & bits[t]
            keep &= np.bincount(root[m], minlength=h * w) > 0
        if clear_border:
            keep &= np.bincount(root[edge & bits[t]], minlength=h * w) == 0
        counts[t] = int(keep.sum())
        kept = np.zeros((h, w), dtype=bool)
        kept[bits[t]] = keep[flat]
        out[t] = bits[t] & ~kept if dropped else kept
    return out, counts


def logic(a, op, b=None):
    """bool [n, h, w] op bool [1 or n, h, w] (None for NOT) -> bool [n, h, w]."""
    a = np.asarray(a, dtype=bool)
    if op == NOT:
        assert b is None
        return ~a
    b = np.broadcast_to(np.asarray(b, dtype=bool), a.shape)
    return {AND: a & b, OR: a | b, XOR: a ^ b, ANDNOT: a & ~b}[op]


def fill_holes(bits, connectivity=8, max_hole=0):
    """bits | holes: the holes are the components of the complement, under
    the dual connectivity, with no pixel on the region's border and (max_hole
    != 0) at most max_hole pixels."""
    bits = np.asarray(bits, dtype=bool)
    holes, _ = select(~bits, None, 12 - connectivity, 1, max_hole, clear_border=True)
    return bits | holes


def select_bytes(mask_bytes, w, marker_bytes=None, **kw):
    """The packed form: (mask bytes [n, h, row_bytes], counts)."""
    out, counts = select(unpack(mask_bytes, w), None if marker_bytes is None else unpack(marker_bytes, w), **kw)
    return pack(out), counts


def logic_bytes(a_bytes, w, op, b_bytes=None):
    return pack(logic(unpack(a_bytes, w), op, None if b_bytes is None else unpack(b_bytes, w)))


def fill_holes_bytes(mask_bytes, w, connectivity=8, max_hole=0):
    return pack(fill_holes(unpack(mask_bytes, w), connectivity, max_hole))
