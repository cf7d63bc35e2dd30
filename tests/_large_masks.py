"""Builders of masks of more than 65,536 words per frame together with what
the labelling family must answer for them, in plain numpy / Python.  At that
size cc_offsets_kernel scans the per-block counts in more than one round of
256 blocks, and every rank behind the first round depends on the carry handed
from round to round.

tiled()        a dense frame of translated copies of small labelled tiles:
               the expected records and labels are exact by construction.
sparse_frame() few set pixels, for _components_ref.components itself.
rings()        rectangular outlines whose filled forms are known.
moving_clip()  sparse frames of small moving rectangles, for _tracks_ref.
shapes_by_box() _shapes_ref.shape_record per component, cut out at its box.

The shapes and arguments of the GPU cases stand here too, so that
test_large_masks_cpu.py can check on the references alone that every case
reaches the paths it is meant for."""
import functools

import numpy as np

import _components_ref as cref

ROUND_WORDS = 256 * 256  # the words whose block counts one round of cc_offsets_kernel scans

TILE_H, TILE_W = 63, 95
PITCH_Y, PITCH_X = 64, 96  # one clear row and one clear column between the copies
DENSITIES = (0.3, 0.5, 0.593, 0.7)

DENSE_W = 2031                # 64 words per row, 15 valid bits in the last
DENSE_HEIGHTS = (1088, 2112)  # 69,632 words: two rounds; 135,168 words: three
DENSE_MIN_AREA = 40           # of the truncating case

# 257 blocks: the second round has a single block.  The sparse frame is three
# rows taller than the clip's: its last round must hold a row-spanning run,
# and in a frame of 1009 rows the last round is 49 words of the last row.
SPARSE_H, SPARSE_W = 1012, 2080
SPARSE_MIN_AREA, SPARSE_K = 20, 64
CLIP_N, CLIP_H, CLIP_W = 27, 1009, 2080
CLIP_MIN_AREA, CLIP_K = 20, 16

RINGS_H, RINGS_W = 2112, 2031
CELL_H, CELL_W = 48, 80
CLOSED, CORNER, SIDE = range(3)  # the kinds of outline rings() draws


def frozen(a):
    a.setflags(write=False)
    return a


# -- the rounds of the offsets scan ---------------------------------------------------

def n_rounds(h, w):
    wpf = ((w + 31) // 32) * h
    return ((wpf + 255) // 256 + 255) // 256


def round_of(anchor, w):
    """The round of cc_offsets_kernel that holds the block of the anchor's word."""
    anchor = np.asarray(anchor, dtype=np.int64)
    ay, ax = anchor // w, anchor % w
    return (ay * ((w + 31) // 32) + ax // 32) // ROUND_WORDS


def kept_per_round(records, h, w, min_area):
    """int64 [rounds]: the records of at least min_area pixels per round."""
    records = np.asarray(records)
    kept = records[records[:, cref.AREA] >= max(int(min_area), 1)]
    return np.bincount(round_of(kept[:, cref.ANCHOR], w), minlength=n_rounds(h, w))


def truncating_k(records, h, w, min_area):
    """A max_boxes that falls strictly inside the kept roots of the second
    round: records on both sides of the first round boundary are written and
    records behind it are cut off."""
    per = kept_per_round(records, h, w, min_area)
    assert per[1] >= 2
    return int(per[0] + per[1] // 2)


# -- tiled ----------------------------------------------------------------------------

def standard_tiles(seed=0):
    rng = np.random.default_rng([101, seed])
    return tuple(frozen(rng.random((TILE_H, TILE_W)) < d) for d in DENSITIES)


def default_pick(r, c):
    return (3 * r + c) % 4  # a tile row is 16 blocks: the pattern repeats in no multiple of a block


class Tiled:
    """bits bool [H, W]; records uint32 [count, 8] by ascending anchor; labels
    uint32 [H, W] (rank + 1); expect(min_area, max_boxes) -> (counts [1],
    boxes [1, K, 8], labels [1, H, W]) as dips_mask_components defines them."""

    def __init__(self, bits, records, labels):
        self.bits, self.records, self.labels = frozen(bits), frozen(records), frozen(labels)
        self.count = records.shape[0]

    def expect(self, min_area=1, max_boxes=64):
        keep = self.records[:, cref.AREA] >= max(int(min_area), 1)
        kept = self.records[keep]
        boxes = np.zeros((1, max_boxes, 8), dtype=np.uint32)
        m = min(max_boxes, kept.shape[0])
        boxes[0, :m] = kept[:m]
        new_label = np.zeros(self.count + 1, dtype=np.uint32)  # dropped components take label 0
        new_label[1:][keep] = np.arange(1, kept.shape[0] + 1, dtype=np.uint32)
        return np.array([kept.shape[0]], dtype=np.uint32), boxes, new_label[self.labels][None]


def tiled(tiles, rows, cols, H, W, connectivity, pick=default_pick):
    """rows x cols copies of the tiles (bool [63, 95]; copy (r, c) is
    tiles[pick(r, c)]) at pitch 64 x 96 in an H x W frame.  A copy that
    reaches over the frame's edge is cut there and labelled as cut.  No
    adjacency crosses the clear row and column between two copies, so the
    frame's components are the translated components of the tiles."""
    assert all(t.shape == (TILE_H, TILE_W) and t.dtype == bool for t in tiles)
    local = {}

    def labelled(k, th, tw):
        if (k, th, tw) not in local:
            tile = np.ascontiguousarray(tiles[k][:th, :tw])
            counts, boxes, lab = cref.components(cref.pack(tile[None]), tw, connectivity, 1, th * tw, labels=True)
            local[k, th, tw] = boxes[0, :int(counts[0])].astype(np.int64), lab[0]
        return local[k, th, tw]

    bits = np.zeros((H, W), dtype=bool)
    parts, places, offset = [], [], 0
    for r in range(rows):
        for c in range(cols):
            y0, x0 = r * PITCH_Y, c * PITCH_X
            th, tw = min(TILE_H, H - y0), min(TILE_W, W - x0)
            assert th > 0 and tw > 0
            k = pick(r, c)
            rec, lab = labelled(k, th, tw)
            bits[y0:y0 + th, x0:x0 + tw] = tiles[k][:th, :tw]
            g = rec.copy()
            ay, ax = rec[:, cref.ANCHOR] // tw, rec[:, cref.ANCHOR] % tw
            g[:, cref.X0] += x0
            g[:, cref.X1] += x0
            g[:, cref.Y0] += y0
            g[:, cref.Y1] += y0
            g[:, cref.ANCHOR] = (ay + y0) * W + ax + x0
            g[:, cref.CX256] += 256 * x0  # _centroid256(s + area * d, area) = _centroid256(s, area) + 256 * d
            g[:, cref.CY256] += 256 * y0
            parts.append(g)
            places.append((y0, x0, th, tw, lab, offset, g.shape[0]))
            offset += g.shape[0]
    every = np.concatenate(parts)
    order = np.argsort(every[:, cref.ANCHOR], kind="stable")
    rank_of = np.empty(order.shape[0], dtype=np.int64)
    rank_of[order] = np.arange(order.shape[0])
    labels = np.zeros((H, W), dtype=np.uint32)
    for y0, x0, th, tw, lab, off, cnt in places:
        to_global = np.concatenate([[0], rank_of[off:off + cnt] + 1]).astype(np.uint32)
        labels[y0:y0 + th, x0:x0 + tw] = to_global[lab]
    return Tiled(bits, every[order].astype(np.uint32), labels)


@functools.lru_cache(maxsize=None)
def dense_case(H, connectivity):
    """The tiled frame of the GPU cases: H x DENSE_W, the last column of
    copies cut at the frame's edge, 15 pixels wide, inside the last word."""
    return tiled(standard_tiles(), -(-H // PITCH_Y), -(-DENSE_W // PITCH_X), H, DENSE_W, connectivity)


def dense_arguments(H, connectivity):
    """The (min_area, max_boxes) of the dense GPU cases: every record, the
    truncating case, counts and labels only."""
    case = dense_case(H, connectivity)
    return ((1, case.count), (DENSE_MIN_AREA, truncating_k(case.records, H, DENSE_W, DENSE_MIN_AREA)), (1, 0))


# -- sparse ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sparse_frame(H=SPARSE_H, W=SPARSE_W, seed=0):
    """(bits bool [H, W], info): specks at density 0.004; 20 rectangles of at
    least 21 pixels from the first row down; one vertical line from row 0 to
    row H - 4, which crosses every round; three bars of 2 x 12 pixels in rows
    H - 4 and H - 3; row H - 2 clear; in row H - 1 one run from pixel 5 to
    pixel W - 11, more than 64 all-ones words, that touches nothing."""
    assert W > 64 * 32 + 16 and H > 64
    rng = np.random.default_rng([103, seed, H, W])
    bits = rng.random((H, W)) < 0.004
    line_x = W - 300
    rects = []
    for i in range(20):
        rh, rw = int(rng.integers(3, 10)), int(rng.integers(7, 25))
        y = i * (H - 6 - rh) // 19
        x = int(rng.integers(0, line_x - 40 - rw))
        bits[y:y + rh, x:x + rw] = True
        rects.append((y, x, rh, rw))
    bits[0:H - 3, line_x] = True
    bars = [(H - 4, line_x - 220 + 80 * i, 2, 12) for i in range(3)]
    for y, x, rh, rw in bars:
        bits[y:y + rh, x:x + rw] = True
    bits[H - 2:] = False
    run = (H - 1, 5, W - 10)
    bits[run[0], run[1]:run[2]] = True
    info = {"line": (line_x, 0, H - 4), "rects": tuple(rects), "bars": tuple(bars), "run": run,
            "run_area": run[2] - run[1]}
    return frozen(bits), info


# -- rings ----------------------------------------------------------------------------

class Rings:
    """bits bool [H, W]; holes int64 [count, 6]: kind, interior area, y0, x0,
    hh, ww of every outline; filled4 / filled8: the frame with its holes
    filled when the foreground is read under 4 / 8 (the background under 8 /
    4); expect(connectivity, max_hole) the same with holes of more than
    max_hole pixels left open."""

    def __init__(self, bits, holes):
        self.bits, self.holes = frozen(bits), frozen(holes)
        self.filled4 = frozen(self.expect(4))
        self.filled8 = frozen(self.expect(8))

    def fillable(self, connectivity):
        kinds = (CLOSED,) if connectivity == 4 else (CLOSED, CORNER)
        return np.isin(self.holes[:, 0], kinds)

    def expect(self, connectivity, max_hole=0):
        out = self.bits.copy()
        for kind, area, y0, x0, hh, ww in self.holes[self.fillable(connectivity)].tolist():
            if max_hole == 0 or area <= max_hole:
                out[y0 + 1:y0 + hh - 1, x0 + 1:x0 + ww - 1] = True
        return out

    def splitting_hole(self, connectivity):
        """A max_hole with fillable holes on both sides of it."""
        areas = np.sort(self.holes[self.fillable(connectivity), 1])
        mid = int(areas[areas.shape[0] // 2])
        assert areas[0] <= mid < areas[-1]
        return mid


@functools.lru_cache(maxsize=None)
def rings(H=RINGS_H, W=RINGS_W, seed=0):
    """One rectangular outline, one pixel thick, per cell of 48 x 80 with a
    clear margin inside the cell: closed, or with one corner pixel removed,
    or with one pixel of its top side removed.  A closed interior is a hole
    under both readings; the interior behind a missing corner meets the
    outside only diagonally, so it is a hole when the background is read
    under 4 (foreground 8) and none under 8; the side gap leaks under both."""
    rng = np.random.default_rng([107, seed, H, W])
    bits = np.zeros((H, W), dtype=bool)
    holes = []
    for r in range(H // CELL_H):
        for c in range(W // CELL_W):
            hh, ww = int(rng.integers(3, CELL_H - 1)), int(rng.integers(4, CELL_W - 1))
            y0 = r * CELL_H + 1 + int(rng.integers(0, CELL_H - 1 - hh))
            x0 = c * CELL_W + 1 + int(rng.integers(0, CELL_W - 1 - ww))
            kind = int(rng.integers(0, 3))
            bits[y0:y0 + hh, x0:x0 + ww] = True
            bits[y0 + 1:y0 + hh - 1, x0 + 1:x0 + ww - 1] = False
            if kind == CORNER:
                cy, cx = [(0, 0), (0, ww - 1), (hh - 1, 0), (hh - 1, ww - 1)][int(rng.integers(0, 4))]
                bits[y0 + cy, x0 + cx] = False
            elif kind == SIDE:
                bits[y0, x0 + 1 + int(rng.integers(0, ww - 2))] = False
            holes.append((kind, (hh - 2) * (ww - 2), y0, x0, hh, ww))
    return Rings(bits, np.array(holes, dtype=np.int64))


# -- the clip -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def moving_clip(n=CLIP_N, H=CLIP_H, W=CLIP_W, seed=0):
    """bool [n, H, W]: 12 rectangles of about 12 x 16 pixels that move 1 or 2
    pixels per frame on each axis, three of them absent every fifth frame;
    three bars of 1 x 24 pixels in the last row, which move to the right (in
    a frame of 1009 x 2080 they are the kept roots of the last round); 300
    specks per frame above row H - 2."""
    rng = np.random.default_rng([109, seed, n, H, W])
    bits = np.zeros((n, H, W), dtype=bool)
    reach = 2 * n + 2
    for i in range(12):
        rh, rw = int(rng.integers(10, 15)), int(rng.integers(13, 20))
        y = int(rng.integers(reach, H - 3 - rh - reach))
        x = int(rng.integers(reach, W - rw - reach))
        vy, vx = (int(v) for v in rng.choice([-2, -1, 1, 2], 2))
        phase = int(rng.integers(0, 5))
        for t in range(n):
            if i < 3 and (t + phase) % 5 == 0:
                continue
            bits[t, y + vy * t:y + vy * t + rh, x + vx * t:x + vx * t + rw] = True
    for i in range(3):
        for t in range(n):
            x = W // 4 + 50 + i * (W // 6) + (1 + i % 2) * t
            bits[t, H - 1, x:x + 24] = True
    for t in range(n):
        bits[t, rng.integers(0, H - 2, 300), rng.integers(0, W, 300)] = True
    return frozen(bits)


def shapes_by_box(mask_bytes, w, weights=None, connectivity=8, min_area=1, max_boxes=64):
    """_shapes_ref.shapes, affordable on large sparse frames: the record of
    every component is _shapes_ref.shape_record of the component cut out at
    its box (x0, y0), with the moments moved back by
      sum (i + x0) = sx + area x0,  sum (i + x0)^2 = sxx + 2 x0 sx + area x0^2,
      sum (i + x0)(j + y0) = sxy + x0 sy + y0 sx + area x0 y0;
    the cracks, the Euler number and the weights under the component do not
    depend on where it lies."""
    import _shapes_ref as sref
    counts, boxes, lab = cref.components(mask_bytes, w, connectivity, min_area, max_boxes, labels=True)
    out = np.zeros((counts.shape[0], max_boxes, sref.WORDS), dtype=np.uint32)
    for t in range(counts.shape[0]):
        for k in range(min(int(counts[t]), max_boxes)):
            x0, y0, x1, y1, area = (int(v) for v in boxes[t, k, :5])
            rec = sref.shape_record(lab[t, y0:y1, x0:x1] == k + 1, connectivity,
                                    None if weights is None else weights[t, y0:y1, x0:x1])
            sx, sy, sxx, syy, sxy = (int(sref.get64(rec, f)) for f in (sref.SX, sref.SY, sref.SXX, sref.SYY, sref.SXY))
            for f, v in ((sref.SX, sx + area * x0), (sref.SY, sy + area * y0),
                         (sref.SXX, sxx + 2 * x0 * sx + area * x0 * x0), (sref.SYY, syy + 2 * y0 * sy + area * y0 * y0),
                         (sref.SXY, sxy + x0 * sy + y0 * sx + area * x0 * y0)):
                sref.put64(rec, f, v)
            out[t, k] = rec
    return counts, boxes, out


@functools.lru_cache(maxsize=None)
def clip_weights(n=CLIP_N, H=CLIP_H, W=CLIP_W, seed=0):
    return frozen(np.random.default_rng([113, seed, n, H, W]).integers(0, 256, (n, H, W), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def clip_marker(n=CLIP_N, H=CLIP_H, W=CLIP_W, seed=0):
    """A marker per frame at density 0.003: it hits about half of the rectangles."""
    return frozen(np.random.default_rng([127, seed, n, H, W]).random((n, H, W), dtype=np.float32) < 0.003)
