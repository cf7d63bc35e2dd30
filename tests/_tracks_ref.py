"""The specification of dips_mask_tracks in plain numpy / Python, written
from the sentences of include/dips_hip.h on top of
_components_ref.components(..., labels=True): the overlap table by counting
label pairs, the argmax rules, the mutual test, the ids in (t, k) order and
the prev_mask / state carry.  Also the generator of moving rectangles the
tests draw their clips from."""
import numpy as np

import _components_ref as cref

PREV, OVERLAP, TRACK, AGE = range(4)
LINK_WORDS = 4
NONE = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def overlap_table(lab_t, lab_p, K):
    """ov[a, b]: pixels with label a + 1 in frame t and b + 1 in frame t - 1,
    records only (labels 1 .. K)."""
    ov = np.zeros((K, K), dtype=np.int64)
    both = (lab_t >= 1) & (lab_t <= K) & (lab_p >= 1) & (lab_p <= K)
    np.add.at(ov, (lab_t[both].astype(np.int64) - 1, lab_p[both].astype(np.int64) - 1), 1)
    return ov


def _argmax_first(v):
    """(index, value) of the largest v > 0, the smallest index on a tie;
    (None, 0) if every v is 0."""
    best, arg = 0, None
    for i, x in enumerate(v.tolist()):
        if x > best:
            best, arg = x, i
    return arg, best


def tracks(mask_bytes, w, connectivity=8, min_area=1, max_boxes=64, prev=None, state=None):
    """(counts [n], boxes [n, K, 8], links [n, K, 4], state [1 + 2K] or None)
    of the mask bytes [n, h, row_bytes(w)]; prev: one frame [h, row_bytes]
    or None; state: uint32 [1 + 2K] or None (not modified)."""
    K = int(max_boxes)
    assert 1 <= K <= 256
    assert prev is None or state is not None
    mask_bytes = np.asarray(mask_bytes, dtype=np.uint8)
    n = mask_bytes.shape[0]
    counts, boxes, lab = cref.components(mask_bytes, w, connectivity, min_area, K, labels=True)
    links = np.zeros((n, K, LINK_WORDS), dtype=np.uint32)
    links[:, :, PREV] = NONE
    links[:, :, TRACK] = NONE
    if n == 0:
        return counts, boxes, links, None if state is None else np.array(state, dtype=np.uint32)
    next_id = int(state[0]) if state is not None else 0
    lab_p, trk_p, age_p = None, None, None
    if prev is not None:
        lab_p = cref.components(np.asarray(prev, dtype=np.uint8)[None], w, connectivity, min_area, K, labels=True)[2][0]
        trk_p = [int(x) for x in state[1:1 + K]]
        age_p = [int(x) for x in state[1 + K:1 + 2 * K]]
    for t in range(n):
        m = min(int(counts[t]), K)
        ov = overlap_table(lab[t], lab_p, K) if lab_p is not None else np.zeros((K, K), dtype=np.int64)
        nxt = [_argmax_first(ov[:, b])[0] for b in range(K)]
        trk, age = [NONE] * K, [0] * K
        for k in range(m):
            b, best = _argmax_first(ov[k])
            links[t, k, PREV] = NONE if b is None else b
            links[t, k, OVERLAP] = best
            if b is not None and nxt[b] == k:
                trk[k], age[k] = trk_p[b], (age_p[b] + 1) & M32
            else:
                trk[k], age[k] = next_id, 0
                next_id = (next_id + 1) & M32
            links[t, k, TRACK], links[t, k, AGE] = trk[k], age[k]
        lab_p, trk_p, age_p = lab[t], trk, age
    out = None
    if state is not None:
        out = np.array([next_id] + trk_p + age_p, dtype=np.uint32)
    return counts, boxes, links, out


def tracks_by_id(counts, links):
    """id -> [(t, k), ...] in ascending order."""
    out = {}
    K = links.shape[1]
    for t in range(links.shape[0]):
        for k in range(min(int(counts[t]), K)):
            out.setdefault(int(links[t, k, TRACK]), []).append((t, k))
    return out


def moving_rectangles(seed, n, h, w, nobj):
    """bool [n, h, w]: nobj rectangles of side 2..8 with a velocity of -3..3
    pixels per frame on each axis, each alive on a random span of frames,
    drawn clipped to the region."""
    rng = np.random.default_rng([97, seed, n, h, w, nobj])
    bits = np.zeros((n, h, w), dtype=bool)
    for _ in range(nobj):
        sw, sh = int(rng.integers(2, 9)), int(rng.integers(2, 9))
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        vx, vy = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
        t0 = int(rng.integers(0, n))
        t1 = int(rng.integers(t0, n)) + 1
        for t in range(t0, t1):
            xx, yy = x + vx * (t - t0), y + vy * (t - t0)
            bits[t, max(yy, 0):max(yy + sh, 0), max(xx, 0):max(xx + sw, 0)] = True
    return bits


# (n, h, w, nobj, K, min_area, connectivity): the generator settings of the tests
SETTINGS = ((12, 29, 70, 10, 4, 2, 8), (12, 29, 70, 14, 6, 2, 4), (10, 33, 65, 12, 5, 1, 8), (16, 40, 97, 16, 8, 3, 8))
SEEDS = tuple(range(8))


def square_clip():
    """A 3x3 square moving 2 pixels per frame over 4 frames."""
    bits = np.zeros((4, 8, 16), dtype=bool)
    for t in range(4):
        bits[t, 2:5, 1 + 2 * t:4 + 2 * t] = True
    return bits


def split_merge_clip():
    """A 9-pixel bar, then its 3 + 5 pixel pieces, then the bar again."""
    bits = np.zeros((3, 3, 12), dtype=bool)
    bits[0, 1, 1:10] = True
    bits[1, 1, 1:4] = True
    bits[1, 1, 5:10] = True
    bits[2, 1, 1:10] = True
    return bits


def tie_clip():
    """Frame 0: two columns; frame 1: two rows that cross each column in
    exactly one pixel, so every ov is 1 and every argmax a tie."""
    bits = np.zeros((2, 3, 8), dtype=bool)
    bits[0, :, 1] = True     # record 0
    bits[0, :, 3] = True     # record 1
    bits[1, 0, 1:4] = True   # record 0
    bits[1, 2, 1:4] = True   # record 1
    return bits


def gap_clip():
    """An object that vanishes for one frame."""
    bits = np.zeros((4, 4, 8), dtype=bool)
    for t in (0, 1, 3):
        bits[t, 1:3, 2:5] = True
    return bits


def excluded_clip():
    """K = 2, min_area = 2.  Frame 0: records 0 and 1, a third component
    beyond K and a single pixel under min_area; frame 1: one bar across all
    four."""
    bits = np.zeros((2, 9, 12), dtype=bool)
    bits[0, 0, 0:2] = True    # record 0, 2 pixels
    bits[0, 2, 0:3] = True    # record 1, 3 pixels
    bits[0, 4, 0:6] = True    # component 2 >= K: takes no part although it overlaps most
    bits[0, 6, 0] = True      # 1 pixel < min_area
    bits[1, 0:8, 0] = True    # a column through all of them
    bits[1, 4, 0:6] = True
    return bits
