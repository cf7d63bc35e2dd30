"""The specification of dips_mask_components in plain numpy / Python: a
union-find over the unpacked bits of every frame, written from the
definitions in include/dips_hip.h (anchor = first pixel in row-major order,
kept = area >= min_area, order = ascending anchor, integer centroid)."""
import numpy as np

FIELDS = ("x0", "y0", "x1", "y1", "area", "anchor", "cx256", "cy256")
X0, Y0, X1, Y1, AREA, ANCHOR, CX256, CY256 = range(8)


def row_bytes(w):
    return 4 * ((w + 31) // 32)


def pack(bits, pad=0):
    """bool [n, h, w] -> the mask bytes [n, h, row_bytes]; pad = 1 sets the
    pad bits of every row."""
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    full = np.full((n, h, 8 * row_bytes(w)), bool(pad))
    full[..., :w] = bits
    return np.packbits(full, axis=-1, bitorder="little")


def unpack(mask_bytes, w):
    return np.unpackbits(np.asarray(mask_bytes, dtype=np.uint8), axis=-1, bitorder="little")[..., :w].astype(bool)


def _centroid256(s, area):
    return (s // area) * 256 + ((s % area) * 256) // area


def label_frame(bits, connectivity):
    """bits bool [h, w] -> (root [h, w] int64: the anchor of the pixel's
    component, -1 for a clear bit)."""
    h, w = bits.shape
    parent = np.arange(h * w, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    def union(x, y):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)

    near = [(0, -1), (-1, 0)] if connectivity == 4 else [(0, -1), (-1, -1), (-1, 0), (-1, 1)]
    ys, xs = np.nonzero(bits)
    for j, i in zip(ys.tolist(), xs.tolist()):
        for dj, di in near:
            jj, ii = j + dj, i + di
            if 0 <= jj and 0 <= ii < w and bits[jj, ii]:
                union(j * w + i, jj * w + ii)
    root = np.full((h, w), -1, dtype=np.int64)
    for j, i in zip(ys.tolist(), xs.tolist()):
        root[j, i] = find(j * w + i)
    return root


def components(mask_bytes, w, connectivity=8, min_area=1, max_boxes=64, labels=True):
    """(counts uint32 [n], boxes uint32 [n, K, 8], labels uint32 [n, h, w] or
    None) of the mask bytes [n, h, row_bytes(w)]."""
    assert connectivity in (4, 8)
    bits = unpack(mask_bytes, w)
    n, h, _ = bits.shape
    counts = np.zeros(n, dtype=np.uint32)
    boxes = np.zeros((n, max_boxes, 8), dtype=np.uint32)
    lab = np.zeros((n, h, w), dtype=np.uint32) if labels else None
    for t in range(n):
        root = label_frame(bits[t], connectivity)
        stats = {}
        ys, xs = np.nonzero(bits[t])
        for j, i in zip(ys.tolist(), xs.tolist()):
            s = stats.setdefault(int(root[j, i]), [i, j, i, j, 0, 0, 0])
            s[0], s[1], s[2], s[3] = min(s[0], i), min(s[1], j), max(s[2], i), max(s[3], j)
            s[4] += 1
            s[5] += i
            s[6] += j
        kept = [a for a in sorted(stats) if stats[a][4] >= min_area]
        counts[t] = len(kept)
        label_of = np.zeros(h * w + 1, dtype=np.uint32)  # by anchor; [-1] (a clear bit) stays 0
        for k, a in enumerate(kept):
            x0, y0, x1, y1, area, si, sj = stats[a]
            if k < max_boxes:
                boxes[t, k] = [x0, y0, x1 + 1, y1 + 1, area, a, _centroid256(si, area), _centroid256(sj, area)]
            label_of[a] = k + 1
        if lab is not None:
            lab[t] = label_of[root]
    return counts, boxes, lab
