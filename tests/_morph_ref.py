"""The specification of dips_mask_morph in plain numpy, written from the
definition in include/dips_hip.h: unpack the mask, pad every frame with the
operation's outside value (clear before a dilation, set before an erosion),
OR / AND the shifted copies over the structuring element, pack again.  Frames
are a batch axis throughout: nothing here reaches across them."""
import numpy as np

from _components_ref import pack, unpack

ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3
BOX, DIAMOND = 0, 1
MAX_RADIUS = 15
OP_NAMES = ("erode", "dilate", "open", "close")
SHAPE_NAMES = ("box", "diamond")


def offsets(shape, rx, ry):
    """The structuring element as a list of (dx, dy)."""
    if shape == BOX:
        return [(dx, dy) for dy in range(-ry, ry + 1) for dx in range(-rx, rx + 1)]
    assert shape == DIAMOND and rx == ry
    return [(dx, dy) for dy in range(-rx, rx + 1) for dx in range(-rx, rx + 1) if abs(dx) + abs(dy) <= rx]


def _elementary(bits, dilate, shape, rx, ry):
    """bool [n, h, w] -> bool [n, h, w]: one dilation or erosion."""
    n, h, w = bits.shape
    padded = np.full((n, h + 2 * ry, w + 2 * rx), not dilate)
    padded[:, ry:ry + h, rx:rx + w] = bits
    if shape == BOX:
        # separable: along the rows, then along the columns
        acc = padded[:, :, 0:w].copy()
        for dx in range(1, 2 * rx + 1):
            acc = (acc | padded[:, :, dx:dx + w]) if dilate else (acc & padded[:, :, dx:dx + w])
        out = acc[:, 0:h].copy()
        for dy in range(1, 2 * ry + 1):
            out = (out | acc[:, dy:dy + h]) if dilate else (out & acc[:, dy:dy + h])
        return out
    out = np.full((n, h, w), not dilate)
    for dx, dy in offsets(shape, rx, ry):
        part = padded[:, ry + dy:ry + dy + h, rx + dx:rx + dx + w]
        out = (out | part) if dilate else (out & part)
    return out


def morph_bits(bits, op, shape=BOX, rx=1, ry=None):
    """bool [n, h, w] -> bool [n, h, w]."""
    ry = rx if ry is None else ry
    assert op in (ERODE, DILATE, OPEN, CLOSE) and shape in (BOX, DIAMOND)
    assert 0 <= rx <= MAX_RADIUS and 0 <= ry <= MAX_RADIUS and (shape == BOX or rx == ry)
    bits = np.asarray(bits, dtype=bool)
    if op == ERODE:
        return _elementary(bits, False, shape, rx, ry)
    if op == DILATE:
        return _elementary(bits, True, shape, rx, ry)
    if op == OPEN:
        return _elementary(_elementary(bits, False, shape, rx, ry), True, shape, rx, ry)
    return _elementary(_elementary(bits, True, shape, rx, ry), False, shape, rx, ry)


def morph(mask_bytes, w, op, shape=BOX, rx=1, ry=None):
    """The mask bytes [n, h, row_bytes(w)] -> the same layout, pad bits 0."""
    return pack(morph_bits(unpack(mask_bytes, w), op, shape, rx, ry))


def draw_case(k):
    """Case k of the randomized draw: (bits bool [n, h, w], op, shape, rx, ry)."""
    W = [1, 2, 31, 32, 33, 63, 64, 65, 97, 130]
    H = [1, 2, 3, 29, 64, 70]
    R = [0, 1, 1, 2, 3, 5, 15]
    P = [.05, .3, .7, .95]
    g = np.random.default_rng([0xD1F5, k])
    w = int(g.choice(W))
    h = int(g.choice(H))
    n = int(g.integers(1, 5))
    op = int(g.integers(0, 4))
    shape = int(g.integers(0, 2))
    rx = int(g.choice(R))
    ry = rx if shape == 1 else int(g.choice(R))
    p = g.choice(P)
    x = g.random((n, h, w)) < p
    for val in (True, False):  # three rectangles set, then three cleared
        for _ in range(3):
            t = g.integers(0, n)
            x0 = g.integers(0, w)
            y0 = g.integers(0, h)
            x1 = g.integers(x0, w) + 1
            y1 = g.integers(y0, h) + 1
            x[t, y0:y1, x0:x1] = val
    return x, op, shape, rx, ry


def nontrivial(bits_in, bits_out):
    """The output has both set and clear bits and differs from the input."""
    return bool(bits_out.any() and not bits_out.all() and not np.array_equal(bits_in, bits_out))
