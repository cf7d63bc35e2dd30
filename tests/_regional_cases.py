"""Drawn cases of the regional products of the difference series -- the grid,
the per-pixel sums, the change mask, the change times and the components of
the mask -- and their reference from the C oracle (oracle/dips_oracle.c).  The
GPU test (test_gpu_regional_fuzz.py) and the CPU checks of the draw
(test_regional_edges_cpu.py) share this module; there are no tests in it.

draw_case(rng) draws one case: format, mode, chroma, tau (test_gpu_fuzz's
_draw_tau: uniform values and the edges 0, k/255 and 2^-5 with their f32
neighbours, 1), a small frame shape (ragged, around the mask's word edges, or
narrower than a vec), the batch length (1..11, one case in ten 33..40, where
the mask and times geometries first cut the frames into parts), the region,
an explicit reference or none, the content, and the arguments of the five
calls.  Every array comes from `rng` alone, so case i of a seed is the same
whichever cases are run.

reference(case) computes every expected output from the oracle: one pass of
oracle.series over the 1x1 crops of the region gives the series per pixel
[n, rh, rw, 4]; the sums are that summed over t, the mask bits its count
column, the times the fold of the bits, the components those of the packed
bits; a grid cell is oracle.series on the cell's crop (SI of a cell is
defined by the oracle on the cell, not by a sum of pixels).  A case that is
run in two chunks has the reference of the whole clip.

step_walk is content that sits on the threshold: every pixel moves by exactly
+-k bytes per frame, all its channels together, so |dI| is an f32 difference
of rounded quotients close to f32(k / 255) and the decision at that tau and
its two neighbours rests on the rounding (rounding_critical_share)."""
import functools

import numpy as np

from _components_ref import components, pack
from oracle import oracle
from test_gpu_fuzz import _draw_tau
from test_grid_cpu import py_cell
from test_pixel_times_cpu import fold_times

F32 = np.float32
ISI_TAU = float(F32(1 / 32))  # series_v2_isi: the integer intensity sum from here on

CONTENT_KINDS = ("iid", "synth", "walk3", "sparse", "step_walk")
ARRAY_KEYS = ("frames", "ref")


def tau_neighbours(k):
    """(below, at, above): f32(k / 255) and its two f32 neighbours, as floats."""
    t = F32(k / 255)
    return float(np.nextafter(t, F32(0))), float(t), float(np.nextafter(t, F32(2)))


def step_numerator(tau):
    """k if tau is f32(k / 255) or one of its f32 neighbours for 1 <= k <= 127, else None."""
    k = int(round(float(tau) * 255))
    if 1 <= k <= 127 and float(tau) in tau_neighbours(k):
        return k
    return None


def step_walk(rng, c, w, h, n, k):
    """Frame 0 i.i.d. bytes; for every later frame each pixel draws a sign and
    all its channels move by +-k together (by the other sign if that would
    take a channel out of [0, 255]), then clip."""
    shape = (h, w) if c == 1 else (h, w, c)
    out = np.empty((n,) + shape, dtype=np.uint8)
    cur = rng.integers(0, 256, shape, dtype=np.int16)
    out[0] = cur
    for t in range(1, n):
        s = np.where(rng.integers(0, 2, (h, w)) == 1, k, -k).astype(np.int16)
        if c != 1:
            s = s[..., None]
        nxt = cur + s
        out_of_range = (nxt < 0) | (nxt > 255)
        if c != 1:
            out_of_range = out_of_range.any(axis=-1, keepdims=True)
        cur = np.clip(np.where(out_of_range, cur - s, nxt), 0, 255).astype(np.int16)
        out[t] = cur
    return out


def _content(rng, kind, c, w, h, n, k):
    shape = (n, h, w) if c == 1 else (n, h, w, c)
    if kind == "iid":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "synth":
        return oracle.synth(c, w, h, int(rng.integers(0, 1 << 30)), int(rng.integers(0, 1000)), n)
    if kind == "walk3":  # the slowly varying clip of test_gpu_fuzz._content
        base = rng.integers(0, 256, shape[1:], dtype=np.int16)
        steps = rng.integers(-3, 4, shape, dtype=np.int16).cumsum(axis=0)
        return np.clip(base[None] + steps, 0, 255).astype(np.uint8)
    if kind == "sparse":  # repeated frames with a few pixels rewritten, extremes included
        f = np.repeat(rng.integers(0, 256, (1,) + shape[1:], dtype=np.uint8), n, axis=0)
        for t in range(1, n):
            m = rng.random(shape[1:]) < 0.05
            f[t][m] = rng.choice(np.array([0, 255, 1, 254, 128], dtype=np.uint8), size=int(m.sum()))
        return f
    return step_walk(rng, c, w, h, n, k)


def _draw_shape(rng):
    kind = int(rng.integers(0, 3))
    if kind == 0:  # ragged
        return int(rng.integers(1, 81)), int(rng.integers(1, 15))
    if kind == 1:  # around the mask's word edges
        return int(rng.choice([31, 32, 33, 63, 64, 65])), int(rng.integers(1, 7))
    return int(rng.integers(1, 4)), int(rng.integers(1, 41))  # narrower than a vec


def _draw_roi(rng, w, h):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return None
    if kind == 1:  # anywhere inside the frame
        rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        return int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh
    # ends at the frame's bottom-right corner, or one pixel short of it
    # (where the frame has a second pixel in that direction)
    ex = w if kind == 2 or w < 2 else w - 1
    ey = h if kind == 2 or h < 2 else h - 1
    x, y = int(rng.integers(0, ex)), int(rng.integers(0, ey))
    return x, y, ex - x, ey - y


def region_of(case):
    """(x, y, rw, rh) of the case's region."""
    return case["roi"] if case["roi"] is not None else (0, 0, case["w"], case["h"])


def draw_case(rng):
    c = int(rng.choice([1, 3, 3, 4, 4]))  # GRAY8 (the generic kernels) at half the weight
    mode = int(rng.integers(0, 2))
    chroma = 0 if c == 1 else int(rng.integers(0, 4))
    tau = _draw_tau(rng)
    w, h = _draw_shape(rng)
    n = int(rng.integers(1, 12)) if rng.random() < 0.9 else int(rng.integers(33, 41))
    roi = _draw_roi(rng, w, h)
    rw, rh = (w, h) if roi is None else roi[2:]
    explicit_ref = bool(rng.random() < 0.5)
    kind = CONTENT_KINDS[int(rng.integers(0, len(CONTENT_KINDS)))]
    k = step_numerator(tau) or 8
    # an explicit reference is the frame before the clip, of the clip's own
    # content, so that frame 0 sits as close to it as the frames to each other
    clip = _content(rng, kind, c, w, h, n + 1 if explicit_ref else n, k)
    frames = np.ascontiguousarray(clip[1:]) if explicit_ref else clip
    ref = np.ascontiguousarray(clip[0]) if explicit_ref else None
    rows, cols = int(rng.integers(1, min(rh, 6) + 1)), int(rng.integers(1, min(rw, 6) + 1))
    if rng.random() < 0.1:  # one-pixel cells
        if rng.random() < 0.5:
            rows = rh
        else:
            cols = rw
    t0 = int(rng.choice([0, 7, 2 ** 31]))
    connectivity = int(rng.choice([4, 8]))
    min_area = int(rng.choice([1, 2, 5]))
    max_boxes = int(rng.choice([0, 1, 8, 64]))
    labels = bool(rng.random() < 0.5)
    split = int(rng.integers(1, n)) if n >= 2 and rng.random() < 0.5 else None
    part_frames = None
    if n >= 33:
        part_frames = [None, 16, 17, n][int(rng.integers(0, 4))]
    device = bool(rng.random() < 0.5)
    offs = [int(x) for x in rng.integers(0, 4, 2)] if rng.random() < 0.5 else [0, 0]  # frames, ref
    guard = int(rng.choice([1, 2, 3, 16]))  # words before a device output: the ABI's alignment and no more
    frames.setflags(write=False)
    if ref is not None:
        ref.setflags(write=False)
    return dict(c=c, mode=mode, chroma=chroma, tau=tau, w=w, h=h, n=n, roi=roi, explicit_ref=explicit_ref,
                content=kind, k=k, rows=rows, cols=cols, t0=t0, connectivity=connectivity, min_area=min_area,
                max_boxes=max_boxes, labels=labels, split=split, part_frames=part_frames, device=device,
                offs=offs, guard=guard, frames=frames, ref=ref)


@functools.lru_cache(maxsize=None)
def drawn_cases(seed, count):
    """Cases 0 .. count - 1 of `seed`, each with its index under "case"."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        case = draw_case(rng)
        case["case"] = i
        out.append(case)
    return tuple(out)


def describe(case):
    """The case without its arrays, for an assertion message."""
    return {k: v for k, v in case.items() if k not in ARRAY_KEYS}


def tau_form(tau):
    """0: tau = 0; 1: 0 < tau < 2^-5 (f64 intensity sum); 2: tau >= 2^-5 (integer sum)."""
    return 0 if tau == 0 else (1 if tau < ISI_TAU else 2)


def _crop_frames(frames, rect):
    x, y, rw, rh = rect
    return np.ascontiguousarray(frames[:, y:y + rh, x:x + rw])


def _crop_ref(ref, rect):
    x, y, rw, rh = rect
    return None if ref is None else np.ascontiguousarray(ref[y:y + rh, x:x + rw])


def pixel_series(frames, mode, tau, chroma, ref, rect):
    """[n, rh, rw, 4] uint64: the oracle's series of the 1x1 crop of every pixel of rect."""
    x0, y0, rw, rh = rect
    out = np.zeros((frames.shape[0], rh, rw, 4), dtype=np.uint64)
    for y in range(rh):
        for x in range(rw):
            one = (x0 + x, y0 + y, 1, 1)
            out[:, y, x] = oracle.series(_crop_frames(frames, one), mode=mode, tau=tau, chroma=chroma,
                                         ref=_crop_ref(ref, one))[0]
    return out


def region_series(frames, mode, tau, chroma, ref, rect):
    """[n, 4] uint64: the oracle's series of the frames and the reference cropped to rect."""
    return oracle.series(_crop_frames(frames, rect), mode=mode, tau=tau, chroma=chroma, ref=_crop_ref(ref, rect))[0]


def oracle_bits(case, tau=None):
    """bool [n, rh, rw]: the count of the oracle's per-pixel series (at the case's tau or another)."""
    cnt = pixel_series(case["frames"], case["mode"], case["tau"] if tau is None else tau, case["chroma"],
                       case["ref"], region_of(case))[..., 2]
    assert cnt.max(initial=0) <= 1
    return cnt != 0


def grid_reference(case):
    """[n, rows, cols, 4] uint64: the oracle's series of every cell's crop."""
    rows, cols = case["rows"], case["cols"]
    grid = np.zeros((case["frames"].shape[0], rows, cols, 4), dtype=np.uint64)
    for r in range(rows):
        for cc in range(cols):
            cell = py_cell(case["w"], case["h"], rows, cols, r, cc, case["roi"])
            grid[:, r, cc] = region_series(case["frames"], case["mode"], case["tau"], case["chroma"], case["ref"], cell)
    return grid


def reference(case):
    frames, ref, rect = case["frames"], case["ref"], region_of(case)
    mode, tau, chroma = case["mode"], case["tau"], case["chroma"]
    _, _, rw, rh = rect
    per_pixel = pixel_series(frames, mode, tau, chroma, ref, rect)
    assert per_pixel[..., 2].max(initial=0) <= 1
    bits = per_pixel[..., 2] != 0
    grid = grid_reference(case)
    mask = pack(bits)
    counts, boxes, lab = components(mask, rw, case["connectivity"], case["min_area"], case["max_boxes"],
                                    case["labels"])
    return dict(per_pixel=per_pixel, bits=bits, mask=mask, sums=per_pixel.sum(axis=0, dtype=np.uint64), grid=grid,
                region=region_series(frames, mode, tau, chroma, ref, rect), times=fold_times(bits, case["t0"]),
                counts=counts, boxes=boxes, labels=lab)


EDGE_W, EDGE_H, EDGE_N, EDGE_ROI = 37, 13, 9, (3, 2, 33, 10)
EDGE_SEED = 0xED6E


@functools.lru_cache(maxsize=None)
def edge_frames(c, k):
    """The clip of the threshold sweep: step_walk(k) at 37x13x9, one seed per (format, k)."""
    a = step_walk(np.random.default_rng([EDGE_SEED, c, k]), c, EDGE_W, EDGE_H, EDGE_N, k)
    a.setflags(write=False)
    return a


def edge_case(c, mode, chroma, k, which):
    """The case dict of one point of the threshold sweep; `which`: below, at or above f32(k / 255)."""
    tau = dict(zip(("below", "at", "above"), tau_neighbours(k)))[which]
    return dict(c=c, mode=mode, chroma=chroma, tau=tau, w=EDGE_W, h=EDGE_H, n=EDGE_N, roi=EDGE_ROI,
                content="step_walk", k=k, which=which, rows=2, cols=3, t0=7, connectivity=4, min_area=1,
                max_boxes=64, labels=True, frames=edge_frames(c, k), ref=None)


def rounding_critical_share(frames, mode, chroma, k):
    """Share of the pixel-frames of frames 1 .. n - 1 whose oracle bit differs
    between the f32 neighbour below f32(k / 255) and the one above it."""
    below, _, above = tau_neighbours(k)
    rect = (0, 0, frames.shape[2], frames.shape[1])
    lo = pixel_series(frames, mode, below, chroma, None, rect)[1:, ..., 2]
    hi = pixel_series(frames, mode, above, chroma, None, rect)[1:, ..., 2]
    return float((lo != hi).mean())
