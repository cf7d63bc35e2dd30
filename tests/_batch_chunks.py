"""The frame chunks of the two batch kernels (compat_batch.hip, alt_batch_kernel
in alt_kernels.hip) restated, and the cases tests/test_gpu_batch_chunks.py
runs at the chunk edges.  No GPU and no library here:
tests/test_batch_chunks_cpu.py checks the restatement against
dips_amd/csrc/batch_chunks.h and the case list against its coverage
conditions.

A launch of n frames is cut into (tile, chunk) items; every chunk after the
first rebuilds its per-pixel state from HBM.  While the items of ceil(n / 16)
chunks still fit the resident wave slots the plan depends on n alone
(plan_small), and `premise` says when that is so on a device of `cus` compute
units for every kernel form: the smallest tile is 128 vecs of 4 pixels
(kUnrollAlt = kUnrollCompatBatch = 2 vecs per lane) and every form has at
least 4 wave slots per compute unit resident.
"""
import numpy as np


def ceil_div(a, b):
    return -(-a // b)


def plan(n, n_tiles, resident):
    """batch_chunks.h batch_chunk_plan: (chunk, n_chunks)."""
    k = ceil_div(resident, n_tiles)
    k = max(min(k, ceil_div(n, 16)), 1)
    chunk = ceil_div(n, k)
    return chunk, ceil_div(n, chunk)


def plan_small(n):
    """The plan wherever n_tiles * ceil(n / 16) <= resident."""
    k = ceil_div(n, 16)
    chunk = ceil_div(n, k)
    return chunk, ceil_div(n, chunk)


def premise(n, n_vec, cus):
    return ceil_div(n_vec, 128) * ceil_div(n, 16) <= 4 * cus


def chunk_starts(n):
    chunk, n_chunks = plan_small(n)
    return [c * chunk for c in range(n_chunks)]


def middle_start(n):
    """First frame of the middle chunk (chunk n_chunks // 2; with two chunks
    the second); 0 when the launch is one chunk."""
    s = chunk_starts(n)
    return s[len(s) // 2]


# width, height: 64 x 32 is 512 vecs, whole tiles of 128 and of 256 vecs;
# 44 x 23 is 253 vecs: the second 128-vec tile is ragged and the one 256-vec
# tile of the table kernels ends past the frame (npx % 4 == 0 still holds)
SHAPES = {"whole": (64, 32), "ragged": (44, 23)}

# launch lengths: 16 one chunk (the control), 17 -> 9 + 8, 33 -> 3 x 11,
# 49 -> 13, 13, 13, 10, 100 -> 6 x 15 + 10
LENGTHS = (16, 17, 33, 49, 100)

# dips_alt snapshot placements, launch-local frame indices
PLACEMENTS = ("none", "first", "before_edge", "on_edge", "both_edge", "last_chunk_start", "last", "every", "random")
# the ones that need a chunk edge inside the launch
EDGE_PLACEMENTS = ("before_edge", "on_edge", "both_edge", "last_chunk_start")


def placement(name, m, seed=0):
    """Sorted launch-local snapshot frames of a placement in a launch of m
    frames (the edge placements need m >= 17)."""
    t0 = middle_start(m)
    if name in EDGE_PLACEMENTS and t0 == 0:
        raise ValueError(f"{name}: a launch of {m} frames is one chunk")
    if name == "none":
        return []
    if name == "first":
        return [0]
    if name == "before_edge":
        return [t0 - 1]
    if name == "on_edge":
        return [t0]
    if name == "both_edge":
        return [t0 - 1, t0]
    if name == "last_chunk_start":
        return [chunk_starts(m)[-1]]
    if name == "last":
        return [m - 1]
    if name == "every":
        return list(range(m))
    if name == "random":
        rng = np.random.default_rng(1000 + 31 * m + seed)
        return np.flatnonzero(rng.random(m) < 0.15).tolist()
    raise ValueError(name)


def moved_by_one(name, m, seed=0):
    """The placement with the flag nearest the middle chunk's first frame
    moved by one frame (onto a flagged frame: dropped); `none` gains a flag
    on that first frame instead.  What an off-by-one at a chunk edge would
    compute."""
    at = placement(name, m, seed)
    t0 = middle_start(m)
    if not at:
        return [t0]
    i = min(at, key=lambda t: (abs(t - t0), t))
    j = i + 1 if i + 1 < m else i - 1
    return sorted((set(at) - {i}) | {j})


def flags_of(at, m):
    f = np.zeros(m, dtype=bool)
    f[list(at)] = True
    return f


CONTENTS = ("random", "ties", "still")


def make_frames(shape, n, content, seed, still_at=None):
    """n RGBA8 frames [n, h, w, 4]: i.i.d. bytes; bytes from {0, 1, 2, 128,
    255} (ties in the 4-way upper median and in min); or i.i.d. bytes with the
    frames still_at-2 .. still_at+1 equal (one frame held across a chunk
    edge at still_at)."""
    w, h = SHAPES[shape]
    rng = np.random.default_rng(seed)
    if content == "ties":
        return np.array([0, 1, 2, 128, 255], dtype=np.uint8)[rng.integers(0, 5, (n, h, w, 4))]
    f = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    if content == "still":
        if still_at is None or still_at < 2 or still_at + 1 >= n:
            raise ValueError("still: no chunk edge to hold a frame across")
        f[still_at - 2:still_at + 2] = f[still_at]
    elif content != "random":
        raise ValueError(content)
    return f


# kernel forms: the epilogue-table kernel (default), or the arithmetic kernel
# (DIPS_FLAG_CROSSCHECK) with the fast or with the specification epilogue
FORMS = ("table", "fast", "spec")
# (filter, scalar or sensitivity) per form: sigmoid 0, inverse sigmoid 1, none 255
FORM_VARIANTS = {
    "table": ((0, 5.0), (1, 0.7), (255, 5.0), (0, 200.0)),
    "fast": ((0, 5.0), (255, 5.0)),
    "spec": ((1, 5.0), (0, 200.0)),
}


def form_of(crosscheck, filt, k):
    """The kernel form the library picks (dips_kernels.h alt_fast_epilogue_ok)."""
    if not crosscheck:
        return "table"
    if filt == 1:
        return "spec"
    if filt != 0:
        return "fast"
    a = abs(float(np.float32(k)))
    return "fast" if a <= 160.0 and (a == 0.0 or a >= 2.0 ** -60) else "spec"


class _Cycle:
    def __init__(self, items, start=0):
        self.items, self.i = tuple(items), start

    def __call__(self):
        v = self.items[self.i % len(self.items)]
        self.i += 1
        return v


def _build(family):
    """(family, shape, m, form, chroma, filter, scalar, colorize, placement,
    content) rows.  ComputeState takes no snapshots: its placement is None."""
    alt = family == "alt"
    out, seen = [], set()
    variant = {f: _Cycle(FORM_VARIANTS[f]) for f in FORMS}
    shape, form, chroma = _Cycle(SHAPES), _Cycle(FORMS), _Cycle(range(4))
    colorize = _Cycle((True, False, False, True, True))
    content = _Cycle(("random", "ties", "still", "ties", "random", "still", "still"))
    place = _Cycle(PLACEMENTS, 2)

    def add(sh, m, fo, ch, pl, co):
        filt, k = variant[fo]()
        row = (family, sh, m, fo, ch, filt, k, colorize(), pl if alt else None, co)
        key = row[:7] + row[8:]
        if key not in seen:
            seen.add(key)
            out.append(row)

    # every kernel form x chroma at 3 chunks of 11
    for fo in FORMS:
        for ch in range(4):
            add(shape(), 33, fo, ch, place(), content())
    # every placement (dips_alt) and every content at every launch length of several chunks
    for m in LENGTHS[1:]:
        for pl in (PLACEMENTS if alt else (None,) * len(CONTENTS)):
            add(shape(), m, form(), chroma(), pl, content())
        for co in CONTENTS:
            add(shape(), m, form(), chroma(), place(), co)
        form(), chroma()  # one step out of phase per length: a placement or content meets other forms and chromas
    # both shapes on every kernel form at 13, 13, 13, 10
    for fo in FORMS:
        for sh in SHAPES:
            add(sh, 49, fo, chroma(), place(), content())
    # the control: one chunk
    for fo, pl in zip(FORMS, ("none", "first", "last")):
        add(shape(), 16, fo, chroma(), pl, "random")
    return out


CASES = _build("alt") + _build("compat")


def case_id(c):
    family, shape, m, form, chroma, filt, k, colorize, pl, content = c
    return f"{family}-{shape}-m{m}-{form}-ch{chroma}-f{filt}-k{k:g}-{'col' if colorize else 'gray'}-{pl}-{content}"


def case_seed(c):
    """A seed that is a function of the case alone."""
    return sum((i + 1) * b for i, b in enumerate(case_id(c).encode())) % (2 ** 31)


def oracle_alt(oracle, shape, colorize, window, k, filt, chroma, frames, flags):
    """oracle.AltCompute(2, ...) run frame by frame."""
    w, h = SHAPES[shape]
    ref = oracle.AltCompute(2, w, h, colorize, window, k, filt, chroma)
    return np.stack([ref.send_frame(f, bool(s)) for f, s in zip(frames, flags)])
