"""The cases that run a mask product on scratch another call left dirty, the
dirt itself, and one way to call every mask product through host arrays or
device tensors.  There are no tests in this module: test_mask_reuse_cpu.py
proves on mask_scratch.h alone that every call under test lies wholly inside
bytes its dirt owned, at other plane offsets; test_gpu_mask_reuse.py runs them
on the device.

The handle's cc_scratch (mask_abi.hip plan_labelling) is never cleared between
calls: the labelling kernels write every slot they later read, and the tracks
clear only ov and next_id.  A dirt is a call made on the same handle directly
before the call under test, at another width, so the call's planes lie on
bytes that held planes of another kind:
  ones     mask_tracks on all-ones frames, K = 256: huge areas and sums,
           label 1 everywhere, every parent pointing low, one large ov entry
  noise    mask_components (4-connectivity) with labels on density-0.5 bits: thousands of
           roots, min_x = ~0 patterns, labels in the thousands
  checker  mask_tracks under 4-connectivity, K = 256, with a state, on a board
           and its complement in alternating pairs of frames: non-zero ov,
           cprev, hrank, heads, base and both carries
dirt_shape gives the dirt's width 2 w + 37, height h + 3 and enough frames
(at least n + 2) for its plan to hold the call's plan."""
import collections
import functools

import numpy as np

import _components_ref as cref
import _select_ref as selref
import _shapes_ref as shref
import _tracks_ref as tref
import test_mask_scratch_cpu as scratch

POISON = 0xA5A5A5A5
DIRTS = ("ones", "noise", "checker")
DIRT_K = 256

# product: components, shapes, tracks, select, fill_holes; kw: the product's arguments.
Call = collections.namedtuple("Call", "name product w h n kw")


def _call(name, product, w, h, n, **kw):
    return Call(name, product, w, h, n, tuple(sorted(kw.items())))


# The suite's word-edge shapes: w in {33, 65, 97}, h in {5, 29}, n in {1, 7}; every value of every argument the
# products take appears at least once.  tracks' mode: "none" no prev and no state, "state" a state without prev,
# "carried" the clip in three calls (frames 0-2, 3-4, 5-6) with prev and state, a dirt between the calls.
CALLS = (
    _call("components-labels-k0", "components", 33, 5, 1, labels=True, max_boxes=0, chunk_frames=0, connectivity=8, min_area=1),
    _call("components-k3-chunk1", "components", 65, 29, 7, labels=False, max_boxes=3, chunk_frames=1, connectivity=4, min_area=4),
    _call("components-labels-k64-chunk3", "components", 97, 5, 7, labels=True, max_boxes=64, chunk_frames=3, connectivity=8, min_area=4),
    _call("components-labels-k3", "components", 97, 29, 7, labels=True, max_boxes=3, chunk_frames=0, connectivity=4, min_area=1),
    _call("components-k64-one-frame", "components", 33, 29, 1, labels=False, max_boxes=64, chunk_frames=1, connectivity=8, min_area=1),
    _call("components-k0-chunk3", "components", 65, 5, 7, labels=False, max_boxes=0, chunk_frames=3, connectivity=4, min_area=1),
    _call("shapes-weights", "shapes", 65, 29, 7, weights=True, max_boxes=8, chunk_frames=0, connectivity=8, min_area=1),
    _call("shapes-chunk3", "shapes", 33, 5, 7, weights=False, max_boxes=3, chunk_frames=3, connectivity=4, min_area=4),
    _call("shapes-weights-one-frame", "shapes", 97, 29, 1, weights=True, max_boxes=64, chunk_frames=0, connectivity=8, min_area=1),
    _call("tracks-k1", "tracks", 33, 29, 7, max_boxes=1, chunk_frames=0, mode="none", connectivity=8, min_area=1),
    _call("tracks-k8-chunk2-state", "tracks", 65, 5, 7, max_boxes=8, chunk_frames=2, mode="state", connectivity=4, min_area=1),
    _call("tracks-k256-chunk2", "tracks", 97, 29, 7, max_boxes=256, chunk_frames=2, mode="none", connectivity=8, min_area=4),
    _call("tracks-k256-state", "tracks", 97, 5, 7, max_boxes=256, chunk_frames=0, mode="state", connectivity=8, min_area=1),
    _call("tracks-k8-one-frame", "tracks", 33, 5, 1, max_boxes=8, chunk_frames=0, mode="none", connectivity=8, min_area=1),
    _call("tracks-k8-chunk2-carried", "tracks", 65, 29, 7, max_boxes=8, chunk_frames=2, mode="carried", connectivity=8, min_area=1),
    _call("tracks-k256-carried", "tracks", 33, 5, 7, max_boxes=256, chunk_frames=0, mode="carried", connectivity=4, min_area=1),
    _call("select-marker-n", "select", 65, 29, 7, marker="n", counts=True, connectivity=8, min_area=2, max_area=0,
          clear_border=False, dropped=False, chunk_frames=0),
    _call("select-marker-1-border", "select", 33, 5, 7, marker="1", counts=False, connectivity=4, min_area=1, max_area=0,
          clear_border=True, dropped=False, chunk_frames=3),
    _call("select-dropped", "select", 97, 29, 1, marker=None, counts=True, connectivity=8, min_area=3, max_area=40,
          clear_border=False, dropped=True, chunk_frames=0),
    _call("select-marker-n-dropped-border", "select", 97, 5, 7, marker="n", counts=False, connectivity=8, min_area=1,
          max_area=0, clear_border=True, dropped=True, chunk_frames=1),
    _call("fill-holes", "fill_holes", 97, 29, 7, connectivity=8, max_hole=0),
    _call("fill-holes-4-small", "fill_holes", 65, 5, 7, connectivity=4, max_hole=3),
)
BY_NAME = {c.name: c for c in CALLS}
CARRIED_CUTS = (0, 3, 5, 7)


def kw_of(call):
    return dict(call.kw)


# -- the scratch plans -------------------------------------------------------------------------

def plan_cases(call):
    """The (w, h, n_frames, chunk, K) of every label_scratch plan the call makes."""
    kw = kw_of(call)
    chunk = kw.get("chunk_frames", 0)
    if call.product != "tracks":
        return [(call.w, call.h, call.n, chunk, 0)]
    K = kw["max_boxes"]
    if kw["mode"] != "carried":
        return [(call.w, call.h, call.n, chunk, K)]
    return [(call.w, call.h, b - a, chunk, K) for a, b in zip(CARRIED_CUTS, CARRIED_CUTS[1:])]


def plan_bytes(case):
    """The bytes of a plan by the formulae of test_mask_scratch_cpu.parent_layout
    (test_mask_reuse_cpu.py asks the header itself)."""
    return scratch.parent_layout(*case)[1]


def dirt_shape(kind, call):
    """(w, h, n) of the dirt of `kind` in front of `call`."""
    w, h = 2 * call.w + 37, call.h + 3
    n = call.n + 2
    need = max(plan_bytes(c) for c in plan_cases(call))
    while plan_bytes(dirt_plan_case(kind, (w, h, n))) < need:
        n += 1
    return w, h, n


def dirt_plan_case(kind, shape):
    w, h, n = shape
    return (w, h, n, 0, 0 if kind == "noise" else DIRT_K)


@functools.lru_cache(maxsize=None)
def dirt_mask(kind, w, h, n):
    if kind == "ones":
        bits = np.ones((n, h, w), dtype=bool)
    elif kind == "noise":
        bits = np.random.default_rng([137, n, h, w]).random((n, h, w)) < 0.5
    else:
        jj, ii = np.mgrid[0:h, 0:w]
        board = (ii + jj) % 2 == 0
        bits = np.stack([board if (t // 2) % 2 == 0 else ~board for t in range(n)])
    m = cref.pack(bits, 1)
    m.setflags(write=False)
    return m


def run_dirt(runner, kind, call):
    """The dirt of `kind` for `call` on the runner's handle; what it returns
    is checked for one figure that shows the call did run."""
    w, h, n = dirt_shape(kind, call)
    mask = dirt_mask(kind, w, h, n)
    if kind == "noise":
        counts, _, labels = runner.components(mask, w, connectivity=4, labels=True, max_boxes=64)
        assert counts.min() > 1 and labels.max() == counts.max()
    elif kind == "ones":
        counts, _, links, _ = runner.tracks(mask, w, max_boxes=DIRT_K)
        assert counts.tolist() == [1] * n and links[n - 1, 0].tolist() == [0, w * h, 0, n - 1]
    else:
        state = np.zeros(1 + 2 * DIRT_K, dtype=np.uint32)
        counts, _, links, state = runner.tracks(mask, w, connectivity=4, max_boxes=DIRT_K, state=state)
        assert counts.min() >= DIRT_K and (links[1, :, tref.OVERLAP] == 1).all() and state[0] >= 2 * DIRT_K


# -- content -----------------------------------------------------------------------------------

def frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def bits_of(w, h, n, seed=0):
    """bool [n, h, w]: moving rectangles (links to follow) over sparse noise
    (components under min_area, holes, border pixels)."""
    rects = tref.moving_rectangles(seed, n, h, w, max(3, w // 12))
    noise = np.random.default_rng([139, seed, n, h, w]).random((n, h, w)) < 0.12
    return frozen(rects ^ noise)


@functools.lru_cache(maxsize=None)
def mask_of(w, h, n, seed=0):
    """The mask bytes of bits_of, every pad bit set."""
    return frozen(cref.pack(bits_of(w, h, n, seed), 1))


@functools.lru_cache(maxsize=None)
def marker_of(w, h, n, seed=0):
    return frozen(cref.pack(np.random.default_rng([149, seed, n, h, w]).random((n, h, w)) < 0.04, 1))


@functools.lru_cache(maxsize=None)
def weights_of(w, h, n, seed=0):
    return frozen(np.random.default_rng([151, seed, n, h, w]).integers(0, 256, (n, h, w), dtype=np.uint8))


# -- one call of every product, and its reference ----------------------------------------------

class Runner:
    """The mask products of one operator through its host handle (kind
    "host": numpy in, numpy out) or its device handle (kind "dev": tensors
    made here, outputs filled with POISON first, results copied back; all on
    torch's current stream)."""

    def __init__(self, op, kind):
        assert kind in ("host", "dev")
        self.op, self.kind = op, kind
        if kind == "dev":
            import torch
            self.torch = torch
            self.device = torch.device("cuda", op._dev.device)

    # device helpers
    def _in(self, a):
        return None if a is None else self.torch.from_numpy(np.array(a)).to(self.device)  # a copy: `a` may be read-only

    def _out(self, *shape):
        return self.torch.full(shape, POISON - (1 << 32), dtype=self.torch.int32, device=self.device)

    def _bytes(self, *shape):
        return self.torch.full(shape, POISON & 0xFF, dtype=self.torch.uint8, device=self.device)

    @staticmethod
    def _u32(t):
        return None if t is None else t.cpu().numpy().view(np.uint32)

    def _cm(self, mask, w):
        from dips_amd import ChangeMask
        return None if mask is None else ChangeMask(np.array(mask), w)  # a copy: `mask` may be read-only

    def components(self, mask, w, connectivity=8, min_area=1, max_boxes=64, labels=False, chunk_frames=0):
        n, h = mask.shape[:2]
        if self.kind == "host":
            r = self.op.mask_components(self._cm(mask, w), connectivity, min_area, max_boxes, labels, chunk_frames)
            return r.counts, r.boxes, r.labels
        counts = self._out(n)
        boxes = self._out(n, max_boxes, 8) if max_boxes else None
        lab = self._out(n, h, w) if labels else None
        self.op.run_mask_components_device(self._in(mask), w, counts, boxes, lab, connectivity, min_area, chunk_frames)
        return (self._u32(counts), self._u32(boxes) if max_boxes else np.zeros((n, 0, 8), dtype=np.uint32),
                self._u32(lab))

    def shapes(self, mask, w, weights=None, connectivity=8, min_area=1, max_boxes=64, chunk_frames=0):
        n = mask.shape[0]
        if self.kind == "host":
            r = self.op.mask_shapes(self._cm(mask, w), weights, connectivity, min_area, max_boxes, chunk_frames)
            return r.counts, r.boxes, r.shapes
        counts, boxes, shapes = self._out(n), self._out(n, max_boxes, 8), self._out(n, max_boxes, 16)
        self.op.run_mask_shapes_device(self._in(mask), w, counts, boxes, shapes, self._in(weights), connectivity,
                                       min_area, chunk_frames)
        return self._u32(counts), self._u32(boxes), self._u32(shapes)

    def tracks(self, mask, w, connectivity=8, min_area=1, max_boxes=64, chunk_frames=0, prev=None, state=None):
        n = mask.shape[0]
        if self.kind == "host":
            r = self.op.mask_tracks(self._cm(mask, w), connectivity, min_area, max_boxes, chunk_frames, prev, state)
            return r.counts, r.boxes, r.links, r.state
        counts, boxes, links = self._out(n), self._out(n, max_boxes, 8), self._out(n, max_boxes, 4)
        st = None if state is None else self._in(np.asarray(state, dtype=np.uint32).view(np.int32))
        self.op.run_mask_tracks_device(self._in(mask), w, counts, boxes, links, self._in(prev), st, connectivity,
                                       min_area, chunk_frames)
        return self._u32(counts), self._u32(boxes), self._u32(links), self._u32(st)

    def select(self, mask, w, marker=None, counts=True, **kw):
        """(mask bytes, counts or None); the host form always gives counts."""
        n = mask.shape[0]
        if self.kind == "host":
            out, c = self.op.mask_select(self._cm(mask, w), self._cm(marker, w), **kw)
            return out.bits, c
        out = self._bytes(*mask.shape)
        c = self._out(n) if counts else None
        self.op.run_mask_select_device(self._in(mask), w, out, self._in(marker), c, **kw)
        return out.cpu().numpy(), self._u32(c)

    def fill_holes(self, mask, w, connectivity=8, max_hole=0):
        """The device handle's composite in both kinds (mask_fill_holes goes there itself)."""
        if self.kind == "host":
            return self.op.mask_fill_holes(self._cm(mask, w), connectivity, max_hole).bits
        out, tmp = self._bytes(*mask.shape), self._bytes(*mask.shape)
        self.op.run_mask_fill_holes_device(self._in(mask), w, out, tmp, connectivity, max_hole)
        return out.cpu().numpy()

    def logic(self, a, w, lop, b=None):
        from dips_amd import MaskLogic
        if self.kind == "host":
            return self.op.mask_logic(self._cm(a, w), MaskLogic(lop), self._cm(b, w)).bits
        out = self._bytes(*a.shape)
        self.op.run_mask_logic_device(self._in(a), w, out, MaskLogic(lop), self._in(b))
        return out.cpu().numpy()

    def morph(self, mask, w, mop, shape, rx, ry):
        from dips_amd import MorphOp, MorphShape
        if self.kind == "host":
            return self.op.mask_morph(self._cm(mask, w), MorphOp(mop), rx, ry, MorphShape(shape)).bits
        out = self._bytes(*mask.shape)
        self.op.run_mask_morph_device(self._in(mask), w, out, MorphOp(mop), rx, ry, MorphShape(shape))
        return out.cpu().numpy()

    def vote(self, mask, w, window, votes, history=None):
        """(voted bytes, next history bytes)."""
        if self.kind == "host":
            out, nxt = self.op.mask_vote(self._cm(mask, w), window, votes, self._cm(history, w))
            return out.bits, nxt.bits
        out = self._bytes(*mask.shape)
        nxt = self._bytes(window - 1, *mask.shape[1:]) if window > 1 else None
        self.op.run_mask_vote_device(self._in(mask), w, out, window, votes, self._in(history), nxt)
        return out.cpu().numpy(), (nxt.cpu().numpy() if nxt is not None else np.zeros((0,) + mask.shape[1:], np.uint8))

    def counts(self, mask, w, rows=1, cols=1):
        if self.kind == "host":
            return self.op.mask_counts(self._cm(mask, w), rows, cols)
        out = self._out(mask.shape[0], rows, cols)
        self.op.run_mask_counts_device(self._in(mask), w, out, rows, cols)
        return self._u32(out)

    def times(self, mask, w, t0=0):
        if self.kind == "host":
            return self.op.mask_times(self._cm(mask, w), t0=t0).as_array()
        out = self._out(4, mask.shape[1], w)
        self.op.run_mask_times_device(self._in(mask), w, out, None, t0=t0)
        return self._u32(out)

    def sums(self, mask, w):
        if self.kind == "host":
            return self.op.mask_sums(self._cm(mask, w))
        out = self._out(mask.shape[1], w)
        self.op.run_mask_times_device(self._in(mask), w, None, out)
        return self._u32(out)

    def change_mask(self, frames):
        n, h, w = frames.shape[:3]
        if self.kind == "host":
            return self.op.change_mask(frames).bits
        out = self._bytes(n, h, cref.row_bytes(w))
        self.op.run_change_mask_device(self._in(frames), out)
        return out.cpu().numpy()

    def pixel_times(self, frames, t0=0):
        n, h, w = frames.shape[:3]
        if self.kind == "host":
            return self.op.pixel_times(frames, t0=t0).as_array()
        out = self._out(4, h, w)
        self.op.run_pixel_times_device(self._in(frames), out, t0=t0)
        return self._u32(out)


def same(got, want, what):
    """Every word of every output: got and want are tuples of arrays or None."""
    assert len(got) == len(want), what
    for k, (g, r) in enumerate(zip(got, want)):
        if r is None:
            assert g is None, (what, k)
            continue
        assert g is not None and g.dtype == r.dtype and g.shape == r.shape, (what, k, None if g is None else g.shape, r.shape)
        assert np.array_equal(g, r), (what, k, np.argwhere(g != r)[:5].tolist())


def _select_kw(kw):
    return {k: kw[k] for k in ("connectivity", "min_area", "max_area", "clear_border", "dropped")}


def _marker(call):
    m = kw_of(call)["marker"]
    return None if m is None else marker_of(call.w, call.h, call.n if m == "n" else 1)


@functools.lru_cache(maxsize=None)
def reference(call):
    """The outputs of the call from the suite's references (a tuple, as run gives it; computed once)."""
    kw, w = kw_of(call), call.w
    mask = mask_of(call.w, call.h, call.n)
    if call.product == "components":
        counts, boxes, lab = cref.components(mask, w, kw["connectivity"], kw["min_area"], kw["max_boxes"], labels=True)
        return tuple(frozen(a) for a in (counts, boxes, lab if kw["labels"] else None))
    if call.product == "shapes":
        wts = weights_of(call.w, call.h, call.n) if kw["weights"] else None
        return tuple(frozen(a) for a in shref.shapes(mask, w, wts, kw["connectivity"], kw["min_area"], kw["max_boxes"]))
    if call.product == "tracks":
        K = kw["max_boxes"]
        state = None if kw["mode"] == "none" else np.zeros(1 + 2 * K, dtype=np.uint32)
        return tuple(frozen(a) for a in tref.tracks(mask, w, kw["connectivity"], kw["min_area"], K, state=state))
    if call.product == "select":
        out, counts = selref.select_bytes(mask, w, _marker(call), **_select_kw(kw))
        return frozen(out), frozen(counts)
    return (frozen(selref.fill_holes_bytes(mask, w, kw["connectivity"], kw["max_hole"])),)


def run(runner, call, between=None):
    """The call on the runner's handle, as the tuple reference(call) gives;
    between(): made between the calls of a carried clip."""
    kw, w = kw_of(call), call.w
    mask = mask_of(call.w, call.h, call.n)
    if call.product == "components":
        return runner.components(mask, w, kw["connectivity"], kw["min_area"], kw["max_boxes"], kw["labels"],
                                 kw["chunk_frames"])
    if call.product == "shapes":
        wts = weights_of(call.w, call.h, call.n) if kw["weights"] else None
        return runner.shapes(mask, w, wts, kw["connectivity"], kw["min_area"], kw["max_boxes"], kw["chunk_frames"])
    if call.product == "tracks":
        K, args = kw["max_boxes"], (kw["connectivity"], kw["min_area"], kw["max_boxes"], kw["chunk_frames"])
        if kw["mode"] != "carried":
            state = None if kw["mode"] == "none" else np.zeros(1 + 2 * K, dtype=np.uint32)
            return runner.tracks(mask, w, *args, state=state)
        parts, state = [], np.zeros(1 + 2 * K, dtype=np.uint32)
        for a, b in zip(CARRIED_CUTS, CARRIED_CUTS[1:]):
            if a and between is not None:
                between()
            r = runner.tracks(mask[a:b], w, *args, prev=mask[a - 1] if a else None, state=state)
            parts.append(r[:3])
            state = r[3]
        return tuple(np.concatenate(x) for x in zip(*parts)) + (state,)
    if call.product == "select":
        out, counts = runner.select(mask, w, _marker(call), kw["counts"], chunk_frames=kw["chunk_frames"], **_select_kw(kw))
        return out, counts
    return (runner.fill_holes(mask, w, kw["connectivity"], kw["max_hole"]),)


def check(runner, call, what, between=None):
    got, want = run(runner, call, between), reference(call)
    if call.product == "select" and got[1] is None:   # the device form without counts
        want = (want[0], None)
    same(got, want, (call.name, runner.kind, what))


# -- the two looped grids ----------------------------------------------------------------------

LOGIC_THREADS = 256
# (name, w, h, n): mask_logic beyond kMaxBlocks blocks of 256 words
LOGIC_CASES = (("many-frames", 1000, 1000, 300), ("long-frame", 16416, 16400, 2))
# (name, w, h, rows, cols, n, chunked): mask_counts with more items than blocks
COUNTS_CASES = (("rows-200", 97, 200, 200, 7, 256, False), ("cells-share-words", 97, 200, 67, 97, 256, False),
                ("three-chunks", 2500, 2, 2, 2500, 8192, True))


def logic_geometry(w, h, n, max_blocks):
    """words, wpf, stride and dr of mask_logic_kernel on n frames of w x h."""
    wpf = ((w + 31) // 32) * h
    words = wpf * n
    stride = min((words + LOGIC_THREADS - 1) // LOGIC_THREADS, max_blocks) * LOGIC_THREADS
    return dict(words=words, wpf=wpf, stride=stride, dr=stride % wpf)


def logic_max_blocks(csrc):
    """kMaxBlocks of launch_mask_logic (mask_select.hip)."""
    import os
    import re
    with open(os.path.join(csrc, "mask_select.hip")) as f:
        m = re.search(r"constexpr uint64_t kMaxBlocks = 1u << (\d+);", f.read())
    return 1 << int(m.group(1))


def counts_rows(cases, chunk_cells, min_band_words, resident):
    """The rows of _mask_stats_ref.counts_geometry for COUNTS_CASES-like cases."""
    return [(w, h, rows, cols, n, chunk_cells, min_band_words, resident) for _, w, h, rows, cols, n, _ in cases]


def check_counts_geometry(case, q, resident):
    """More items than the 2 * resident blocks the kernel launches, so blocks
    take a second trip, and the path the case names."""
    assert q["ok"] == 1 and q["items"] >= 2 * resident + 1 and q["blocks"] < q["items"], (case[0], resident, q)
    if case[6]:
        assert q["col_chunks"] >= 2, (case[0], resident, q)
    else:
        assert q["bands"] == 1 and q["col_chunks"] == 1, (case[0], resident, q)

