"""The mask products on what an earlier call left in the handle: every output
word against the suite's references (np.array_equal, nothing left out).

The handle's scratch is shared and never cleared between calls: cc_scratch by
components, shapes, select and tracks (mask_scratch.h), times_parts by
dips_diff_pixel_times and dips_mask_pixel_times, and the staging buffers
stage_frames, stage_series and stage_map by every host-pointer call
(mask_host.h HostStaging).  Each product is right only if it writes whatever
it later reads.  Here every call under test follows, on the same handle, a
call that left other values under its planes:

  A  the cases of tests/_reuse_cases.py behind each kind of dirt, then once
     more on their own leftovers; a clip carried over three calls with a dirt
     between the calls; the products in alternation at one shape
  B  times_parts under the two change-times products in both orders, each
     call shown (from the schedule header) to run in several parts
  C  host pointers: a small call with absent pieces behind a large one of
     another product, outputs inside sentinel-filled arrays at odd addresses
  D  device pointers on two streams with no synchronisation, the scratch
     growing while the call before may still be queued
  E  seeded random walks over every mask product, change_mask and pixel_times

test_mask_reuse_cpu.py shows without a GPU that the calls of A lie inside
their dirt's bytes at other offsets.  An operator has a host handle and a
device handle; a sequence stays on one of them, and both kinds run."""
import functools
import os

import numpy as np
import pytest

import _components_ref as cref
import _mask_stats_ref as sref
import _morph_ref as mref
import _reuse_cases as rc
import _round_cases as rounds
import _select_ref as selref
import _shapes_ref as shref
import _tracks_ref as tref
import _vote_ref as vref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")
TAU = 8 / 255
SENTINEL = 0xA5


def make_op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    return DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, TAU)


@pytest.fixture(scope="module")
def op():
    o = make_op()
    yield o
    o.close()


# -- A: the labelling family on a dirty cc_scratch -----------------------------------------

# mask_fill_holes runs on the device handle whatever its input: one kind
A_CASES = [(c, k) for c in rc.CALLS for k in ("host", "dev") if not (c.product == "fill_holes" and k == "host")]


@pytest.mark.parametrize("dirt", rc.DIRTS)
@pytest.mark.parametrize("call,kind", A_CASES, ids=lambda v: v if isinstance(v, str) else v.name)
def test_call_behind_a_dirt_and_on_its_own_leftovers(op, call, kind, dirt):
    r = rc.Runner(op, kind)

    def make_dirt():
        rc.run_dirt(r, dirt, call)

    make_dirt()
    rc.check(r, call, "behind " + dirt, make_dirt)
    rc.check(r, call, "on its own leftovers")


ALTERNATION = ("components-labels-k3", "tracks-k256-chunk2", "select-marker-n", "shapes-weights",
               "components-labels-k3")


@pytest.mark.parametrize("kind", ["host", "dev"])
def test_products_in_alternation_at_one_shape(op, kind):
    """Components, tracks (K = 256), select with a marker, shapes, components
    at 97 x 29 x 7, a call at another shape between each two: the area slot is
    the label after cc_select_kernel and carries the hit flag (bit 31) in
    select, and neither may reach the next product."""
    r = rc.Runner(op, kind)
    w, h, n = 97, 29, 7
    others = ("tracks-k8-chunk2-state", "components-labels-k64-chunk3", "select-marker-1-border", "shapes-chunk3")
    for k, name in enumerate(ALTERNATION):
        call = rc.BY_NAME[name]._replace(w=w, h=h, n=n)
        rc.check(r, call, ("alternation", k))
        if k < len(others):
            rc.check(r, rc.BY_NAME[others[k]], ("alternation, between", k))


# -- B: times_parts shared by two products ---------------------------------------------------

PIXEL = (37, 29, 37, 17)    # w, h, n, DIPS_PIXEL_PART_FRAMES: test_gpu_pixel_times.py's pinned parts
MASKED = (33, 2, 600)       # test_part_seams of test_gpu_mask_stats.py: one tile, so the schedule cuts parts


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("reuse_sched")
    return rounds.build_geometry(d), sref.build_geometry(d, CSRC)


@functools.lru_cache(maxsize=None)
def _pixel_clip():
    from test_pixel_times_cpu import event_frames, py_pixel_times
    w, h, n, _ = PIXEL
    frames = event_frames(3, w, h, n)
    return frames, rc.frozen(py_pixel_times(frames, 1, TAU, t0=5))


@functools.lru_cache(maxsize=None)
def _masked_clip():
    w, h, n = MASKED
    bits = np.random.default_rng([157, n, h, w]).random((n, h, w)) < 0.5
    bits[:, 0, 0] = True    # one run across every part boundary
    bits[:, 1, 32] = False  # never set
    return rc.frozen(cref.pack(bits, 1)), rc.frozen(sref.times_bits(bits, 9)), rc.frozen(sref.sums_bits(bits))


@pytest.mark.parametrize("kind", ["host", "dev"])
def test_times_parts_under_both_change_times_products(op, kind, programs, monkeypatch):
    sched, mask_sched = programs
    w, h, n, pin = PIXEL
    px, _, _ = sref.kernel_constants(CSRC)
    for slots in (1024, 4096, 8192, 16384):
        q = rounds.schedule(sched, rounds._case("pixel", "times", w, h, n, pin=pin), 3, slots)
        assert q["ok"] == 1 and q["parts"] >= 2, q
        mw, mh, mn = MASKED
        for times, sums in ((True, False), (False, True), (True, True)):
            q = sref.times_geometry(mask_sched, [(sref.frame_slots(mw, mh, px), mn, sref.summary_bytes(mw, mh, times, sums),
                                                  sref.PARTS_BYTES, slots)])[0]
            assert q["ok"] == 1 and q["parts"] >= 2, q
    monkeypatch.setenv("DIPS_PIXEL_PART_FRAMES", str(pin))
    frames, want_pixel = _pixel_clip()
    mask, want_times, want_sums = _masked_clip()
    r = rc.Runner(op, kind)
    for rep in range(2):   # pixel, mask, pixel, mask: each product behind the other
        rc.same((r.pixel_times(frames, t0=5),), (want_pixel,), ("pixel times", kind, rep))
        rc.same((r.times(mask, MASKED[0], t0=9),), (want_times,), ("mask times", kind, rep))
        rc.same((r.sums(mask, MASKED[0]),), (want_sums,), ("mask sums", kind, rep))
    if kind == "dev":   # times and sums from one read of the mask, behind the pixel times
        import torch
        rc.same((r.pixel_times(frames, t0=5),), (want_pixel,), "pixel times")
        t, s = r._out(4, MASKED[1], MASKED[0]), r._out(MASKED[1], MASKED[0])
        op.run_mask_times_device(torch.from_numpy(np.array(mask)).cuda(), MASKED[0], t, s, t0=9)
        rc.same((r._u32(t), r._u32(s)), (want_times, want_sums), "mask times and sums")


# -- C: shared staging buffers, host pointers -------------------------------------------------

class Guarded:
    """`nbytes` at an odd host address inside a sentinel-filled array."""
    GUARD = 64

    def __init__(self, nbytes, fill=None):
        self.nbytes = int(nbytes)
        self.raw = np.full(self.nbytes + 2 * self.GUARD + 2, SENTINEL, dtype=np.uint8)
        self.at = self.GUARD + (1 if (self.raw.ctypes.data + self.GUARD) % 2 == 0 else 2)
        if fill is not None:
            self.raw[self.at:self.at + self.nbytes] = np.ascontiguousarray(fill).view(np.uint8).reshape(-1)
        assert self.ptr % 2 == 1

    @property
    def ptr(self):
        return self.raw.ctypes.data + self.at

    def get(self, dtype, shape):
        return self.raw[self.at:self.at + self.nbytes].copy().view(dtype).reshape(shape)

    def intact(self):
        return bool((self.raw[:self.at] == SENTINEL).all() and (self.raw[self.at + self.nbytes:] == SENTINEL).all())


def _ins(*arrays):
    return [None if a is None else Guarded(a.nbytes, a) for a in arrays]


def _p(g):
    return None if g is None else g.ptr


def _host_components(hd, mask, w, K, labels, connectivity=8, min_area=1):
    n, h = mask.shape[:2]
    (m,) = _ins(mask)
    counts, boxes = Guarded(4 * n), Guarded(32 * n * K) if K else None
    lab = Guarded(4 * n * h * w) if labels else None
    hd.check(hd._lib.dips_mask_components(hd.ptr, m.ptr, n, w, h, connectivity, min_area, K, 0, counts.ptr, _p(boxes),
                                          _p(lab)))
    want = cref.components(mask, w, connectivity, min_area, K, labels=True)
    got = (counts.get(np.uint32, (n,)), boxes.get(np.uint32, (n, K, 8)) if K else want[1],
           lab.get(np.uint32, (n, h, w)) if labels else None)
    rc.same(got, (want[0], want[1], want[2] if labels else None), ("components", w, h, n, K, labels))
    assert all(g.intact() for g in (m, counts, boxes, lab) if g is not None)


def _host_shapes(hd, mask, w, K, weights, connectivity=8):
    n, h = mask.shape[:2]
    m, wt = _ins(mask, weights)
    counts = Guarded(4 * n)
    boxes, shapes = (Guarded(32 * n * K), Guarded(64 * n * K)) if K else (None, None)
    hd.check(hd._lib.dips_mask_shapes(hd.ptr, m.ptr, _p(wt), n, w, h, connectivity, 1, K, 0, counts.ptr, _p(boxes),
                                      _p(shapes)))
    want = shref.shapes(mask, w, weights, connectivity, 1, K)
    got = (counts.get(np.uint32, (n,)), boxes.get(np.uint32, (n, K, 8)) if K else want[1],
           shapes.get(np.uint32, (n, K, 16)) if K else want[2])
    rc.same(got, want, ("shapes", w, h, n, K, weights is not None))
    assert all(g.intact() for g in (m, wt, counts, boxes, shapes) if g is not None)


def _host_tracks(hd, mask, w, K, prev=None, state=None, connectivity=8):
    n, h = mask.shape[:2]
    m, pv, st = _ins(mask, prev, state)
    counts, boxes, links = Guarded(4 * n), Guarded(32 * n * K), Guarded(16 * n * K)
    hd.check(hd._lib.dips_mask_tracks(hd.ptr, m.ptr, n, w, h, connectivity, 1, K, 0, _p(pv), _p(st), counts.ptr,
                                      boxes.ptr, links.ptr))
    want = tref.tracks(mask, w, connectivity, 1, K, prev=prev, state=state)
    got = (counts.get(np.uint32, (n,)), boxes.get(np.uint32, (n, K, 8)), links.get(np.uint32, (n, K, 4)),
           None if state is None else st.get(np.uint32, (1 + 2 * K,)))
    rc.same(got, want, ("tracks", w, h, n, K))
    assert all(g.intact() for g in (m, pv, st, counts, boxes, links) if g is not None)
    return got[3]


def _host_select(hd, mask, w, marker, with_counts, **kw):
    n, h = mask.shape[:2]
    m, mk = _ins(mask, marker)
    out, counts = Guarded(mask.nbytes), Guarded(4 * n) if with_counts else None
    sel = (1 if kw.get("clear_border") else 0) | (2 if kw.get("dropped") else 0)
    hd.check(hd._lib.dips_mask_select(hd.ptr, m.ptr, n, w, h, kw.get("connectivity", 8), kw.get("min_area", 1), 0, sel,
                                      _p(mk), 0 if marker is None else marker.shape[0], 0, out.ptr, _p(counts)))
    want, want_counts = selref.select_bytes(mask, w, marker, **kw)
    rc.same((out.get(np.uint8, mask.shape), counts.get(np.uint32, (n,)) if with_counts else None),
            (want, want_counts if with_counts else None), ("select", w, h, n))
    assert all(g.intact() for g in (m, mk, out, counts) if g is not None)


def _host_vote(hd, mask, w, window, votes, history, with_next):
    n, h = mask.shape[:2]
    m, hi = _ins(mask, history)
    out = Guarded(mask.nbytes)
    nxt = Guarded((window - 1) * mask[0].nbytes) if with_next else None
    hd.check(hd._lib.dips_mask_vote(hd.ptr, m.ptr, n, w, h, window, votes, _p(hi), _p(nxt), out.ptr))
    want, want_next = vref.vote(mask, w, window, votes, history)
    rc.same((out.get(np.uint8, mask.shape), nxt.get(np.uint8, want_next.shape) if with_next else None),
            (want, want_next if with_next else None), ("vote", w, h, n))
    assert all(g.intact() for g in (m, hi, out, nxt) if g is not None)


def _host_logic(hd, a, w, lop, b):
    n, h = a.shape[:2]
    ga, gb = _ins(a, b)
    out = Guarded(a.nbytes)
    hd.check(hd._lib.dips_mask_logic(hd.ptr, ga.ptr, n, w, h, lop, _p(gb), 0 if b is None else b.shape[0], out.ptr))
    rc.same((out.get(np.uint8, a.shape),), (selref.logic_bytes(a, w, lop, b),), ("logic", w, h, n, lop))
    assert all(g.intact() for g in (ga, gb, out) if g is not None)


def test_small_calls_with_absent_pieces_behind_large_ones_host_pointers(op):
    """Every pair is (a large call with every piece, a small call of another
    product with pieces absent): the small call's pieces lie at other offsets
    of buffers the large call filled, and an absent piece must neither be
    downloaded nor shift the others."""
    hd = op._host
    assert SENTINEL == rc.POISON & 0xFF
    big, small, one = (97, 29, 7), (33, 5, 3), (33, 5, 1)
    mask_b, mask_s, mask_1 = rc.mask_of(*big), rc.mask_of(*small), rc.mask_of(*one)
    marker_b = rc.marker_of(*big)
    K = 64
    zero = np.zeros(1 + 2 * K, dtype=np.uint32)
    # tracks with prev and state, then shapes whose weights (165 bytes, not a multiple of 4) lie behind the mask
    # and whose shapes lie in front of boxes and counts
    state = _host_tracks(hd, mask_b[:3], 97, K, state=zero)
    _host_tracks(hd, mask_b[3:], 97, K, prev=mask_b[2], state=state)
    assert rc.weights_of(*one).nbytes % 4 != 0
    _host_shapes(hd, mask_1, 33, 3, rc.weights_of(*one))
    # components with labels and boxes, then counts alone
    _host_components(hd, mask_b, 97, K, labels=True)
    _host_components(hd, mask_s, 33, 0, labels=False)
    # select with a marker of n frames and counts, then neither
    _host_select(hd, mask_b, 97, marker_b, True, min_area=2)
    _host_select(hd, mask_s, 33, None, False, clear_border=True)
    # shapes with weights, then tracks with neither prev nor state
    _host_shapes(hd, mask_b, 97, K, rc.weights_of(*big))
    _host_tracks(hd, mask_s, 33, 1)
    # tracks again, then shapes with no weights and, at max_boxes = 0, neither boxes nor shapes
    _host_tracks(hd, mask_b, 97, K, state=zero, connectivity=4)
    _host_shapes(hd, mask_s, 33, 3, None)
    _host_shapes(hd, mask_s, 33, 0, None)
    # the vote with both histories, then with neither
    hist = rc.marker_of(97, 29, 4)
    _host_vote(hd, mask_b, 97, 5, 2, hist, True)
    _host_vote(hd, mask_s, 33, 3, 2, None, False)
    # the logic of n frames with n frames, then with a b of one frame, then select with a marker of one frame
    _host_logic(hd, mask_b, 97, selref.XOR, marker_b)
    _host_logic(hd, mask_s, 33, selref.ANDNOT, rc.marker_of(33, 5, 1))
    _host_select(hd, mask_s, 33, rc.marker_of(33, 5, 1), True, dropped=True)
    _host_components(hd, mask_1, 33, 3, labels=True)


# -- D: stream switches on the labelling scratch ----------------------------------------------

@pytest.mark.parametrize("grow", [False, True], ids=["same-scratch", "scratch-grows"])
def test_stream_switch_orders_the_labelling_scratch(grow):
    """Tracks on stream 1, components with labels on stream 2 at another
    shape, select on stream 1 again, three times over with no synchronisation:
    cc_scratch is one buffer, so dips_set_stream has to order each call behind
    the one before.  scratch-grows: the second call's plan is larger than the
    first's, so the buffer is reallocated while the first may still be queued
    (a fresh operator: its scratch starts empty)."""
    import torch
    K = 8
    tw, th, tn = 65, 29, 7
    cw, ch, cn = (33, 29, 7) if not grow else (197, 32, 12)
    assert (rc.plan_bytes((cw, ch, cn, 0, 0)) > rc.plan_bytes((tw, th, tn, 0, K))) == grow
    t_mask, c_mask = rc.mask_of(tw, th, tn), rc.mask_of(cw, ch, cn, 1)
    marker = rc.marker_of(tw, th, tn)
    want_t = tref.tracks(t_mask, tw, 8, 1, K, state=np.zeros(1 + 2 * K, dtype=np.uint32))
    want_c = cref.components(c_mask, cw, 4, 2, K, labels=True)
    want_s = selref.select_bytes(t_mask, tw, marker, min_area=2)
    o = make_op()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        dt, dc, dm = (torch.from_numpy(np.array(a)).cuda() for a in (t_mask, c_mask, marker))
        r = rc.Runner(o, "dev")
        outs = []
        for rep in range(3):
            state = torch.zeros(1 + 2 * K, dtype=torch.int32, device="cuda")
            tr = (r._out(tn), r._out(tn, K, 8), r._out(tn, K, 4), state)
            co = (r._out(cn), r._out(cn, K, 8), r._out(cn, ch, cw))
            se = (r._bytes(*t_mask.shape), r._out(tn))
            outs.append((tr, co, se))
        torch.cuda.synchronize()
        for tr, co, se in outs:
            with torch.cuda.stream(s1):
                o.run_mask_tracks_device(dt, tw, tr[0], tr[1], tr[2], state=tr[3])
            with torch.cuda.stream(s2):
                o.run_mask_components_device(dc, cw, co[0], co[1], co[2], connectivity=4, min_area=2)
            with torch.cuda.stream(s1):
                o.run_mask_select_device(dt, tw, se[0], marker=dm, counts_out=se[1], min_area=2)
        torch.cuda.synchronize()
        for rep, (tr, co, se) in enumerate(outs):
            rc.same(tuple(r._u32(t) for t in tr), want_t, ("tracks", rep))
            rc.same(tuple(r._u32(t) for t in co), want_c, ("components", rep))
            rc.same((se[0].cpu().numpy(), r._u32(se[1])), want_s, ("select", rep))
    finally:
        o.close()


# -- E: seeded random walks -------------------------------------------------------------------

SHAPES = ((33, 5, 1), (65, 29, 7), (97, 5, 7), (37, 29, 5), (64, 17, 3), (130, 9, 4))
PRODUCTS = ("components", "shapes", "tracks", "select", "fill_holes", "logic", "morph", "vote", "counts", "times", "sums",
            "change_mask", "pixel_times")
WALK_CALLS = 26


def _walk_step(op, rng, product, kind):
    from test_change_mask_cpu import noise_frames, py_change_mask
    from test_pixel_times_cpu import py_pixel_times
    w, h, n = SHAPES[int(rng.integers(len(SHAPES)))]
    seed = int(rng.integers(3))
    mask = rc.mask_of(w, h, n, seed)
    conn = int(rng.choice([4, 8]))
    area = int(rng.integers(1, 6))
    chunk = int(rng.integers(0, 4))
    r = rc.Runner(op, kind)
    what = dict(product=product, kind=kind, shape=(w, h, n), content=seed, connectivity=conn, min_area=area, chunk=chunk)
    if product == "components":
        K, labels = int(rng.choice([0, 1, 5, 64])), bool(rng.integers(2))
        want = cref.components(mask, w, conn, area, K, labels=True)
        return r.components(mask, w, conn, area, K, labels, chunk), (want[0], want[1], want[2] if labels else None), what
    if product == "shapes":
        K = int(rng.choice([1, 5, 64]))
        wts = rc.weights_of(w, h, n, seed) if rng.integers(2) else None
        return r.shapes(mask, w, wts, conn, area, K, chunk), shref.shapes(mask, w, wts, conn, area, K), what
    if product == "tracks":
        K, mode = int(rng.choice([1, 8, 256])), int(rng.integers(3))
        state = None if mode == 0 else rng.integers(0, 1000, 1 + 2 * K).astype(np.uint32)
        prev = np.array(rc.mask_of(w, h, 1, seed + 1)[0]) if mode == 2 else None
        if prev is not None:   # a state that fits the frame before: what a call on it returns
            state = tref.tracks(prev[None], w, conn, area, K, state=state)[3]
        return (r.tracks(mask, w, conn, area, K, chunk, prev, state),
                tref.tracks(mask, w, conn, area, K, prev=prev, state=state), what)
    if product == "select":
        mk = [None, rc.marker_of(w, h, 1, seed), rc.marker_of(w, h, n, seed)][int(rng.integers(3))]
        kw = dict(connectivity=conn, min_area=area, max_area=int(rng.choice([0, area, 50])),
                  clear_border=bool(rng.integers(2)), dropped=bool(rng.integers(2)))
        counts = bool(rng.integers(2)) or kind == "host"
        want = selref.select_bytes(mask, w, mk, **kw)
        return r.select(mask, w, mk, counts, chunk_frames=chunk, **kw), (want[0], want[1] if counts else None), what
    if product == "fill_holes":
        hole = int(rng.choice([0, 2, 9]))
        return (r.fill_holes(mask, w, conn, hole),), (selref.fill_holes_bytes(mask, w, conn, hole),), what
    if product == "logic":
        lop = int(rng.integers(5))
        b = None if lop == selref.NOT else rc.marker_of(w, h, 1 if rng.integers(2) else n, seed)
        return (r.logic(mask, w, lop, b),), (selref.logic_bytes(mask, w, lop, b),), what
    if product == "morph":
        mop, shape, rx = int(rng.integers(4)), int(rng.integers(2)), int(rng.integers(0, 4))
        ry = rx if shape == mref.DIAMOND else int(rng.integers(0, 4))
        return (r.morph(mask, w, mop, shape, rx, ry),), (mref.morph(mask, w, mop, shape, rx, ry),), what
    if product == "vote":
        window = int(rng.integers(1, 7))
        votes = int(rng.integers(1, window + 1))
        hist = rc.mask_of(w, h, window - 1, seed + 1) if window > 1 and rng.integers(2) else None
        return r.vote(mask, w, window, votes, hist), vref.vote(mask, w, window, votes, hist), what
    if product == "counts":
        rows, cols = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        return (r.counts(mask, w, rows, cols),), (sref.counts(mask, w, rows, cols),), what
    if product == "times":
        t0 = int(rng.integers(0, 1000))
        return (r.times(mask, w, t0),), (sref.times(mask, w, t0),), what
    if product == "sums":
        return (r.sums(mask, w),), (sref.sums(mask, w),), what
    frames = noise_frames(3, w, h, max(n, 2))
    if product == "change_mask":
        return (r.change_mask(frames),), (py_change_mask(frames, 1, TAU),), what
    t0 = int(rng.integers(0, 1000))
    return (r.pixel_times(frames, t0),), (py_pixel_times(frames, 1, TAU, t0=t0),), what


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_walk_over_every_product(op, seed):
    """About two rounds over all products in a seeded order, each call at a
    random shape of the pool with random arguments in their documented ranges,
    on the host or the device handle; a failure names the seed and the call."""
    rng = np.random.default_rng([163, seed])
    order = list(rng.permutation(PRODUCTS)) + list(rng.permutation(PRODUCTS))
    assert len(order) == WALK_CALLS
    for i, product in enumerate(order):
        kind = "host" if rng.integers(2) else "dev"
        got, want, what = _walk_step(op, rng, str(product), kind)
        rc.same(got, tuple(want), dict(seed=seed, call=i, **what))
