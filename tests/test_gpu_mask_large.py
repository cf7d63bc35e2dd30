"""The labelling family on frames of more than 65,536 mask words with many
components: dips_mask_components, dips_mask_shapes, dips_mask_tracks,
dips_mask_select and mask_fill_holes against the builders of
tests/_large_masks.py and the specifications, every word of every output.
At this size cc_offsets_kernel hands a carry from round to round, and the
rank, label and record slot of every component anchored behind word 65,536
depend on it; the clips are taken by the planners of mask_abi.hip in rounds
of their own choice (chunk_frames = 0: 25 frames, then 2).  The conditions
that keep these cases from being vacuous are checked, without a GPU, by
tests/test_large_masks_cpu.py."""
import functools

import numpy as np
import pytest

import _components_ref as cref
import _large_masks as lm
import _select_ref as selref
import _shapes_ref as sref
import _tracks_ref as tref

pytestmark = pytest.mark.gpu

GUARD = 2  # words in front of and behind every device output; 8 bytes keep shapes_out aligned


@pytest.fixture(scope="module")
def op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    yield o
    o.close()


def frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


def same(got, want, names, what=""):
    assert len(got) == len(want) == len(names)
    for name, g, r in zip(names, got, want):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.shape)
        assert np.array_equal(g, r), (what, name, np.argwhere(g != r)[:5].tolist())


BOXES = ("counts", "boxes", "labels")
SHAPES = ("counts", "boxes", "shapes")
TRACKS = ("counts", "boxes", "links", "state")


class Out:
    """A 4-byte device output of `shape` inside a larger tensor filled with
    0xFFFFFFFF, GUARD words in front of it and behind it."""

    def __init__(self, shape, device):
        import torch
        self.n = int(np.prod(shape))
        self.whole = torch.full((self.n + 2 * GUARD,), -1, dtype=torch.int32, device=device)
        self.view = self.whole[GUARD:GUARD + self.n].view(*shape)
        self.check_guards()

    def check_guards(self):
        assert (self.whole[:GUARD] == -1).all().item() and (self.whole[GUARD + self.n:] == -1).all().item()

    def numpy(self):
        self.check_guards()
        return self.view.cpu().numpy().view(np.uint32)


def device_of(op):
    import torch
    return torch.device("cuda", op._dev.device)


def to_device(op, a):
    import torch
    return torch.from_numpy(np.array(a)).to(device_of(op))  # a copy: the cached arrays are read-only


# -- the references, once each --------------------------------------------------------

def sparse_mask(pad=0):
    return cref.pack(lm.sparse_frame()[0][None], pad)


@functools.lru_cache(maxsize=None)
def sparse_weights():
    return frozen(np.random.default_rng(131).integers(0, 256, (1, lm.SPARSE_H, lm.SPARSE_W), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def sparse_components_ref(connectivity):
    return tuple(frozen(a) for a in cref.components(sparse_mask(), lm.SPARSE_W, connectivity, lm.SPARSE_MIN_AREA,
                                                    lm.SPARSE_K))


@functools.lru_cache(maxsize=None)
def sparse_shapes_ref(connectivity, weighted):
    return tuple(frozen(a) for a in sref.shapes(sparse_mask(), lm.SPARSE_W, sparse_weights() if weighted else None,
                                                connectivity, lm.SPARSE_MIN_AREA, lm.SPARSE_K))


@functools.lru_cache(maxsize=None)
def clip_mask():
    return frozen(cref.pack(lm.moving_clip()))


def zero_state():
    return np.zeros(1 + 2 * lm.CLIP_K, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def clip_tracks_ref():
    """(counts, boxes, links, state) of the whole clip from a zero state;
    counts and boxes are those of _components_ref.components."""
    return tuple(frozen(a) for a in tref.tracks(clip_mask(), lm.CLIP_W, 8, lm.CLIP_MIN_AREA, lm.CLIP_K,
                                                state=zero_state()))


# -- 1. components, dense tiled -------------------------------------------------------

def host_components(op, mask, w, connectivity, min_area, k, labels=True):
    from dips_amd import ChangeMask
    r = op.mask_components(ChangeMask(mask, w), connectivity, min_area, k, labels, 0)
    return (r.counts, r.boxes, r.labels) if labels else (r.counts, r.boxes)


def device_components(op, mask, w, connectivity, min_area, k, labels=True):
    import torch
    dev = device_of(op)
    n, h = mask.shape[:2]
    counts = Out((n,), dev)
    boxes = Out((n, k, 8), dev) if k else None
    lab = Out((n, h, w), dev) if labels else None
    op.run_mask_components_device(to_device(op, mask), w, counts.view, None if boxes is None else boxes.view,
                                  None if lab is None else lab.view, connectivity=connectivity, min_area=min_area)
    torch.cuda.synchronize()
    got = (counts.numpy(), np.zeros((n, 0, 8), dtype=np.uint32) if boxes is None else boxes.numpy())
    return got + (lab.numpy(),) if labels else got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H", lm.DENSE_HEIGHTS)
def test_components_of_a_dense_tiled_frame(op, H, connectivity):
    """Every record, a max_boxes that cuts inside the second round, and counts
    and labels only; host pointers, and device pointers with the pad bits set."""
    case = lm.dense_case(H, connectivity)
    for min_area, k in lm.dense_arguments(H, connectivity):
        want = case.expect(min_area, k)
        assert want[0][0] > k or k == case.count
        same(host_components(op, cref.pack(case.bits[None]), lm.DENSE_W, connectivity, min_area, k), want, BOXES,
             ("host", min_area, k))
        same(device_components(op, cref.pack(case.bits[None], 1), lm.DENSE_W, connectivity, min_area, k), want, BOXES,
             ("device", min_area, k))


# -- 2. components, sparse ------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [4, 8])
def test_components_of_a_sparse_frame(op, connectivity):
    want = sparse_components_ref(connectivity)
    args = (lm.SPARSE_W, connectivity, lm.SPARSE_MIN_AREA, lm.SPARSE_K)
    same(host_components(op, sparse_mask(1), *args), want, BOXES, "host")
    got = device_components(op, sparse_mask(), *args)
    same(got, want, BOXES, "device")
    # the specks take part in the labelling and get label 0
    bits, info = lm.sparse_frame()
    assert (bits & (got[2][0] == 0)).sum() > 5000
    # the run of more than 64 all-ones words in the last round is one component
    y, x0, x1 = info["run"]
    last = int(got[0][0]) - 1
    assert got[1][0, last, cref.AREA] == info["run_area"] and (got[2][0, y, x0:x1] == last + 1).all()


# -- 3. shapes ------------------------------------------------------------------------

def host_shapes(op, mask, w, weights, connectivity, min_area, k):
    from dips_amd import ChangeMask
    return op.mask_shapes(ChangeMask(mask, w), weights, connectivity, min_area, k, 0).as_arrays()


def device_shapes(op, mask, w, weights, connectivity, min_area, k):
    """weights: None or a device tensor."""
    import torch
    dev = device_of(op)
    n = mask.shape[0]
    outs = [Out(s, dev) for s in ((n,), (n, k, 8), (n, k, sref.WORDS))]
    op.run_mask_shapes_device(to_device(op, mask), w, outs[0].view, outs[1].view, outs[2].view, weights,
                              connectivity=connectivity, min_area=min_area)
    torch.cuda.synchronize()
    return tuple(o.numpy() for o in outs)


def at_odd_address(op, a):
    """A uint8 array on the device, one byte inside a larger tensor."""
    import torch
    buf = torch.zeros(a.size + 1, dtype=torch.uint8, device=device_of(op))
    t = buf[1:].view(*a.shape)
    t.copy_(torch.from_numpy(np.array(a)))
    assert t.data_ptr() % 2 == 1
    return t


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_shapes_of_a_sparse_frame(op, connectivity, weighted):
    want = sparse_shapes_ref(connectivity, weighted)
    assert int(want[0][0]) > 20 and want[2][0, int(want[0][0]) - 1].any()
    assert want[2][0, :, sref.WMAX].any() == weighted
    args = (connectivity, lm.SPARSE_MIN_AREA, lm.SPARSE_K)
    weights = sparse_weights() if weighted else None
    same(host_shapes(op, sparse_mask(), lm.SPARSE_W, weights, *args), want, SHAPES, "host")
    wdev = at_odd_address(op, weights) if weighted else None
    same(device_shapes(op, sparse_mask(1), lm.SPARSE_W, wdev, *args), want, SHAPES, "device")
    # counts and boxes are those of dips_mask_components
    assert np.array_equal(want[0], sparse_components_ref(connectivity)[0])
    assert np.array_equal(want[1], sparse_components_ref(connectivity)[1])


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H", lm.DENSE_HEIGHTS)
def test_counts_and_boxes_of_shapes_on_a_dense_tiled_frame(op, H, connectivity):
    case = lm.dense_case(H, connectivity)
    mask = cref.pack(case.bits[None], 1)
    for min_area, k in lm.dense_arguments(H, connectivity)[:2]:
        counts, boxes, _ = case.expect(min_area, k)
        got = host_shapes(op, mask, lm.DENSE_W, None, connectivity, min_area, k)
        same(got[:2], (counts, boxes), SHAPES[:2], (min_area, k))
        # the moments of order 0 and 1 behind the boxes: area from SX and the centroid
        m = min(int(counts[0]), k)
        area = boxes[0, :m, cref.AREA].astype(np.uint64)
        sx, sy = sref.get64(got[2][0, :m], sref.SX), sref.get64(got[2][0, :m], sref.SY)
        assert np.array_equal((sx // area) * 256 + ((sx % area) * 256) // area, boxes[0, :m, cref.CX256])
        assert np.array_equal((sy // area) * 256 + ((sy % area) * 256) // area, boxes[0, :m, cref.CY256])
        assert not got[2][0, m:].any()


# -- 4. tracks ------------------------------------------------------------------------

def device_tracks(op, mask_dev, prev, state):
    import torch
    dev = device_of(op)
    n, k = mask_dev.shape[0], lm.CLIP_K
    outs = [Out(s, dev) for s in ((n,), (n, k, 8), (n, k, tref.LINK_WORDS))]
    op.run_mask_tracks_device(mask_dev, lm.CLIP_W, outs[0].view, outs[1].view, outs[2].view, prev=prev, state=state,
                              connectivity=8, min_area=lm.CLIP_MIN_AREA)
    torch.cuda.synchronize()
    return [o.numpy() for o in outs]


def test_tracks_of_a_clip_the_planner_splits(op):
    from dips_amd import ChangeMask
    want = clip_tracks_ref()
    assert (want[2][1:, :, tref.AGE] > 0).any() and want[3][0] > lm.CLIP_K  # tracks that last, and ids that end
    r = op.mask_tracks(ChangeMask(clip_mask(), lm.CLIP_W), 8, lm.CLIP_MIN_AREA, lm.CLIP_K, 0, None, zero_state())
    same((r.counts, r.boxes, r.links, r.state), want, TRACKS, "host")
    # one device call, then the same clip in two, cut at frame 13, prev and state carried
    mask_dev = to_device(op, clip_mask())
    state = Out((1 + 2 * lm.CLIP_K,), device_of(op))
    state.view.zero_()
    one = device_tracks(op, mask_dev, None, state.view)
    same(one + [state.numpy()], want, TRACKS, "device, one call")
    state.view.zero_()
    a = device_tracks(op, mask_dev[:13], None, state.view)
    b = device_tracks(op, mask_dev[13:], mask_dev[12], state.view)
    same([np.concatenate(p) for p in zip(a, b)] + [state.numpy()], want, TRACKS, "device, two calls")


# -- 5. the planner's rounds for the other products ----------------------------------

def test_components_of_a_clip_the_planner_splits(op):
    counts, boxes = clip_tracks_ref()[:2]
    args = (lm.CLIP_W, 8, lm.CLIP_MIN_AREA, lm.CLIP_K)
    same(host_components(op, clip_mask(), *args, labels=False), (counts, boxes), BOXES[:2], "host")
    same(device_components(op, clip_mask(), *args, labels=False), (counts, boxes), BOXES[:2], "device")
    # labels for the clip's tail, frames 24 .. 26, in a call of their own
    tail = clip_mask()[lm.CLIP_N - 3:]
    want = cref.components(tail, *args)
    assert np.array_equal(want[0], counts[-3:]) and np.array_equal(want[1], boxes[-3:])
    same(host_components(op, tail, *args), want, BOXES, "tail, host")
    same(device_components(op, tail, *args), want, BOXES, "tail, device")


def test_shapes_of_a_clip_the_planner_splits(op):
    weights = lm.clip_weights()
    args = (8, lm.CLIP_MIN_AREA, lm.CLIP_K)
    # _shapes_ref.shapes itself looks at the whole frame once per record: 10 s on this clip
    want = lm.shapes_by_box(clip_mask(), lm.CLIP_W, weights, *args)
    assert np.array_equal(want[0], clip_tracks_ref()[0]) and want[2][-1, :, sref.WSUM].any()
    same(host_shapes(op, clip_mask(), lm.CLIP_W, weights, *args), want, SHAPES, "host")
    same(device_shapes(op, clip_mask(), lm.CLIP_W, at_odd_address(op, weights), *args), want, SHAPES, "device")


def test_select_of_a_clip_the_planner_splits(op):
    import torch
    from dips_amd import ChangeMask
    clip, marker = lm.moving_clip(), lm.clip_marker()
    kw = dict(connectivity=8, min_area=lm.CLIP_MIN_AREA, clear_border=True)
    want_bits, want_counts = selref.select(clip, marker, **kw)
    selref._roots.cache_clear()  # 27 frames of int64 roots
    want = cref.pack(want_bits)
    # something is kept and something dropped in the planner's second round too
    assert (want_counts > 0).all() and (want_counts < clip_tracks_ref()[0]).all()
    assert not want_bits[:, -1].any() and clip[:, -1].any()  # the bars of the last round touch the border
    got, counts = op.mask_select(ChangeMask(clip_mask(), lm.CLIP_W), marker=ChangeMask(cref.pack(marker), lm.CLIP_W), **kw)
    same((got.bits, counts), (want, want_counts), ("mask", "counts"), "host")
    out = to_device(op, np.full(want.shape, 0xA5, dtype=np.uint8))
    counts_dev = Out((lm.CLIP_N,), device_of(op))
    op.run_mask_select_device(to_device(op, clip_mask()), lm.CLIP_W, out, marker=to_device(op, cref.pack(marker, 1)),
                              counts_out=counts_dev.view, **kw)
    torch.cuda.synchronize()
    same((out.cpu().numpy(), counts_dev.numpy()), (want, want_counts), ("mask", "counts"), "device")


# -- 6. select and fill-holes on one large frame --------------------------------------

@pytest.mark.parametrize("connectivity", [4, 8])
def test_select_on_a_sparse_frame(op, connectivity):
    from dips_amd import ChangeMask
    bits, info = lm.sparse_frame()
    lx, ly0, ly1 = info["line"]
    ry, rx, rh, rw = info["rects"][7]
    marker = np.zeros((1,) + bits.shape, dtype=bool)
    marker[0, ly1, lx] = True                      # the far end of the line, in the last round
    marker[0, ry + rh // 2, rx + rw // 2] = True   # a rectangle
    marker[0, lm.SPARSE_H - 2, 100] = True         # a clear pixel
    assert lm.round_of(ly1 * lm.SPARSE_W + lx, lm.SPARSE_W) == 1 and not bits[lm.SPARSE_H - 2, 100]
    rects_only = dict(min_area=lm.SPARSE_MIN_AREA, max_area=300)
    cases = ((marker, {}), (marker, dict(dropped=True)), (None, dict(rects_only, clear_border=True, dropped=True)),
             (None, dict(rects_only, clear_border=True)), (marker, dict(rects_only, clear_border=True, dropped=True)))
    wants = []
    for pad, (mk, kw) in enumerate(cases):
        want_bits, want_counts = selref.select(bits[None], mk, connectivity=connectivity, **kw)
        wants.append((want_bits, want_counts))
        got, counts = op.mask_select(ChangeMask(sparse_mask(pad % 2), lm.SPARSE_W),
                                     marker=None if mk is None else ChangeMask(cref.pack(mk, pad % 2), lm.SPARSE_W),
                                     connectivity=connectivity, **kw)
        same((got.bits, counts), (cref.pack(want_bits), want_counts), ("mask", "counts"), kw)
    # the marker at the line's far end keeps the line up to its anchor in the first round
    assert wants[0][1].tolist() == [2] and wants[0][0][0, ly0, lx] and wants[0][0][0, ry, rx]
    # the area range keeps the rectangles and the bars, not the line, the run or the specks
    kept = wants[3][0][0]
    assert 15 <= int(wants[3][1][0]) <= 23 and not kept[:, lx].any() and not kept[-1].any() and not kept[0].any()
    assert kept[info["bars"][0][0], info["bars"][0][1]]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_fill_holes_of_a_thousand_rings(op, connectivity):
    """The complement is one giant component on the border, every word of
    which reports to one root, and about a thousand holes beside it."""
    from dips_amd import ChangeMask
    r = lm.rings()
    assert lm.n_rounds(*r.bits.shape) == 3
    for pad, max_hole in enumerate((0, r.splitting_hole(connectivity))):
        got = op.mask_fill_holes(ChangeMask(cref.pack(r.bits[None], pad), lm.RINGS_W), connectivity, max_hole)
        want = cref.pack(r.expect(connectivity, max_hole)[None])
        assert got.width == lm.RINGS_W and got.bits.shape == want.shape
        assert np.array_equal(got.bits, want), (max_hole, np.argwhere(got.bits != want)[:5].tolist())
