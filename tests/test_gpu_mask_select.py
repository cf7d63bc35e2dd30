"""dips_mask_select, dips_mask_logic and their composites on the GPU against
tests/_select_ref.py: every byte of every output, pad bytes included.  The
shapes are the smallest at which each mechanism of mask_select.hip can go
wrong: word and row edges, every side of the border, pad bits, a marker far
from the anchor of a spiral and of a comb, runs longer than cc_rows_kernel
walks back, frames and chunks, one 4K frame under the one-address hot spot,
the logic beyond its grid's 2^15 blocks (the second trip of the stride loop),
the pointer kinds, the refused arguments and a randomized draw."""
import functools
import os

import numpy as np
import pytest

import _components_ref as cref
import _reuse_cases as rc
import _select_ref as sref

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 31, 32, 33, 63, 64, 65, 97]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dips_amd", "csrc")
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    yield o
    o.close()


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_bits(n, h, w, density, seed=0):
    return frozen(np.random.default_rng([71, seed, n, h, w]).random((n, h, w)) < density)


def run(op, bits, marker=None, pad=0, **kw):
    """The host form on bool arrays: (mask bytes, counts)."""
    from dips_amd import ChangeMask
    w = bits.shape[2]
    mk = None if marker is None else ChangeMask(cref.pack(marker, pad), w)
    got, counts = op.mask_select(ChangeMask(cref.pack(bits, pad), w), marker=mk, **kw)
    assert got.width == w and got.bits.dtype == np.uint8 and counts.dtype == np.uint32
    return got.bits, counts


def check(op, bits, marker=None, pad=0, chunk_frames=0, **kw):
    """GPU == reference for bool bits [n, h, w], byte for byte, counts too;
    returns the reference's (bits, counts)."""
    bits = np.asarray(bits, dtype=bool)
    want_bits, want_counts = sref.select(bits, marker, **kw)
    want = cref.pack(want_bits)
    got, counts = run(op, bits, marker, pad, chunk_frames=chunk_frames, **kw)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (kw, np.argwhere(got != want)[:5].tolist())
    assert np.array_equal(counts, want_counts), (kw, counts.tolist(), want_counts.tolist())
    return want_bits, want_counts


def edge_frames(h, w):
    corners = np.zeros((h, w), dtype=bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    return np.stack([random_bits(1, h, w, 0.3)[0], random_bits(1, h, w, 0.8)[0], np.ones((h, w), dtype=bool),
                     np.zeros((h, w), dtype=bool), corners, ~corners])


# -- word and row edges, connectivity, area, border -----------------------------------

@pytest.mark.parametrize("h", [1, 2, 3, 29])
@pytest.mark.parametrize("w", WIDTHS)
def test_word_and_row_edges(op, w, h):
    bits = edge_frames(h, w)
    marker = random_bits(6, h, w, 0.1, seed=3)
    for connectivity in (4, 8):
        for min_area in (1, 2, 5):
            for max_area in (0, 1, 7):
                if max_area and max_area < min_area:
                    continue
                for clear_border in (False, True):
                    check(op, bits, connectivity=connectivity, min_area=min_area, max_area=max_area,
                          clear_border=clear_border)
        check(op, bits, connectivity=connectivity, min_area=2, dropped=True)
        check(op, bits, marker, connectivity=connectivity)
        check(op, bits, marker[:1], connectivity=connectivity, clear_border=True, dropped=True)


@pytest.mark.parametrize("w", [45, 64, 97])
def test_every_side_of_the_border(op, w):
    """Components that touch the border through one side only, column w - 1
    in a partly used word included, and one that touches nothing."""
    h = 11
    bits = np.zeros((5, h, w), dtype=bool)
    bits[:, 4:7, 10:14] = True            # inside, in every frame
    bits[0, 3:8, w - 3:] = True           # column w - 1 only
    bits[1, h - 2:, 20:30] = True         # the last row only
    bits[2, :2, 20:30] = True             # row 0 only
    bits[3, 3:8, :2] = True               # column 0 only
    for connectivity in (4, 8):           # frame 4: the inside one alone
        want, counts = check(op, bits, connectivity=connectivity, clear_border=True)
        assert counts.tolist() == [1] * 5 and all(want[t].sum() == 12 for t in range(5))
        _, counts = check(op, bits, connectivity=connectivity, clear_border=True, dropped=True)
        assert counts.tolist() == [1] * 5
        _, counts = check(op, bits, connectivity=connectivity)
        assert counts.tolist() == [2, 2, 2, 2, 1]


@pytest.mark.parametrize("w", [1, 33, 63, 97])
def test_garbage_pad_bits_change_nothing(op, w):
    bits = random_bits(3, 7, w, 0.5, seed=1)
    marker = random_bits(3, 7, w, 0.1, seed=2)
    for kw in (dict(min_area=2), dict(clear_border=True), dict(max_area=3, dropped=True)):
        check(op, bits, pad=1, **kw)
        check(op, bits, marker, pad=1, **kw)
    # marker bits on clear pixels only (and in the pad): nothing is kept
    want, counts = check(op, bits, ~bits, pad=1)
    assert not want.any() and not counts.any()


# -- union-find shapes, long runs, the diagonal ----------------------------------------

def _comb(h, w):
    b = np.zeros((h, w), dtype=bool)
    b[:, ::2] = True
    b[-1, :] = True
    return b


def _spiral(h, w):
    """A rectangular spiral of one-pixel lines two pixels apart, from (0, 0) inwards."""
    b = np.zeros((h, w), dtype=bool)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    first = True
    while top <= bottom and left <= right:
        b[top, (left if first else max(left - 1, 0)):right + 1] = True
        b[top:bottom + 1, right] = True
        if bottom - top >= 2 and right - left >= 2:
            b[bottom, left:right + 1] = True
            b[top + 2:bottom + 1, left] = True
        first = False
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return b


@pytest.mark.parametrize("name", ["spiral", "comb"])
def test_marker_on_the_last_pixel_far_from_the_anchor(op, name):
    h, w = 41, 70
    shape = {"spiral": _spiral, "comb": _comb}[name](h, w)
    bits = np.zeros((1, h + 4, w + 4), dtype=bool)  # off the border, with a speck beside it
    bits[0, 2:-2, 2:-2] = shape
    bits[0, 0, 0] = True
    ys, xs = np.nonzero(bits[0])
    marker = np.zeros_like(bits)
    marker[0, ys[-1], xs[-1]] = True  # the last pixel in row-major order
    for connectivity in (4, 8):
        want, counts = check(op, bits, marker, connectivity=connectivity)
        assert counts.tolist() == [1] and want.sum() == shape.sum() and not want[0, 0, 0]
        want, counts = check(op, bits, marker, connectivity=connectivity, dropped=True)
        assert counts.tolist() == [1] and want.sum() == 1
        check(op, bits, marker, connectivity=connectivity, clear_border=True)


def test_runs_longer_than_the_walk_back(op):
    """A row-spanning run over more than 64 all-ones words (cc_rows_kernel's
    kBackWords path) with the only marker bit in its last word."""
    h, w = 3, 2200
    bits = np.zeros((1, h, w), dtype=bool)
    bits[0, 1, :] = True
    marker = np.zeros_like(bits)
    marker[0, 1, w - 3] = True
    for connectivity in (4, 8):
        want, counts = check(op, bits, marker, connectivity=connectivity)
        assert counts.tolist() == [1] and want.sum() == w
        check(op, bits, marker, connectivity=connectivity, dropped=True)
    # two such runs, one marked; a third short one unmarked
    bits = np.zeros((1, 5, w), dtype=bool)
    bits[0, 0, :] = True
    bits[0, 2, 7:] = True
    bits[0, 4, 100:103] = True
    marker = np.zeros_like(bits)
    marker[0, 2, w - 1] = True
    want, counts = check(op, bits, marker, connectivity=8)
    assert counts.tolist() == [1] and want.sum() == w - 7
    want, counts = check(op, bits, connectivity=8, min_area=4, clear_border=True)
    assert not want.any()


def test_diagonal_chain_4_against_8(op):
    bits = np.zeros((1, 12, 40), dtype=bool)
    bits[0, 2:5, 3:6] = True
    bits[0, 5:8, 6:9] = True   # touches the first at one corner only
    marker = np.zeros_like(bits)
    marker[0, 2, 3] = True
    want8, c8 = check(op, bits, marker, connectivity=8)
    want4, c4 = check(op, bits, marker, connectivity=4)
    assert c8.tolist() == [1] and want8.sum() == 18 and c4.tolist() == [1] and want4.sum() == 9
    _, c = check(op, bits, connectivity=8, min_area=10)
    assert c.tolist() == [1]
    _, c = check(op, bits, connectivity=4, min_area=10)
    assert c.tolist() == [0]


# -- frames and chunks -------------------------------------------------------------------

def test_frames_markers_and_chunks(op):
    n, h, w = 6, 45, 70
    bits = random_bits(n, h, w, 0.45, seed=4).copy()
    bits[1] = bits[0]  # the same frame twice: a marker that acted on the wrong frame would show
    marker = random_bits(n, h, w, 0.01, seed=5).copy()
    marker[1] = False
    want, counts = check(op, bits, marker)
    assert want[0].any() and not want[1].any() and counts[1] == 0
    dropped, _ = check(op, bits, marker, dropped=True)
    assert dropped.any() and want.any()
    check(op, bits, marker[:1])                       # one frame for all
    want1, _ = sref.select(bits, marker[:1])
    assert np.array_equal(want1[1], want1[0]) and want1[0].any()
    outs = []
    for chunk in (1, 4, 0):  # 1: six rounds, 4: two rounds, the second shorter
        for mk in (marker, marker[:1], None):
            check(op, bits, mk, chunk_frames=chunk, min_area=2, clear_border=True)
        outs.append(run(op, bits, marker, chunk_frames=chunk, min_area=3))
    for got in outs[1:]:
        assert np.array_equal(got[0], outs[0][0]) and np.array_equal(got[1], outs[0][1])


# -- the one-address hot spot ----------------------------------------------------------

def test_4k_all_ones_under_an_all_ones_marker(op):
    """Every word of the frame reports to one root: sel_mark_kernel's flag
    test and its wave leaders keep that from being one atomic per word."""
    h, w = 2160, 3840
    ones = np.full((1, h, cref.row_bytes(w)), 0xFF, dtype=np.uint8)
    from dips_amd import ChangeMask
    for connectivity in (4, 8):
        got, counts = op.mask_select(ChangeMask(ones, w), marker=ChangeMask(ones, w), connectivity=connectivity)
        assert counts.tolist() == [1] and np.array_equal(got.bits, ones)  # w is a multiple of 32: no pad bits
    got, counts = op.mask_select(ChangeMask(ones, w), marker=ChangeMask(ones, w), clear_border=True, dropped=True)
    assert counts.tolist() == [0] and np.array_equal(got.bits, ones)


def test_4k_random_frame(op):
    """One 4K frame at density 0.5: a giant component among specks.  The
    Python union-find of the specification would take minutes on 8.3 M
    pixels, so the reference here is scipy's labelling where scipy is
    installed, and otherwise the packed labels != 0 of dips_mask_components,
    which its own suite pins to the specification."""
    from dips_amd import ChangeMask
    h, w = 2160, 3840
    bits = random_bits(1, h, w, 0.5, seed=6)
    mask = ChangeMask(cref.pack(bits), w)
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    for connectivity in (8, 4):
        if ndi is not None:
            structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
            lab, num = ndi.label(bits[0], structure=structure)
            area = np.bincount(lab.ravel())
            keep = area >= 16
            keep[0] = False
            want, want_count = keep[lab][None], int(keep.sum())
        else:
            boxes = op.mask_components(mask, connectivity, 16, 0, labels=True)
            want, want_count = boxes.labels != 0, int(boxes.counts[0])
        assert want.any() and (bits & ~want).any()
        got, counts = op.mask_select(mask, connectivity=connectivity, min_area=16)
        assert np.array_equal(got.bits, cref.pack(want)) and counts.tolist() == [want_count]
        gone, counts = op.mask_select(mask, connectivity=connectivity, min_area=16, dropped=True)
        assert np.array_equal(gone.bits, cref.pack(bits & ~want)) and counts.tolist() == [want_count]


# -- parity with dips_mask_components, the partition -------------------------------------

def test_parity_with_mask_components(op):
    from dips_amd import ChangeMask
    from oracle import oracle
    frames = oracle.synth(3, 128, 64, 0xD1B5, 0, 6)
    masks = [op.change_mask(frames), ChangeMask(cref.pack(random_bits(4, 33, 97, 0.5, seed=7), pad=1), 97)]
    assert masks[0].bits.any()
    for mask in masks:
        for connectivity in (4, 8):
            boxes = op.mask_components(mask, connectivity=connectivity, max_boxes=1, labels=True)
            got, counts = op.mask_select(mask, connectivity=connectivity)
            assert np.array_equal(counts, boxes.counts)
            assert np.array_equal(got.bits, cref.pack(boxes.labels != 0))
            ref, ref_counts = sref.select_bytes(mask.bits, mask.width, connectivity=connectivity)
            assert np.array_equal(got.bits, ref) and np.array_equal(counts, ref_counts)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_kept_and_dropped_partition_the_mask(op, connectivity):
    bits = random_bits(3, 40, 100, 0.5, seed=8)
    marker = random_bits(3, 40, 100, 0.02, seed=9)
    for mk, kw in ((None, dict(min_area=4)), (marker, {}), (marker[:1], dict(clear_border=True, max_area=30))):
        kept, counts = run(op, bits, mk, connectivity=connectivity, **kw)
        gone, counts_d = run(op, bits, mk, connectivity=connectivity, dropped=True, **kw)
        assert kept.any() and gone.any()
        assert np.array_equal(kept | gone, cref.pack(bits)) and not (kept & gone).any()
        assert np.array_equal(counts, counts_d)


# -- dips_mask_logic -----------------------------------------------------------------------

def run_logic(op, a, lop, b=None, pad=0):
    from dips_amd import ChangeMask
    w = a.shape[2]
    got = op.mask_logic(ChangeMask(cref.pack(a, pad), w), lop, None if b is None else ChangeMask(cref.pack(b, pad), w))
    assert got.width == w
    return got.bits


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("w", WIDTHS)
def test_logic_ops_at_word_edges(op, w, h):
    a = random_bits(5, h, w, 0.5, seed=10)
    b = random_bits(5, h, w, 0.5, seed=11)
    for pad in (0, 1):
        for lop in (sref.AND, sref.OR, sref.XOR, sref.ANDNOT):
            assert np.array_equal(run_logic(op, a, lop, b, pad), cref.pack(sref.logic(a, lop, b)))
            assert np.array_equal(run_logic(op, a, lop, b[:1], pad), cref.pack(sref.logic(a, lop, b[:1])))
        assert np.array_equal(run_logic(op, a, sref.NOT, None, pad), cref.pack(~a))
    zeros = np.zeros((2, h, w), dtype=bool)
    got = run_logic(op, zeros, sref.NOT, None, pad=1)
    assert np.unpackbits(got, axis=-1).sum(axis=-1).tolist() == [[w] * h] * 2  # exactly roi_w bits per row


def test_logic_on_more_frames_than_a_grid_dimension(op):
    n, h, w = 70000, 1, 33
    a = random_bits(n, h, w, 0.5, seed=12)
    b = random_bits(1, h, w, 0.5, seed=13)
    assert np.array_equal(run_logic(op, a, sref.XOR, b, pad=1), cref.pack(a ^ b))
    assert np.array_equal(run_logic(op, a, sref.NOT, None, pad=1), cref.pack(~a))
    assert np.array_equal(run_logic(op, a, sref.ANDNOT, a[::-1]), cref.pack(a & ~a[::-1]))


# -- beyond 2^15 blocks: the second trip of the grid stride ----------------------------------

def _random_words(seed, n, h, wpr):
    """uint32 [n, h, wpr]: a packed mask with random bits, the pad bits too."""
    return np.random.default_rng([73, seed, n, h, wpr]).integers(0, 1 << 32, (n, h, wpr), dtype=np.uint32)


def _logic_words(x, lop, y, pad_mask):
    """The reference on the packed words themselves: (a op b) & pad_mask."""
    v = {sref.AND: lambda: x & y, sref.OR: lambda: x | y, sref.XOR: lambda: x ^ y, sref.ANDNOT: lambda: x & ~y,
         sref.NOT: lambda: ~x}[lop]()
    return v & pad_mask


def _check_logic_beyond_the_grid(op, case, runs):
    """mask_logic_kernel's grid ends at kMaxBlocks blocks; beyond, a thread
    strides on and carries r, its word's index in the frame, forward by dr
    with a wrap.  r picks b's word under the broadcast and the words that get
    the pad mask.  runs: (op, frames of b: 0 none, 1 broadcast, n)."""
    import torch
    from dips_amd import MaskLogic
    name, w, h, n = case
    g = rc.logic_geometry(w, h, n, rc.logic_max_blocks(CSRC))
    assert g["words"] > g["stride"] and g["words"] % g["stride"] != 0 and g["dr"] != 0, g  # a second, ragged trip
    wpr = (w + 31) // 32
    a, b = _random_words(1, n, h, wpr), _random_words(2, n, h, wpr)
    pad_mask = np.full(wpr, 0xFFFFFFFF, dtype=np.uint32)
    if w % 32:
        pad_mask[-1] = (1 << (w % 32)) - 1
    dev = torch.device("cuda", op._dev.device)
    da, db = (torch.from_numpy(x.view(np.uint8).reshape(n, h, 4 * wpr)).to(dev) for x in (a, b))
    out = torch.empty_like(da)
    for lop, b_frames in runs:
        out.fill_(SENTINEL)
        op.run_mask_logic_device(da, w, out, MaskLogic(lop), None if b_frames == 0 else db[:b_frames])
        got = out.cpu().numpy().view(np.uint32).reshape(n, h, wpr)
        want = _logic_words(a, lop, None if b_frames == 0 else b[:b_frames], pad_mask)
        assert np.array_equal(got, want), (name, lop, b_frames, np.argwhere(got != want)[:5].tolist())
        if w % 32:
            assert not (got[..., -1] & ~pad_mask[-1]).any()  # the output's pad bits are 0


def test_logic_beyond_the_grid_many_frames(op):
    """300 frames of 1000 x 1000: 9.6 M words in frames of 32,000, dr = 4,608,
    so r wraps on every trip at another place and the last trip is ragged."""
    case = rc.LOGIC_CASES[0]
    n = case[3]
    runs = [(lop, k) for lop in (sref.AND, sref.OR, sref.XOR, sref.ANDNOT) for k in (n, 1)] + [(sref.NOT, 0)]
    _check_logic_beyond_the_grid(op, case, runs)


def test_logic_beyond_the_grid_one_frame_longer_than_the_grid(op):
    """2 frames of 16,416 x 16,400: a frame of 8,413,200 words is longer than
    the grid's 2^15 * 256 threads, so dr is the stride itself."""
    _check_logic_beyond_the_grid(op, rc.LOGIC_CASES[1], [(sref.XOR, 1), (sref.NOT, 0)])


# -- the composites -------------------------------------------------------------------------

def _hole_cases():
    h, w = 20, 75
    f = np.zeros((6, h, w), dtype=bool)
    f[0, 3:12, 5:40] = True
    f[0, 5:10, 8:30] = False               # a ring
    f[1, 1:19, 2:70] = True
    f[1, 3:17, 5:66] = False
    f[1, 6:14, 20:50] = True
    f[1, 8:12, 25:45] = False              # a ring inside a ring's hole
    f[2, 4, 31:34] = f[2, 6, 31:34] = True
    f[2, 5, 30] = f[2, 5, 34] = True       # a ring around (5, 31..33) closed only diagonally
    f[3, 0:8, 60:75] = True
    f[3, 2:6, 64:75] = False               # a bay open to column w - 1: no hole
    f[4, 2:18, 10:60] = True
    f[4, 4, 12] = False                    # holes of 1, 4 and 40 pixels
    f[4, 7:9, 20:22] = False
    f[4, 11:15, 30:40] = False
    f[5] = random_bits(1, h, w, 0.6, seed=14)[0]
    return frozen(f)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_fill_holes(op, connectivity):
    from dips_amd import ChangeMask
    f = _hole_cases()
    w = f.shape[2]
    for pad in (0, 1):
        for max_hole in (0, 1, 4, 39, 40):
            got = op.mask_fill_holes(ChangeMask(cref.pack(f, pad), w), connectivity, max_hole)
            want = sref.fill_holes(f, connectivity, max_hole)
            assert np.array_equal(got.bits, cref.pack(want)), (connectivity, max_hole)
    full = sref.fill_holes(f, connectivity)
    assert full[0, 7, 20] and full[1, 10, 30] and not full[3, 4, 70] and (full[5] & ~f[5]).any()
    assert full[2, 5, 32] == (connectivity == 8)  # the diagonal ring holds only when the mask is 8-connected
    assert not sref.fill_holes(f, connectivity, 39)[4, 12, 35] and sref.fill_holes(f, connectivity, 40)[4, 12, 35]


def _flash_clip(w, h, n):
    """A noise-free background on which, in every odd frame, a faint
    rectangle with a bright core and one unlit pixel, a faint rectangle
    without a core and a few single bright pixels light up: the faint parts
    fire only a low threshold, against frame 0 and against the frame before."""
    rng = np.random.default_rng([73, w, h, n])
    base = rng.integers(60, 90, (h, w, 3), dtype=np.uint8)
    frames = np.repeat(base[None], n, axis=0)
    for t in range(1, n, 2):
        frames[t, 10:22, 5:25] = 120
        frames[t, 14:16, 9:12] = 250
        frames[t, 17, 20] = base[17, 20]
        frames[t, 40:50, 70:84] = 115
        for y, x in rng.integers((0, 30), (h, 60), (6, 2)):  # clear of the rectangles
            frames[t, y, x] = 255
    return frames


@pytest.mark.parametrize("mode", [0, 1])
def test_hysteresis_mask(mode):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    frames = _flash_clip(96, 64, 5)
    lo, hi = 12 / 255, 100 / 255
    weak_op = DiffSeriesOperator(PixelFormat.RGB8, Mode(mode), lo)
    strong_op = DiffSeriesOperator(PixelFormat.RGB8, Mode(mode), hi)
    try:
        for roi in (None, (3, 2, 90, 60)):
            weak, strong = weak_op.change_mask(frames, roi=roi), strong_op.change_mask(frames, roi=roi)
            for connectivity in (4, 8):
                want, _ = sref.select_bytes(weak.bits, weak.width, strong.bits, connectivity=connectivity)
                assert want.any() and (weak.bits & ~want).any() and (want & ~strong.bits).any()
                got = weak_op.hysteresis_mask(frames, hi, roi=roi, connectivity=connectivity)
                assert got.width == weak.width and np.array_equal(got.bits, want)
        assert len(weak_op._strong) == 1  # one handle per tau_high, reused
        assert np.array_equal(weak_op.hysteresis_mask(frames, lo).bits, weak_op.change_mask(frames).bits)
        with pytest.raises(ValueError):
            weak_op.hysteresis_mask(frames, lo / 2)
    finally:
        weak_op.close()
        strong_op.close()
    assert not weak_op._strong


def test_select_option_of_the_change_products(op):
    from dips_amd import ChangeMask
    frames = _flash_clip(96, 64, 5)
    mask = op.change_mask(frames)
    sel = {"min_area": 4, "clear_border": True, "connectivity": 4, "fill_holes": True}
    kept, _ = op.mask_select(mask, connectivity=4, min_area=4, clear_border=True)
    assert kept.bits.any() and (mask.bits & ~kept.bits).any()
    want_mask = op.mask_fill_holes(kept, connectivity=4)
    assert (want_mask.bits & ~kept.bits).any()  # the unlit pixel is a hole
    assert np.array_equal(want_mask.bits, sref.fill_holes_bytes(
        sref.select_bytes(mask.bits, mask.width, connectivity=4, min_area=4, clear_border=True)[0], mask.width, 4))
    boxes = op.change_boxes(frames, connectivity=8, max_boxes=16, labels=True, select=sel)
    want = op.mask_components(want_mask, connectivity=8, max_boxes=16, labels=True)
    assert want.counts.any()
    assert all(np.array_equal(g, x) for g, x in zip(boxes.as_arrays(), want.as_arrays()))
    tracks = op.change_tracks(frames, max_boxes=16, select=sel)
    want_t = op.mask_tracks(want_mask, max_boxes=16, state=np.zeros(33, dtype=np.uint32))
    assert all(np.array_equal(g, x) for g, x in zip(tracks.as_arrays(), want_t.as_arrays()))
    # the statistics see the selected mask, not only the records (change_activity's own
    # parameter list is pinned by tests/test_mask_stats_cpu.py, so the option has a method of its own)
    counts, times, sums = op.change_activity_selected(frames, {"min_area": 4}, rows=2, cols=3)
    area4, _ = op.mask_select(mask, min_area=4)
    assert np.array_equal(counts, op.mask_counts(area4, 2, 3))
    assert np.array_equal(times.as_array(), op.mask_times(area4).as_array())
    assert np.array_equal(sums, op.mask_sums(area4)) and sums.sum() == area4.unpack().sum() < mask.unpack().sum()
    # a select that selects nothing away changes nothing
    plain = op.change_boxes(frames, max_boxes=16)
    same = op.change_boxes(frames, max_boxes=16, select={})
    assert all(np.array_equal(g, x) for g, x in zip(plain.as_arrays()[:2], same.as_arrays()[:2]))


# -- pointer kinds ------------------------------------------------------------------------------

def test_device_pointers_equal_the_reference(op):
    import torch
    from dips_amd import MaskLogic
    n, h, w = 3, 33, 97
    bits, marker = random_bits(n, h, w, 0.5, seed=15), random_bits(n, h, w, 0.03, seed=16)
    mask = torch.from_numpy(cref.pack(bits, pad=1)).cuda()
    mk = torch.from_numpy(cref.pack(marker, pad=1)).cuda()
    out = torch.full_like(mask, SENTINEL)
    counts = torch.full((n + 1,), 7, dtype=torch.int32, device="cuda")
    for marker_t, marker_b in ((None, None), (mk, marker), (mk[:1], marker[:1])):
        for kw in (dict(min_area=3), dict(clear_border=True, dropped=True, connectivity=4)):
            out.fill_(SENTINEL)
            op.run_mask_select_device(mask, w, out, marker=marker_t, counts_out=counts[1:], **kw)
            want, want_counts = sref.select(bits, marker_b, **kw)
            assert np.array_equal(out.cpu().numpy(), cref.pack(want))
            assert np.array_equal(counts.cpu().numpy().view(np.uint32), np.concatenate([[7], want_counts]))
            out.fill_(SENTINEL)
            op.run_mask_select_device(mask, w, out, marker=marker_t, **kw)  # no counts
            assert np.array_equal(out.cpu().numpy(), cref.pack(want))
    for lop, b_t, b_b in ((MaskLogic.AndNot, mk, marker), (MaskLogic.Or, mk[:1], marker[:1]), (MaskLogic.Not, None, None)):
        out.fill_(SENTINEL)
        op.run_mask_logic_device(mask, w, out, lop, b_t)
        assert np.array_equal(out.cpu().numpy(), cref.pack(sref.logic(bits, int(lop), b_b)))
    scratch = torch.empty_like(mask)
    op.run_mask_fill_holes_device(mask, w, out, scratch, 8, 5)
    assert np.array_equal(out.cpu().numpy(), cref.pack(sref.fill_holes(bits, 8, 5)))
    with pytest.raises(ValueError):
        op.run_mask_select_device(mask, w, mask)                       # in place
    with pytest.raises(ValueError):
        op.run_mask_select_device(mask, w, out, marker=out[:1])        # the output over the marker
    with pytest.raises(ValueError):
        op.run_mask_logic_device(mask, w, out, MaskLogic.And, out)     # the output over b


def test_host_pointers_at_odd_alignment(op):
    n, h, w = 2, 9, 45
    bits, marker = random_bits(n, h, w, 0.5, seed=17), random_bits(1, h, w, 0.05, seed=18)
    mb, kb = cref.pack(bits), cref.pack(marker)
    raw = [np.zeros(mb.size + 8, dtype=np.uint8) for _ in range(3)]
    m, k, o = raw[0][1:1 + mb.size], raw[1][3:3 + kb.size], raw[2][1:1 + mb.size]
    m[:], k[:] = mb.reshape(-1), kb.reshape(-1)
    counts = np.zeros(n, dtype=np.uint32)
    hd = op._host
    hd.check(hd._lib.dips_mask_select(hd.ptr, m.ctypes.data, n, w, h, 8, 2, 0, 0, k.ctypes.data, 1, 0, o.ctypes.data,
                                      counts.ctypes.data))
    want, want_counts = sref.select(bits, marker, min_area=2)
    assert np.array_equal(o.reshape(mb.shape), cref.pack(want)) and np.array_equal(counts, want_counts)
    assert raw[2][0] == 0 and not raw[2][1 + mb.size:].any()
    hd.check(hd._lib.dips_mask_logic(hd.ptr, m.ctypes.data, n, w, h, sref.XOR, k.ctypes.data, 1, o.ctypes.data))
    assert np.array_equal(o.reshape(mb.shape), cref.pack(bits ^ marker))


# -- errors ---------------------------------------------------------------------------------------

def test_select_refused_arguments_leave_the_outputs_untouched(op):
    from dips_amd import DipsError, _lib
    w, h, n = 37, 5, 2
    buf = np.zeros(4 * n * h * 8, dtype=np.uint8)  # room for the overlaps below
    fb = h * 8
    buf[:n * fb] = cref.pack(random_bits(n, h, w, 0.5)).reshape(-1)
    out = np.full(n * fb, SENTINEL, dtype=np.uint8)
    counts = np.full(n + n * fb // 4, 0xA5A5A5A5, dtype=np.uint32)
    hd = op._host
    M, K, O, C = buf.ctypes.data, buf.ctypes.data + n * fb, out.ctypes.data, counts.ctypes.data
    #        mask n  w  h  conn min max sel marker mf out counts
    cases = [(None, n, w, h, 8, 1, 0, 0, None, 0, O, C),
             (M, n, w, h, 8, 1, 0, 0, None, 0, None, C),
             (M, n, w, h, 6, 1, 0, 0, None, 0, O, C),
             (M, n, w, h, 0, 1, 0, 0, None, 0, O, C),
             (M, n, 0, h, 8, 1, 0, 0, None, 0, O, C),
             (M, n, w, 0, 8, 1, 0, 0, None, 0, O, C),
             (M, n, 1 << 24, 1, 8, 1, 0, 0, None, 0, O, C),
             (M, n, 1, 1 << 24, 8, 1, 0, 0, None, 0, O, C),
             (M, n, 1 << 15, 1 << 15, 8, 1, 0, 0, None, 0, O, C),
             (M, n, w, h, 8, 1, 0, 4, None, 0, O, C),             # an unknown select bit
             (M, n, w, h, 8, 1, 0, 0x80000001, None, 0, O, C),
             (M, n, w, h, 8, 5, 4, 0, None, 0, O, C),             # max_area below min_area
             (M, n, w, h, 8, 1, 0, 0, K, 0, O, C),                # a marker of no frames
             (M, n, w, h, 8, 1, 0, 0, K, 3, O, C),                # ... of neither 1 nor n
             (M, n, w, h, 8, 1, 0, 0, None, 1, O, C),             # frames of no marker
             (M, n, w, h, 8, 1, 0, 0, None, 0, M, C),             # in place
             (M, n, w, h, 8, 1, 0, 0, None, 0, M + fb, C),        # mask_out over the mask's second frame
             (M, n, w, h, 8, 1, 0, 0, O + fb, 1, O, C),           # mask_out over the marker
             (M, n, w, h, 8, 1, 0, 0, None, 0, O, M + 4),         # counts inside the mask
             (M, n, w, h, 8, 1, 0, 0, C + 4, n, O, C),            # counts over the marker
             (M, n, w, h, 8, 1, 0, 0, None, 0, C, C)]             # counts over mask_out
    before = buf.copy()
    for m_, n_, w_, h_, conn, lo, hi, sel, k_, kf, o_, c_ in cases:
        st = hd._lib.dips_mask_select(hd.ptr, m_, n_, w_, h_, conn, lo, hi, sel, k_, kf, 0, o_, c_)
        assert st == _lib.DIPS_ERR_INVALID, (n_, w_, h_, conn, lo, hi, sel, kf)
        with pytest.raises(DipsError, match="mask_select: "):
            hd.check(st)
        assert (out == SENTINEL).all() and (counts == 0xA5A5A5A5).all() and np.array_equal(buf, before)
    # n_frames == 0: fine, nothing written
    assert hd._lib.dips_mask_select(hd.ptr, None, 0, w, h, 8, 1, 0, 0, None, 0, 0, None, None) == 0
    assert hd._lib.dips_mask_select(hd.ptr, M, 0, w, h, 8, 1, 0, 0, None, 0, 0, O, C) == 0
    assert (out == SENTINEL).all() and (counts == 0xA5A5A5A5).all()
    # and the same buffers serve a call that is fine: counts may be NULL
    assert hd._lib.dips_mask_select(hd.ptr, M, n, w, h, 8, 1, 0, 0, None, 0, 0, O, None) == 0
    assert np.array_equal(out, buf[:n * fb]) and (counts == 0xA5A5A5A5).all()  # the pad bits were 0 already


def test_logic_refused_arguments_leave_the_output_untouched(op):
    from dips_amd import DipsError, _lib
    w, h, n = 37, 5, 2
    fb = h * 8
    a = cref.pack(random_bits(n, h, w, 0.5)).reshape(-1).copy()
    b = cref.pack(random_bits(n, h, w, 0.5, seed=1)).reshape(-1).copy()
    out = np.full(2 * n * fb, SENTINEL, dtype=np.uint8)
    hd = op._host
    A, B, O = a.ctypes.data, b.ctypes.data, out.ctypes.data
    #        a  n  w  h  op  b  bf out
    cases = [(None, n, w, h, 0, B, n, O),
             (A, n, w, h, 0, B, n, None),
             (A, n, w, h, 5, B, n, O),
             (A, n, w, h, 4, B, n, O),                  # NOT with a b
             (A, n, w, h, 4, None, 1, O),               # NOT with frames of no b
             (A, n, w, h, 1, None, 0, O),               # a binary op without b
             (A, n, w, h, 1, B, 0, O),
             (A, 3, w, h, 1, B, 2, O),                  # b_frames neither 1 nor n
             (A, n, 0, h, 1, B, n, O),
             (A, n, w, 0, 1, B, n, O),
             (A, n, 1 << 15, 1 << 15, 1, B, n, O),
             (A, n, w, h, 1, B, n, A),                  # in place
             (A, n, w, h, 1, B, n, A + fb),
             (A, n, w, h, 1, O + n * fb, 1, O + fb)]    # the output over b's one frame
    for a_, n_, w_, h_, lop, b_, bf, o_ in cases:
        st = hd._lib.dips_mask_logic(hd.ptr, a_, n_, w_, h_, lop, b_, bf, o_)
        assert st == _lib.DIPS_ERR_INVALID, (n_, w_, h_, lop, bf)
        with pytest.raises(DipsError, match="mask_logic: "):
            hd.check(st)
        assert (out == SENTINEL).all()
    assert hd._lib.dips_mask_logic(hd.ptr, None, 0, w, h, 1, None, 0, None) == 0
    assert hd._lib.dips_mask_logic(hd.ptr, A, 0, w, h, 1, B, 0, O) == 0
    assert (out == SENTINEL).all()


def test_misaligned_device_pointers_are_refused(op):
    import torch
    from dips_amd import _lib
    w, h, n = 37, 5, 2
    fb = h * 8
    mask = torch.from_numpy(np.concatenate([cref.pack(random_bits(n, h, w, 0.5)).reshape(-1),
                                            np.zeros(8, dtype=np.uint8)])).cuda()
    marker = mask.clone()
    out = torch.full((n * fb + 8,), 7, dtype=torch.uint8, device="cuda")
    counts = torch.full((n + 1,), 7, dtype=torch.int32, device="cuda")
    hd = op._dev
    ptrs = [mask.data_ptr(), marker.data_ptr(), out.data_ptr(), counts.data_ptr()]
    for bad in range(4):
        for off in (1, 2):
            p = list(ptrs)
            p[bad] += off
            st = hd._lib.dips_mask_select(hd.ptr, p[0], n, w, h, 8, 1, 0, 0, p[1], n, 0, p[2], p[3])
            assert st == _lib.DIPS_ERR_INVALID, (bad, off)
            if bad != 3:
                st = hd._lib.dips_mask_logic(hd.ptr, p[0], n, w, h, 0, p[1], n, p[2])
                assert st == _lib.DIPS_ERR_INVALID, (bad, off)
    torch.cuda.synchronize()
    assert (out == 7).all() and (counts == 7).all()


def test_kernel_time_has_one_entry_per_call():
    import torch
    from dips_amd import DiffSeriesOperator, MaskLogic, Mode, PixelFormat
    bits = random_bits(7, 33, 65, 0.45)
    mask = torch.from_numpy(cref.pack(bits)).cuda()
    out = torch.empty_like(mask)
    counts = torch.zeros((7,), dtype=torch.int32, device="cuda")
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255, time_kernel=True)
    try:
        o.run_mask_select_device(mask, 65, out, counts_out=counts, min_area=2)               # one chunk
        o.run_mask_select_device(mask, 65, out, marker=mask[:1], chunk_frames=2)             # four chunks
        o.run_mask_logic_device(mask, 65, out, MaskLogic.Not)
        ms, launches = o.kernel_time()
        each = o.kernel_times()
    finally:
        o.close()
    assert launches == 3 and len(each) == 3 and ms > 0.0 and all(t > 0.0 for t in each)
    assert np.array_equal(out.cpu().numpy(), cref.pack(~bits))


# -- a randomized draw -------------------------------------------------------------------------------

def _draw(seed):
    """One case whose reference keeps something and drops something: drawn
    again, from the next sub-seed, until it does."""
    for sub in range(50):
        rng = np.random.default_rng([79, seed, sub])
        n, h, w = int(rng.integers(1, 4)), int(rng.integers(4, 25)), int(rng.integers(8, 101))
        bits = rng.random((n, h, w)) < rng.choice([0.2, 0.35, 0.5, 0.62])
        kind = int(rng.integers(0, 3))  # no marker, one per frame, one for all
        marker = None if kind == 0 else rng.random((n if kind == 1 else 1, h, w)) < rng.choice([0.01, 0.05])
        kw = dict(connectivity=int(rng.choice([4, 8])), min_area=int(rng.choice([1, 1, 2, 3, 6])),
                  clear_border=bool(rng.integers(0, 2)), dropped=bool(rng.integers(0, 2)))
        kw["max_area"] = int(rng.choice([0, 0, kw["min_area"], kw["min_area"] + 5]))
        kept, _ = sref.select(bits, marker, **dict(kw, dropped=False))
        if kept.any() and (bits & ~kept).any():
            return bits, marker, int(rng.integers(0, 2)), int(rng.integers(0, 3)), kw
    raise AssertionError("no non-trivial case drawn")


@pytest.mark.parametrize("block", range(10))
def test_randomized_draw(op, block):
    for seed in range(15 * block, 15 * block + 15):
        bits, marker, pad, chunk, kw = _draw(seed)
        want, _ = check(op, bits, marker, pad=pad, chunk_frames=chunk, **kw)
        other, _ = sref.select(bits, marker, **dict(kw, dropped=not kw["dropped"]))
        assert want.any() and other.any()  # kept and dropped are both non-empty
