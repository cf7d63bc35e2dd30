"""dips_mask_select, dips_mask_logic and mask_fill_holes without a GPU: the
specification code of tests/_select_ref.py against definitions that share
nothing with it (a dilation fixpoint, a border flood fill, scipy.ndimage where
it is installed), its algebraic properties, the header's declarations and
constants, the ctypes binding and every argument error the Python layer raises
before any device work."""
import os
import re

import numpy as np
import pytest

import _components_ref as cref
import _select_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1), (1, 33), (7, 1), (9, 31), (29, 37), (13, 70)]


def _random_bits(seed, n, h, w, density):
    return np.random.default_rng([97, seed, n, h, w]).random((n, h, w)) < density


def _dilate(x, connectivity):
    """x bool [h, w] dilated by the plus (4) or the 3 x 3 box (8); outside is clear."""
    p = np.pad(x, 1)
    h, w = x.shape
    out = np.zeros_like(x)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            if connectivity == 4 and dj != 0 and di != 0:
                continue
            out |= p[1 + dj:1 + dj + h, 1 + di:1 + di + w]
    return out


def _reconstruct(mask, marker, connectivity):
    """The fixpoint of X <- dilate(X) & mask from X = marker & mask."""
    x = marker & mask
    while True:
        nxt = _dilate(x, connectivity) & mask
        if np.array_equal(nxt, x):
            return x
        x = nxt


def _ring(h, w):
    edge = np.zeros((h, w), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    return edge


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("h,w", SHAPES)
def test_reconstruction_is_the_dilation_fixpoint(connectivity, h, w):
    for density, mdensity in ((0.45, 0.05), (0.62, 0.02), (0.9, 0.01)):
        bits = _random_bits(1, 3, h, w, density)
        marker = _random_bits(2, 3, h, w, mdensity)
        got, counts = sref.select(bits, marker, connectivity)
        for t in range(3):
            assert np.array_equal(got[t], _reconstruct(bits[t], marker[t], connectivity))
        one, _ = sref.select(bits, marker[:1], connectivity)  # a one-frame marker serves every frame
        for t in range(3):
            assert np.array_equal(one[t], _reconstruct(bits[t], marker[0], connectivity))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("h,w", SHAPES)
def test_fill_holes_is_the_complement_of_the_border_flood_fill(connectivity, h, w):
    for density in (0.4, 0.6, 0.8):
        bits = _random_bits(3, 2, h, w, density)
        got = sref.fill_holes(bits, connectivity)
        for t in range(2):
            outside = _reconstruct(~bits[t], _ring(h, w), 12 - connectivity)
            assert np.array_equal(got[t], ~outside)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("h,w", SHAPES)
def test_clear_border_is_the_dropped_reconstruction_from_the_border_ring(connectivity, h, w):
    bits = _random_bits(4, 3, h, w, 0.5)
    got, _ = sref.select(bits, None, connectivity, clear_border=True)
    want, _ = sref.select(bits, _ring(h, w)[None], connectivity, dropped=True)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_against_scipy(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    dual = np.ones((3, 3), dtype=bool) if connectivity == 4 else ndi.generate_binary_structure(2, 1)
    for h, w in SHAPES:
        bits = _random_bits(5, 2, h, w, 0.6)
        marker = _random_bits(6, 2, h, w, 0.03)
        rec, _ = sref.select(bits, marker, connectivity)
        filled = sref.fill_holes(bits, connectivity)
        for t in range(2):
            assert np.array_equal(rec[t], ndi.binary_propagation(marker[t] & bits[t], structure=structure, mask=bits[t]))
            # scipy fills the holes of the complement taken under `structure`: the dual of the mask's
            assert np.array_equal(filled[t], ndi.binary_fill_holes(bits[t], structure=dual))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_properties(connectivity):
    for h, w in SHAPES:
        bits = _random_bits(7, 3, h, w, 0.5)
        marker = _random_bits(8, 3, h, w, 0.05)
        for kw in (dict(min_area=3), dict(max_area=4), dict(min_area=2, max_area=9, clear_border=True),
                   dict(marker=marker), dict(marker=marker, clear_border=True, min_area=2)):
            kw = dict(kw)
            mk = kw.pop("marker", None)
            kept, counts = sref.select(bits, mk, connectivity, **kw)
            gone, counts_d = sref.select(bits, mk, connectivity, dropped=True, **kw)
            assert np.array_equal(kept | gone, bits) and not (kept & gone).any()  # a partition of the mask
            assert np.array_equal(counts, counts_d)  # the kept components either way
            again, counts2 = sref.select(kept, mk, connectivity, **kw)
            assert np.array_equal(again, kept) and np.array_equal(counts2, counts)  # idempotent
        for min_area in (1, 2, 5):
            kept, counts = sref.select(bits, None, connectivity, min_area)
            c, _, labels = cref.components(cref.pack(bits), w, connectivity, min_area, 1, labels=True)
            assert np.array_equal(counts, c) and np.array_equal(kept, labels != 0)


def test_cases_worked_by_hand():
    bits = np.zeros((1, 5, 8), dtype=bool)
    bits[0, 0, 0] = True           # area 1, on the border
    bits[0, 2, 2:4] = True         # area 2, inside
    bits[0, 1:4, 6] = True         # area 3, inside
    bits[0, 3, 7] = True           # joins the area-3 one: area 4, now on the border
    kept, counts = sref.select(bits, None, 8, min_area=2)
    assert counts.tolist() == [2] and kept.sum() == 6 and not kept[0, 0, 0]
    kept, counts = sref.select(bits, None, 8, min_area=2, max_area=3)
    assert counts.tolist() == [1] and np.array_equal(np.argwhere(kept[0]), [[2, 2], [2, 3]])
    kept, counts = sref.select(bits, None, 8, clear_border=True)
    assert counts.tolist() == [1] and kept.sum() == 2
    marker = np.zeros_like(bits)
    marker[0, 3, 7] = marker[0, 4, 4] = True  # the second on a clear pixel: no effect
    kept, counts = sref.select(bits, marker, 8)
    assert counts.tolist() == [1] and kept.sum() == 4 and kept[0, 1, 6]
    # a diagonal: one component under 8, pixels under 4
    diag = np.eye(4, dtype=bool)[None]
    assert sref.select(diag, None, 8, min_area=4)[0].sum() == 4
    assert sref.select(diag, None, 4, min_area=2)[0].sum() == 0
    # a ring closed only diagonally holds its hole under 8 and leaks under 4
    ring = np.zeros((1, 5, 5), dtype=bool)
    ring[0, 1, 2] = ring[0, 2, 1] = ring[0, 2, 3] = ring[0, 3, 2] = True
    assert sref.fill_holes(ring, 8)[0, 2, 2] and not sref.fill_holes(ring, 4)[0, 2, 2]
    # max_hole, and a hole that touches the border
    box = np.zeros((1, 6, 9), dtype=bool)
    box[0, 0:5, 0:5] = True
    box[0, 1:4, 1:4] = False       # a hole of 9
    box[0, 1:4, 6:9] = True
    box[0, 2, 7] = False           # a hole of 1
    box[0, 2, 8] = False           # ... that now touches the border: not a hole
    assert np.array_equal(sref.fill_holes(box, 8)[0, 1:4, 1:4], np.ones((3, 3), dtype=bool))
    assert not sref.fill_holes(box, 8)[0, 2, 7]
    assert not sref.fill_holes(box, 8, max_hole=8)[0, 2, 2] and sref.fill_holes(box, 8, max_hole=9)[0, 2, 2]
    # logic: NOT stays inside the region
    z = np.zeros((2, 3, 33), dtype=bool)
    assert np.unpackbits(sref.logic_bytes(cref.pack(z, pad=1), 33, sref.NOT), axis=-1).sum() == 2 * 3 * 33


def test_packed_forms_ignore_input_pad_bits():
    bits = _random_bits(9, 2, 5, 37, 0.5)
    marker = _random_bits(10, 2, 5, 37, 0.1)
    for pad in (0, 1):
        got, counts = sref.select_bytes(cref.pack(bits, pad), 37, cref.pack(marker, pad), min_area=2)
        want, wc = sref.select(bits, marker, min_area=2)
        assert np.array_equal(got, cref.pack(want)) and np.array_equal(counts, wc)
        for op in (sref.AND, sref.OR, sref.XOR, sref.ANDNOT):
            assert np.array_equal(sref.logic_bytes(cref.pack(bits, pad), 37, op, cref.pack(marker, pad)),
                                  cref.pack(sref.logic(bits, op, marker)))
        assert np.array_equal(sref.fill_holes_bytes(cref.pack(bits, pad), 37), cref.pack(sref.fill_holes(bits)))


# -- the header, the binding, the Python layer's own checks -------------------------

def test_header_declares_the_calls_and_constants():
    with open(os.path.join(ROOT, "include", "dips_hip.h")) as f:
        text = f.read()
    flat = re.sub(r"\s+", " ", text)
    assert ("dips_status dips_mask_select(dips_handle *h, const uint8_t *mask, uint32_t n_frames, uint32_t roi_w, "
            "uint32_t roi_h, uint32_t connectivity, uint32_t min_area, uint32_t max_area, uint32_t select, "
            "const uint8_t *marker, uint32_t marker_frames, uint32_t chunk_frames, uint8_t *mask_out, "
            "uint32_t *counts);") in flat
    assert ("dips_status dips_mask_logic(dips_handle *h, const uint8_t *a, uint32_t n_frames, uint32_t roi_w, "
            "uint32_t roi_h, uint32_t op, const uint8_t *b, uint32_t b_frames, uint8_t *mask_out);") in flat
    from dips_amd import MaskLogic, _lib
    consts = dict(re.findall(r"#define (DIPS_(?:SELECT|LOGIC)_[A-Z_]+) (0x[0-9a-f]+|\d+)u", text))
    assert {k: int(v, 0) for k, v in consts.items()} == {
        "DIPS_SELECT_CLEAR_BORDER": _lib.SELECT_CLEAR_BORDER, "DIPS_SELECT_DROPPED": _lib.SELECT_DROPPED,
        "DIPS_LOGIC_AND": MaskLogic.And, "DIPS_LOGIC_OR": MaskLogic.Or, "DIPS_LOGIC_XOR": MaskLogic.Xor,
        "DIPS_LOGIC_ANDNOT": MaskLogic.AndNot, "DIPS_LOGIC_NOT": MaskLogic.Not}
    assert (sref.AND, sref.OR, sref.XOR, sref.ANDNOT, sref.NOT) == tuple(int(v) for v in MaskLogic)
    assert {"dips_mask_select", "dips_mask_logic"} <= set(_lib.header_functions())


def test_kernel_unit_is_built():
    with open(os.path.join(ROOT, "dips_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert "mask_select.hip" in mk and "mask_labelling.h" in mk


class _NoHandle:
    """Stands where a handle would: any use of it is device work."""
    def __getattr__(self, name):
        raise AssertionError("the argument check must come before any device work")


def _operator():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    op = DiffSeriesOperator.__new__(DiffSeriesOperator)
    op.fmt, op.mode, op.tau = PixelFormat.RGB8, Mode.PerFrame, 8 / 255
    op._host = op._dev = _NoHandle()
    op._strong = {}
    return op


def test_python_argument_checks_come_first():
    from dips_amd import ChangeMask, MaskLogic
    op = _operator()
    good = ChangeMask(np.zeros((2, 3, 8), dtype=np.uint8), 40)
    with pytest.raises(ValueError, match="ChangeMask"):
        op.mask_select(np.zeros((2, 3, 8), dtype=np.uint8))
    with pytest.raises(ValueError, match="mask.bits"):
        op.mask_select(ChangeMask(np.zeros((2, 3, 4), dtype=np.uint8), 40))
    with pytest.raises(ValueError, match="connectivity"):
        op.mask_select(good, connectivity=6)
    with pytest.raises(ValueError, match="min_area"):
        op.mask_select(good, min_area=-1)
    with pytest.raises(ValueError, match="max_area"):
        op.mask_select(good, max_area=1 << 32)
    with pytest.raises(ValueError, match="max_area must be 0"):
        op.mask_select(good, min_area=5, max_area=4)
    with pytest.raises(ValueError, match="chunk_frames"):
        op.mask_select(good, chunk_frames=-1)
    with pytest.raises(ValueError, match="marker"):
        op.mask_select(good, marker=ChangeMask(np.zeros((3, 3, 8), dtype=np.uint8), 40))  # 3 frames for 2
    with pytest.raises(ValueError, match="marker"):
        op.mask_select(good, marker=ChangeMask(np.zeros((1, 4, 8), dtype=np.uint8), 40))  # another height
    with pytest.raises(ValueError, match="marker"):
        op.mask_select(good, marker=ChangeMask(np.zeros((1, 3, 8), dtype=np.uint8), 33))  # another width
    with pytest.raises(ValueError, match="MaskLogic"):
        op.mask_logic(good, 5, good)
    with pytest.raises(ValueError, match="takes no b"):
        op.mask_logic(good, MaskLogic.Not, good)
    with pytest.raises(ValueError, match="needs one"):
        op.mask_logic(good, MaskLogic.And)
    with pytest.raises(ValueError, match="b must hold"):
        op.mask_logic(good, MaskLogic.Or, ChangeMask(np.zeros((3, 3, 8), dtype=np.uint8), 40))
    with pytest.raises(ValueError, match="connectivity"):
        op.mask_fill_holes(good, connectivity=5)
    with pytest.raises(ValueError, match="max_hole"):
        op.mask_fill_holes(good, max_hole=-1)
    with pytest.raises(ValueError, match="tau_high"):
        op.hysteresis_mask(np.zeros((2, 4, 4, 3), dtype=np.uint8), 4 / 255)
    frames = np.zeros((2, 4, 4, 3), dtype=np.uint8)
    for bad in ({"area": 3}, {"connectivity": 5}, {"min_area": 4, "max_area": 2}, {"fill_holes": -1}, [("min_area", 2)]):
        for call in (op.change_boxes, op.change_tracks, op.change_activity_selected):
            with pytest.raises(ValueError):
                call(frames, select=bad)
    with pytest.raises(ValueError):
        op.change_activity_selected(frames, None)


def test_ctypes_binding_lists_the_calls():
    import inspect
    from dips_amd import _lib
    src = inspect.getsource(_lib.load)
    assert '"dips_mask_select": ([_vp, _u8p, u32, u32, u32, u32, u32, u32, u32, _u8p, u32, u32, _u8p, _vp], st)' in src
    assert '"dips_mask_logic": ([_vp, _u8p, u32, u32, u32, u32, _u8p, u32, _u8p], st)' in src
