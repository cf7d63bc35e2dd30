"""dips_mask_shapes without a GPU: the specification code of
tests/_shapes_ref.py against closed forms and hand-drawn figures, the
identities that tie a shape record to its box and to the frame, the derived
values of ChangeShapes, the Python layer's argument checks, and the header's
and the Rust binding's declarations."""
import math
import os
import re

import numpy as np
import pytest

import _components_ref as cref
import _shapes_ref as sref

from dips_amd import ChangeShapes, _lib
from dips_amd.api import _shapes_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _figure(rows):
    return np.array([[c == "#" for c in r] for r in rows], dtype=bool)


RING = _figure(["###",
                "#.#",
                "###"])
EIGHT = _figure(["###",
                 "#.#",
                 "###",
                 "#.#",
                 "###"])
DIAGONAL_HOLES = _figure(["####",
                          "#.##",
                          "##.#",
                          "####"])
NESTED = _figure(["#######",
                  "#.....#",
                  "#.###.#",
                  "#.#.#.#",
                  "#.###.#",
                  "#.....#",
                  "#######"])
BLOB_IN_RING = _figure(["#####",
                        "#...#",
                        "#.#.#",
                        "#...#",
                        "#####"])


def _one(bits, connectivity, weights=None, k=8):
    """(counts, boxes, shapes) of the single frame `bits`."""
    w = None if weights is None else weights[None]
    return sref.shapes(cref.pack(bits[None]), bits.shape[1], w, connectivity, 1, k)


def _euler(shapes):
    return shapes[..., sref.EULER].view(np.int32)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (33, 4), (8, 7)])
def test_all_ones_frame_has_the_closed_forms(connectivity, w, h):
    counts, boxes, shapes = _one(np.ones((h, w), dtype=bool), connectivity)
    assert counts.tolist() == [1] and boxes[0, 0, cref.AREA] == w * h
    rec = shapes[0, 0]
    assert int(sref.get64(rec, sref.SX)) == h * w * (w - 1) // 2
    assert int(sref.get64(rec, sref.SY)) == w * h * (h - 1) // 2
    assert int(sref.get64(rec, sref.SXX)) == h * ((w - 1) * w * (2 * w - 1) // 6)
    assert int(sref.get64(rec, sref.SYY)) == w * ((h - 1) * h * (2 * h - 1) // 6)
    assert int(sref.get64(rec, sref.SXY)) == (w * (w - 1) // 2) * (h * (h - 1) // 2)
    assert (int(rec[sref.CRACKS_V]), int(rec[sref.CRACKS_H])) == (2 * h, 2 * w)
    assert int(_euler(rec)) == 1 and int(sref.get64(rec, sref.WSUM)) == 0 and rec[sref.WMAX] == 0
    assert not shapes[0, 1:].any()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_ring_eight_and_nested_rings(connectivity):
    _, _, ring = _one(RING, connectivity)
    assert int(_euler(ring[0, 0])) == 0
    assert int(ring[0, 0, sref.CRACKS_V]) + int(ring[0, 0, sref.CRACKS_H]) == 16
    _, _, eight = _one(EIGHT, connectivity)
    assert int(_euler(eight[0, 0])) == -1
    counts, _, nested = _one(NESTED, connectivity)
    # the outer ring, the inner ring: one hole each, whatever lies in it
    assert counts.tolist() == [2] and _euler(nested[0, :2]).tolist() == [0, 0]


def test_blob_inside_a_ring_does_not_fill_the_hole():
    for connectivity in (4, 8):
        counts, boxes, shapes = _one(BLOB_IN_RING, connectivity)
        assert counts.tolist() == [2]
        assert boxes[0, :2, cref.AREA].tolist() == [16, 1] and _euler(shapes[0, :2]).tolist() == [0, 1]


def test_holes_touching_diagonally_are_two_under_8_and_one_under_4():
    # the holes are taken under the dual connectivity
    assert int(_euler(_one(DIAGONAL_HOLES, 8)[2][0, 0])) == -1
    assert int(_euler(_one(DIAGONAL_HOLES, 4)[2][0, 0])) == 0


@pytest.mark.parametrize("connectivity", [4, 8])
def test_ring_along_the_border_has_one_hole(connectivity):
    bits = np.ones((5, 9), dtype=bool)
    bits[1:-1, 1:-1] = False
    counts, _, shapes = _one(bits, connectivity)
    assert counts.tolist() == [1] and int(_euler(shapes[0, 0])) == 0
    assert (int(shapes[0, 0, sref.CRACKS_V]), int(shapes[0, 0, sref.CRACKS_H])) == (2 * 5 + 2 * 3, 2 * 9 + 2 * 7)


def test_checkerboard_is_one_lace_under_8_and_pixels_under_4():
    bits = (np.add.outer(np.arange(4), np.arange(5)) % 2) == 0
    counts4, _, s4 = _one(bits, 4, k=16)
    assert counts4.tolist() == [10] and _euler(s4[0, :10]).tolist() == [1] * 10
    counts8, _, s8 = _one(bits, 8, k=16)
    # the clear pixels are 4-isolated: the bounded ones are holes, those on the border are open
    inner_clear = int((~bits[1:-1, 1:-1]).sum())
    assert counts8.tolist() == [1] and int(_euler(s8[0, 0])) == 1 - inner_clear


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("seed,h,w,density", [(0, 9, 31, 0.3), (1, 13, 40, 0.55), (2, 7, 33, 0.8), (3, 1, 17, 0.5)])
def test_identities_with_the_box_and_the_frame(connectivity, seed, h, w, density):
    rng = np.random.default_rng([41, seed])
    bits = rng.random((2, h, w)) < density
    weights = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    k = h * w
    counts, boxes, shapes = sref.shapes(cref.pack(bits), w, weights, connectivity, 1, k)
    for t in range(2):
        m = int(counts[t])
        assert m <= k
        area = boxes[t, :m, cref.AREA].astype(object)
        sx, sy = sref.get64(shapes[t, :m], sref.SX).astype(object), sref.get64(shapes[t, :m], sref.SY).astype(object)
        assert boxes[t, :m, cref.CX256].tolist() == ((sx // area) * 256 + ((sx % area) * 256) // area).tolist()
        assert boxes[t, :m, cref.CY256].tolist() == ((sy // area) * 256 + ((sy % area) * 256) // area).tolist()
        assert not (shapes[t, :m, sref.CRACKS_V] & 1).any()
        frame_v, frame_h = sref.cracks(bits[t])
        assert int(shapes[t, :, sref.CRACKS_V].sum()) == frame_v and int(shapes[t, :, sref.CRACKS_H].sum()) == frame_h
        # the maximal row runs of the frame
        runs = int((bits[t] & ~np.pad(bits[t], ((0, 0), (1, 0)))[:, :-1]).sum())
        assert frame_v == 2 * runs
        assert int(_euler(shapes[t]).sum()) == sref.frame_euler(bits[t], connectivity)
        assert int(sref.get64(shapes[t], sref.WSUM).sum()) == int(weights[t][bits[t]].sum())
        assert int(shapes[t, :, sref.WMAX].max(initial=0)) == int(weights[t][bits[t]].max(initial=0))


def test_selection_and_truncation_leave_zero_records():
    bits = np.random.default_rng(5).random((1, 9, 20)) < 0.4
    full = sref.shapes(cref.pack(bits), 20, None, 8, 1, 64)
    counts, boxes, shapes = sref.shapes(cref.pack(bits), 20, None, 8, 1, 2)
    assert counts[0] == full[0][0] > 2 and np.array_equal(shapes[0], full[2][0, :2])
    counts, boxes, shapes = sref.shapes(cref.pack(bits), 20, None, 8, 3, 64)
    keep = full[1][0, :, cref.AREA] >= 3
    assert np.array_equal(shapes[0, :int(counts[0])], full[2][0][keep])


def _shapes_of(bits, connectivity=8):
    counts, boxes, shapes = _one(bits, connectivity)
    return ChangeShapes.from_arrays(counts, boxes, shapes)


@pytest.mark.parametrize("a,b", [(7, 3), (3, 7), (12, 1), (1, 12), (5, 5)])
def test_rectangle_moments_and_orientation(a, b):
    bits = np.zeros((b + 3, a + 4), dtype=bool)
    bits[2:2 + b, 3:3 + a] = True
    s = _shapes_of(bits)
    assert s.mu20[0, 0] == pytest.approx((a * a - 1) / 12, rel=1e-15)
    assert s.mu02[0, 0] == pytest.approx((b * b - 1) / 12, rel=1e-15)
    assert s.mu11[0, 0] == 0.0
    assert s.orientation[0, 0] == (0.0 if a >= b else math.pi / 2)
    major, minor = 4 * math.sqrt((max(a, b) ** 2 - 1) / 12), 4 * math.sqrt((min(a, b) ** 2 - 1) / 12)
    assert s.axes[0, 0].tolist() == pytest.approx([major, minor], rel=1e-14, abs=1e-14)
    assert s.eccentricity[0, 0] == pytest.approx(math.sqrt(1 - (minor / major) ** 2) if major else 0.0, abs=1e-12)
    assert s.compactness[0, 0] == pytest.approx((2 * a + 2 * b) ** 2 / (4 * math.pi * a * b), rel=1e-15)
    assert s.perimeter[0, 0] == 2 * a + 2 * b and s.holes[0, 0] == 0 and s.euler[0, 0] == 1
    assert np.isnan(s.mu20[0, 1]) and np.isnan(s.orientation[0, 1]) and s.holes[0, 1] == 0
    assert s.valid[0].tolist() == [True] + [False] * 7


def test_staircase_orientation_and_the_integer_accessors():
    n = 9
    stair = np.eye(n, dtype=bool) | np.eye(n, k=1, dtype=bool)  # down and to the right: +x towards +y
    weights = np.arange(n * n, dtype=np.uint8).reshape(n, n)
    counts, boxes, shapes = _one(stair, 4, weights)
    s = ChangeShapes.from_arrays(counts, boxes, shapes)
    assert s.orientation[0, 0] == pytest.approx(math.pi / 4, abs=0.05)
    diag = _shapes_of(np.eye(n, dtype=bool), 8)
    assert diag.orientation[0, 0] == pytest.approx(math.pi / 4, abs=1e-15)
    anti = _shapes_of(np.eye(n, dtype=bool)[::-1].copy(), 8)
    assert anti.orientation[0, 0] == pytest.approx(-math.pi / 4, abs=1e-15)
    ys, xs = np.nonzero(stair)
    assert s.sx.dtype == np.uint64 and s.sx[0, 0] == xs.sum() and s.sy[0, 0] == ys.sum()
    assert s.sxx[0, 0] == (xs * xs).sum() and s.syy[0, 0] == (ys * ys).sum() and s.sxy[0, 0] == (xs * ys).sum()
    assert s.wsum[0, 0] == int(weights[stair].sum()) and s.wmax[0, 0] == int(weights[stair].max())
    assert s.mean_weight[0, 0] == pytest.approx(float(weights[stair].mean()), rel=1e-15)
    assert s.euler.dtype == np.int32 and s.area[0, 0] == stair.sum()
    ring = _shapes_of(EIGHT)
    assert ring.euler[0, 0] == -1 and ring.holes[0, 0] == 2


def test_moments_are_exact_where_float64_sums_are_not():
    # one component far from the origin: A * SXX and SX^2 agree in their first 50 bits
    counts = np.array([1], dtype=np.uint32)
    boxes = np.zeros((1, 1, 8), dtype=np.uint32)
    shapes = np.zeros((1, 1, 16), dtype=np.uint32)
    x0, a = 60000, 3
    xs = [x0, x0 + 1, x0 + 2]
    boxes[0, 0, cref.AREA] = a
    sref.put64(shapes[0, 0], sref.SX, sum(xs))
    sref.put64(shapes[0, 0], sref.SXX, sum(x * x for x in xs))
    s = ChangeShapes.from_arrays(counts, boxes, shapes)
    assert s.mu20[0, 0] == 2 / 3 and s.mu02[0, 0] == 0.0


def test_from_arrays_round_trips_and_refuses():
    counts, boxes, shapes = _one(NESTED, 8)
    s = ChangeShapes.from_arrays(counts.tolist(), boxes.tolist(), shapes.tolist())
    for got, want in zip(s.as_arrays(), (counts, boxes, shapes)):
        assert got.dtype == np.uint32 and np.array_equal(got, want)
    b, r = s.frame(0)
    assert b.shape == (2, 8) and r.shape == (2, 16)
    with pytest.raises(ValueError):
        ChangeShapes.from_arrays(counts, boxes, shapes[:, :, :15])
    with pytest.raises(ValueError):
        ChangeShapes.from_arrays(counts, boxes, shapes[:, :4])
    with pytest.raises(ValueError):
        ChangeShapes.from_arrays(counts, boxes[:, :, :7], shapes)


def test_shapes_args_refusals():
    assert _shapes_args(8, 1, 64, 0, 5, 65536, 16383) == (8, 1, 64, 0)
    assert _shapes_args(4, 0, 0, 3, 5, 1, 1) == (4, 0, 0, 3)
    for bad in ((6, 1, 64, 0, 5, 10, 10),          # connectivity
                (8, -1, 64, 0, 5, 10, 10),         # min_area
                (8, 1, 1 << 32, 0, 5, 10, 10),     # max_boxes
                (8, 1, 64, -2, 5, 10, 10),         # chunk_frames
                (8, 1, 64, 0, 5, 65537, 10),       # width
                (8, 1, 64, 0, 5, 10, 65537),       # height
                (8, 1, 1 << 20, 0, 256, 10, 10),   # n * K * 16 = 2^32
                (8, 1, 1 << 21, 0, 256, 10, 10)):  # n * K * 8 = 2^32
        with pytest.raises(ValueError):
            _shapes_args(*bad)
    assert _shapes_args(8, 1, (1 << 20) - 1, 0, 256, 10, 10)[2] == (1 << 20) - 1


def test_header_binding_and_build_declare_the_call():
    with open(os.path.join(ROOT, "include", "dips_hip.h")) as f:
        text = f.read()
    flat = re.sub(r"\s+", " ", text)
    assert ("dips_status dips_mask_shapes(dips_handle *h, const uint8_t *mask, const uint8_t *weights, "
            "uint32_t n_frames, uint32_t roi_w, uint32_t roi_h, uint32_t connectivity, uint32_t min_area, "
            "uint32_t max_boxes, uint32_t chunk_frames, uint32_t *counts, uint32_t *boxes, uint32_t *shapes);") in flat
    for name, value in (("SX", sref.SX), ("SY", sref.SY), ("SXX", sref.SXX), ("SYY", sref.SYY), ("SXY", sref.SXY),
                        ("WSUM", sref.WSUM), ("WMAX", sref.WMAX), ("CRACKS_V", sref.CRACKS_V),
                        ("CRACKS_H", sref.CRACKS_H), ("EULER", sref.EULER), ("WORDS", 16)):
        assert re.search(rf"#define DIPS_SHAPE_{name} {value}u\b", text), name
    assert _lib.SHAPE_WORDS == sref.WORDS == 16
    assert _lib.SHAPE_OFFSETS == dict(zip(sref.COLUMNS, (sref.SX, sref.SY, sref.SXX, sref.SYY, sref.SXY, sref.WSUM,
                                                         sref.WMAX, sref.CRACKS_V, sref.CRACKS_H, sref.EULER)))
    assert "dips_mask_shapes" in _lib.header_functions()
    with open(os.path.join(ROOT, "rust", "dips-hip", "src", "ffi.rs")) as f:
        rs = re.sub(r"\s+", " ", f.read())
    assert ("pub fn dips_mask_shapes(h: *mut DipsHandle, mask: *const u8, weights: *const u8, n_frames: u32, "
            "roi_w: u32, roi_h: u32, connectivity: u32, min_area: u32, max_boxes: u32, chunk_frames: u32, "
            "counts: *mut u32, boxes: *mut u32, shapes: *mut u32) -> DipsStatus;") in rs
    with open(os.path.join(ROOT, "dips_amd", "csrc", "Makefile")) as f:
        assert "mask_shapes.hip" in f.read()
