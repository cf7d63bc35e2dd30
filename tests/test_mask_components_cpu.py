"""dips_mask_components without a GPU: the specification code of
tests/_components_ref.py against scipy.ndimage (where scipy is installed),
the header's declaration and constants, the ctypes binding, the ChangeBoxes
result type and every argument error the Python layer raises itself."""
import os
import re

import numpy as np
import pytest

import _components_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_bits(seed, n, h, w, density):
    return np.random.default_rng([31, seed, n, h, w]).random((n, h, w)) < density


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("h,w,density", [(29, 37, 0.3), (29, 37, 0.593), (33, 65, 0.5), (7, 130, 0.8)])
def test_reference_agrees_with_scipy(connectivity, h, w, density):
    """The same partition, areas, boxes and the order by anchor."""
    ndi = pytest.importorskip("scipy.ndimage")
    bits = _random_bits(connectivity, 3, h, w, density)
    counts, boxes, labels = cref.components(cref.pack(bits), w, connectivity, 1, h * w, labels=True)
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    for t in range(bits.shape[0]):
        lab, num = ndi.label(bits[t], structure=structure)
        assert counts[t] == num
        assert np.array_equal(labels[t] != 0, bits[t])
        # scipy numbers the components in the order of their first pixel too:
        # the partition, with the order, is the label image itself
        assert np.array_equal(labels[t], lab.astype(np.uint32))
        for k, sl in enumerate(ndi.find_objects(lab)):
            rec = boxes[t, k]
            assert (rec[cref.Y0], rec[cref.Y1], rec[cref.X0], rec[cref.X1]) == (
                sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)
            ys, xs = np.nonzero(lab == k + 1)
            assert rec[cref.AREA] == ys.size
            assert rec[cref.ANCHOR] == ys[0] * w + xs[0]  # np.nonzero is row-major
            cx, cy = xs.mean(), ys.mean()
            assert 0 <= cx * 256 - rec[cref.CX256] < 1 + 1e-6 and 0 <= cy * 256 - rec[cref.CY256] < 1 + 1e-6
        assert not boxes[t, num:].any()


def test_reference_on_cases_worked_by_hand():
    # a diagonal: one component under 8, one per pixel under 4
    bits = np.eye(5, dtype=bool)[None]
    c8, b8, l8 = cref.components(cref.pack(bits), 5, 8, 1, 4)
    assert c8.tolist() == [1] and b8[0, 0].tolist() == [0, 0, 5, 5, 5, 0, 512, 512] and not b8[0, 1:].any()
    assert np.array_equal(l8[0], np.eye(5, dtype=np.uint32))
    c4, b4, l4 = cref.components(cref.pack(bits), 5, 4, 1, 3)
    assert c4.tolist() == [5] and b4[0, :, cref.ANCHOR].tolist() == [0, 6, 12]
    assert np.array_equal(l4[0], np.diag(np.arange(1, 6)).astype(np.uint32))
    # min_area renumbers; a component of exactly min_area pixels is kept
    bits = np.zeros((1, 3, 8), dtype=bool)
    bits[0, 0, 0] = True          # area 1, anchor 0
    bits[0, 0, 3:5] = True        # area 2, anchor 3
    bits[0, 2, 1:4] = True        # area 3, anchor 17
    c, b, lab = cref.components(cref.pack(bits), 8, 4, 2, 8)
    assert c.tolist() == [2] and b[0, :2, cref.AREA].tolist() == [2, 3] and b[0, :2, cref.ANCHOR].tolist() == [3, 17]
    assert lab[0, 0].tolist() == [0, 0, 0, 1, 1, 0, 0, 0] and lab[0, 2].tolist() == [0, 2, 2, 2, 0, 0, 0, 0]
    # centroid: sum i = 3 + 4 = 7 over 2 pixels -> 3.5 -> 896
    assert b[0, 0, cref.CX256] == 896 and b[0, 0, cref.CY256] == 0
    # the pad bits are ignored
    assert all(np.array_equal(x, y) for x, y in zip(cref.components(cref.pack(bits, pad=1), 8, 4, 2, 8), (c, b, lab)))


def test_header_declares_the_function_and_the_constants():
    from dips_amd import _lib
    assert "dips_mask_components" in _lib.header_functions()
    with open(os.path.join(ROOT, "include", "dips_hip.h")) as f:
        text = f.read()
    for k, name in enumerate(cref.FIELDS):
        assert re.search(r"^#define DIPS_BOX_%s %du$" % (name.upper(), k), text, flags=re.M), name
    assert re.search(r"^#define DIPS_BOX_WORDS 8u$", text, flags=re.M)
    assert re.search(r"^#define DIPS_ABI_VERSION 3$", text, flags=re.M)  # no new struct: the version stays
    decl = re.search(r"dips_status dips_mask_components\((.*?)\);", text, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["dips_handle *h", "const uint8_t *mask", "uint32_t n_frames", "uint32_t roi_w", "uint32_t roi_h",
                    "uint32_t connectivity", "uint32_t min_area", "uint32_t max_boxes", "uint32_t chunk_frames",
                    "uint32_t *counts", "uint32_t *boxes", "uint32_t *labels"]
    assert _lib.BOX_WORDS == 8 and _lib.BOX_FIELDS == cref.FIELDS


def test_ctypes_signature_matches():
    import ctypes

    from dips_amd import _lib
    fn = _lib.load().dips_mask_components
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    assert list(fn.argtypes) == [vp, vp] + [u32] * 7 + [vp] * 3
    assert fn.restype is ctypes.c_int


def test_change_boxes_round_trips():
    import dips_amd
    bits = _random_bits(5, 3, 9, 11, 0.4)
    counts, boxes, labels = cref.components(cref.pack(bits), 11, 8, 1, 2)
    cb = dips_amd.ChangeBoxes.from_arrays(counts, boxes, labels)
    assert dips_amd.ChangeBoxes.FIELDS == cref.FIELDS
    back = dips_amd.ChangeBoxes.from_arrays(*cb.as_arrays())
    assert np.array_equal(back.counts, counts) and np.array_equal(back.boxes, boxes)
    assert np.array_equal(back.labels, labels)
    assert (counts > 2).any() and (counts <= 2).any(), "the case must truncate some frames only"
    assert np.array_equal(cb.truncated, counts > 2)
    for t in range(3):
        m = min(int(counts[t]), 2)
        assert cb.frame(t).shape == (m, 8) and np.array_equal(cb.frame(t), boxes[t, :m])
    assert dips_amd.ChangeBoxes.from_arrays(counts, boxes).labels is None
    with pytest.raises(ValueError):
        dips_amd.ChangeBoxes.from_arrays(counts, boxes[:, :, :7])
    with pytest.raises(ValueError):
        dips_amd.ChangeBoxes.from_arrays(counts[:2], boxes)
    with pytest.raises(ValueError):
        dips_amd.ChangeBoxes.from_arrays(counts, boxes, labels[:2])


def test_python_argument_errors():
    """Raised before the library is reached, so an operator without handles will do."""
    import dips_amd
    op = dips_amd.DiffSeriesOperator.__new__(dips_amd.DiffSeriesOperator)
    good = dips_amd.ChangeMask(cref.pack(_random_bits(6, 2, 5, 33, 0.5)), 33)
    with pytest.raises(ValueError):
        op.mask_components(good.bits)                       # not a ChangeMask
    with pytest.raises(ValueError):
        op.mask_components(dips_amd.ChangeMask(good.bits, 65))   # width and row bytes disagree
    with pytest.raises(ValueError):
        op.mask_components(dips_amd.ChangeMask(good.bits[0], 33))  # not [n, h, row_bytes]
    for kw in ({"connectivity": 6}, {"connectivity": 0}, {"min_area": -1}, {"min_area": 1 << 32}, {"max_boxes": -1},
               {"max_boxes": 1 << 32}, {"chunk_frames": -1}, {"chunk_frames": 1 << 32}, {"max_boxes": 1 << 28}):
        with pytest.raises(ValueError):
            op.mask_components(good, **kw)
