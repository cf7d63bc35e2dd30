"""dips_mask_morph without a GPU: the specification code of
tests/_morph_ref.py against scipy.ndimage (where scipy is installed) and on
cases worked by hand, the algebra the border choice buys, the header's
declaration and constants, the ctypes binding, every argument error the
Python layer raises itself, and the condition on the randomized draw that the
GPU fuzz relies on."""
import os
import re

import numpy as np
import pytest

import _components_ref as cref
import _morph_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_bits(seed, n, h, w, density):
    return np.random.default_rng([53, seed, n, h, w]).random((n, h, w)) < density


def _scipy(ndi, frame, op, shape, rx, ry):
    if shape == mref.BOX:
        st = np.ones((2 * ry + 1, 2 * rx + 1), dtype=bool)
    else:
        yy, xx = np.mgrid[-rx:rx + 1, -rx:rx + 1]
        st = np.abs(yy) + np.abs(xx) <= rx

    def dil(x):
        return ndi.binary_dilation(x, structure=st, border_value=0)

    def ero(x):
        return ndi.binary_erosion(x, structure=st, border_value=1)

    return {mref.ERODE: lambda x: ero(x), mref.DILATE: lambda x: dil(x), mref.OPEN: lambda x: dil(ero(x)),
            mref.CLOSE: lambda x: ero(dil(x))}[op](frame)


RADII = [(0, 0), (1, 1), (2, 2), (5, 5), (15, 15), (1, 0), (0, 2), (5, 1), (2, 15)]


@pytest.mark.parametrize("op", [mref.ERODE, mref.DILATE, mref.OPEN, mref.CLOSE])
@pytest.mark.parametrize("h,w,density", [(29, 37, 0.3), (33, 65, 0.8), (7, 130, 0.97), (64, 97, 0.03)])
def test_reference_agrees_with_scipy(op, h, w, density):
    ndi = pytest.importorskip("scipy.ndimage")
    bits = _random_bits(op, 2, h, w, density)
    for rx, ry in RADII:
        got = mref.morph_bits(bits, op, mref.BOX, rx, ry)
        for t in range(bits.shape[0]):
            assert np.array_equal(got[t], _scipy(ndi, bits[t], op, mref.BOX, rx, ry)), ("box", rx, ry, t)
        if rx == ry:
            got = mref.morph_bits(bits, op, mref.DIAMOND, rx, rx)
            for t in range(bits.shape[0]):
                assert np.array_equal(got[t], _scipy(ndi, bits[t], op, mref.DIAMOND, rx, rx)), ("diamond", rx, t)


def test_reference_on_cases_worked_by_hand():
    # one pixel dilates to the box or the diamond, clipped to the region
    one = np.zeros((1, 5, 7), dtype=bool)
    one[0, 1, 5] = True
    box = np.zeros_like(one)
    box[0, 0:3, 3:7] = True                      # |dx| <= 2 clipped at i = 6, |dy| <= 1
    assert np.array_equal(mref.morph_bits(one, mref.DILATE, mref.BOX, 2, 1), box)
    dia = np.zeros_like(one)
    dia[0, 1, 3:7] = True
    dia[0, 0, 4:7] = dia[0, 2, 4:7] = True
    dia[0, 3, 5] = True                          # the row above the region's top is cut off
    assert np.array_equal(mref.morph_bits(one, mref.DILATE, mref.DIAMOND, 2), dia)
    # all ones erode to all ones, whatever the radius
    ones = np.ones((2, 3, 33), dtype=bool)
    for shape, rx, ry in ((mref.BOX, 15, 15), (mref.BOX, 1, 0), (mref.DIAMOND, 15, 15)):
        assert mref.morph_bits(ones, mref.ERODE, shape, rx, ry).all()
        assert mref.morph_bits(ones, mref.OPEN, shape, rx, ry).all()
    # open removes an isolated pixel and keeps a 3 x 3 block
    x = np.zeros((1, 8, 40), dtype=bool)
    x[0, 2:5, 30:33] = True
    x[0, 6, 3] = True
    kept = x.copy()
    kept[0, 6, 3] = False
    assert np.array_equal(mref.morph_bits(x, mref.OPEN, mref.BOX, 1), kept)
    # close fills a one-pixel hole
    x = np.zeros((1, 8, 40), dtype=bool)
    x[0, 2:6, 29:36] = True                      # a row away from the border: closing would extend it there
    filled = x.copy()
    x[0, 3, 32] = False
    assert np.array_equal(mref.morph_bits(x, mref.CLOSE, mref.BOX, 1), filled)
    assert np.array_equal(mref.morph_bits(x, mref.CLOSE, mref.DIAMOND, 1), filled)
    # a set last row of frame 0 does not reach frame 1, nor a row's end the next row
    x = np.zeros((2, 4, 33), dtype=bool)
    x[0, 3, :] = True
    x[0, 0, 32] = True
    got = mref.morph_bits(x, mref.DILATE, mref.BOX, 2, 2)
    assert not got[1].any() and got[0, 1:].all() and not got[0, 0, :30].any() and got[0, 0, 30:].all()
    # the packed form: pad bits of the input ignored, of the output zero; (0, 0) is the identity
    bits = _random_bits(0, 2, 3, 33, 0.5)
    for op in range(4):
        for shape in (mref.BOX, mref.DIAMOND):
            assert np.array_equal(mref.morph(cref.pack(bits, pad=1), 33, op, shape, 0, 0), cref.pack(bits))
    assert np.array_equal(mref.morph(cref.pack(bits, pad=1), 33, mref.CLOSE, mref.BOX, 2, 1),
                          mref.morph(cref.pack(bits), 33, mref.CLOSE, mref.BOX, 2, 1))


@pytest.mark.parametrize("shape,rx,ry", [(mref.BOX, 1, 1), (mref.BOX, 3, 0), (mref.BOX, 2, 5), (mref.BOX, 15, 15),
                                         (mref.DIAMOND, 1, 1), (mref.DIAMOND, 4, 4), (mref.DIAMOND, 15, 15)])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 33), (29, 65), (64, 97)])
def test_algebra_on_random_frames(shape, rx, ry, h, w):
    for density in (0.2, 0.8):
        x = _random_bits(rx + 16 * shape, 2, h, w, density)
        ero, dil = (mref.morph_bits(x, op, shape, rx, ry) for op in (mref.ERODE, mref.DILATE))
        opened, closed = (mref.morph_bits(x, op, shape, rx, ry) for op in (mref.OPEN, mref.CLOSE))
        # duality: erode(X) = D \ dilate(D \ X)
        assert np.array_equal(ero, ~mref.morph_bits(~x, mref.DILATE, shape, rx, ry))
        # open <= X <= close, erode <= X <= dilate
        assert not (opened & ~x).any() and not (x & ~closed).any()
        assert not (ero & ~x).any() and not (x & ~dil).any()
        # idempotence
        assert np.array_equal(mref.morph_bits(opened, mref.OPEN, shape, rx, ry), opened)
        assert np.array_equal(mref.morph_bits(closed, mref.CLOSE, shape, rx, ry), closed)
        if shape == mref.DIAMOND:
            # the diamond of radius r is r rounds of the radius-1 cross
            for op in (mref.ERODE, mref.DILATE):
                y = x
                for _ in range(rx):
                    y = mref.morph_bits(y, op, mref.DIAMOND, 1)
                assert np.array_equal(y, ero if op == mref.ERODE else dil)


def test_header_declares_the_function_and_the_constants():
    from dips_amd import _lib
    assert "dips_mask_morph" in _lib.header_functions()
    with open(os.path.join(ROOT, "include", "dips_hip.h")) as f:
        text = f.read()
    for name, value in (("ERODE", 0), ("DILATE", 1), ("OPEN", 2), ("CLOSE", 3), ("BOX", 0), ("DIAMOND", 1),
                        ("MAX_RADIUS", 15)):
        assert re.search(r"^#define DIPS_MORPH_%s %du\b" % (name, value), text, flags=re.M), name
    assert re.search(r"^#define DIPS_ABI_VERSION 3$", text, flags=re.M)  # no new struct: the version stays
    decl = re.search(r"dips_status dips_mask_morph\((.*?)\);", text, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["dips_handle *h", "const uint8_t *mask_in", "uint32_t n_frames", "uint32_t roi_w",
                    "uint32_t roi_h", "uint32_t op", "uint32_t shape", "uint32_t rx", "uint32_t ry",
                    "uint8_t *mask_out"]
    assert (_lib.MORPH_ERODE, _lib.MORPH_DILATE, _lib.MORPH_OPEN, _lib.MORPH_CLOSE) == (0, 1, 2, 3)
    assert (_lib.MORPH_BOX, _lib.MORPH_DIAMOND, _lib.MORPH_MAX_RADIUS) == (0, 1, 15)
    import dips_amd
    assert [int(v) for v in dips_amd.MorphOp] == [mref.ERODE, mref.DILATE, mref.OPEN, mref.CLOSE]
    assert [int(v) for v in dips_amd.MorphShape] == [mref.BOX, mref.DIAMOND]


def test_ctypes_signature_matches():
    import ctypes

    from dips_amd import _lib
    fn = _lib.load().dips_mask_morph
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    assert list(fn.argtypes) == [vp, vp] + [u32] * 7 + [vp]
    assert fn.restype is ctypes.c_int


def test_python_argument_errors():
    """Raised before the library is reached, so an operator without handles will do."""
    import dips_amd
    from dips_amd import MorphOp, MorphShape
    op = dips_amd.DiffSeriesOperator.__new__(dips_amd.DiffSeriesOperator)
    good = dips_amd.ChangeMask(cref.pack(_random_bits(6, 2, 5, 33, 0.5)), 33)
    with pytest.raises(ValueError):
        op.mask_morph(good.bits, MorphOp.Open)                            # not a ChangeMask
    with pytest.raises(ValueError):
        op.mask_morph(dips_amd.ChangeMask(good.bits, 65), MorphOp.Open)   # width and row bytes disagree
    with pytest.raises(ValueError):
        op.mask_morph(dips_amd.ChangeMask(good.bits[0], 33), MorphOp.Open)  # not [n, h, row_bytes]
    with pytest.raises(ValueError):
        op.mask_morph(dips_amd.ChangeMask(good.bits[:, :0], 33), MorphOp.Open)  # no rows
    with pytest.raises(ValueError):
        op.mask_morph(dips_amd.ChangeMask(good.bits[:, :, :0], 0), MorphOp.Open)  # no columns
    for kw in ({"op": 4}, {"op": -1}, {"shape": 2}, {"shape": -1}, {"rx": 16}, {"rx": -1}, {"ry": 16}, {"ry": -1},
               {"shape": MorphShape.Diamond, "rx": 2, "ry": 1}, {"shape": MorphShape.Diamond, "rx": 0, "ry": 1}):
        args = {"op": MorphOp.Open, **kw}
        with pytest.raises(ValueError):
            op.mask_morph(good, **args)
    # change_boxes checks its steps before it touches the device
    from dips_amd.api import _morph_steps
    assert _morph_steps([(MorphOp.Open, MorphShape.Box, 1, None), (3, 1, 2, 2)], 33, 5) == [(2, 0, 1, 1), (3, 1, 2, 2)]
    for bad in ([(MorphOp.Open, MorphShape.Box, 1)], [(0, 0, 16, 0)], [(0, 1, 2, 3)], [(9, 0, 1, 1)]):
        with pytest.raises(ValueError):
            _morph_steps(bad, 33, 5)


def test_randomized_draw_is_not_trivial():
    """The condition the GPU fuzz stands on: at least half of the 300 cases,
    and at least 40 % of each operation's, have an output with both set and
    clear bits that differs from the input."""
    total = [0] * 4
    good = [0] * 4
    for k in range(300):
        x, op, shape, rx, ry = mref.draw_case(k)
        total[op] += 1
        good[op] += mref.nontrivial(x, mref.morph_bits(x, op, shape, rx, ry))
    print("qualifying per op (erode, dilate, open, close):", list(zip(good, total)))
    assert sum(total) == 300 and 2 * sum(good) >= 300, (good, total)
    for op in range(4):
        assert total[op] > 0 and good[op] >= 0.4 * total[op], (mref.OP_NAMES[op], good[op], total[op])
