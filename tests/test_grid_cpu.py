"""CPU checks of the grid form of the series (dips_grid_cell,
dips_diff_series_grid): the cell split of the C ABI against a pure-Python
restatement, its refusals, and the ctypes bindings.  The library loads
without a device; dips_grid_cell is host only."""
import ctypes

import numpy as np
import pytest

from dips_amd import _lib, grid_cell
from dips_amd._lib import DipsError


def py_cell(width, height, rows, cols, row, col, roi=None):
    """The split restated: column c covers [x + c*w//cols, x + (c+1)*w//cols)."""
    x, y, w, h = roi if roi is not None else (0, 0, width, height)
    x0, x1 = x + col * w // cols, x + (col + 1) * w // cols
    y0, y1 = y + row * h // rows, y + (row + 1) * h // rows
    return x0, y0, x1 - x0, y1 - y0


def _random_cases(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        width, height = int(rng.integers(1, 5000)), int(rng.integers(1, 3000))
        if rng.integers(0, 2):
            w, h = int(rng.integers(1, width + 1)), int(rng.integers(1, height + 1))
            roi = (int(rng.integers(0, width - w + 1)), int(rng.integers(0, height - h + 1)), w, h)
        else:
            roi, w, h = None, width, height
        rows, cols = int(rng.integers(1, min(h, 40) + 1)), int(rng.integers(1, min(w, 40) + 1))
        yield width, height, roi, rows, cols


def test_lib_binds_both_functions():
    lib = _lib.load()
    assert lib.dips_grid_cell.restype is ctypes.c_int
    assert len(lib.dips_grid_cell.argtypes) == 8
    assert len(lib.dips_diff_series_grid.argtypes) == 10
    assert {"dips_grid_cell", "dips_diff_series_grid"} <= set(_lib.header_functions())


def test_grid_cell_equals_the_python_split():
    for width, height, roi, rows, cols in _random_cases(60, 1):
        for row, col in {(0, 0), (rows - 1, cols - 1), (rows // 2, cols // 3)}:
            assert grid_cell(width, height, rows, cols, row, col, roi) == \
                py_cell(width, height, rows, cols, row, col, roi), (width, height, roi, rows, cols, row, col)


def test_cells_tile_the_roi_and_differ_by_at_most_one():
    for width, height, roi, rows, cols in _random_cases(25, 2):
        x, y, w, h = roi if roi is not None else (0, 0, width, height)
        xs = [grid_cell(width, height, rows, cols, 0, c, roi) for c in range(cols)]
        ys = [grid_cell(width, height, rows, cols, r, 0, roi) for r in range(rows)]
        # columns: contiguous from x to x + w, every width >= 1 and within 1 of the others
        assert xs[0][0] == x and xs[-1][0] + xs[-1][2] == x + w
        assert all(a[0] + a[2] == b[0] for a, b in zip(xs, xs[1:]))
        widths = [c[2] for c in xs]
        assert min(widths) >= 1 and max(widths) - min(widths) <= 1
        assert ys[0][1] == y and ys[-1][1] + ys[-1][3] == y + h
        assert all(a[1] + a[3] == b[1] for a, b in zip(ys, ys[1:]))
        heights = [r[3] for r in ys]
        assert min(heights) >= 1 and max(heights) - min(heights) <= 1
        # a cell is the product of its column and its row
        r, c = rows - 1, cols // 2
        assert grid_cell(width, height, rows, cols, r, c, roi) == (xs[c][0], ys[r][1], xs[c][2], ys[r][3])


def test_issue_examples():
    assert [grid_cell(37, 29, 4, 3, 0, c)[2] for c in range(3)] == [12, 12, 13]
    assert [grid_cell(37, 29, 2, 5, 0, c, (3, 2, 21, 17))[2] for c in range(5)] == [4, 4, 4, 4, 5]
    assert grid_cell(37, 29, 1, 1, 0, 0, (1, 0, 3, 29)) == (1, 0, 3, 29)


@pytest.mark.parametrize("args", [
    dict(rows=0, cols=1), dict(rows=1, cols=0),                        # no cells
    dict(rows=30, cols=1), dict(rows=1, cols=38),                      # more cells than pixels
    dict(rows=1, cols=1, roi=(0, 0, 0, 5)), dict(rows=1, cols=1, roi=(0, 0, 5, 0)),  # zero extent
    dict(rows=1, cols=1, roi=(30, 0, 8, 5)), dict(rows=1, cols=1, roi=(0, 25, 5, 5)),  # leaves the frame
    dict(rows=1, cols=1, roi=(0xFFFFFFFF, 0, 2, 2)),                   # x + w wraps in 32 bits
    dict(rows=2, cols=2, row=2), dict(rows=2, cols=2, col=2),          # no such cell
    dict(rows=3, cols=1, roi=(0, 0, 5, 2)),                            # rows > roi height
])
def test_invalid_arguments_return_minus_one(args):
    lib = _lib.load()
    rect = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    roi = args.get("roi")
    roi_c = (ctypes.c_uint32 * 4)(*roi) if roi is not None else None
    st = lib.dips_grid_cell(37, 29, roi_c, args["rows"], args["cols"], args.get("row", 0), args.get("col", 0), rect)
    assert st == _lib.DIPS_ERR_INVALID == -1
    assert list(rect) == [7, 7, 7, 7]  # nothing written
    with pytest.raises(DipsError):
        grid_cell(37, 29, args["rows"], args["cols"], args.get("row", 0), args.get("col", 0), roi)


def test_null_rect_and_empty_frame():
    lib = _lib.load()
    assert lib.dips_grid_cell(37, 29, None, 1, 1, 0, 0, None) == -1
    rect = (ctypes.c_uint32 * 4)()
    assert lib.dips_grid_cell(0, 29, None, 1, 1, 0, 0, rect) == -1
    assert lib.dips_grid_cell(37, 0, None, 1, 1, 0, 0, rect) == -1
    assert lib.dips_grid_cell(37, 29, None, 1, 1, 0, 0, rect) == 0 and list(rect) == [0, 0, 37, 29]
