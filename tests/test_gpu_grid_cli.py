"""`dips_raw series ... --grid RxC [--roi x,y,w,h]`: the CSV of the native
host program equals the oracle on the cell crops, line for line; a malformed
--grid is a usage error."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from test_grid_cpu import py_cell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("mode", ["overall", "per-frame"])
def test_grid_csv_matches_oracle_crops(tmp_path, mode):
    w, h, n, rows, cols, roi = 40, 30, 7, 3, 4, (5, 2, 33, 27)
    frames = np.random.default_rng(11).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    src = tmp_path / "in.raw"
    frames.tofile(src)
    r = _run(["series", src, w, h, "rgb8", "--mode", mode, "--tau", 8 / 255, "--grid", f"{rows}x{cols}",
              "--roi", ",".join(str(v) for v in roi)])
    assert r.returncode == 0, r.stderr
    want = ["t,row,col,sad,sj,count,si_fixed"]
    per_cell = {}
    for row in range(rows):
        for col in range(cols):
            x, y, cw, ch = py_cell(w, h, rows, cols, row, col, roi)
            per_cell[row, col] = oracle.series(np.ascontiguousarray(frames[:, y:y + ch, x:x + cw]),
                                               mode=0 if mode == "overall" else 1, tau=8 / 255)[0]
    bites = False
    for t in range(n):
        for row in range(rows):
            for col in range(cols):
                e = per_cell[row, col][t]
                want.append(f"{t},{row},{col},{e[0]},{e[1]},{e[2]},{e[3]}")
                cw, ch = py_cell(w, h, rows, cols, row, col, roi)[2:]
                bites |= 0 < int(e[2]) < cw * ch
    assert bites  # the threshold selects some pixels of some cell, not all
    assert r.stdout.strip().splitlines() == want


@pytest.mark.parametrize("grid", ["3", "3x", "x4", "0x4", "3x4x", "axb"])
def test_malformed_grid_is_a_usage_error(tmp_path, grid):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    r = _run(["series", src, 40, 30, "rgb8", "--grid", grid])
    assert r.returncode == 1 and "usage" in r.stderr and "--grid RxC" in r.stderr


def test_roi_without_grid_and_bad_roi_are_usage_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    assert _run(["series", src, 40, 30, "rgb8", "--roi", "0,0,8,8"]).returncode == 1
    assert _run(["series", src, 40, 30, "rgb8", "--grid", "2x2", "--roi", "0,0,8"]).returncode == 1
    r = _run(["series", src, 40, 30, "rgb8", "--grid", "2x2", "--roi", "38,0,8,8"])
    assert r.returncode == 2 and "leaves the frame" in r.stderr  # the library's refusal, with its message
