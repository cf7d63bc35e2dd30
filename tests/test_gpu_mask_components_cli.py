"""`dips_raw series ... --boxes FILE [--connectivity 4|8] [--min-area A]
[--max-boxes K] [--roi x,y,w,h]`: the CSV holds one row per stored record and
a `# frame,count` line per frame, equal to the Python call (and to the
reference applied to the Python mask); the summary line carries the region,
the frames, the arguments, the components and the records."""
import os
import subprocess

import numpy as np
import pytest

import _components_ref as cref
from test_gpu_mask_components import _moving_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _parse(path):
    counts, rows = {}, []
    lines = path.read_text().splitlines()
    assert lines[0] == "frame,k,x0,y0,x1,y1,area,anchor,cx256,cy256"
    for line in lines[1:]:
        if line.startswith("# "):
            t, c = line[2:].split(",")
            counts[int(t)] = int(c)
        else:
            rows.append([int(v) for v in line.split(",")])
    return counts, rows


@pytest.mark.parametrize("roi,opts", [(None, []), ((5, 2, 81, 55), ["--connectivity", 4, "--min-area", 3, "--max-boxes", 2])])
def test_boxes_file_and_summary(tmp_path, roi, opts):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    w, h, n = 96, 64, 6
    frames = _moving_clip(3, w, h, n)
    src, dst = tmp_path / "in.raw", tmp_path / "boxes.csv"
    frames.tofile(src)
    args = ["series", src, w, h, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--boxes", dst] + opts
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    conn, area, k = (4, 3, 2) if opts else (8, 1, 64)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    try:
        mask = op.change_mask(frames, roi=roi)
        py = op.mask_components(mask, conn, area, k)
    finally:
        op.close()
    ref_counts, ref_boxes, _ = cref.components(mask.bits, mask.width, conn, area, k, labels=False)
    assert np.array_equal(py.counts, ref_counts) and np.array_equal(py.boxes, ref_boxes)
    counts, rows = _parse(dst)
    assert [counts[t] for t in range(n)] == py.counts.tolist() and py.counts.any()
    if opts:
        assert py.truncated.any()
    want_rows = [[t, i] + rec.tolist() for t in range(n) for i, rec in enumerate(py.frame(t))]
    assert rows == want_rows
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    assert r.stdout.strip().splitlines() == [
        f"boxes roi={rx},{ry},{rw},{rh} frames={n} connectivity={conn} min_area={area} max_boxes={k} "
        f"components={int(py.counts.sum())} records={len(want_rows)}"]


def test_usage_and_library_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    o = tmp_path / "o"
    r = _run(["series", src, 40, 30, "rgb8", "--connectivity", 4])  # belongs to --boxes
    assert r.returncode == 1 and "usage" in r.stderr and "--boxes FILE" in r.stderr
    assert _run(["series", src, 40, 30, "rgb8", "--boxes", o, "--connectivity", 6]).returncode == 1
    assert _run(["series", src, 40, 30, "rgb8", "--mask", tmp_path / "p", "--boxes", o]).returncode == 1
    assert _run(["series", src, 40, 30, "rgb8", "--grid", "2x2", "--boxes", o]).returncode == 1
    r = _run(["series", src, 40, 30, "rgb8", "--boxes", o, "--roi", "38,0,8,8"])
    assert r.returncode == 2 and "leaves the frame" in r.stderr
    assert not o.exists()
    r = _run(["series", src, 40, 30, "rgb8", "--boxes", o, "--roi", "3,0,8,8", "--max-boxes", 0])
    assert r.returncode == 0
    assert r.stdout.strip() == "boxes roi=3,0,8,8 frames=1 connectivity=8 min_area=1 max_boxes=0 components=0 records=0"
    assert o.read_text().splitlines() == ["frame,k,x0,y0,x1,y1,area,anchor,cx256,cy256", "# 0,0"]
