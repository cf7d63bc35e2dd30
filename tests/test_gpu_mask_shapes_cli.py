"""`dips_raw series ... --boxes FILE | --tracks FILE --shapes [--shape-weights
FILE.raw]`: the ten shape columns behind every record equal the Python call's
on the same mask, with and without weights, and the summary line ends with
shapes=1."""
import os
import subprocess

import numpy as np
import pytest

import _shapes_ref as sref
from test_gpu_mask_components import _moving_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu

W, H, N = 96, 64, 5
BOX_HEADER = "frame,k,x0,y0,x1,y1,area,anchor,cx256,cy256"
SHAPE_HEADER = "," + ",".join(sref.COLUMNS)


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _parse(path, header):
    counts, rows = {}, []
    lines = path.read_text().splitlines()
    assert lines[0] == header
    for line in lines[1:]:
        if line.startswith("# "):
            t, c = line[2:].split(",")
            counts[int(t)] = int(c)
        else:
            rows.append([int(v) for v in line.split(",")])
    return counts, rows


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    frames = _moving_clip(3, W, H, N)
    src = tmp_path_factory.mktemp("shapes_cli") / "in.raw"
    frames.tofile(src)
    return frames, src


@pytest.fixture(scope="module")
def op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    yield o
    o.close()


@pytest.mark.parametrize("roi", [None, (5, 2, 81, 55)])
@pytest.mark.parametrize("weighted", [False, True])
def test_boxes_file_with_shape_columns(tmp_path, clip, op, roi, weighted):
    frames, src = clip
    dst = tmp_path / "boxes.csv"
    mask = op.change_mask(frames, roi=roi)
    rx, ry, rw, rh = roi if roi is not None else (0, 0, W, H)
    args = ["series", src, W, H, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--boxes", dst, "--shapes",
            "--connectivity", 4, "--min-area", 2, "--max-boxes", 6]
    weights = None
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]
    if weighted:
        weights = np.random.default_rng(3).integers(0, 256, (N, rh, rw), dtype=np.uint8)
        weights.tofile(tmp_path / "weights.raw")
        args += ["--shape-weights", tmp_path / "weights.raw"]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    py = op.mask_shapes(mask, weights, 4, 2, 6)
    plain = op.mask_components(mask, 4, 2, 6)
    assert np.array_equal(py.boxes, plain.boxes) and py.counts.any()
    counts, rows = _parse(dst, BOX_HEADER + SHAPE_HEADER)
    assert [counts[t] for t in range(N)] == py.counts.tolist()
    want_rows = [[t, k] + b.tolist() + sref.csv_columns(s) for t in range(N) for k, (b, s) in enumerate(zip(*py.frame(t)))]
    assert rows == want_rows
    assert any(row[-5] != 0 for row in rows) == weighted  # wsum
    assert r.stdout.strip().splitlines() == [
        f"boxes roi={rx},{ry},{rw},{rh} frames={N} connectivity=4 min_area=2 max_boxes=6 "
        f"components={int(py.counts.sum())} records={len(want_rows)} shapes=1"]


def test_tracks_file_with_shape_columns(tmp_path, clip, op):
    frames, src = clip
    dst = tmp_path / "tracks.csv"
    r = _run(["series", src, W, H, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--tracks", dst, "--shapes",
              "--max-boxes", 8])
    assert r.returncode == 0, r.stderr
    mask = op.change_mask(frames)
    tracks = op.mask_tracks(mask, max_boxes=8)
    py = op.mask_shapes(mask, max_boxes=8)
    counts, rows = _parse(dst, BOX_HEADER + ",prev,overlap,track,age" + SHAPE_HEADER)
    assert [counts[t] for t in range(N)] == py.counts.tolist()
    want_rows = []
    for t in range(N):
        boxes, links = tracks.frame(t)
        for k, (b, l, s) in enumerate(zip(boxes, links, py.frame(t)[1])):
            want_rows.append([t, k] + b.tolist() + l.tolist() + sref.csv_columns(s))
    assert rows == want_rows and rows
    assert r.stdout.strip().startswith("tracks roi=0,0,") and r.stdout.strip().endswith(" shapes=1")


def test_usage_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    o = tmp_path / "o"
    r = _run(["series", src, 40, 30, "rgb8", "--shapes"])  # belongs to --boxes or --tracks
    assert r.returncode == 1 and "usage" in r.stderr and "--shapes" in r.stderr
    assert _run(["series", src, 40, 30, "rgb8", "--mask", o, "--shapes"]).returncode == 1
    assert _run(["series", src, 40, 30, "rgb8", "--boxes", o, "--shape-weights", src]).returncode == 1
    r = _run(["series", src, 40, 30, "rgb8", "--boxes", o, "--shapes", "--shape-weights", src])  # 3600 bytes, not 1200
    assert r.returncode == 1 and "planes" in r.stderr
    assert not o.exists()
    r = _run(["series", src, 40, 30, "rgb8", "--boxes", o, "--shapes", "--max-boxes", 0])
    assert r.returncode == 0 and r.stdout.strip().endswith("records=0 shapes=1")
    assert o.read_text().splitlines() == [BOX_HEADER + SHAPE_HEADER, "# 0,0"]
