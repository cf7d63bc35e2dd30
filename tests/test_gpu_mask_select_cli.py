"""`dips_raw series ... --select ITEMS`, `--hysteresis TAU_HIGH` and
`--fill-holes [MAX]` with `--mask FILE` (the file holds the selected mask) and
with `--boxes FILE` (the components of the selected mask): equal to the Python
path and to the specification applied to the Python mask."""
import os
import subprocess

import numpy as np
import pytest

import _components_ref as cref
import _select_ref as sref
from test_gpu_mask_components_cli import _parse
from test_gpu_mask_select import _flash_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu

W, H, N = 96, 64, 5
TAU, TAU_HIGH = 12 / 255, 100 / 255


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    frames = _flash_clip(W, H, N)
    src = tmp_path_factory.mktemp("select_cli") / "in.raw"
    frames.tofile(src)
    return frames, src


@pytest.fixture(scope="module")
def op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, TAU)
    yield o
    o.close()


@pytest.mark.parametrize("roi", [None, (3, 2, 90, 60)])
def test_mask_file_holds_the_selected_mask(tmp_path, clip, op, roi):
    frames, src = clip
    dst = tmp_path / "mask.bin"
    base = ["series", src, W, H, "rgb8", "--mode", "per-frame", "--tau", TAU, "--mask", dst]
    if roi is not None:
        base += ["--roi", ",".join(str(v) for v in roi)]
    mask = op.change_mask(frames, roi=roi)
    x, y, rw, rh = roi if roi is not None else (0, 0, W, H)

    def expect(args, want, tail):
        r = _run(base + args)
        assert r.returncode == 0, r.stderr
        assert want.any() and not np.array_equal(want, mask.bits)
        assert np.array_equal(np.fromfile(dst, dtype=np.uint8).reshape(want.shape), want), args
        assert r.stdout.strip().splitlines() == [
            f"mask roi={x},{y},{rw},{rh} frames={N} row_bytes={want.shape[2]} set={int(cref.unpack(want, rw).sum())} "
            + tail], r.stdout

    # an area opening under 4-connectivity, border cleared
    want, _ = sref.select_bytes(mask.bits, rw, connectivity=4, min_area=4, clear_border=True)
    py, _ = op.mask_select(mask, connectivity=4, min_area=4, clear_border=True)
    assert np.array_equal(py.bits, want)
    expect(["--select", "min-area=4,clear-border,connectivity=4"], want, "select=4,0,1,4")
    # what it dropped
    want, _ = sref.select_bytes(mask.bits, rw, min_area=2, max_area=200, dropped=True)
    expect(["--select", "min-area=2,max-area=200,dropped"], want, "select=2,200,2,8")
    # hysteresis: the components of the mask at --tau that hold a pixel of the mask at TAU_HIGH
    py = op.hysteresis_mask(frames, TAU_HIGH, roi=roi)
    expect(["--hysteresis", TAU_HIGH], py.bits, f"hysteresis={float(np.float32(TAU_HIGH)):g}")
    # the holes, all of them and none of more than 0 < MAX pixels
    py = op.mask_fill_holes(mask)
    assert np.array_equal(py.bits, sref.fill_holes_bytes(mask.bits, rw))
    expect(["--fill-holes"], py.bits, "fill_holes=0")
    expect(["--fill-holes", 1], py.bits, "fill_holes=1")  # the one hole is one pixel
    # select, then fill-holes, behind a morph step
    from dips_amd import MorphOp
    opened = op.mask_morph(mask, MorphOp.Open, 1)
    kept, _ = op.mask_select(opened, min_area=100)
    py = op.mask_fill_holes(kept)
    expect(["--fill-holes", "--select", "min-area=100", "--morph", "open:box:1x1"], py.bits,
           "morph=1 select=100,0,0,8 fill_holes=0")


def test_boxes_of_the_selected_mask(tmp_path, clip, op):
    frames, src = clip
    dst = tmp_path / "boxes.csv"
    r = _run(["series", src, W, H, "rgb8", "--mode", "per-frame", "--tau", TAU, "--boxes", dst, "--max-boxes", 16,
              "--select", "min-area=4,clear-border", "--fill-holes"])
    assert r.returncode == 0, r.stderr
    py = op.change_boxes(frames, max_boxes=16, select={"min_area": 4, "clear_border": True, "fill_holes": True})
    plain = op.change_boxes(frames, max_boxes=16)
    assert py.counts.any() and not np.array_equal(py.counts, plain.counts)
    counts, rows = _parse(dst)
    assert [counts[t] for t in range(N)] == py.counts.tolist()
    want_rows = [[t, i] + rec.tolist() for t in range(N) for i, rec in enumerate(py.frame(t))]
    assert rows == want_rows
    assert r.stdout.strip().splitlines() == [
        f"boxes roi=0,0,{W},{H} frames={N} connectivity=8 min_area=1 max_boxes=16 "
        f"components={int(py.counts.sum())} records={len(want_rows)} select=4,0,1,8 fill_holes=0"]


def test_usage_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    o = tmp_path / "o"
    for opt in (["--select", "min-area=2"], ["--hysteresis", "0.5"], ["--fill-holes"]):
        r = _run(["series", src, 40, 30, "rgb8"] + opt)  # belongs to what takes a mask
        assert r.returncode == 1 and "usage" in r.stderr and "--select" in r.stderr
    for bad in ("", "min-area", "min-area=x", "area=3", "connectivity=6", "min-area=5,max-area=4", "clear-border,",
                "dropped=1"):
        assert _run(["series", src, 40, 30, "rgb8", "--mask", o, "--select", bad]).returncode == 1, bad
    assert _run(["series", src, 40, 30, "rgb8", "--mask", o, "--hysteresis", "x"]).returncode == 1
    assert _run(["series", src, 40, 30, "rgb8", "--tau", 0.5, "--mask", o, "--hysteresis", 0.25]).returncode == 1
    for model in (["--background", 3], ["--sigma-delta", 2]):
        assert _run(["series", src, 40, 30, "rgb8", "--mask", o, "--hysteresis", 0.5] + model).returncode == 1
        assert _run(["series", src, 40, 30, "rgb8", "--mask", o, "--fill-holes"] + model).returncode == 1
    assert not o.exists()
    r = _run(["series", src, 40, 30, "rgb8", "--mask", o, "--select", "max-area=0", "--fill-holes", 7, "--hysteresis", 0.5])
    assert r.returncode == 0 and r.stdout.strip() == (
        "mask roi=0,0,40,30 frames=1 row_bytes=8 set=0 select=1,0,0,8 hysteresis=0.5 fill_holes=7")
    # --select alone goes with a background model
    r = _run(["series", src, 40, 30, "rgb8", "--mask", o, "--select", "min-area=2", "--background", 3])
    assert r.returncode == 0 and r.stdout.strip().endswith("select=2,0,0,8 background=3")
