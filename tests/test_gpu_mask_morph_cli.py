"""`dips_raw series ... --morph OP:SHAPE:RXxRY` with `--mask FILE` (the file
holds the cleaned mask) and with `--boxes FILE` (the components of the cleaned
mask), the steps applied in the order given: equal to the Python path and to
the reference applied to the Python mask."""
import os
import subprocess

import numpy as np
import pytest

import _components_ref as cref
import _morph_ref as mref
from test_gpu_mask_components_cli import _parse
from test_gpu_mask_morph import _moving_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("roi", [None, (5, 2, 81, 55)])
def test_mask_file_holds_the_cleaned_mask(tmp_path, roi):
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, PixelFormat
    w, h, n = 96, 64, 6
    frames = _moving_clip(3, w, h, n)
    src, dst = tmp_path / "in.raw", tmp_path / "mask.bin"
    frames.tofile(src)
    args = ["series", src, w, h, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--mask", dst, "--morph",
            "open:box:1x1"]
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    try:
        mask = op.change_mask(frames, roi=roi)
        py = op.mask_morph(mask, MorphOp.Open, 1)
    finally:
        op.close()
    want = mref.morph(mask.bits, mask.width, mref.OPEN, mref.BOX, 1, 1)
    assert np.array_equal(py.bits, want) and want.any() and not np.array_equal(want, mask.bits)
    assert np.array_equal(np.fromfile(dst, dtype=np.uint8).reshape(want.shape), want)
    x, y, rw, rh = roi if roi is not None else (0, 0, w, h)
    assert r.stdout.strip().splitlines() == [
        f"mask roi={x},{y},{rw},{rh} frames={n} row_bytes={want.shape[2]} set={int(cref.unpack(want, rw).sum())} "
        "morph=1"]


def test_boxes_of_two_chained_steps(tmp_path):
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, MorphShape, PixelFormat
    w, h, n = 96, 64, 6
    frames = _moving_clip(3, w, h, n)
    src, dst = tmp_path / "in.raw", tmp_path / "boxes.csv"
    frames.tofile(src)
    r = _run(["series", src, w, h, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--boxes", dst, "--morph",
              "open:diamond:1x1", "--morph", "close:box:3x2", "--max-boxes", 16])
    assert r.returncode == 0, r.stderr
    steps = [(MorphOp.Open, MorphShape.Diamond, 1, 1), (MorphOp.Close, MorphShape.Box, 3, 2)]
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    try:
        mask = op.change_mask(frames)
        py = op.change_boxes(frames, max_boxes=16, morph=steps)
        plain = op.change_boxes(frames, max_boxes=16)
    finally:
        op.close()
    cleaned = mask.bits
    for mop, shape, rx, ry in steps:
        cleaned = mref.morph(cleaned, w, int(mop), int(shape), rx, ry)
    ref_counts, ref_boxes, _ = cref.components(cleaned, w, 8, 1, 16, labels=False)
    assert np.array_equal(py.counts, ref_counts) and np.array_equal(py.boxes, ref_boxes)
    assert py.counts.any() and not np.array_equal(py.counts, plain.counts)
    # the other order is another result: the steps are not commuted
    swapped = mref.morph(mref.morph(mask.bits, w, mref.CLOSE, mref.BOX, 3, 2), w, mref.OPEN, mref.DIAMOND, 1, 1)
    assert not np.array_equal(swapped, cleaned)
    counts, rows = _parse(dst)
    assert [counts[t] for t in range(n)] == py.counts.tolist()
    want_rows = [[t, i] + rec.tolist() for t in range(n) for i, rec in enumerate(py.frame(t))]
    assert rows == want_rows
    assert r.stdout.strip().splitlines() == [
        f"boxes roi=0,0,{w},{h} frames={n} connectivity=8 min_area=1 max_boxes=16 "
        f"components={int(py.counts.sum())} records={len(want_rows)} morph=2"]


def test_usage_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    o = tmp_path / "o"
    r = _run(["series", src, 40, 30, "rgb8", "--morph", "open:box:1x1"])  # belongs to --mask or --boxes
    assert r.returncode == 1 and "usage" in r.stderr and "--morph" in r.stderr
    assert _run(["series", src, 40, 30, "rgb8", "--grid", "2x2", "--morph", "open:box:1x1"]).returncode == 1
    for bad in ("open:box:1", "open:box:16x1", "open:box:1x16", "open:diamond:2x1", "shut:box:1x1", "open:disc:1x1",
                "open:box", "open", "open:box:x1", "open:box:-1x1"):
        assert _run(["series", src, 40, 30, "rgb8", "--mask", o, "--morph", bad]).returncode == 1, bad
    assert not o.exists()
    r = _run(["series", src, 40, 30, "rgb8", "--mask", o, "--morph", "dilate:box:0x15", "--morph", "erode:diamond:0x0"])
    assert r.returncode == 0 and r.stdout.strip() == "mask roi=0,0,40,30 frames=1 row_bytes=8 set=0 morph=2"
