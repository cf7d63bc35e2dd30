"""`dips_raw series ... --mask FILE --background K[,selective]
[--background-out FILE]`: the mask file and the state file (raw u16 planes)
equal the Python call's and the definition (tests/_background_ref.py); the
summary line ends with background=...; --boxes takes the components of that
mask; the options are legal with --mask or --boxes alone."""
import os
import subprocess

import numpy as np
import pytest

import _components_ref as cref
from _background_ref import background_fold, drift_clip
from test_change_mask_cpu import unpack_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("roi", [None, (5, 2, 30, 25)])
@pytest.mark.parametrize("spec,selective", [("3", False), ("3,selective", True)])
def test_mask_and_state_files(tmp_path, spec, selective, roi):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    w, h, n = 37, 29, 24
    frames = drift_clip(3, w, h, n)
    src, dst, bgf = tmp_path / "in.raw", tmp_path / "mask.bin", tmp_path / "bg.bin"
    frames.tofile(src)
    args = ["series", src, w, h, "rgb8", "--tau", 8 / 255, "--mask", dst, "--background", spec, "--background-out", bgf]
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    row_bytes = 4 * ((rw + 31) // 32)
    got = np.fromfile(dst, dtype=np.uint8).reshape(n, rh, row_bytes)
    state = np.fromfile(bgf, dtype="<u2").reshape(3, rh, rw)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.Overall, 8 / 255)
    try:
        m, b = op.background_mask(frames, roi=roi, rate_shift=3, selective=selective)
    finally:
        op.close()
    want = background_fold(frames, 3, selective, 8 / 255, 0, None, roi)
    assert 0.05 < unpack_mask(want[0], rw)[1:].mean() < 0.95
    assert np.array_equal(got, m.bits) and np.array_equal(state, b.state)
    assert np.array_equal(got, want[0]) and np.array_equal(state, want[1])
    assert r.stdout.strip().splitlines() == [
        f"mask roi={rx},{ry},{rw},{rh} frames={n} row_bytes={row_bytes} set={int(m.counts().sum())} background={spec}"]


def test_boxes_take_the_background_mask(tmp_path):
    w, h, n = 37, 29, 24
    frames = drift_clip(3, w, h, n)
    src, dst = tmp_path / "in.raw", tmp_path / "boxes.csv"
    frames.tofile(src)
    r = _run(["series", src, w, h, "rgb8", "--tau", 8 / 255, "--boxes", dst, "--min-area", 4, "--background", "2"])
    assert r.returncode == 0, r.stderr
    counts, boxes, _ = cref.components(background_fold(frames, 2, False, 8 / 255)[0], w, 8, 4, 64)
    assert counts.any()
    rows = [line for line in open(dst).read().splitlines()[1:] if not line.startswith("#")]
    assert len(rows) == int(np.minimum(counts, 64).sum())
    t, k = (int(v) for v in rows[-1].split(",")[:2])
    assert [int(v) for v in rows[-1].split(",")[2:]] == boxes[t, k].tolist()
    assert r.stdout.strip().endswith(f"components={int(counts.sum())} records={len(rows)} background=2")


def test_usage_and_library_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    o = tmp_path / "o"
    for extra in (["--background", "3"], ["--mask", o, "--background-out", o], ["--mask", o, "--background", "9"],
                  ["--mask", o, "--background", "3,eager"], ["--mask", o, "--background", "x"],
                  ["--pixel-times", o, "--background", "3"]):
        r = _run(["series", src, 40, 30, "rgb8"] + extra)
        assert r.returncode == 1 and "--background K[,selective]" in r.stderr, extra
    r = _run(["series", src, 40, 30, "rgb8", "--mask", o, "--background", "3", "--roi", "38,0,8,8"])
    assert r.returncode == 2 and "diff_background_mask: " in r.stderr and "leaves the frame" in r.stderr
    assert not o.exists()
    r = _run(["series", src, 40, 30, "rgb8", "--mask", o, "--background", "0", "--background-out", tmp_path / "b",
              "--roi", "3,0,8,8"])
    assert r.returncode == 0 and r.stdout.strip() == "mask roi=3,0,8,8 frames=1 row_bytes=4 set=0 background=0"
    assert o.read_bytes() == bytes(8 * 4) and (tmp_path / "b").read_bytes() == bytes(3 * 8 * 8 * 2)
