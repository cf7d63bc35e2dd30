"""`dips_raw series ... --pixel-times FILE [--roi x,y,w,h]`: the file holds the
four planes first, last, run_max, run_cur of roi_h x roi_w little-endian u32
the Python call gives (and the fold of the oracle's pixel crops), the summary
line the region, the frames, the pixels that never changed, the smallest
first, the largest last and the largest run_max; --roi is legal with
--pixel-times alone."""
import os
import subprocess

import numpy as np
import pytest

from test_pixel_times_cpu import NONE, check_informative, event_frames, oracle_pixel_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("roi", [None, (5, 2, 30, 25)])
@pytest.mark.parametrize("mode", ["overall", "per-frame"])
def test_times_file_and_summary(tmp_path, mode, roi):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    w, h, n = 37, 29, 9
    frames = event_frames(3, w, h, n)
    src, dst = tmp_path / "in.raw", tmp_path / "times.bin"
    frames.tofile(src)
    args = ["series", src, w, h, "rgb8", "--mode", mode, "--tau", 8 / 255, "--pixel-times", dst]
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]  # --roi with --pixel-times alone
    r = _run(args)
    assert r.returncode == 0, r.stderr
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    got = np.fromfile(dst, dtype="<u4").reshape(4, rh, rw)
    m = 0 if mode == "overall" else 1
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode(m), 8 / 255)
    try:
        py = op.pixel_times(frames, roi=roi)
    finally:
        op.close()
    want = oracle_pixel_times(frames, m, 8 / 255, roi=roi)
    check_informative(want, n)
    assert np.array_equal(got, py.as_array())
    assert np.array_equal(got, want)
    changed = py.first != NONE
    assert r.stdout.strip().splitlines() == [
        f"pixel-times roi={rx},{ry},{rw},{rh} frames={n} never={int((~changed).sum())} "
        f"min_first={int(py.first[changed].min())} max_last={int(py.last[changed].max())} "
        f"max_run={int(py.run_max.max())}"]


def test_usage_and_library_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    r = _run(["series", src, 40, 30, "rgb8", "--roi", "0,0,8,8"])
    assert r.returncode == 1 and "usage" in r.stderr and "--pixel-times FILE" in r.stderr
    assert _run(["series", src, 40, 30, "rgb8", "--grid", "2x2", "--pixel-times", tmp_path / "o"]).returncode == 1
    assert _run(["series", src, 40, 30, "rgb8", "--mask", tmp_path / "p", "--pixel-times", tmp_path / "o"]).returncode == 1
    r = _run(["series", src, 40, 30, "rgb8", "--pixel-times", tmp_path / "o", "--roi", "38,0,8,8"])
    assert r.returncode == 2 and "diff_pixel_times: " in r.stderr and "leaves the frame" in r.stderr
    assert not (tmp_path / "o").exists()
    r = _run(["series", src, 40, 30, "rgb8", "--pixel-times", tmp_path / "o", "--roi", "3,0,8,8"])
    assert r.returncode == 0
    assert r.stdout.strip() == "pixel-times roi=3,0,8,8 frames=1 never=64 min_first=-1 max_last=-1 max_run=0"
    blob = np.frombuffer((tmp_path / "o").read_bytes(), dtype="<u4").reshape(4, 8, 8)
    assert (blob[:2] == NONE).all() and (blob[2:] == 0).all()
