"""`dips_raw series ... --pixel-sums FILE [--roi x,y,w,h]`: the file holds the
roi_h x roi_w x 4 little-endian u64 sums the Python call gives (and the
oracle's pixel crops), the summary line their totals; --roi still needs
--grid or --pixel-sums."""
import os
import subprocess

import numpy as np
import pytest

from test_pixel_sums_cpu import oracle_pixel_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("roi", [None, (5, 2, 33, 27)])
@pytest.mark.parametrize("mode", ["overall", "per-frame"])
def test_pixel_sums_file_and_summary(tmp_path, mode, roi):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    w, h, n = 40, 30, 7
    frames = np.random.default_rng(11).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    src, dst = tmp_path / "in.raw", tmp_path / "sums.u64"
    frames.tofile(src)
    args = ["series", src, w, h, "rgb8", "--mode", mode, "--tau", 8 / 255, "--pixel-sums", dst]
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    got = np.fromfile(dst, dtype="<u8").reshape(rh, rw, 4)
    m = 0 if mode == "overall" else 1
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode(m), 8 / 255)
    try:
        py = op.pixel_sums(frames, roi=roi).as_array()
    finally:
        op.close()
    assert np.array_equal(got, py)
    assert np.array_equal(got, oracle_pixel_sums(frames, m, 8 / 255, roi=roi))
    assert got[..., 2].min() < got[..., 2].max()  # the threshold selects some differences, not all
    tot = got.sum(axis=(0, 1), dtype=np.uint64)
    assert r.stdout.strip().splitlines() == [
        f"pixel-sums roi={rx},{ry},{rw},{rh} frames={n} sad={tot[0]} sj={tot[1]} count={tot[2]} si_fixed={tot[3]}"]


def test_roi_alone_and_grid_with_pixel_sums_are_usage_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    r = _run(["series", src, 40, 30, "rgb8", "--roi", "0,0,8,8"])
    assert r.returncode == 1 and "usage" in r.stderr and "--pixel-sums FILE" in r.stderr
    assert _run(["series", src, 40, 30, "rgb8", "--grid", "2x2", "--pixel-sums", tmp_path / "o"]).returncode == 1
    r = _run(["series", src, 40, 30, "rgb8", "--pixel-sums", tmp_path / "o", "--roi", "38,0,8,8"])
    assert r.returncode == 2 and "diff_pixel_sums: " in r.stderr and "leaves the frame" in r.stderr
    assert not (tmp_path / "o").exists()
