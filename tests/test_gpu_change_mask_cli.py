"""`dips_raw series ... --mask FILE [--roi x,y,w,h]`: the file holds the frames
x roi_h x row_bytes mask bytes the Python call gives (and the oracle's pixel
crops), the summary line the region, the frames, the row bytes and the
popcount; --roi is legal with --mask alone."""
import os
import subprocess

import numpy as np
import pytest

from test_change_mask_cpu import check_share, noise_frames, oracle_change_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("roi", [None, (5, 2, 33, 27)])
@pytest.mark.parametrize("mode", ["overall", "per-frame"])
def test_mask_file_and_summary(tmp_path, mode, roi):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    w, h, n = 40, 30, 7
    frames = noise_frames(3, w, h, n)
    src, dst = tmp_path / "in.raw", tmp_path / "mask.bin"
    frames.tofile(src)
    args = ["series", src, w, h, "rgb8", "--mode", mode, "--tau", 8 / 255, "--mask", dst]
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]  # --roi with --mask alone
    r = _run(args)
    assert r.returncode == 0, r.stderr
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    row_bytes = 4 * ((rw + 31) // 32)
    got = np.fromfile(dst, dtype=np.uint8).reshape(n, rh, row_bytes)
    m = 0 if mode == "overall" else 1
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode(m), 8 / 255)
    try:
        py = op.change_mask(frames, roi=roi)
    finally:
        op.close()
    want = oracle_change_mask(frames, m, 8 / 255, roi=roi)
    check_share(want, rw, 8, first=1)
    assert np.array_equal(got, py.bits)
    assert np.array_equal(got, want)
    assert r.stdout.strip().splitlines() == [
        f"mask roi={rx},{ry},{rw},{rh} frames={n} row_bytes={row_bytes} set={int(py.counts().sum())}"]


def test_usage_and_library_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    r = _run(["series", src, 40, 30, "rgb8", "--roi", "0,0,8,8"])
    assert r.returncode == 1 and "usage" in r.stderr and "--mask FILE" in r.stderr
    assert _run(["series", src, 40, 30, "rgb8", "--grid", "2x2", "--mask", tmp_path / "o"]).returncode == 1
    assert _run(["series", src, 40, 30, "rgb8", "--pixel-sums", tmp_path / "p", "--mask", tmp_path / "o"]).returncode == 1
    r = _run(["series", src, 40, 30, "rgb8", "--mask", tmp_path / "o", "--roi", "38,0,8,8"])
    assert r.returncode == 2 and "diff_change_mask: " in r.stderr and "leaves the frame" in r.stderr
    assert not (tmp_path / "o").exists()
    r = _run(["series", src, 40, 30, "rgb8", "--mask", tmp_path / "o", "--roi", "3,0,8,8"])
    assert r.returncode == 0 and r.stdout.strip() == "mask roi=3,0,8,8 frames=1 row_bytes=4 set=0"
    assert (tmp_path / "o").read_bytes() == bytes(8 * 4)
