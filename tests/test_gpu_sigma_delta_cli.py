"""`dips_raw series ... --mask FILE --sigma-delta N[,VMIN[,VMAX]]
[--sigma-delta-out FILE]`: the mask file and the state file (raw u16 planes M
and V) equal the Python call's and the definition
(tests/_sigma_delta_ref.py); the summary line ends with sigma_delta=...;
--boxes takes the components of that mask; the options are legal with --mask,
--boxes or --tracks alone and not with --background."""
import os
import subprocess

import numpy as np
import pytest

import _components_ref as cref
from _background_ref import drift_clip
from _sigma_delta_ref import sigma_delta_fold
from test_change_mask_cpu import unpack_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("roi", [None, (5, 2, 30, 25)])
@pytest.mark.parametrize("spec,params", [("2", (2, 2, 510)), ("4,1", (4, 1, 510)), ("4,1,6", (4, 1, 6))])
def test_mask_and_state_files(tmp_path, spec, params, roi):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    w, h, n = 37, 29, 24
    frames = drift_clip(3, w, h, n)
    src, dst, sdf = tmp_path / "in.raw", tmp_path / "mask.bin", tmp_path / "sd.bin"
    frames.tofile(src)
    args = ["series", src, w, h, "rgb8", "--mask", dst, "--sigma-delta", spec, "--sigma-delta-out", sdf]
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    row_bytes = 4 * ((rw + 31) // 32)
    got = np.fromfile(dst, dtype=np.uint8).reshape(n, rh, row_bytes)
    state = np.fromfile(sdf, dtype="<u2").reshape(2, rh, rw)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.Overall, 8 / 255)
    try:
        m, s = op.sigma_delta_mask(frames, roi=roi, n_amp=params[0], v_min=params[1], v_max=params[2])
    finally:
        op.close()
    want = sigma_delta_fold(frames, *params, 0, None, roi)
    assert 0.05 < unpack_mask(want[0], rw)[1:].mean() < 0.95
    assert np.array_equal(got, m.bits) and np.array_equal(state, s.state)
    assert np.array_equal(got, want[0]) and np.array_equal(state, want[1])
    assert r.stdout.strip().splitlines() == [
        f"mask roi={rx},{ry},{rw},{rh} frames={n} row_bytes={row_bytes} set={int(m.counts().sum())} "
        f"sigma_delta={params[0]},{params[1]},{params[2]}"]


def test_boxes_take_the_sigma_delta_mask(tmp_path):
    w, h, n = 37, 29, 24
    frames = drift_clip(3, w, h, n)
    src, dst = tmp_path / "in.raw", tmp_path / "boxes.csv"
    frames.tofile(src)
    r = _run(["series", src, w, h, "rgb8", "--boxes", dst, "--min-area", 4, "--sigma-delta", "4,1,6"])
    assert r.returncode == 0, r.stderr
    counts, boxes, _ = cref.components(sigma_delta_fold(frames, 4, 1, 6)[0], w, 8, 4, 64)
    assert counts.any()
    rows = [line for line in open(dst).read().splitlines()[1:] if not line.startswith("#")]
    assert len(rows) == int(np.minimum(counts, 64).sum())
    t, k = (int(v) for v in rows[-1].split(",")[:2])
    assert [int(v) for v in rows[-1].split(",")[2:]] == boxes[t, k].tolist()
    assert r.stdout.strip().endswith(f"components={int(counts.sum())} records={len(rows)} sigma_delta=4,1,6")


def test_usage_and_library_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3))
    o = tmp_path / "o"
    for extra in (["--sigma-delta", "2"], ["--mask", o, "--sigma-delta-out", o], ["--mask", o, "--sigma-delta", "0"],
                  ["--mask", o, "--sigma-delta", "16"], ["--mask", o, "--sigma-delta", "2,5,4"],
                  ["--mask", o, "--sigma-delta", "2,2,511"], ["--mask", o, "--sigma-delta", "2,2,510,1"],
                  ["--mask", o, "--sigma-delta", "2,"], ["--mask", o, "--sigma-delta", "x"],
                  ["--mask", o, "--sigma-delta", "2", "--background", "3"], ["--pixel-times", o, "--sigma-delta", "2"]):
        r = _run(["series", src, 40, 30, "rgb8"] + extra)
        assert r.returncode == 1 and "--sigma-delta N[,VMIN[,VMAX]]" in r.stderr, extra
    r = _run(["series", src, 40, 30, "rgb8", "--mask", o, "--sigma-delta", "2", "--roi", "38,0,8,8"])
    assert r.returncode == 2 and "diff_sigma_delta_mask: " in r.stderr and "leaves the frame" in r.stderr
    assert not o.exists()
    r = _run(["series", src, 40, 30, "rgb8", "--mask", o, "--sigma-delta", "3,7,7", "--sigma-delta-out", tmp_path / "s",
              "--roi", "3,0,8,8"])
    assert r.returncode == 0 and r.stdout.strip() == "mask roi=3,0,8,8 frames=1 row_bytes=4 set=0 sigma_delta=3,7,7"
    assert o.read_bytes() == bytes(8 * 4)
    assert np.array_equal(np.frombuffer((tmp_path / "s").read_bytes(), dtype="<u2"), np.repeat([0, 7], 64))
