"""`dips_raw series ... --tracks FILE`: --boxes' file with the four link words
behind every record, equal to the Python path (change_tracks) and to the
specification applied to the Python mask; with --roi, --morph and
--background; and its usage errors."""
import os
import subprocess

import numpy as np
import pytest

import _tracks_ref as tref
from test_gpu_mask_morph import _moving_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _parse(path):
    counts, rows = {}, []
    lines = path.read_text().splitlines()
    assert lines[0] == "frame,k,x0,y0,x1,y1,area,anchor,cx256,cy256,prev,overlap,track,age"
    for line in lines[1:]:
        if line.startswith("# "):
            t, c = line[2:].split(",")
            counts[int(t)] = int(c)
        else:
            rows.append([int(v) for v in line.split(",")])
    return counts, rows


@pytest.mark.parametrize("roi,opts,kw", [
    (None, [], {}),
    ((5, 2, 81, 55), ["--connectivity", 4, "--min-area", 3, "--max-boxes", 2],
     {"connectivity": 4, "min_area": 3, "max_boxes": 2}),
    (None, ["--morph", "close:box:1x1", "--max-boxes", 16], {"max_boxes": 16, "morph": "close"}),
    (None, ["--background", "2,selective"], {"background": (2, True)}),
])
def test_tracks_file_and_summary(tmp_path, roi, opts, kw):
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, MorphShape, PixelFormat
    w, h, n = 96, 64, 6
    frames = _moving_clip(3, w, h, n)
    src, dst = tmp_path / "in.raw", tmp_path / "tracks.csv"
    frames.tofile(src)
    args = ["series", src, w, h, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--tracks", dst] + opts
    if roi is not None:
        args += ["--roi", ",".join(str(v) for v in roi)]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    kw = dict(kw)
    tail = ""
    if kw.get("morph"):
        kw["morph"] = [(MorphOp.Close, MorphShape.Box, 1, 1)]
        tail = " morph=1"
    if kw.get("background"):
        tail = " background=2,selective"
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    try:
        py = op.change_tracks(frames, roi=roi, **kw)
        if "background" in kw:
            mask = op.background_mask(frames, roi=roi, rate_shift=2, selective=True)[0]
        else:
            mask = op.change_mask(frames, roi=roi)
        if "morph" in kw:
            mask = op.mask_morph(mask, MorphOp.Close, 1)
    finally:
        op.close()
    K = kw.get("max_boxes", 64)
    ref = tref.tracks(mask.bits, mask.width, kw.get("connectivity", 8), kw.get("min_area", 1), K,
                      state=np.zeros(1 + 2 * K, dtype=np.uint32))
    for g, want in zip(py.as_arrays(), ref):
        assert np.array_equal(g, want)
    assert (py.links[..., tref.AGE] > 0).any(), "the clip must hold a track of more than one frame"
    counts, rows = _parse(dst)
    assert [counts[t] for t in range(n)] == py.counts.tolist()
    want_rows = [[t, i] + b.tolist() + l.tolist() for t in range(n) for i, (b, l) in enumerate(zip(*py.frame(t)))]
    assert rows == want_rows
    x, y, rw, rh = roi if roi is not None else (0, 0, w, h)
    assert r.stdout.strip().splitlines() == [
        f"tracks roi={x},{y},{rw},{rh} frames={n} connectivity={kw.get('connectivity', 8)} "
        f"min_area={kw.get('min_area', 1)} max_boxes={K} components={int(py.counts.sum())} "
        f"records={len(want_rows)} tracks={int(py.state[0])}" + tail]


def test_usage_and_library_errors(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(40 * 30 * 3 * 2))
    o, o2 = tmp_path / "o", tmp_path / "o2"
    base = ["series", src, 40, 30, "rgb8"]
    r = _run(base + ["--tracks", o, "--boxes", o2])  # one product per run
    assert r.returncode == 1 and "usage" in r.stderr and "--tracks" in r.stderr
    assert _run(base + ["--tracks", o, "--connectivity", 6]).returncode == 1
    assert _run(base + ["--tracks"]).returncode == 1
    for k in (0, 257):  # the library refuses, nothing is written
        r = _run(base + ["--tracks", o, "--max-boxes", k])
        assert r.returncode != 0 and "dips_mask_tracks" in r.stderr, k
    assert not o.exists() and not o2.exists()
    r = _run(base + ["--tracks", o, "--max-boxes", 256])
    assert r.returncode == 0 and r.stdout.strip() == (
        "tracks roi=0,0,40,30 frames=2 connectivity=8 min_area=1 max_boxes=256 components=0 records=0 tracks=0")
    assert o.read_text().splitlines() == ["frame,k,x0,y0,x1,y1,area,anchor,cx256,cy256,prev,overlap,track,age",
                                          "# 0,0", "# 1,0"]
