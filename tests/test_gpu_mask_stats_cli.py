"""`dips_raw series ... --mask-counts FILE [--mask-grid RxC] --mask-times FILE
--mask-sums FILE`: the statistics of the final mask, on their own and beside
`--mask`, `--boxes` and `--tracks`, behind `--sigma-delta`, `--vote`, `--morph`
and `--roi`, equal to the Python calls on the same mask; the flag errors."""
import os
import subprocess

import numpy as np
import pytest

import _components_ref as cref
import _mask_stats_ref as sref
from test_gpu_mask_stats import moving_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")
W, H, N = 96, 64, 10

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("stats_cli")
    src = d / "in.raw"
    frames = moving_clip(W, H, N, seed=2)
    frames.tofile(src)
    return src, frames


@pytest.fixture(scope="module")
def op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    yield o
    o.close()


def read_counts(path, n, rows, cols):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "t,row,col,count" and len(lines) == 1 + n * rows * cols
    out = np.zeros((n, rows, cols), dtype=np.uint32)
    for i, line in enumerate(lines[1:]):
        t, r, c, v = (int(x) for x in line.split(","))
        assert (t, r, c) == (i // (rows * cols), (i // cols) % rows, i % cols)
        out[t, r, c] = v
    return out


def check_files(op, mask, counts_file, times_file, sums_file, rows, cols):
    n, rh, rw = mask.bits.shape[0], mask.bits.shape[1], mask.width
    assert np.array_equal(read_counts(counts_file, n, rows, cols), op.mask_counts(mask, rows, cols))
    assert np.array_equal(np.fromfile(times_file, dtype="<u4").reshape(4, rh, rw), op.mask_times(mask).as_array())
    assert np.array_equal(np.fromfile(sums_file, dtype="<u4").reshape(rh, rw), op.mask_sums(mask))


def test_statistics_on_their_own_and_beside_the_mask(tmp_path, clip, op):
    src, frames = clip
    c, t, s, m = (tmp_path / x for x in ("c.csv", "t.bin", "s.bin", "m.bin"))
    base = ["series", src, W, H, "rgb8", "--mode", "per-frame", "--tau", 8 / 255]
    r = _run(base + ["--mask-counts", c, "--mask-grid", "3x4", "--mask-times", t, "--mask-sums", s])
    assert r.returncode == 0, r.stderr
    mask = op.change_mask(frames)
    assert mask.bits.any()
    check_files(op, mask, c, t, s, 3, 4)
    assert r.stdout.strip().splitlines() == [
        f"mask-stats roi=0,0,{W},{H} frames={N} row_bytes={mask.bits.shape[2]} set={int(mask.counts().sum())} "
        "mask_stats=counts:3x4,times,sums"]
    assert not m.exists()
    # beside --mask, with a region; the default grid is 1x1
    roi = (5, 3, 70, 50)
    r = _run(base + ["--mask", m, "--roi", ",".join(str(v) for v in roi), "--mask-counts", c, "--mask-sums", s,
                     "--mask-times", t])
    assert r.returncode == 0, r.stderr
    mask = op.change_mask(frames, roi=roi)
    assert np.array_equal(np.fromfile(m, dtype=np.uint8).reshape(mask.bits.shape), mask.bits)
    check_files(op, mask, c, t, s, 1, 1)
    assert np.array_equal(read_counts(c, N, 1, 1)[:, 0, 0], mask.counts())
    assert r.stdout.startswith("mask roi=5,3,70,50 ") and r.stdout.rstrip().endswith(" mask_stats=counts:1x1,times,sums")
    # one statistic alone
    s.unlink()
    t.unlink()
    r = _run(base + ["--mask-sums", s])
    assert r.returncode == 0 and r.stdout.rstrip().endswith(" mask_stats=sums") and not t.exists()
    assert np.array_equal(np.fromfile(s, dtype="<u4").reshape(H, W), sref.sums(op.change_mask(frames).bits, W))


def test_statistics_of_the_cleaned_mask_beside_boxes_and_tracks(tmp_path, clip):
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, PixelFormat
    src, frames = clip
    c, t, s, b = (tmp_path / x for x in ("c.csv", "t.bin", "s.bin", "b.csv"))
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.Overall, 8 / 255)
    try:
        raw, _ = o.sigma_delta_mask(frames)
        final = o.mask_morph(o.mask_vote(raw, 3)[0], MorphOp.Open, 1, 1)
        assert final.bits.any() and not np.array_equal(final.bits, raw.bits)
        for flag in ("--boxes", "--tracks"):
            r = _run(["series", src, W, H, "rgb8", "--tau", 8 / 255, flag, b, "--sigma-delta", "2", "--vote", "3",
                      "--morph", "open:box:1x1", "--mask-counts", c, "--mask-grid", "2x2", "--mask-times", t,
                      "--mask-sums", s])
            assert r.returncode == 0, r.stderr
            assert r.stdout.startswith(flag[2:] + " ") and r.stdout.rstrip().endswith(
                " vote=3,2 morph=1 sigma_delta=2,2,510 mask_stats=counts:2x2,times,sums")
            check_files(o, final, c, t, s, 2, 2)
            same = sref.unpack(final.bits, W)
            assert np.array_equal(read_counts(c, N, 2, 2), sref.counts_bits(same, 2, 2))
    finally:
        o.close()


def test_flag_errors(tmp_path, clip):
    src, _ = clip
    o = tmp_path / "o"
    base = ["series", src, W, H, "rgb8"]
    # --mask-grid belongs to --mask-counts; the statistics do not go with --grid, --pixel-sums or --pixel-times
    for bad in (["--mask-grid", "2x2"], ["--mask-sums", o, "--mask-grid", "2x2"], ["--mask-counts", o, "--mask-grid", "2"],
                ["--mask-counts", o, "--mask-grid", "0x2"], ["--mask-counts", o, "--grid", "2x2"],
                ["--mask-sums", o, "--pixel-sums", o], ["--mask-times", o, "--pixel-times", o], ["--mask-counts"]):
        r = _run(base + bad)
        assert r.returncode == 1 and "usage" in r.stderr and "--mask-counts" in r.stderr, bad
    assert not o.exists()
    # a grid finer than the region is the library's refusal
    r = _run(base + ["--mask-counts", o, "--mask-grid", f"{H + 1}x1"])
    assert r.returncode == 2 and "mask_counts:" in r.stderr and not o.exists()
    r = _run(base + ["--mask-counts", o, "--mask-grid", "2x2", "--roi", "0,0,1,1"])
    assert r.returncode == 2 and "mask_counts:" in r.stderr and not o.exists()
    # --vote and --morph go with the statistics alone
    r = _run(base + ["--mask-sums", o, "--vote", "3", "--morph", "open:box:1x1"])
    assert r.returncode == 0 and r.stdout.startswith("mask-stats ") and " vote=3,2 morph=1 mask_stats=sums" in r.stdout
