"""`dips_raw series ... --vote K[,M]` with `--mask FILE` (the file holds the
voted mask) and with `--boxes FILE` (the components of the voted, then cleaned,
mask): equal to the reference applied to the plain `--mask` file; bad values
exit with status 2."""
import os
import subprocess

import numpy as np
import pytest

import _components_ref as cref
import _morph_ref as mref
import _vote_ref as vref
from test_gpu_mask_components_cli import _parse
from test_gpu_mask_vote import _flicker_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dips_amd", "bin", "dips_raw")
W, H, N = 96, 64, 9

pytestmark = pytest.mark.gpu


def _run(args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """(the clip's file, its plain --mask file as bytes [n, h, row_bytes])."""
    d = tmp_path_factory.mktemp("vote_cli")
    src, plain = d / "in.raw", d / "plain.bin"
    _flicker_clip(W, H, N).tofile(src)
    r = _run(["series", src, W, H, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--mask", plain])
    assert r.returncode == 0, r.stderr
    return src, np.fromfile(plain, dtype=np.uint8).reshape(N, H, cref.row_bytes(W))


@pytest.mark.parametrize("arg,k,m", [("3", 3, 2), ("5,5", 5, 5), ("31,1", 31, 1), ("1", 1, 1)])
def test_mask_file_holds_the_voted_mask(tmp_path, clip, arg, k, m):
    src, plain = clip
    dst = tmp_path / "mask.bin"
    r = _run(["series", src, W, H, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--mask", dst, "--vote", arg])
    assert r.returncode == 0, r.stderr
    want = vref.vote(plain, W, k, m)[0]
    assert plain.any() and (k == 1 or not np.array_equal(want, plain))
    assert np.array_equal(np.fromfile(dst, dtype=np.uint8).reshape(want.shape), want)
    assert r.stdout.strip().splitlines() == [
        f"mask roi=0,0,{W},{H} frames={N} row_bytes={want.shape[2]} set={int(cref.unpack(want, W).sum())} vote={k},{m}"]


def test_boxes_of_the_voted_then_opened_mask(tmp_path, clip):
    src, plain = clip
    dst = tmp_path / "boxes.csv"
    r = _run(["series", src, W, H, "rgb8", "--mode", "per-frame", "--tau", 8 / 255, "--boxes", dst, "--morph",
              "open:box:1x1", "--vote", "3,2", "--max-boxes", 16])  # the vote comes first wherever it stands
    assert r.returncode == 0, r.stderr
    cleaned = mref.morph(vref.vote(plain, W, 3, 2)[0], W, mref.OPEN, mref.BOX, 1, 1)
    ref_counts, ref_boxes, _ = cref.components(cleaned, W, 8, 1, 16, labels=False)
    assert ref_counts.any() and not np.array_equal(ref_counts, cref.components(plain, W, 8, 1, 16, labels=False)[0])
    counts, rows = _parse(dst)
    assert [counts[t] for t in range(N)] == ref_counts.tolist()
    want_rows = [[t, i] + ref_boxes[t, i].tolist() for t in range(N) for i in range(min(int(ref_counts[t]), 16))]
    assert rows == want_rows
    assert r.stdout.strip().splitlines() == [
        f"boxes roi=0,0,{W},{H} frames={N} connectivity=8 min_area=1 max_boxes=16 "
        f"components={int(ref_counts.sum())} records={len(want_rows)} vote=3,2 morph=1"]


def test_bad_values_exit_with_status_2(tmp_path, clip):
    src, _ = clip
    o = tmp_path / "o"
    for bad in ("0", "32", "3,0", "3,4", "1,2", "x", "3,", ",2", "3,2,1", "-3", "3.5"):
        r = _run(["series", src, W, H, "rgb8", "--mask", o, "--vote", bad])
        assert r.returncode == 2, (bad, r.returncode)
    assert not o.exists()
    # --vote belongs to --mask, --boxes or --tracks: a usage error like --morph's
    r = _run(["series", src, W, H, "rgb8", "--vote", "3"])
    assert r.returncode == 1 and "usage" in r.stderr and "--vote" in r.stderr
    r = _run(["series", src, W, H, "rgb8", "--tracks", o, "--vote", "3"])
    assert r.returncode == 0 and r.stdout.startswith("tracks ") and " vote=3,2" in r.stdout
