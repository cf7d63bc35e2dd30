"""CPU checks of the temporal vote (dips_mask_vote): the numpy specification
tests/_vote_ref.py against the definition's own triple loop and against the
identities the definition implies, chunked equals whole on the specification,
the Python argument checks, the exported name, and the schedule
(series_sched.h vote_geometry, compiled alone with g++) for the shapes
tests/test_gpu_mask_vote.py runs."""
import os

import numpy as np
import pytest

import _vote_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")

# (k, m) of the GPU test's window edges
WINDOWS = [(1, 1), (2, 1), (2, 2), (3, 2), (5, 3), (16, 8), (31, 1), (31, 16), (31, 31)]
# (w, h, n, k) of the GPU test's part-seam, many-words and chunk cases
GPU_SHAPES = [(40, 3, 300, 3), (40, 3, 600, 3), (40, 3, 600, 5), (40, 3, 600, 31), (3840, 2160, 2, 2),
              (3840, 2160, 8, 5), (65, 3, 300, 31), (65, 3, 300, 3), (200, 8, 80, 31), (1, 1, 1, 1)]
RESIDENTS = [256, 1024, 4096, 8192, 16384]


def bits_of(n, h, w, density, seed=0):
    return np.random.default_rng([83, seed, n, h, w]).random((n, h, w)) < density


@pytest.mark.parametrize("k,m", WINDOWS)
def test_reference_equals_the_definition(k, m):
    for n in sorted({1, max(k - 2, 0), k - 1, k, k + 1, 2 * k + 1}):
        x = bits_of(n, 2, 5, 0.5, seed=k * 32 + m)
        hist = bits_of(k - 1, 2, 5, 0.5, seed=1000 + k)
        for h_ in (None, hist):
            got, nxt = vref.vote_bits(x, k, m, h_)
            assert got.shape == x.shape and np.array_equal(got, vref.vote_naive(x, k, m, h_))
            seq = np.concatenate([np.zeros_like(hist) if h_ is None else hist, x])
            assert nxt.shape == hist.shape and np.array_equal(nxt, seq[seq.shape[0] - (k - 1):])


def test_identities_on_random_bits():
    for k in (1, 2, 3, 5, 16, 31):
        x = bits_of(2 * k + 3, 3, 37, 0.5, seed=k)
        hist = bits_of(k - 1, 3, 37, 0.5, seed=100 + k)
        seq = np.concatenate([hist, x])
        windows = np.stack([seq[t:t + k] for t in range(x.shape[0])])  # [n, k, h, w]
        outs = [vref.vote_bits(x, k, m, hist)[0] for m in range(1, k + 1)]
        assert np.array_equal(outs[0], windows.any(axis=1))    # m = 1: the OR of the window
        assert np.array_equal(outs[-1], windows.all(axis=1))   # m = k: the AND
        for lo, hi in zip(outs, outs[1:]):                     # monotone decreasing in m
            assert not (hi & ~lo).any()
        for m in range(1, k + 1):                              # duality, with the full history given
            assert np.array_equal(outs[m - 1], ~vref.vote_bits(~x, k, k - m + 1, ~hist)[0])
    x = bits_of(7, 3, 37, 0.5)
    out, nxt = vref.vote_bits(x, 1, 1)
    assert np.array_equal(out, x) and nxt.shape == (0, 3, 37)  # k = 1: the identity
    # NULL history and m = k: the first k - 1 frames are clear
    assert not vref.vote_bits(np.ones((6, 1, 3), dtype=bool), 4, 4)[0][:3].any()


@pytest.mark.parametrize("k,m", [(3, 2), (5, 5), (16, 8), (31, 1), (31, 16)])
def test_chunked_equals_whole_on_the_reference(k, m):
    x = bits_of(100, 2, 33, 0.5, seed=k)
    for hist in (None, bits_of(k - 1, 2, 33, 0.7, seed=k + 1)):
        whole, end = vref.vote_bits(x, k, m, hist)
        for chunk in sorted({1, max(k - 2, 1), max(k - 1, 1), k, 2 * k + 1}):
            got, got_end = vref.chunked(x, k, m, chunk, hist)
            assert np.array_equal(got, whole) and np.array_equal(got_end, end), chunk


def test_packed_form_ignores_and_clears_pad_bits():
    import _components_ref as cref
    x, hist = bits_of(6, 2, 33, 0.5), bits_of(2, 2, 33, 0.5, seed=1)
    clean = vref.vote(cref.pack(x), 33, 3, 2, cref.pack(hist))
    dirty = vref.vote(cref.pack(x, 1), 33, 3, 2, cref.pack(hist, 1))
    want = vref.vote_bits(x, 3, 2, hist)
    for c, d, w_ in zip(clean, dirty, want):
        assert np.array_equal(c, d) and np.array_equal(c, cref.pack(w_))


def test_vote_args_defaults_and_refusals():
    from dips_amd import VOTE_MAX_WINDOW, _lib
    from dips_amd.api import _vote_args, _vote_option
    assert VOTE_MAX_WINDOW == _lib.VOTE_MAX_WINDOW == vref.MAX_WINDOW == 31
    assert [_vote_args(k) for k in (1, 2, 3, 4, 5, 30, 31)] == [(1, 1), (2, 2), (3, 2), (4, 3), (5, 3), (30, 16), (31, 16)]
    assert _vote_args(5, 1) == (5, 1) and _vote_args(5, 5) == (5, 5) and _vote_args(31, 31) == (31, 31)
    assert _vote_option(3) == (3, 2) and _vote_option((5, 4)) == (5, 4) and _vote_option([2, 1]) == (2, 1)
    for bad in ((0, None), (32, None), (-1, None), (3, 0), (3, 4), (1, 2), (31, 32)):
        with pytest.raises(ValueError):
            _vote_args(*bad)
    for bad in ((3,), (3, 2, 1), (0, 1), 0, 32):
        with pytest.raises(ValueError):
            _vote_option(bad)


def test_python_surface():
    import inspect

    import dips_amd
    op = dips_amd.DiffSeriesOperator
    sig = inspect.signature(op.mask_vote)
    assert list(sig.parameters)[1:] == ["mask", "window", "votes", "history"]
    assert [sig.parameters[k].default for k in ("window", "votes", "history")] == [3, None, None]
    sig = inspect.signature(op.run_mask_vote_device)
    assert list(sig.parameters)[1:] == ["mask", "width", "out", "window", "votes", "history", "history_out", "stream"]
    for f in (op.change_boxes, op.change_tracks):
        assert inspect.signature(f).parameters["vote"].default is None


def test_the_function_is_exported_and_declared():
    import ctypes

    from dips_amd import _lib
    assert "dips_mask_vote" in _lib.header_functions()
    with open(os.path.join(ROOT, "include", "dips_hip.h")) as f:
        assert "#define DIPS_VOTE_MAX_WINDOW 31u" in f.read()
    with open(os.path.join(ROOT, "rust", "dips-hip", "src", "ffi.rs")) as f:
        rs = f.read()
    assert "pub fn dips_mask_vote(" in rs and "pub const DIPS_VOTE_MAX_WINDOW: u32 = 31;" in rs
    fn = _lib.load().dips_mask_vote
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10


# -- the schedule -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    return vref.build_geometry(tmp_path_factory.mktemp("vote_sched"), CSRC)


def test_vote_geometry_tiles_the_frames(sched):
    words = vref.words_per_lane(CSRC)
    assert words in (1, 2, 4)
    rows = [(vref.frame_words(w, h), n, k, words, res) for (w, h, n, k) in GPU_SHAPES for res in RESIDENTS]
    several = 0
    for (fw, n, k, _, res), q in zip(rows, vref.geometry(sched, rows)):
        assert q["ok"] == 1 and q["n_tiles"] == -(-fw // (64 * words))
        L, parts = q["part_frames"], q["parts"]
        # the parts [p L, min(n, (p + 1) L)) tile [0, n): none is empty, the last ends at n
        assert L >= 1 and parts == -(-n // L) and (parts - 1) * L < n <= parts * L
        # every part but the last has L frames, at least the stated minimum
        assert q["min_part"] == max(16, 8 * (k - 1))
        assert parts == 1 or L >= q["min_part"]
        # so a part other than the first starts at or after frame k - 1: it primes from input frames alone
        assert parts == 1 or L >= k - 1
        assert 1 <= q["n_waves"] <= min(res, parts * q["n_tiles"]) and q["blocks"] == -(-q["n_waves"] // 4)
        several += parts >= 2
    assert several >= 2 * len(RESIDENTS)


def test_vote_geometry_of_the_part_seam_shapes_does_not_depend_on_the_device(sched):
    """tests/test_gpu_mask_vote.py reads the part count of its small region
    from the same harness: with one tile and any realistic number of wave
    slots the cut is n / max(16, 8 (k - 1)) parts."""
    words = vref.words_per_lane(CSRC)
    for n, k, parts, L in ((300, 3, 18, 17), (600, 5, 18, 34), (600, 31, 2, 300), (600, 3, 36, 17)):
        got = vref.geometry(sched, [(vref.frame_words(40, 3), n, k, words, res) for res in RESIDENTS])
        assert {(q["parts"], q["part_frames"]) for q in got} == {(parts, L)}, (n, k, got)


def test_vote_geometry_refuses_what_it_cannot_schedule(sched):
    got = vref.geometry(sched, [(6, 0, 3, 2, 4096), (6, 10, 3, 2, 0), (6, 2 ** 31, 3, 2, 4096)])
    assert [q["ok"] for q in got] == [0, 0, 0]
    # the largest region: 2^30 - 1 rows of one word
    big = vref.geometry(sched, [(2 ** 30 - 1, 5, 31, 2, 8192)])[0]
    assert big["ok"] == 1 and big["parts"] == 1 and big["n_waves"] == 8192
