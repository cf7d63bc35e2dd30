"""GPU parity of the two batch kernels at their frame-chunk edges
(compat_batch_kernel / compat_batch_lut_kernel in compat_batch.hip,
alt_batch_kernel in alt_kernels.hip), bit-exact against the CPU oracle run
frame by frame.

A launch of 17 or more frames of a small frame is cut into chunks
(dips_amd/csrc/batch_chunks.h); every chunk after the first rebuilds its
per-pixel state from HBM: the previous q bytes or intensities from the frames
before it, dips_alt's snapshot in force from chunk_snap.  The last chunk (or
the one holding the last snapshot) writes the state the next call reads: the
ring through the second slot set and its swap, snap_out and the flip of cur.
tests/_batch_chunks.py holds the launch lengths, shapes, snapshot placements,
frame contents and the case list; tests/test_batch_chunks_cpu.py checks that
list's coverage.  Every test first asserts _batch_chunks.premise with the
device's compute units: the chunk edges it aims at are then the library's.
The calls that follow each launch on the same object read what it left."""
import numpy as np
import pytest

import _batch_chunks as bc
from oracle import oracle

pytestmark = pytest.mark.gpu

ALT_CASES = [c for c in bc.CASES if c[0] == "alt"]
COMPAT_CASES = [c for c in bc.CASES if c[0] == "compat"]
# placements whose launch follows a 3-frame call that took a snapshot (_alt_calls)
LEAD_PLACEMENTS = ("none", "first")


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _premise(launches, shape, cus):
    w, h = bc.SHAPES[shape]
    for n in launches:
        assert bc.premise(n, w * h // 4, cus), (n, shape, cus)


def _first_diff(got, want):
    return np.argwhere(got != want)[:4].tolist()


# ---------------------------------------------------------------------------
# dips_alt
# ---------------------------------------------------------------------------

def _alt_props(colorize, window, k, filt, chroma):
    from dips_amd.alt import ChromaFilter, DiPsProperties
    return DiPsProperties(colorize=colorize, window_size=window, sigmoid_horizontal_scalar=k, filter_type=filt,
                          chroma_filter=ChromaFilter(chroma))


def _alt_device_calls(shape, colorize, window, k, filt, chroma, crosscheck, frames, calls):
    """send_frames_device once per (n, flags) of `calls` on one fresh
    DiPsCompute; the outputs of all frames and the flags as one array."""
    import torch
    from dips_amd.alt import DiPsCompute
    w, h = bc.SHAPES[shape]
    dev = torch.from_numpy(frames).cuda()
    out = torch.zeros_like(dev)
    gpu = DiPsCompute(2, h, w, _alt_props(colorize, window, k, filt, chroma), crosscheck=crosscheck)
    try:
        s = 0
        for n, flags in calls:
            gpu.send_frames_device(dev[s:s + n], out[s:s + n], flags)
            s += n
        assert s == frames.shape[0]
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    finally:
        gpu.close()
    return got, np.concatenate([bc.flags_of([], n) if f is None else np.asarray(f, dtype=bool) for n, f in calls])


def _alt_calls(m, at, lead):
    """The launch under test, then 5 frames without flags and 17 with a flag
    on their frame 9: every output of those depends on the snapshot, on cur
    and on the slots the launch left.  lead: a 3-frame call with a snapshot
    first.  A launch without a snapshot then does not start from the zero
    texture; and a snapshot on the launch's frame 0 is the min with a real
    previous frame (on a fresh object it would be min(I, 0) = 0, the zero
    texture itself, and a chunk reading the wrong one would go unnoticed)."""
    calls = [(3, bc.flags_of([1], 3))] if lead else []
    return calls + [(m, bc.flags_of(at, m) if at else None), (5, None), (17, bc.flags_of([9], 17))]


@pytest.mark.parametrize("case", ALT_CASES, ids=bc.case_id)
def test_alt_device_launch_matches_oracle(case, cus):
    """One send_frames_device launch of m frames per case of the list."""
    _, shape, m, form, chroma, filt, k, colorize, pl, content = case
    _premise([m, 17], shape, cus)
    at = bc.placement(pl, m)
    lead = pl in LEAD_PLACEMENTS
    calls = _alt_calls(m, at, lead)
    t_launch = 3 if lead else 0
    n = sum(c[0] for c in calls)
    frames = bc.make_frames(shape, n, content, bc.case_seed(case),
                            still_at=t_launch + bc.middle_start(m) if content == "still" else None)
    got, flags = _alt_device_calls(shape, colorize, 1, k, filt, chroma, form != "table", frames, calls)
    assert flags[t_launch:t_launch + m].nonzero()[0].tolist() == at
    want = bc.oracle_alt(oracle, shape, colorize, 1, k, filt, chroma, frames, flags)
    bad = [t for t in range(n) if not np.array_equal(got[t], want[t])]
    assert not bad, (bad[:8], bc.chunk_starts(m), at, _first_diff(got[bad[0]], want[bad[0]]))


def _window_placements(batch_frames):
    """Launch-local snapshot frames of the W > 1 runs of 49 frames: frame 0,
    the edge of the rounds of 20, a chunk edge inside the first round (chunks
    of 13 in one round of 49, of 10 in a round of 20), none."""
    t0 = bc.plan_small(49 if batch_frames is None else batch_frames)[0]
    return {"first": [0], "round_edge": [19, 20], "chunk_edge": [t0 - 1, t0], "none": []}


@pytest.mark.parametrize("pl", ["first", "round_edge", "chunk_edge", "none"])
@pytest.mark.parametrize("batch_frames", [None, 20])
@pytest.mark.parametrize("crosscheck", [False, True])
@pytest.mark.parametrize("window,chroma", [(2, 0), (2, 2), (5, 0), (5, 2)])
def test_alt_window_launch_matches_oracle(window, chroma, crosscheck, batch_frames, pl, cus, monkeypatch):
    """W > 1: the batch kernel on prefiltered intensities (run_prefiltered), 49
    frames in one round of 4 chunks, or with DIPS_WINDOW_BATCH_FRAMES = 20 in
    rounds of 20, 20 and 9 (chunks of 10, 10 and a single one) -- against the
    oracle, not the per-frame kernel."""
    if batch_frames is None:
        monkeypatch.delenv("DIPS_WINDOW_BATCH_FRAMES", raising=False)
    else:
        monkeypatch.setenv("DIPS_WINDOW_BATCH_FRAMES", str(batch_frames))
    m = 49
    shape = "whole" if chroma == 0 else "ragged"
    _premise([m, 20, 17], shape, cus)
    assert bc.plan_small(49) == (13, 4) and bc.plan_small(20) == (10, 2) and bc.plan_small(9) == (9, 1)
    at = _window_placements(batch_frames)[pl]
    lead = pl in LEAD_PLACEMENTS
    calls = _alt_calls(m, at, lead)
    n = sum(c[0] for c in calls)
    frames = bc.make_frames(shape, n, "ties" if window == 5 else "random", 500 + 10 * window + chroma)
    filt, k = (1, 0.7) if chroma else (0, 5.0)
    got, flags = _alt_device_calls(shape, True, window, k, filt, chroma, crosscheck, frames, calls)
    want = bc.oracle_alt(oracle, shape, True, window, k, filt, chroma, frames, flags)
    bad = [t for t in range(n) if not np.array_equal(got[t], want[t])]
    assert not bad, (bad[:8], at, _first_diff(got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("crosscheck", [False, True])
@pytest.mark.parametrize("shape", list(bc.SHAPES))
def test_alt_host_feeds_of_several_chunks_match_oracle(shape, crosscheck, cus):
    """One send_frames call of 136 host frames feeds the kernel 34 per launch
    (host_stream.h feed_chunk_frames): 3 chunks of 12, 12 and 10.  Blue
    channel; snapshots on a feed edge (33, 34), on a chunk edge inside the
    second feed (45, 46), on the first frame of the third feed's last chunk
    (92) and on the first frame of the last feed (102), whose later chunks
    rebuild it from that frame and the slot before it."""
    from dips_amd.alt import DiPsCompute
    w, h = bc.SHAPES[shape]
    n, feed = 136, 34
    _premise([feed], shape, cus)
    assert bc.ceil_div(n, 4) == feed and bc.plan_small(feed) == (12, 3)
    at = [33, 34, 45, 46, 92, 102]
    tail = 5
    frames = bc.make_frames(shape, n + tail, "random", 900 + crosscheck)
    flags = np.concatenate([bc.flags_of(at, n), bc.flags_of([], tail)])
    want = bc.oracle_alt(oracle, shape, False, 1, 5.0, 0, 3, frames, flags)
    gpu = DiPsCompute(2, h, w, _alt_props(False, 1, 5.0, 0, 3), crosscheck=crosscheck)
    try:
        got = gpu.send_frames(frames[:n], flags[:n])
        snap = gpu.snapshot_texture()
        rest = gpu.send_frames(frames[n:])
    finally:
        gpu.close()
    bad = [t for t in range(n) if not np.array_equal(got[t], want[t])]
    assert not bad, (bad[:8], _first_diff(got[bad[0]], want[bad[0]]))
    # the snapshot frame's output is the stored gray texture
    assert np.array_equal(snap, want[at[-1]][..., 0])
    assert np.array_equal(rest, want[n:])


# ---------------------------------------------------------------------------
# ComputeState
# ---------------------------------------------------------------------------

def _oracle_callbacks(frames, params):
    ref = oracle.ComputeState(*params)
    h, w = frames.shape[1], frames.shape[2]
    return np.stack([oracle.frame_callback(w, h, f, ref) for f in frames]), ref.start_texture()


def _compat_device_calls(params, crosscheck, frames, pieces):
    """frame_callback_batch_device once per piece on one fresh ComputeState;
    the outputs and the start texture after the first and after the last call."""
    import torch
    from dips_amd import ChromaFilter, ComputeState, DiPsFilter
    colorize, window, sens, filt, chroma = params
    dev = torch.from_numpy(frames).cuda()
    out = torch.zeros_like(dev)
    starts = [torch.zeros_like(dev[0]) for _ in range(2)]
    cs = ComputeState(colorize, window, sens, DiPsFilter(filt), ChromaFilter(chroma), crosscheck=crosscheck)
    try:
        s = 0
        for i, n in enumerate(pieces):
            cs.frame_callback_batch_device(dev[s:s + n], out[s:s + n])
            s += n
            if i == 0:
                assert cs.start_texture_device(starts[0])
        assert s == frames.shape[0]
        assert cs.start_texture_device(starts[1])
        torch.cuda.synchronize()
        return out.cpu().numpy(), [x.cpu().numpy() for x in starts]
    finally:
        cs.close()


def _check_compat(got, starts, frames, params, note):
    want, want_start = _oracle_callbacks(frames, params)
    bad = [t for t in range(frames.shape[0]) if not np.array_equal(got[t], want[t])]
    assert not bad, (bad[:8], note, _first_diff(got[bad[0]], want[bad[0]]))
    assert np.array_equal(starts[0], want_start) and np.array_equal(starts[1], want_start)


@pytest.mark.parametrize("case", COMPAT_CASES, ids=bc.case_id)
def test_compat_device_launch_matches_oracle(case, cus):
    """One call of 7 + m frames: the first seven go frame by frame, then one
    batch_steady launch of m.  Calls of 1, 2 and 3 frames follow (single
    chunks that read the ring the launch left through the swap, the
    re-derived q of frame m - 4 included), then m frames again (the swap
    back), then 4."""
    _, shape, m, form, chroma, filt, k, colorize, _, content = case
    _premise([m], shape, cus)
    pieces = [7 + m, 1, 2, 3, m, 4]
    n = sum(pieces)
    frames = bc.make_frames(shape, n, content, bc.case_seed(case),
                            still_at=7 + bc.middle_start(m) if content == "still" else None)
    params = (colorize, 1, k, filt, chroma)
    got, starts = _compat_device_calls(params, form != "table", frames, pieces)
    _check_compat(got, starts, frames, params, (pieces, bc.chunk_starts(m)))


@pytest.mark.parametrize("batch_frames", [None, 20])
@pytest.mark.parametrize("crosscheck", [False, True])
@pytest.mark.parametrize("window,chroma", [(2, 0), (2, 2), (5, 0), (5, 2)])
def test_compat_window_launch_matches_oracle(window, chroma, crosscheck, batch_frames, cus, monkeypatch):
    """W > 1: compat_filter_frames, then the batch kernel on the filtered
    ring texels -- 49 steady-state frames in one launch of 4 chunks, or with
    DIPS_WINDOW_BATCH_FRAMES = 20 in launches of 20, 20 and 9 (each of the
    first two swaps the ring sets); calls of 1, 2 and 3 frames follow."""
    if batch_frames is None:
        monkeypatch.delenv("DIPS_WINDOW_BATCH_FRAMES", raising=False)
    else:
        monkeypatch.setenv("DIPS_WINDOW_BATCH_FRAMES", str(batch_frames))
    m = 49
    shape = "whole" if chroma == 0 else "ragged"
    _premise([m, 20], shape, cus)
    pieces = [7 + m, 1, 2, 3]
    frames = bc.make_frames(shape, sum(pieces), "ties" if window == 5 else "random", 700 + 10 * window + chroma)
    params = (True, window, 0.7, 1, chroma) if chroma else (False, window, 5.0, 0, chroma)
    got, starts = _compat_device_calls(params, crosscheck, frames, pieces)
    _check_compat(got, starts, frames, params, pieces)


@pytest.mark.parametrize("crosscheck", [False, True])
@pytest.mark.parametrize("shape", list(bc.SHAPES))
def test_compat_host_feeds_of_several_chunks_match_oracle(shape, crosscheck, cus):
    """One frame_callback_batch of 143 host frames is fed 36 per launch: the
    first feed runs 7 frames one by one and 29 as chunks of 15 and 14, the
    others 3 chunks of 12 (the last feed 12, 12 and 11).  Red channel;
    per-frame frame_callback calls follow."""
    from dips_amd import ChromaFilter, ComputeState, DiPsFilter, frame_callback
    w, h = bc.SHAPES[shape]
    n, feed, tail = 143, 36, 4
    _premise([feed], shape, cus)
    assert bc.ceil_div(n, 4) == feed and [bc.plan_small(x) for x in (29, 36, 35)] == [(15, 2), (12, 3), (12, 3)]
    frames = bc.make_frames(shape, n + tail, "random", 950 + crosscheck)
    params = (True, 1, 5.0, 0, 1)
    want, want_start = _oracle_callbacks(frames, params)
    cs = ComputeState(True, 1, 5.0, DiPsFilter.Sigmoid, ChromaFilter.Red, crosscheck=crosscheck)
    try:
        got = cs.frame_callback_batch(w, h, frames[:n])
        rest = np.stack([frame_callback(w, h, f, cs) for f in frames[n:]])
        start = cs.start_texture()
    finally:
        cs.close()
    bad = [t for t in range(n) if not np.array_equal(got[t], want[t])]
    assert not bad, (bad[:8], _first_diff(got[bad[0]], want[bad[0]]))
    assert np.array_equal(rest, want[n:])
    assert np.array_equal(start, want_start)
