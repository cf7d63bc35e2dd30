"""GPU parity of the frame-range sharding of the two visual operators
(dips_frame_callback_batch_sharded in shard_abi.hip, dips_alt_run_sharded in
alt_abi.hip) where every rank's launch is cut into frame chunks
(dips_amd/csrc/batch_chunks.h), bit-exact against the CPU oracle run once over
the whole clip, frame by frame.

Ranks are loopback threads on the one device (tests/_shard_loopback.py).  At a
rank's first chunked launch three pieces of state meet: what the replay
(dips_alt) or the resume and the broadcast (ComputeState) left in the handle,
what chunk 0 takes from the handle, and what the later chunks rebuild from
HBM.  tests/_shard_chunks.py holds the layouts, the snapshot placements
relative to a target rank r > 0 and the case lists;
tests/test_shard_chunks_cpu.py checks their coverage.  Every test first
asserts _batch_chunks.premise with the device's compute units, so the chunk
edges it aims at are the library's.  After the call the last rank's object
carries on with ordinary calls, which read the state the sharded call left:
dips_alt the slots, the snapshot texture and the loop state, ComputeState the
swapped ring and the start texture."""
import functools

import numpy as np
import pytest

import _batch_chunks as bc
import _shard_chunks as sc
from _shard_loopback import alt_sharded, compat_loopback
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _premise(case, cus):
    w, h = bc.SHAPES[case.shape]
    longest = max(sc.counts(case.world, case.n_total) + [17])
    assert bc.premise(longest, w * h // 4, cus), (longest, case.shape, cus)


def _rounds_env(case, monkeypatch):
    if case.batch_frames is None:
        monkeypatch.delenv("DIPS_WINDOW_BATCH_FRAMES", raising=False)
    else:
        monkeypatch.setenv("DIPS_WINDOW_BATCH_FRAMES", str(case.batch_frames))


@functools.lru_cache(maxsize=None)
def _clip(shape, content, at):
    """The one clip of a (shape, content, held frame): every layout takes its
    frames, and the frames after the sharded call, from its head."""
    f = bc.make_frames(shape, sc.CLIP, content, sc.clip_seed(shape, content, at), still_at=at)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _oracle_alt(shape, content, at, colorize, window, k, filt, chroma, n, markers):
    w, h = bc.SHAPES[shape]
    out = oracle.AltCompute(2, w, h, colorize, window, k, filt, chroma).run(_clip(shape, content, at)[:n], markers)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_compat(shape, content, at, colorize, window, k, filt, chroma):
    """One ComputeState over the whole clip: serves every layout."""
    w, h = bc.SHAPES[shape]
    ref = oracle.ComputeState(colorize, window, k, filt, chroma)
    out = np.stack([oracle.frame_callback(w, h, f, ref) for f in _clip(shape, content, at)])
    start = ref.start_texture()
    out.setflags(write=False)
    start.setflags(write=False)
    return out, start


def _differing_ranks(case, got, want, launches_of, flags=None):
    """None, or the failure message: every rank with a differing frame, its
    range, its chunk starts, the flags and the first differing global frames."""
    n = case.n_total
    bad = [t for t in range(n) if not np.array_equal(got[t], want[t])]
    if not bad:
        return None
    rows = []
    for r in range(case.world):
        s, e = sc.shard_range(n, case.world, r)
        mine = [t for t in bad if s <= t < e]
        if mine:
            starts = [s + t for t in sc.edges_of(launches_of(r, e - s))]
            rows.append(f"rank {r} [{s}, {e}) chunks start at {starts}: frames {mine[:8]} differ ({len(mine)})")
    at = "" if flags is None else f"; flags on {np.flatnonzero(flags).tolist()}"
    first = np.argwhere(got[bad[0]] != want[bad[0]])[:4].tolist()
    return "; ".join(rows) + at + f"; frame {bad[0]} first differs at (y, x, channel) {first}"


# ---------------------------------------------------------------------------
# dips_alt
# ---------------------------------------------------------------------------

def _alt_continue(runner, host, frames):
    """The ordinary run loop (dips_alt_run) on the object the sharded call
    used: the runner's host handle, or its device handle."""
    if host:
        return runner(frames)
    import torch
    from dips_amd import _lib
    hd = runner.compute._device_handle()
    dev = torch.from_numpy(frames.copy()).cuda()
    out = torch.empty_like(dev)
    mk = runner.markers
    with _lib.on_stream(hd._lib.dips_alt_set_stream, hd.ptr, hd.check, torch.cuda.current_stream().cuda_stream):
        hd.check(hd._lib.dips_alt_run(hd.ptr, dev.data_ptr(), int(dev.shape[0]), mk.ctypes.data if mk.size else None,
                                      int(mk.size), out.data_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _alt_snapshot(runner, host):
    if host:
        return runner.compute.snapshot_texture()
    c = runner.compute
    hd = c._device_handle()
    out = np.empty((c.rows, c.cols), dtype=np.uint8)
    hd.check(hd._lib.dips_alt_snapshot_texture(hd.ptr, out.ctypes.data, out.nbytes))
    return out


def _run_alt(case, cus):
    from dips_amd.alt import ChromaFilter, DiPsProperties
    _premise(case, cus)
    n, tail = case.n_total, sum(sc.ALT_TAIL)
    markers = sc.markers_of(case)
    flags = sc.loop_flags(n + tail, markers)
    wanted = sc.wanted_flags(case)
    assert wanted is None or np.flatnonzero(flags[:n]).tolist() == wanted
    at = sc.still_at(case)
    frames = _clip(case.shape, case.content, at)[:n + tail]
    want = _oracle_alt(case.shape, case.content, at, case.colorize, case.window, case.k, case.filt, case.chroma,
                       n + tail, tuple(markers))
    props = DiPsProperties(colorize=case.colorize, window_size=case.window, sigmoid_horizontal_scalar=case.k,
                           filter_type=case.filt, chroma_filter=ChromaFilter(case.chroma))
    got, last = alt_sharded(case.world, frames[:n], props, markers, 2, not case.host, keep_last=True,
                            crosscheck=case.form != "table")
    try:
        snap_after = _alt_snapshot(last, case.host)
        more, s = [], n
        for m in sc.ALT_TAIL:
            more.append(_alt_continue(last, case.host, frames[s:s + m]))
            s += m
        snap_end = _alt_snapshot(last, case.host)
    finally:
        last.close()
    msg = _differing_ranks(case, got, want, lambda r, c: sc.alt_launches(c, case.host, case.batch_frames), flags[:n])
    assert msg is None, msg
    # a snapshot frame's output is the stored gray texture
    assert np.array_equal(snap_after, want[np.flatnonzero(flags[:n])[-1]][..., 0]), "snapshot texture after the call"
    more = np.concatenate(more)
    bad = [n + t for t in range(tail) if not np.array_equal(more[t], want[n + t])]
    assert not bad, f"the last rank's next calls differ at global frames {bad[:8]} (flags {np.flatnonzero(flags)})"
    assert flags[n:].nonzero()[0].tolist() == [sc.ALT_TAIL[0] + 9]
    assert np.array_equal(snap_end, want[n + sc.ALT_TAIL[0] + 9][..., 0]), "snapshot texture after the next calls"


@pytest.mark.parametrize("case", sc.ALT_CASES, ids=sc.case_id)
def test_alt_sharded_chunked_ranks_match_oracle(case, cus):
    """dips_alt_run_sharded (N = 2, W = 1) with the flag placed relative to
    the case's target rank; then the last rank runs 5 and 17 more frames."""
    _run_alt(case, cus)


@pytest.mark.parametrize("case", sc.ALT_WINDOW_CASES, ids=sc.case_id)
def test_alt_sharded_window_ranks_match_oracle(case, cus, monkeypatch):
    """N = 2, W > 1: run_prefiltered under sharding, a rank in one round or in
    rounds of 20 frames."""
    _rounds_env(case, monkeypatch)
    _run_alt(case, cus)


# ---------------------------------------------------------------------------
# ComputeState
# ---------------------------------------------------------------------------

def _compat_continue(cs, host, w, h, frames):
    """Batches of 1, 3 and 17 frames, then two single frames: frame_callback
    on the host handle; the device handle has no per-frame entry and takes them
    as batches of one."""
    outs, s = [], 0
    if host:
        from dips_amd import frame_callback
        for m in sc.COMPAT_TAIL[:3]:
            outs.append(cs.frame_callback_batch(w, h, frames[s:s + m]))
            s += m
        for _ in sc.COMPAT_TAIL[3:]:
            outs.append(frame_callback(w, h, frames[s], cs)[None])
            s += 1
        return np.concatenate(outs)
    import torch
    dev = torch.from_numpy(frames.copy()).cuda()
    out = torch.zeros_like(dev)
    for m in sc.COMPAT_TAIL:
        cs.frame_callback_batch_device(dev[s:s + m], out[s:s + m])
        s += m
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _compat_start(cs, host, w, h):
    if host:
        return cs.start_texture()
    import torch
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    assert cs.start_texture_device(out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _run_compat(case, cus):
    from dips_amd import ChromaFilter, DiPsFilter
    _premise(case, cus)
    w, h = bc.SHAPES[case.shape]
    n, tail = case.n_total, sum(sc.COMPAT_TAIL)
    at = sc.still_at(case)
    frames = _clip(case.shape, case.content, at)[:n + tail]
    want, want_start = _oracle_compat(case.shape, case.content, at, case.colorize, case.window, case.k, case.filt,
                                      case.chroma)
    props = (case.colorize, case.window, case.k, DiPsFilter(case.filt), ChromaFilter(case.chroma))
    _, got, states = compat_loopback(case.world, n, w, h, props, not case.host, frames=frames[:n],
                                     crosscheck=case.form != "table", keep=True)
    try:
        starts = [_compat_start(cs, case.host, w, h) for cs in states]
        more = _compat_continue(states[-1], case.host, w, h, frames[n:])
        start_end = _compat_start(states[-1], case.host, w, h)
    finally:
        for cs in states:
            cs.close()
    msg = _differing_ranks(case, got, want, lambda r, c: sc.compat_launches(r, c, case.host, case.batch_frames))
    assert msg is None, msg
    wrong = [r for r, s in enumerate(starts) if not np.array_equal(s, want_start)]
    assert not wrong and np.array_equal(start_end, want_start), f"start texture differs on ranks {wrong}"
    bad = [n + t for t in range(tail) if not np.array_equal(more[t], want[n + t])]
    assert not bad, f"the last rank's next calls {sc.COMPAT_TAIL} differ at global frames {bad[:8]}"


@pytest.mark.parametrize("case", sc.COMPAT_CASES, ids=sc.case_id)
def test_compat_sharded_chunked_ranks_match_oracle(case, cus):
    """dips_frame_callback_batch_sharded (W = 1); every rank's start texture;
    then the last rank's ComputeState carries on through the swapped ring."""
    _run_compat(case, cus)


@pytest.mark.parametrize("case", sc.COMPAT_WINDOW_CASES, ids=sc.case_id)
def test_compat_sharded_window_ranks_match_oracle(case, cus, monkeypatch):
    """W > 1: compat_filter_frames inside a shard, a rank's launch in one
    round or in rounds of 20 frames."""
    _rounds_env(case, monkeypatch)
    _run_compat(case, cus)
