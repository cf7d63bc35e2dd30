"""CPU checks of the cases tests/test_gpu_shard_chunks.py runs
(tests/_shard_chunks.py): the sharded visual operators at rank ranges whose
launches are cut into frame chunks.

* The layouts: the restated rank ranges are the library's dips_shard_range,
  every rank's frames and chunk plan are the documented ones, rank 0 of
  ComputeState launches n_local - 7 frames with chunk edges of its own, and the
  host-pointer calls are cut into feeds first.
* The flags: for every dips_alt case the restated run loop, its closed form
  and dips_amd.alt.run_loop_flags agree, they are the frames the placement
  wants, no two flags are closer than 3 frames, and the one marker past the
  sharded clip flags frame 9 of the 17 frames the last rank runs afterwards.
* The case lists meet their coverage conditions, so the GPU file cannot
  quietly lose a combination."""
import numpy as np
import pytest

import _batch_chunks as bc
import _shard_chunks as sc

ALT = sc.ALT_CASES
COMPAT = sc.COMPAT_CASES


def _cuts(launches):
    """Chunk lengths of every launch, in order."""
    out = []
    for _, m in launches:
        starts = bc.chunk_starts(m) + [m]
        out.append([b - a for a, b in zip(starts, starts[1:])])
    return out


def test_ranges_are_the_librarys():
    from dips_amd.comm import shard_range
    for world, n in sc.LAYOUTS + ((5, 7), (8, 5), (7, 1000)):
        for r in range(world):
            assert sc.shard_range(n, world, r) == shard_range(n, world, r), (world, n, r)


def test_layouts_cut_as_documented():
    assert [sc.counts(*lay) for lay in sc.LAYOUTS] == [[16, 17, 17], [33, 33], [33, 33, 33, 34], [49] * 3, [17] * 8,
                                                       [100, 100]]
    per_count = {16: [16], 17: [9, 8], 33: [11] * 3, 34: [12, 12, 10], 49: [13, 13, 13, 10], 100: [15] * 6 + [10]}
    for world, n in sc.LAYOUTS:
        for r, c in enumerate(sc.counts(world, n)):
            # dips_alt and ComputeState ranks r > 0, device pointers: one launch of the rank's frames
            assert sc.alt_launches(c) == [(0, c)] and _cuts(sc.alt_launches(c)) == [per_count[c]]
            if r > 0:
                assert sc.compat_launches(r, c) == [(0, c)]
                assert sc.middle(sc.edges_of(sc.alt_launches(c))) == bc.middle_start(c)
    # every rank r > 0 is chunked; in (3, 50) a one-chunk rank sits next to them
    assert all(len(per_count[c]) > 1 for world, n in sc.LAYOUTS for c in sc.counts(world, n)[1:])
    assert len(per_count[sc.counts(3, 50)[0]]) == 1
    # (8, 136): the chunked ranks start at 17 r, every residue mod 4
    assert {sc.shard_range(136, 8, r)[0] % 4 for r in range(1, 8)} == {0, 1, 2, 3}
    assert [sc.shard_range(136, 8, r)[0] for r in range(8)] == [17 * r for r in range(8)]
    # ComputeState's rank 0: frames 0..3 in one call, 4..6 one by one, then a batch of n_local - 7
    rank0 = [sc.compat_launches(0, sc.counts(*lay)[0]) for lay in sc.LAYOUTS]
    assert rank0 == [[(7, 9)], [(7, 26)], [(7, 26)], [(7, 42)], [(7, 10)], [(7, 93)]]
    assert [_cuts(la)[0] for la in rank0] == [[9], [13, 13], [13, 13], [14, 14, 14], [10], [16] * 5 + [13]]
    assert [sc.edges_of(la) for la in rank0] == [[7], [7, 20], [7, 20], [7, 21, 35], [7], [7, 23, 39, 55, 71, 87]]


def test_host_calls_are_cut_into_feeds_first():
    # a rank's host frames go up a quarter at a time; each feed is a launch with a chunk plan of its own
    assert sc.alt_launches(100, host=True) == [(0, 25), (25, 25), (50, 25), (75, 25)]
    assert _cuts(sc.alt_launches(100, host=True)) == [[13, 12]] * 4
    assert sc.alt_launches(33, host=True) == [(0, 9), (9, 9), (18, 9), (27, 6)]
    assert sc.alt_launches(17, host=True) == [(0, 5), (5, 5), (10, 5), (15, 2)]
    # rank 0 of ComputeState: 96 frames after the first four in feeds of 24, three of the first go one by one
    assert sc.compat_launches(0, 100, host=True) == [(7, 21), (28, 24), (52, 24), (76, 24)]
    assert _cuts(sc.compat_launches(0, 100, host=True)) == [[11, 10], [12, 12], [12, 12], [12, 12]]
    assert sc.compat_launches(0, 16, host=True) == [(7, 3), (10, 3), (13, 3)]
    assert sc.compat_launches(0, 33, host=True) == [(7, 5), (12, 8), (20, 8), (28, 5)]
    # rounds of 20 (W > 1): 20 + 13, 20 + 14; chunks of 10 in the first round, a single one after it
    assert sc.alt_launches(33, batch_frames=20) == [(0, 20), (20, 13)]
    assert sc.compat_launches(3, 34, batch_frames=20) == [(0, 20), (20, 14)]
    assert sc.compat_launches(0, 33, batch_frames=20) == [(7, 20), (27, 6)]
    assert sc.edges_of(sc.alt_launches(33, batch_frames=20)) == [0, 10, 20]


@pytest.mark.parametrize("case", ALT + sc.ALT_WINDOW_CASES, ids=sc.case_id)
def test_flags_are_the_restated_loops(case):
    from dips_amd.alt import run_loop_flags
    n, tail = case.n_total, sum(sc.ALT_TAIL)
    markers = sc.markers_of(case)
    flags = sc.loop_flags(n + tail, markers)
    assert np.array_equal(flags, sc.closed_form_flags(n + tail, markers))
    assert np.array_equal(flags, run_loop_flags(n + tail, markers))
    at = np.flatnonzero(flags)
    assert at[0] == 2 and np.diff(at).min() >= 3
    # the frames after the sharded call: one flag, on frame 9 of the 17
    assert at[at >= n].tolist() == [n + sc.ALT_TAIL[0] + 9]
    f, c, edges = sc.target(case)
    assert case.rank > 0 and f >= 16 and len(edges) >= 2
    wanted = sc.wanted_flags(case)
    inside = [t for t in at.tolist() if f - 4 <= t < f + c]
    if wanted is not None:
        assert at[at < n].tolist() == wanted
    local = {"far": [], "edge-1": [-1], "edge-2": [-2], "first": [0], "before_edge": [sc.middle(edges) - 1],
             "on_edge": [sc.middle(edges)], "last_chunk_start": [edges[-1]], "last": [c - 1], "round_edge": [20]}
    if case.placement in local:
        assert [t - f for t in inside] == local[case.placement]
        # the edge placements sit on a chunk's first frame of the target rank, or just before one
        if case.placement in ("on_edge", "last_chunk_start"):
            assert inside[0] - f in edges[1:]
        if case.placement == "before_edge":
            assert inside[0] - f + 1 in edges[1:]
        if case.placement == "round_edge" and case.batch_frames == 20:
            assert 20 in [s for s, _ in sc.alt_launches(c, False, 20)]
    elif case.placement == "every_third":
        assert at[at < n].tolist() == list(range(2, n, 3))
    else:
        assert case.placement == "random" and len(inside) >= 1 and len(at) >= n // 20
    if case.placement == "far":
        # the snapshot in force over the whole rank lies in an earlier rank's range
        assert at[at < f].tolist() == [2, f - 7] and sc.shard_range(n, case.world, case.rank - 1)[0] <= f - 7
    if case.placement == "last" and case.world > 2:
        assert case.rank + 1 < case.world  # the next rank's edge-1


def _n_chunks(case):
    return len(sc.target(case)[2])


def _common_coverage(rows, dev):
    assert len({sc.case_id(c) for c in rows}) == len(rows)
    for c in rows:
        assert (c.world, c.n_total) in sc.LAYOUTS and c.shape in bc.SHAPES and c.chroma in range(4)
        assert c.content in bc.CONTENTS and (c.still in ("rank", "chunk")) == (c.content == "still")
        assert (c.filt, c.k) in bc.FORM_VARIANTS[c.form]
        assert c.form == "table" or bc.form_of(True, c.filt, c.k) == c.form
        assert 0 < c.rank < c.world and c.window == 1 and c.batch_frames is None
    # every kernel form x chroma at (2, 66); both shapes on every form at (3, 147)
    assert {(c.form, c.chroma) for c in dev if (c.world, c.n_total) == (2, 66)} >= \
        {(f, ch) for f in bc.FORMS for ch in range(4)}
    assert {(c.shape, c.form) for c in dev if (c.world, c.n_total) == (3, 147)} == \
        {(s, f) for s in bc.SHAPES for f in bc.FORMS}
    # every content on every layout; a frame held across a rank edge and across a chunk edge
    assert {((c.world, c.n_total), c.content) for c in dev} == {(lay, co) for lay in sc.LAYOUTS for co in bc.CONTENTS}
    assert {c.still for c in dev if c.content == "still"} == {"rank", "chunk"}
    assert {(c.form, c.colorize) for c in rows} == {(f, col) for f in bc.FORMS for col in (False, True)}
    for c in rows:
        at = sc.still_at(c)
        if at is not None:
            f, n_local, edges = sc.target(c)
            assert at == (f if c.still == "rank" else f + sc.middle(edges)) and 2 <= at < c.n_total - 1
            assert c.still == "rank" or at - f in edges[1:]


def test_alt_cases_meet_the_coverage_conditions():
    dev = [c for c in ALT if not c.host]
    host = [c for c in ALT if c.host]
    assert 60 <= len(ALT) <= 90
    _common_coverage(ALT, dev)
    # every placement on a rank r > 0 of two chunks, of three, and of four or more (device pointers)
    for pl in sc.PLACEMENTS:
        ns = {_n_chunks(c) for c in dev if c.placement == pl}
        assert 2 in ns and 3 in ns and any(k >= 4 for k in ns), (pl, ns)
    # every placement with host and with device pointers; host feeds of several chunks among them
    assert {c.placement for c in dev} == {c.placement for c in host} == set(sc.PLACEMENTS)
    assert any(len(bc.chunk_starts(m)) > 1 for c in host
               for _, m in sc.alt_launches(sc.target(c)[1], True)) and {c.form for c in host} == set(bc.FORMS)
    assert {(c.world, c.n_total) for c in ALT} == set(sc.LAYOUTS)


def test_compat_cases_meet_the_coverage_conditions():
    dev = [c for c in COMPAT if not c.host]
    host = [c for c in COMPAT if c.host]
    assert 30 <= len(COMPAT) <= 60
    _common_coverage(COMPAT, dev)
    assert {(c.world, c.n_total) for c in dev} == set(sc.LAYOUTS)
    # host pointers: (3, 50), (4, 133) and (2, 200), the table and the arithmetic kernel on each
    assert {((c.world, c.n_total), c.form == "table") for c in host} == \
        {(lay, t) for lay in ((3, 50), (4, 133), (2, 200)) for t in (False, True)}


def test_window_cases_meet_the_coverage_conditions():
    want = {(w, table, lay, g) for w in (2, 5) for table in (False, True) for lay in ((2, 66), (4, 133))
            for g in (None, 20)}
    rows = sc.ALT_WINDOW_CASES
    assert {(c.window, c.form == "table", (c.world, c.n_total), c.batch_frames, c.placement) for c in rows} == \
        {k + (pl,) for k in want for pl in sc.WINDOW_PLACEMENTS}
    assert len(rows) == 64 and len({sc.case_id(c) for c in rows}) == 64
    rows = sc.COMPAT_WINDOW_CASES
    assert {(c.window, c.form == "table", (c.world, c.n_total), c.batch_frames) for c in rows} == want
    assert len(rows) == 16 and len({sc.case_id(c) for c in rows}) == 16
    for c in sc.ALT_WINDOW_CASES + sc.COMPAT_WINDOW_CASES:
        assert not c.host and 0 < c.rank < c.world and c.form == bc.form_of(c.form != "table", c.filt, c.k)
        # rounds of 20 + 13 (20 + 14 on the 34-frame rank) inside every rank r > 0
        for n_local in sc.counts(c.world, c.n_total):
            assert [m for _, m in sc.rounds(0, n_local, 20)] == [20, n_local - 20]


def test_clips_hold_their_frame_and_serve_every_layout():
    assert sc.CLIP == 200 + 23 == max(n for _, n in sc.LAYOUTS) + sum(sc.COMPAT_TAIL)
    assert sum(sc.ALT_TAIL) <= sum(sc.COMPAT_TAIL)
    for c in (ALT + COMPAT):
        at = sc.still_at(c)
        if at is None:
            continue
        f = bc.make_frames(c.shape, sc.CLIP, "still", sc.clip_seed(c.shape, "still", at), still_at=at)
        assert all(np.array_equal(f[t], f[at]) for t in range(at - 2, at + 2))
        assert not np.array_equal(f[at - 3], f[at]) and not np.array_equal(f[at + 2], f[at])
