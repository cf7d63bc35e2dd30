"""The cases tests/test_gpu_shard_chunks.py runs: the frame-range sharding of
the two visual operators (dips_frame_callback_batch_sharded in shard_abi.hip,
dips_alt_run_sharded in alt_abi.hip) at rank ranges long enough for every
rank's launch to be cut into frame chunks (dips_amd/csrc/batch_chunks.h).  No
GPU and no library here: tests/test_shard_chunks_cpu.py checks the
restatements against the library's shard_range and this list against its
coverage conditions.

Three pieces of state meet at a rank's first chunked launch: what the replay
(dips_alt) or the resume and broadcast (ComputeState) left in the handle, what
chunk 0 takes from the handle, and what the later chunks rebuild from HBM.
The snapshot placements of dips_alt are therefore taken relative to a target
rank r > 0: its first frame f, its count c, and the chunk edges of its launches.
"""
from collections import namedtuple

import numpy as np

import _batch_chunks as bc

# (world, n_total): frames per rank and their chunks
#   3,  50: 16, 17, 17      1, 9+8, 9+8 (a one-chunk rank next to chunked ones)
#   2,  66: 33, 33          3 x 11
#   4, 133: 33, 33, 33, 34  3 x 11; the last 3 x 12 (ragged)
#   3, 147: 49 each         13, 13, 13, 10
#   8, 136: 17 each         9+8; the ranks start at 17 r: first mod 4 takes all four values
#   2, 200: 100 each        6 x 15 + 10
LAYOUTS = ((3, 50), (2, 66), (4, 133), (3, 147), (8, 136), (2, 200))

# frames after the sharded call on the last rank's object: dips_alt 5 + 17 through the ordinary run,
# ComputeState batches of 1, 3 and 17 and two per-frame calls
ALT_TAIL = (5, 17)
COMPAT_TAIL = (1, 3, 17, 1, 1)
# every case cuts its frames from the head of one clip of this length per (shape, content)
CLIP = max(n for _, n in LAYOUTS) + max(sum(ALT_TAIL), sum(COMPAT_TAIL))


def shard_range(n_total, world, r):
    """[first, end) of rank r (dips_shard_range)."""
    return n_total * r // world, n_total * (r + 1) // world


def counts(world, n_total):
    return [e - s for s, e in (shard_range(n_total, world, r) for r in range(world))]


def feeds(n, host):
    """(start, length) of the device launches one call of n frames makes: one
    for device pointers; host frames go up a quarter of the call at a time
    (host_stream.h feed_chunk_frames; 8 KiB frames are far below its byte
    budget)."""
    if not host or n == 0:
        return [(0, n)] if n else []
    q = bc.ceil_div(n, 4)
    return [(s, min(q, n - s)) for s in range(0, n, q)]


def rounds(start, m, batch_frames):
    """W > 1: a launch is filtered and run batch_frames at a time
    (DIPS_WINDOW_BATCH_FRAMES; unset, a clip this small is one round)."""
    if batch_frames is None:
        return [(start, m)]
    return [(start + s, min(batch_frames, m - s)) for s in range(0, m, batch_frames)]


def alt_launches(c, host=False, batch_frames=None):
    """Rank-local (start, length) of the batch kernel launches over a rank's
    own c frames (dips_alt: the replay is a launch of its own before them)."""
    return [x for s, m in feeds(c, host) for x in rounds(s, m, batch_frames)]


def compat_launches(rank, c, host=False, batch_frames=None):
    """The same for ComputeState.  Rank 0 runs frames 0..3 in one call and the
    rest in a second one, whose first three frames still go one by one (the
    ring is raw before frame 7); the other ranks resume in steady state."""
    if rank > 0:
        return [x for s, m in feeds(c, host) for x in rounds(s, m, batch_frames)]
    out = []
    for i, (s, m) in enumerate(feeds(c - 4, host)):
        lead = min(3, m) if i == 0 else 0
        if m > lead:
            out += rounds(4 + s + lead, m - lead, batch_frames)
    return out


def edges_of(launches):
    """Rank-local first frames of every chunk of every launch."""
    return [s + t for s, m in launches for t in bc.chunk_starts(m)]


def middle(edges):
    """The first frame of the middle chunk (_batch_chunks.middle_start where
    the rank is one launch)."""
    return edges[len(edges) // 2]


# ---------------------------------------------------------------------------
# the run loop's snapshot flags (dips_alt/src/lib.rs:636-670) restated
# ---------------------------------------------------------------------------

def loop_flags(n, markers):
    ms = set(int(m) for m in markers)
    flags = np.zeros(n, dtype=bool)
    index = overall = 0
    for t in range(n):
        flags[t] = index == 2
        if index <= 2:
            index += 1
        overall += 1
        if overall in ms:
            index = 0
    return flags


def closed_form_flags(n, markers):
    """Frame 2 is flagged and a marker m flags frame m + 2, unless a marker
    m + 1 or m + 2 restarts the count first: two markers closer than 3 apart
    give one flag, so no two flags are closer than 3."""
    ms = set(int(m) for m in markers) | {0}
    return np.array([(t - 2) in ms and (t - 1) not in ms and t not in ms for t in range(n)], dtype=bool)


PLACEMENTS = ("far", "edge-1", "edge-2", "first", "before_edge", "on_edge", "last_chunk_start", "last",
              "every_third", "random")
# W > 1 adds the flag on the edge of the rounds of 20
WINDOW_PLACEMENTS = ("far", "first", "on_edge", "round_edge")

Alt = namedtuple("Alt", "group world n_total rank placement host shape form chroma filt k colorize content still "
                        "window batch_frames")
Compat = namedtuple("Compat", "group world n_total rank host shape form chroma filt k colorize content still "
                              "window batch_frames")


def target(case):
    """(f, c, chunk edges) of the case's target rank, rank-local edges."""
    f, e = shard_range(case.n_total, case.world, case.rank)
    if isinstance(case, Alt):
        la = alt_launches(e - f, case.host, case.batch_frames)
    else:
        la = compat_launches(case.rank, e - f, case.host, case.batch_frames)
    return f, e - f, edges_of(la)


def wanted_flags(case):
    """The global frames of the sharded clip a placement wants flagged (None
    for the two placements given by their markers)."""
    f, c, edges = target(case)
    pl = case.placement
    if pl in ("every_third", "random"):
        return None
    at = {
        "far": f - 7,  # in an earlier rank's range; none in [f - 4, f + c)
        "edge-1": f - 1,
        "edge-2": f - 2,
        "first": f,
        "before_edge": f + middle(edges) - 1,
        "on_edge": f + middle(edges),
        "last_chunk_start": f + edges[-1],
        "last": f + c - 1,
        "round_edge": f + 20,
    }[pl]
    return [2, at]


def tail_marker(case):
    """The refresh marker that flags frame 9 of the 17 frames the last rank
    runs after the sharded call and the 5 before them."""
    return case.n_total + ALT_TAIL[0] + 9 - 2


def markers_of(case):
    """The refresh markers of a case; the markers inside the sharded clip flag
    frames of that clip only (m + 2 < n_total)."""
    pl = case.placement
    if pl == "every_third":
        ms = list(range(3, case.n_total - 2, 3))
    elif pl == "random":
        rng = np.random.default_rng(4000 + 7 * case.n_total + case.world + case.rank)
        ms = (3 + np.flatnonzero(rng.random(case.n_total - 5) < 0.1)).tolist()
    else:
        ms = [t - 2 for t in wanted_flags(case) if t != 2]
    return ms + [tail_marker(case)]


def still_at(case):
    """Where a `still` clip holds its frame (frames at-2 .. at+1 equal): across
    the target rank's first frame, or across its middle chunk edge."""
    if case.content != "still":
        return None
    f, _, edges = target(case)
    return f if case.still == "rank" else f + middle(edges)


def clip_seed(shape, content, at):
    return sum((i + 1) * b for i, b in enumerate(f"{shape}-{content}-{at}".encode())) % (2 ** 31)


def case_id(c):
    ptr = "host" if c.host else "dev"
    col = "col" if c.colorize else "gray"
    pl = f"-{c.placement}" if isinstance(c, Alt) else ""
    rounds_ = "" if c.window == 1 else f"-W{c.window}-g{c.batch_frames}"
    return (f"{c.group}-w{c.world}n{c.n_total}r{c.rank}{pl}-{ptr}-{c.shape}-{c.form}-ch{c.chroma}-f{c.filt}-k{c.k:g}-"
            f"{col}-{c.content}{'@' + c.still if c.still else ''}{rounds_}")


# ---------------------------------------------------------------------------
# the case lists
# ---------------------------------------------------------------------------

def _target_ranks():
    """Per layout, the ranks r > 0 a case may aim at, cycled: (3, 50) both
    chunked ranks, (4, 133) an inner rank and the ragged last one, (8, 136)
    ranks whose first frames 17 r differ mod 4."""
    return {(3, 50): bc._Cycle((1, 2)), (2, 66): bc._Cycle((1,)), (4, 133): bc._Cycle((1, 3, 2)),
            (3, 147): bc._Cycle((1, 2)), (8, 136): bc._Cycle((1, 2, 3, 4, 6)), (2, 200): bc._Cycle((1,))}


def _build(family):
    alt = family == "alt"
    out, seen = [], set()
    variant = {f: bc._Cycle(bc.FORM_VARIANTS[f]) for f in bc.FORMS}
    shape, form, chroma = bc._Cycle(bc.SHAPES), bc._Cycle(bc.FORMS), bc._Cycle(range(4))
    colorize = bc._Cycle((True, False, False, True, True))
    content = bc._Cycle(("random", "ties", "still", "ties", "random", "still", "still"))
    place = bc._Cycle(PLACEMENTS, 3)
    still = bc._Cycle(("rank", "chunk"))
    ranks = _target_ranks()

    def add(group, layout, fo, ch, pl, co, host=False, sh=None, rank=None):
        filt, k = variant[fo]()
        r = ranks[layout]() if rank is None else rank
        if alt and pl == "last" and r + 1 == layout[0] and layout[0] > 2:
            r -= 1  # a next rank exists: its edge-1
        head = (group, layout[0], layout[1], r) + ((pl,) if alt else ())
        row = (Alt if alt else Compat)(*head, host, sh or shape(), fo, ch, filt, k, colorize(), co,
                                       still() if co == "still" else None, 1, None)
        key = case_id(row._replace(group=""))
        if key not in seen:
            seen.add(key)
            out.append(row)

    # every kernel form x chroma at 2 x (3 x 11)
    for fo in bc.FORMS:
        for ch in range(4):
            add("forms", (2, 66), fo, ch, place(), content())
    # both shapes on every kernel form at 3 x (13, 13, 13, 10)
    for fo in bc.FORMS:
        for sh in bc.SHAPES:
            add("shapes", (3, 147), fo, chroma(), place(), content(), sh=sh)
    # every content on every layout
    for layout in LAYOUTS:
        for co in bc.CONTENTS:
            add("contents", layout, form(), chroma(), place(), co)
        form()
    if alt:
        # every placement on a rank of 2 chunks, of 3 and of 4 or more, device pointers ...
        for layouts in (((3, 50), (8, 136)), ((2, 66), (4, 133)), ((3, 147), (2, 200))):
            pick = bc._Cycle(layouts)
            for pl in PLACEMENTS:
                add("placements", pick(), form(), chroma(), pl, content())
            form(), chroma()
        # ... and with host pointers, whose launches are the feeds: (2, 200) gives feeds of 25 = 13 + 12
        pick = bc._Cycle(((2, 200), (4, 133), (2, 200), (3, 50)))
        host_form = bc._Cycle(("table", "fast", "table", "spec"))
        for pl in PLACEMENTS:
            add("host", pick(), host_form(), chroma(), pl, content(), host=True)
    else:
        # host pointers: table and arithmetic kernel
        for layout in ((3, 50), (4, 133), (2, 200)):
            for fo in ("table", "fast" if layout[0] != 4 else "spec"):
                add("host", layout, fo, chroma(), None, content(), host=True)
    return out


def _build_window(family):
    """W > 1 (windows 2 and 5; table and arithmetic kernel), device pointers:
    one round per launch, and DIPS_WINDOW_BATCH_FRAMES = 20 -- rounds of 20 + 13
    (20 + 14 on the 34-frame rank of (4, 133)) inside every rank."""
    alt = family == "alt"
    out = []
    for window, chroma, filt, k, shape in ((2, 0, 0, 5.0, "whole"), (5, 2, 1, 0.7, "ragged")):
        for crosscheck in (False, True):
            fo = bc.form_of(crosscheck, filt, k)
            for layout, rank in (((2, 66), 1), ((4, 133), 3)):
                for g in (None, 20):
                    content = "ties" if window == 5 else "random"
                    if alt:
                        for pl in WINDOW_PLACEMENTS:
                            out.append(Alt("window", layout[0], layout[1], rank, pl, False, shape, fo, chroma, filt, k,
                                           True, content, None, window, g))
                    else:
                        out.append(Compat("window", layout[0], layout[1], rank, False, shape, fo, chroma, filt, k,
                                          window == 2, content, None, window, g))
    return out


ALT_CASES = _build("alt")
ALT_WINDOW_CASES = _build_window("alt")
COMPAT_CASES = _build("compat")
COMPAT_WINDOW_CASES = _build_window("compat")
