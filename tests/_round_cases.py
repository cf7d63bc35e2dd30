"""The cases that make a wave of a persistent grid take several items, and the
schedule each of them runs.  There are no tests in this module:
test_round_cases_cpu.py proves the cases on the schedule header alone,
test_gpu_persistent_rounds.py runs them on the device.

Every fast regional kernel (series_mask, series_grid, series_pixels,
series_times, series_background, series_sigma_delta) and, on the mask side,
mask_vote and mask_times_kernel launch n_waves waves, at most the device's
wave slots; wave w takes items w, w + n_waves, ... of the (frame part, tile)
pairs.  With DIPS_SERIES_WAVES_PER_SIMD = 1 a device has 4 slots per CU, 1,024
on 256 CUs, and frames of 1 to 2 Mpixel give every wave two or three items.

geometry(exe, rows) asks the stand-alone program of test_sched_cpu.py
(series_sched.h alone, compiled with g++) for the schedule of a case at a slot
count; regime(q) counts its items and trips; check_schedule asserts what makes
a case worth running: the fast kernel, more items than waves, a ragged last
round, a partial last tile and, for the parts cases, consecutive items of a
wave that differ in part and tile."""
import collections
import functools
import os
import subprocess

import numpy as np

import test_sched_cpu as sched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")

CAP_ENV = "DIPS_SERIES_WAVES_PER_SIMD"
PIN_ENV = "DIPS_PIXEL_PART_FRAMES"
SLOTS_256_CUS = 4 * 256  # 4 SIMDs per CU, one wave each under the cap (series_host.h resident_at)

# The kernels' constants, restated; test_round_cases_cpu.py reads each from its header.
UNROLL_MASK = 4                  # dips_kernels.h:201 DIPS_UNROLL_MASK (kUnrollMask)
UNROLL_PIX = 2                   # dips_kernels.h:160 DIPS_UNROLL_PIX (kUnrollPix)
PIX_MAX_PART = 2048              # dips_kernels.h:163 kPixMaxPart
UNROLL_TIMES = 2                 # dips_kernels.h:242 DIPS_UNROLL_TIMES (kUnrollTimes)
TIMES_PARTS_BYTES = 1 << 30      # region_abi.hip:424 kTimesPartsBytes
UNROLL_BACKGROUND = 2            # dips_kernels.h:300 DIPS_UNROLL_BACKGROUND (kUnrollBackground)
UNROLL_SIGMA_DELTA = 4           # series_sigma_delta.h:14 DIPS_UNROLL_SIGMA_DELTA (kUnrollSigmaDelta)
UNROLL_GRID = {3: 5, 4: 4}       # series_kernels.hip:640 fast_unroll(C): dips_kernels.h:21 kUnrollV2Rgb, :20 kUnrollV2
VOTE_WORDS = 1                   # dips_kernels.h:462 DIPS_VOTE_WORDS (kVoteWords)
MASK_TIMES_PX = 8                # dips_kernels.h:504 DIPS_MASK_TIMES_PX: mask_abi.hip:458 gives a lane slot
#                                  8 / kMaskTimesPx of a mask byte, so a frame has frame_bytes * 8 / kMaskTimesPx slots
MASK_TIMES_PARTS_BYTES = 1 << 30  # mask_abi.hip:396 kMaskTimesPartsBytes

# product -> the program's product number (test_sched_cpu.py)
PROD = dict(grid=2, sums=3, mask=4, times=5, background=6, sigma_delta=7, vote=8, mask_times=9)
FRAME_SIDE = ("mask", "sums", "times", "grid", "background", "sigma_delta")

# name: of the test ids; fmts: the formats the case runs in (the mask side has
# none: 0); roi None: the whole frame; pin: DIPS_PIXEL_PART_FRAMES (0: unset);
# trips: the trips every wave makes at least (2: items > 2 n_waves); parts:
# the frames are cut; small: the models' tiles of 64 vecs; window, votes: of
# the vote.  For the mask side w x h is the mask itself.
Case = collections.namedtuple("Case", "name product w h n roi pin fmts rows cols trips parts small window votes")


def _case(name, product, w, h, n, roi=None, pin=0, fmts=(3, 4), rows=1, cols=1, trips=1, parts=False, small=False,
          window=0, votes=0):
    return Case(name, product, w, h, n, roi, pin, fmts, rows, cols, trips, parts, small, window, votes)


# The schedules in the comments are those at 1,024 slots (test_round_cases_cpu.py asserts them).
CASES = (
    # 2,130 tiles, one part, 2.08 trips: 82 waves take a third item; the frame's last vec goes to the generic kernel
    _case("mask-whole", "mask", 1931, 1117, 5, trips=2),
    # 583 tiles x 2 parts of 20 frames: a wave's second item is another part and another tile (the issue's 1001 x 601
    # region is 601 whole tiles: 970 pixels are 31 mask words a row, and the last tile is partial)
    _case("mask-parts", "mask", 1283, 857, 40, roi=(101, 90, 970, 601), parts=True),
    # 2,150 tiles, one part, 2.10 trips
    _case("sums-whole", "sums", 1283, 857, 5, trips=2),
    # 356 tiles x 6 parts of 7 frames, 2,136 items: the atomics of six parts from waves on different trips
    _case("sums-parts", "sums", 1283, 857, 40, roi=(161, 90, 601, 301), pin=7, trips=2, parts=True),
    _case("times-whole", "times", 1283, 857, 5, pin=7, trips=2),
    _case("times-parts", "times", 1283, 857, 40, roi=(161, 90, 601, 301), pin=7, trips=2, parts=True),
    # 2,146 tiles, two per cell, 2.10 trips
    _case("grid-cells", "grid", 1283, 857, 5, fmts=(4,), rows=29, cols=37, trips=2),
    # 1,008 tiles (seven per cell) x 2 parts of 20 frames, 2,016 items
    _case("grid-parts", "grid", 1283, 857, 40, fmts=(3,), rows=9, cols=16, parts=True),
    # 2,197 large tiles, 2.15 trips
    _case("background", "background", 1283, 857, 5, trips=2),
    # 2,130 large tiles, 2.08 trips
    _case("sigma-delta-large", "sigma_delta", 1931, 1117, 5, trips=2),
    # 1,428 small tiles, 1.39 trips
    _case("sigma-delta-small", "sigma_delta", 1283, 857, 5, roi=(161, 90, 601, 601), small=True),
    # 2,205 tiles, 2.15 trips
    _case("vote-whole", "vote", 3001, 1501, 8, fmts=(0,), trips=2, window=5, votes=3),
    # 550 tiles x 2 parts of 50 frames, 1,100 items
    _case("vote-parts", "vote", 1283, 857, 100, fmts=(0,), parts=True, window=5, votes=3),
    # 2,197 tiles, one part, 2.15 trips
    _case("mask-times-whole", "mask_times", 1283, 857, 5, fmts=(0,), trips=2),
    # 772 tiles x 2 parts of 20 frames, 1,544 items (857 rows are 2,197 tiles, which fill the slots: one part)
    _case("mask-times-parts", "mask_times", 1283, 301, 40, fmts=(0,), parts=True),
)

BY_NAME = {c.name: c for c in CASES}


def region(case):
    """(x, y, rw, rh) of the case's region."""
    return case.roi if case.roi is not None else (0, 0, case.w, case.h)


def unroll(case, c):
    return {"mask": UNROLL_MASK, "sums": UNROLL_PIX, "times": UNROLL_TIMES, "grid": UNROLL_GRID.get(c),
            "background": UNROLL_BACKGROUND, "sigma_delta": UNROLL_SIGMA_DELTA, "vote": VOTE_WORDS,
            "mask_times": 1}[case.product]


def mask_times_summary_bytes(case):
    """A part's summaries with times and sums together (mask_abi.hip run_mask_times_device)."""
    return 4 * (5 + 1) * case.w * case.h


def row(case, c, slots):
    """The program's input row (test_sched_cpu._IN) of a case in format c (0: the mask side) at `slots` wave
    slots: the cap leaves every kernel form one wave per SIMD, so both forms have the same slots."""
    x, y, rw, rh = region(case)
    aux = {"sums": PIX_MAX_PART, "times": TIMES_PARTS_BYTES, "vote": case.window,
           "mask_times": mask_times_summary_bytes(case)}.get(case.product, 0)
    ppv = MASK_TIMES_PX if case.product == "mask_times" else 4
    pin = MASK_TIMES_PARTS_BYTES if case.product == "mask_times" else case.pin
    return [PROD[case.product], max(c, 1), 1, case.w, case.h, case.n, x, y, rw, rh, case.rows, case.cols, ppv,
            unroll(case, c), aux, slots, slots, pin]


def build_geometry(tmp, csrc=CSRC):
    """The schedule program of test_sched_cpu.py (series_sched.h alone), compiled with g++ into `tmp`."""
    src = tmp / "round_sched.cpp"
    src.write_text(sched._PROGRAM)
    exe = tmp / "round_sched"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    return exe


FIELDS = "ok small_tile tiles_per_cell part_frames parts n_tiles n_waves tail_rows".split()
_OUT = "ok small_tile tiles_per_cell part_frames parts n_tiles n_waves blocks items vec_bytes tail_px0 tail_rows".split()


def geometry(exe, rows):
    """dicts of FIELDS for rows in test_sched_cpu._IN order."""
    out = sched._run(exe, rows)
    return [{f: int(r[_OUT.index(f)]) for f in FIELDS} for r in out]


def schedule(exe, case, c, slots):
    return geometry(exe, [row(case, c, slots)])[0]


Regime = collections.namedtuple("Regime", "items trips extra")


def regime(q):
    """items: the (part, tile) pairs of a schedule; trips: the items every
    wave takes; extra: the waves that take one more."""
    items = max(q["parts"], 1) * q["n_tiles"]
    return Regime(items, items // q["n_waves"] if q["n_waves"] else 0, items % q["n_waves"] if q["n_waves"] else 0)


def tile_slots(case, c, q):
    """(slots of the region, slots of a tile) in the kernel's own unit: vecs
    of the region rows padded to whole mask words (the mask and the models),
    vecs of the region rows (sums, times), vecs of the largest cell (grid),
    mask words (vote), lane slots (mask times)."""
    _, _, rw, rh = region(case)
    p, u = case.product, unroll(case, c)
    if p in ("mask", "background", "sigma_delta"):
        return 8 * ((rw + 31) // 32) * rh, 64 if q["small_tile"] else 64 * u
    if p in ("sums", "times"):
        return ((rw + 3) // 4) * rh, 64 * u
    if p == "grid":
        max_w, max_h = -(-rw // case.cols), -(-rh // case.rows)
        return ((max_w + 3) // 4) * max_h, 64 * u
    if p == "vote":
        return ((rw + 31) // 32) * rh, 64 * u
    return 4 * ((rw + 31) // 32) * rh * (8 // MASK_TIMES_PX), 64


def check_schedule(case, c, q, slots):
    """What makes the case worth running, asserted on its schedule q at
    `slots` wave slots; the message carries the schedule."""
    r = regime(q)
    what = f"{case.name} (format {c}) at {slots} wave slots: {q}, {r}"
    assert q["ok"] == 1, f"{what}: the generic kernel would run"
    assert q["n_waves"] <= slots, what
    assert r.items > q["n_waves"], f"{what}: no wave takes a second item"
    assert r.extra != 0, f"{what}: the last round is not ragged"
    if case.trips >= 2:
        assert r.items > 2 * q["n_waves"], f"{what}: no wave takes a third item"
    total, per_tile = tile_slots(case, c, q)
    assert total % per_tile != 0, f"{what}: the last tile is whole ({total} slots in tiles of {per_tile})"
    cells = case.rows * case.cols if case.product == "grid" else 1
    assert q["n_tiles"] == cells * -(-total // per_tile), f"{what}: not the tiles of {total} slots"
    if case.parts:
        assert q["parts"] >= 2, f"{what}: one part"
        # wave w's next item is w + n_waves: another tile unless n_tiles divides n_waves
        nt = q["n_tiles"]
        assert q["n_waves"] % nt != 0, f"{what}: a wave stays on its tile"
        w = np.arange(q["n_waves"], dtype=np.int64)
        nxt = w + q["n_waves"]
        both = (nxt < r.items) & (w // nt != nxt // nt) & (w % nt != nxt % nt)
        assert both.any(), f"{what}: no wave goes on to another part and another tile"
    else:
        assert q["parts"] <= 1, f"{what}: the frames are cut"
    assert bool(q["small_tile"]) == case.small, f"{what}: the other tile size"
    if case.product in FRAME_SIDE and case.roi is None and case.w % 4 != 0:
        assert q["tail_rows"] == 1, f"{what}: no vec at the frame's end for the generic kernel"


def header_constants(csrc=CSRC):
    """The constants above as their headers define them."""
    import re

    def read(name):
        with open(os.path.join(csrc, name)) as f:
            return f.read()

    k, sd = read("dips_kernels.h"), read("series_sigma_delta.h")
    region_abi, mask_abi, kernels = read("region_abi.hip"), read("mask_abi.hip"), read("series_kernels.hip")

    def num(txt, pattern):
        return int(re.search(pattern, txt).group(1))

    assert re.search(r"int fast_unroll\(int channels\) \{ return channels == 1 \? kUnrollGray : "
                     r"\(channels == 3 \? kUnrollV2Rgb : kUnrollV2\); \}", kernels)
    assert "constexpr uint64_t kTimesPartsBytes = 1ull << 30;" in region_abi
    assert "constexpr uint64_t kMaskTimesPartsBytes = 1ull << 30;" in mask_abi
    assert "(uint64_t)a.frame_bytes * (8 / dips::kMaskTimesPx)" in mask_abi
    return dict(UNROLL_MASK=num(k, r"#define DIPS_UNROLL_MASK (\d+)"), UNROLL_PIX=num(k, r"#define DIPS_UNROLL_PIX (\d+)"),
                PIX_MAX_PART=num(k, r"kPixMaxPart = (\d+);"), UNROLL_TIMES=num(k, r"#define DIPS_UNROLL_TIMES (\d+)"),
                UNROLL_BACKGROUND=num(k, r"#define DIPS_UNROLL_BACKGROUND (\d+)"),
                UNROLL_SIGMA_DELTA=num(sd, r"#define DIPS_UNROLL_SIGMA_DELTA (\d+)"),
                UNROLL_GRID={3: num(k, r"kUnrollV2Rgb = (\d+);"), 4: num(k, r"kUnrollV2 = (\d+);")},
                VOTE_WORDS=num(k, r"#define DIPS_VOTE_WORDS (\d+)"), MASK_TIMES_PX=num(k, r"#define DIPS_MASK_TIMES_PX (\d+)"),
                TIMES_PARTS_BYTES=1 << 30, MASK_TIMES_PARTS_BYTES=1 << 30)


# -- content -----------------------------------------------------------------------------------

CHROMAS = (0, 2)   # no filter and one other (green)
MODES = (0, 1)     # overall, per-frame
TAU = 8 / 255
TIMES_T0 = 7
BITS_DENSITY = 0.5


@functools.lru_cache(maxsize=None)
def _clip(kind, c, w, h, n):
    from test_change_mask_cpu import noise_frames
    from test_pixel_times_cpu import event_frames
    # the generators' own caches are never emptied: these clips are up to 176 MB each and go with clear_caches
    return (event_frames if kind == "event" else noise_frames).__wrapped__(c, w, h, n)


def frames_of(case, c):
    """The clip of a frame-side case: event_frames for the change times (runs
    that start and end inside the clip), noise_frames for every other one."""
    return _clip("event" if case.product == "times" else "noise", c, case.w, case.h, case.n)


def clear_caches():
    """Drops the clips and bits this module holds (the test modules call it when they are done)."""
    _clip.cache_clear()
    bits_of.cache_clear()


def ref_of(case, c):
    """The explicit reference of the change times (frame 0 changes against
    it, so a run can cross from an earlier state into the call)."""
    from test_pixel_times_cpu import event_ref
    return event_ref(c, case.w, case.h)


def crop(a, rect, lead=1):
    """The pixels of rect out of [n, h, w(, c)] frames (lead 1) or one [h, w(, c)] frame (lead 0)."""
    x, y, rw, rh = rect
    sl = (slice(None),) * lead + (slice(y, y + rh), slice(x, x + rw))
    return np.ascontiguousarray(a[sl])


@functools.lru_cache(maxsize=None)
def bits_of(case):
    """The input of a mask-side case: random bits [n, h, w] at density 0.5,
    random_bits of test_gpu_mask_stats.py frame by frame (one draw of the
    whole clip would hold a float64 per bit)."""
    from test_gpu_mask_stats import random_bits
    a = np.concatenate([random_bits.__wrapped__(1, case.h, case.w, BITS_DENSITY, seed=31 + t) for t in range(case.n)])
    a.setflags(write=False)
    return a


def check_share(bits, what):
    """Bits that exercise the compare: 5-95 % of them set."""
    share = float(np.asarray(bits, dtype=bool).mean())
    assert 0.05 < share < 0.95, (what, share)
