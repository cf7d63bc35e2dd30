"""The cases of tests/_round_cases.py are not vacuous, shown without a GPU on
the schedule header alone (series_sched.h through the stand-alone program of
test_sched_cpu.py).  At 1,024 wave slots -- 256 CUs under
DIPS_SERIES_WAVES_PER_SIMD = 1 -- every case runs its fast kernel, gives its
waves more than one item (more than two where the case says so), ends on a
ragged round and a partial tile, and the parts cases send a wave on to
another part and another tile (check_schedule).  The schedules recorded in
the comments of CASES are asserted figure by figure.

The other half of the argument: without the cap, at the 4,096 or 8,192 slots
the kernels have, the shapes the suite had before run one item per wave.  If
the schedule rule changes, these assertions say so.

The content is checked too, on a band of rows of every clip: the change mask
the products are built on has 5-95 % of its bits set from frame 1 on, and the
clips of the change times have runs that cross a part boundary in at least
10 % of the pixels."""
import numpy as np
import pytest

import _round_cases as rc
from test_change_mask_cpu import py_change_mask, unpack_mask
from test_pixel_times_cpu import crossing_share

SLOTS = rc.SLOTS_256_CUS
BAND_ROWS = 24  # the rows of a region the content checks look at


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return rc.build_geometry(tmp_path_factory.mktemp("round_cases"))


@pytest.fixture(scope="module", autouse=True)
def _drop_the_clips():
    yield
    rc.clear_caches()


def test_constants_are_those_of_the_headers():
    for name, value in rc.header_constants().items():
        assert getattr(rc, name) == value, name


def test_cases_are_the_issue_s_products_and_forms():
    assert {c.product for c in rc.CASES} == set(rc.PROD)
    assert len(rc.BY_NAME) == len(rc.CASES)
    for product in rc.PROD:
        mine = [c for c in rc.CASES if c.product == product]
        if product != "background":  # one part always, and one tile size at these shapes
            assert len(mine) == 2
        assert any(c.trips >= 2 for c in mine), product
    for product in ("mask", "sums", "times", "grid", "vote", "mask_times"):
        assert [c.parts for c in rc.CASES if c.product == product] == [False, True], product
    assert [c.small for c in rc.CASES if c.product == "sigma_delta"] == [False, True]


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_case_takes_several_items_per_wave(program, case):
    for c in case.fmts:
        rc.check_schedule(case, c, rc.schedule(program, case, c, SLOTS), SLOTS)


# name: (n_tiles, parts, part_frames, items, waves that take one more item)
RECORDED = {
    "mask-whole": (2130, 1, 5, 2130, 82),
    "mask-parts": (583, 2, 20, 1166, 142),
    "sums-whole": (2150, 1, 5, 2150, 102),
    "sums-parts": (356, 6, 7, 2136, 88),
    "times-whole": (2150, 1, 5, 2150, 102),
    "times-parts": (356, 6, 7, 2136, 88),
    "grid-cells": (2146, 1, 5, 2146, 98),
    "grid-parts": (1008, 2, 20, 2016, 992),
    "background": (2197, 0, 0, 2197, 149),
    "sigma-delta-large": (2130, 0, 0, 2130, 82),
    "sigma-delta-small": (1428, 0, 0, 1428, 404),
    "vote-whole": (2205, 1, 8, 2205, 157),
    "vote-parts": (550, 2, 50, 1100, 76),
    "mask-times-whole": (2197, 1, 5, 2197, 149),
    "mask-times-parts": (772, 2, 20, 1544, 520),
}


def test_recorded_schedules_at_1024_slots(program):
    assert set(RECORDED) == set(rc.BY_NAME)
    for name, want in RECORDED.items():
        case = rc.BY_NAME[name]
        for c in case.fmts:
            q = rc.schedule(program, case, c, SLOTS)
            r = rc.regime(q)
            assert (q["n_tiles"], q["parts"], q["part_frames"], r.items, r.extra) == want, (name, c, q, r)
            assert q["n_waves"] == SLOTS and r.trips == (2 if case.trips >= 2 else 1)
    assert rc.schedule(program, rc.BY_NAME["grid-cells"], 4, SLOTS)["tiles_per_cell"] == 2
    assert rc.schedule(program, rc.BY_NAME["grid-parts"], 3, SLOTS)["tiles_per_cell"] == 7


def test_the_shapes_the_suite_had_run_one_item_per_wave(program):
    """The largest regional shapes of the other test files, at the slots the
    kernels have without the cap (4 or 8 waves per SIMD on 256 CUs) and, for
    the two test_large_tiles, under the cap."""
    hd_mask = rc._case("hd", "mask", 1280, 720, 5)                    # test_gpu_change_mask: ..._products_hd
    hd_grid = rc._case("full-hd", "grid", 1920, 1080, 12, rows=9, cols=16)  # test_gpu_grid: test_full_hd_heat_map
    vote_4k = rc._case("4k", "vote", 3840, 2160, 8, window=5, votes=3)  # test_gpu_mask_vote: test_4k_frames
    bg_large = rc._case("large", "background", 1021, 400, 5)          # test_gpu_background: test_large_tiles
    sd_large = rc._case("large", "sigma_delta", 1021, 520, 5)         # test_gpu_sigma_delta: test_large_tiles
    for slots in (4096, 8192):
        for case, c in ((hd_mask, 3), (hd_grid, 3), (vote_4k, 0), (bg_large, 3), (sd_large, 3)):
            q = rc.schedule(program, case, c, slots)
            assert q["ok"] == 1 and rc.regime(q).items <= q["n_waves"], (case.name, case.product, slots, q)
    assert rc.schedule(program, hd_mask, 3, 4096)["n_tiles"] == 900
    for case in (bg_large, sd_large):
        q = rc.schedule(program, case, 3, SLOTS)
        assert q["ok"] == 1 and not q["small_tile"] and rc.regime(q).items <= q["n_waves"], (case.product, q)
    assert rc.schedule(program, bg_large, 3, SLOTS)["n_tiles"] == 800


def _band(case):
    """The first BAND_ROWS rows of the case's region."""
    x, y, rw, rh = rc.region(case)
    return x, y, rw, min(rh, BAND_ROWS)


@pytest.mark.parametrize("case", [c for c in rc.CASES if c.product in rc.FRAME_SIDE], ids=lambda c: c.name)
def test_frame_side_content_sets_and_clears_bits(case):
    """py_change_mask of a band of the clip, every format, mode and chroma the GPU test runs."""
    band = _band(case)
    for c in case.fmts:
        frames = rc.crop(rc.frames_of(case, c), band)
        for mode in rc.MODES:
            for chroma in rc.CHROMAS:
                bits = unpack_mask(py_change_mask(frames, mode, rc.TAU, chroma), band[2])
                rc.check_share(bits[1:], (case.name, c, mode, chroma))
                if case.product == "times" and case.parts:
                    assert crossing_share(bits, case.pin) >= 0.10, (case.name, c, mode, chroma)
                if case.product == "times":  # against the explicit reference frame 0 changes too
                    ref = rc.crop(rc.ref_of(case, c), band, lead=0)
                    first = unpack_mask(py_change_mask(frames[:1], mode, rc.TAU, chroma, ref), band[2])
                    rc.check_share(first, (case.name, c, mode, chroma, "frame 0"))


@pytest.mark.parametrize("case", [c for c in rc.CASES if c.product not in rc.FRAME_SIDE], ids=lambda c: c.name)
def test_mask_side_content_sets_and_clears_bits(case):
    bits = rc.bits_of(case)[:, :BAND_ROWS]
    rc.check_share(bits, case.name)
    if case.product == "mask_times" and case.parts:
        q_frames = RECORDED[case.name][2]
        assert crossing_share(bits, q_frames) >= 0.10
    if case.product == "vote":
        import _vote_ref as vref
        voted, _ = vref.vote_bits(bits, case.window, case.votes)
        rc.check_share(voted[case.window:], (case.name, "voted"))
