"""The cases of tests/_reuse_cases.py are what they claim, shown without a GPU.

Scratch plans, on mask_scratch.h alone (the stand-alone program of
test_mask_scratch_cpu.py): for every (dirt, call under test) pair the dirt's
plan has at least the bytes of every plan the call makes, so the call runs
wholly inside bytes the dirt owned, and at least one plane lies at another
offset, so it finds planes of another kind under its own.

The second trip of the two looped grids: both logic cases have more words
than kMaxBlocks blocks of 256 threads hold (kMaxBlocks read from
mask_select.hip), end on a ragged trip and move r, the word's index in its
frame, from trip to trip; every counts case has at least 2 * resident + 1
items, more than the blocks launched, at 256, 2,048 and 8,192 resident blocks (series_sched.h mask_counts_geometry
through _mask_stats_ref.counts_geometry), one band on the plain-store path and
several column chunks where the case says so."""
import os

import pytest

import _mask_stats_ref as sref
import _reuse_cases as rc
import test_mask_scratch_cpu as scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")

program = scratch.program  # the fixture: mask_scratch.h alone, compiled with g++


def test_cases_cover_the_arguments_of_every_product():
    assert len(rc.BY_NAME) == len(rc.CALLS)
    assert {(c.w, c.h) for c in rc.CALLS} == {(w, h) for w in (33, 65, 97) for h in (5, 29)}
    assert {c.n for c in rc.CALLS} == {1, 7}

    def values(product, key):
        return {rc.kw_of(c)[key] for c in rc.CALLS if c.product == product}

    assert values("components", "labels") == {True, False} and values("components", "max_boxes") == {0, 3, 64}
    assert values("components", "chunk_frames") == {0, 1, 3} and values("components", "connectivity") == {4, 8}
    assert values("components", "min_area") == {1, 4}
    assert values("shapes", "weights") == {True, False}
    assert values("tracks", "max_boxes") == {1, 8, 256} and values("tracks", "chunk_frames") == {0, 2}
    assert values("tracks", "mode") == {"none", "state", "carried"}
    assert values("select", "marker") == {None, "1", "n"} and values("select", "counts") == {True, False}
    assert values("select", "clear_border") == {True, False} and values("select", "dropped") == {True, False}
    assert {c.product for c in rc.CALLS} == {"components", "shapes", "tracks", "select", "fill_holes"}


@pytest.mark.parametrize("kind", rc.DIRTS)
def test_every_call_runs_inside_its_dirt_at_other_offsets(program, kind):
    for call in rc.CALLS:
        shape = rc.dirt_shape(kind, call)
        assert shape[0] != call.w and shape[2] > call.n, (call.name, shape)
        cases = rc.plan_cases(call)
        plans = scratch.plan(program, [rc.dirt_plan_case(kind, shape)] + cases)
        (_, dirt_bytes, dirt_off), mine = plans[0], plans[1:]
        assert dirt_bytes == rc.plan_bytes(rc.dirt_plan_case(kind, shape))
        for case, (_, total, off) in zip(cases, mine):
            assert total == rc.plan_bytes(case), (call.name, case)
            assert dirt_bytes >= total, (call.name, kind, shape, dirt_bytes, total)
            used = [k for k in scratch.PLANES if k in ("sum_j", "area", "min_x", "max_x", "max_y", "parent", "block_count")]
            assert any(off[k] != dirt_off[k] for k in used), (call.name, kind)
            # and the planes the call reads lie on bytes that held another plane of the dirt
            assert off["parent"] != dirt_off["parent"] and off["area"] != dirt_off["area"], (call.name, kind)


def test_logic_cases_take_a_second_ragged_trip_that_moves_r():
    max_blocks = rc.logic_max_blocks(CSRC)
    assert max_blocks == 1 << 15
    got = {}
    for name, w, h, n in rc.LOGIC_CASES:
        g = rc.logic_geometry(w, h, n, max_blocks)
        assert g["words"] > max_blocks * rc.LOGIC_THREADS, name
        assert g["words"] % (max_blocks * rc.LOGIC_THREADS) != 0, name
        assert g["stride"] == max_blocks * rc.LOGIC_THREADS and g["dr"] != 0, name
        assert g["wpf"] < 1 << 30, name   # launch_mask_logic's limit
        got[name] = g
    many, long_ = got["many-frames"], got["long-frame"]
    assert (many["wpf"], many["words"], many["dr"]) == (32000, 9600000, 4608)
    assert 1000 % 32 == 8 and many["wpf"] % many["dr"] != 0   # a pad mask to place; r wraps elsewhere on every trip
    assert long_["wpf"] == 8413200 and long_["wpf"] > long_["stride"] and long_["dr"] == long_["stride"]
    # the largest logic case the suite had: one trip
    old = rc.logic_geometry(33, 1, 70000, max_blocks)
    assert old["words"] == 140000 and old["words"] <= max_blocks * rc.LOGIC_THREADS


def test_counts_cases_have_more_items_than_blocks(tmp_path):
    exe = sref.build_geometry(tmp_path, CSRC)
    _, chunk_cells, min_band_words = sref.kernel_constants(CSRC)
    for resident in (256, 2048, 8192):
        qs = sref.counts_geometry(exe, rc.counts_rows(rc.COUNTS_CASES, chunk_cells, min_band_words, resident))
        for case, q in zip(rc.COUNTS_CASES, qs):
            rc.check_counts_geometry(case, q, resident)
            assert q["blocks"] == 2 * resident and q["bands"] == 1
    items = [q["items"] for q in qs]
    assert items == [51200, 256 * 67, 49152] and qs[2]["col_chunks"] == 3
    # the largest counts call the suite had gives every block one item at most
    old = sref.counts_geometry(exe, [(100, 17, 3, 7, 7, chunk_cells, min_band_words, 256)])[0]
    assert old["items"] <= old["blocks"]
