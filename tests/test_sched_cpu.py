"""CPU checks of the schedule header (dips_amd/csrc/series_sched.h): how many
waves every series and regional launch runs and how its frames are cut.

* A stand-alone program that includes only that header, compiled with g++,
  must give on every row of tests/golden/sched_parent.npz every field that
  row records.  The table was recorded from the geometry functions
  series_abi.hip held before the header existed (compiled unchanged around a
  stub handle and a stubbed occupancy query); a field the struct of that
  function did not have is -1 and is not compared.  Inputs: product (0 series
  RGB8 / RGBA8 / f32 GRAY8, 1 GRAY8 table, 2 grid, 3 pixel sums, 4 mask, 5
  times, 6 background, 7 Sigma-Delta), frame, frame count, region, grid, the
  resident wave slots of the one or two kernel forms (from CUs x waves per
  SIMD under the DIPS_SERIES_WAVES_PER_SIMD cap), the DIPS_PIXEL_PART_FRAMES
  pin, and the kernels' constants (pixels per vec, vecs per lane, kPixMaxPart /
  the summaries' byte budget / the table kernel's waves per group).  Two more
  products, not in the table, serve tests/_round_cases.py: 8 the vote on a
  mask rw x rh (unroll: words per lane, aux: the window), 9 the times and sums
  of a mask (ppv: pixels per lane slot, aux: a part's summary bytes, pin: the
  summaries' byte budget).
* The schedules the project has recorded, at 4,096 wave slots.
* tests/_sched.py part_schedule agrees with the header on the series rows."""
import os
import subprocess

import numpy as np
import pytest

from _sched import part_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "sched_parent.npz")

# stdin rows: prod C per_frame width height n_frames roi_x roi_y roi_w roi_h
# rows cols ppv unroll aux res_a res_b pin; stdout rows: the fixture's outputs
_PROGRAM = r'''
#include "series_sched.h"
#include <cstdio>
using namespace dips_sched;
int main() {
    long long v[18];
    for (;;) {
        for (int i = 0; i < 18; ++i)
            if (std::scanf("%lld", &v[i]) != 1) return 0;
        const int prod = (int)v[0], C = (int)v[1];
        const bool pf = v[2] != 0;
        const uint32_t width = (uint32_t)v[3], height = (uint32_t)v[4], n = (uint32_t)v[5];
        const uint32_t rx = (uint32_t)v[6], ry = (uint32_t)v[7], rw = (uint32_t)v[8], rh = (uint32_t)v[9];
        const uint32_t rows = (uint32_t)v[10], cols = (uint32_t)v[11];
        const int ppv = (int)v[12], unroll = (int)v[13];
        const uint64_t aux = (uint64_t)v[14], res_a = (uint64_t)v[15], res_b = (uint64_t)v[16], pin = (uint64_t)v[17];
        const uint64_t fb = (uint64_t)width * height * (uint64_t)C;
        auto two = [&](bool first) { return first ? res_a : res_b; };
        Geom q;
        FastGeom f;
        switch (prod) {
            case 0: q = f = fast_geometry(width, height, n, C, ppv, unroll, res_a); break;
            case 1: q = f = gray_lut_geometry(width, height, n, unroll, (uint32_t)aux, pf, res_a); break;
            case 2: q = grid_geometry(fb, n, unroll, rw, rh, rows, cols, res_a); break;
            case 3: q = pix_geometry(fb, n, unroll, rw, rh, res_a, (uint32_t)aux, pin); break;
            case 4: q = mask_geometry(fb, n, unroll, rw, rh, res_a); break;
            case 5: q = times_geometry(fb, n, unroll, rw, rh, aux, pin, two); break;
            case 8: q = vote_geometry(mask_words_per_row(rw) * rh, n, (uint32_t)aux, unroll, res_a); break;
            case 9: {
                // as run_mask_times_device asks: the several-parts form first, then the one-part form's slots
                const uint64_t slots = 4u * mask_words_per_row(rw) * rh * (8u / (uint64_t)ppv);
                q = mask_times_geometry(slots, n, aux, pin, res_a);
                if (q.ok && q.parts == 1u) q = mask_times_geometry(slots, n, aux, 0u, res_b);
                break;
            }
            default: q = background_geometry(fb, n, unroll, rw, rh, [&](bool small) { return two(!small); }); break;
        }
        int tail_rows = 0;
        for_frame_end_tail_rows(width, height, rx, ry, rw, rh, [&](uint32_t, uint32_t) { ++tail_rows; return 0; });
        std::printf("%d %d %u %u %u %llu %llu %llu %llu %llu %llu %d\n", (int)q.ok, (int)q.small_tile, q.tiles_per_cell,
                    q.part_frames, q.parts, (unsigned long long)q.n_tiles, (unsigned long long)q.n_waves,
                    (unsigned long long)q.blocks, (unsigned long long)f.items, (unsigned long long)f.vec_bytes,
                    (unsigned long long)f.tail_px0, tail_rows);
    }
}
'''

_IN = "prod C per_frame width height n_frames roi_x roi_y roi_w roi_h rows cols ppv unroll aux res_a res_b pin".split()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("sched")
    src = d / "sched.cpp"
    src.write_text(_PROGRAM)
    exe = d / "sched"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return exe


def _run(exe, rows):
    """The program's output fields for input rows given as dicts or sequences in _IN order."""
    txt = "".join(" ".join(str(int(x)) for x in r) + "\n" for r in rows)
    r = subprocess.run([str(exe)], input=txt, capture_output=True, text=True, timeout=120, check=True)
    out = np.array([[int(x) for x in line.split()] for line in r.stdout.splitlines()], dtype=np.int64)
    assert out.shape[0] == len(rows)
    return out


@pytest.fixture(scope="module")
def table():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return z["inputs"], z["outputs"], z["in_cols"].tolist(), z["out_cols"].tolist()


def test_fixture_covers_what_it_should(table):
    inputs, outputs, in_cols, _ = table
    assert inputs.shape[0] <= 4000 and os.path.getsize(FIXTURE) <= 104780
    col = {c: inputs[:, i] for i, c in enumerate(in_cols)}
    assert set(col["prod"].tolist()) == set(range(8))
    assert {(cu, occ, cap) for cu, occ, cap in zip(col["cu"].tolist(), col["occ_a"].tolist(), col["cap"].tolist())} >= {
        (cu, occ, cap) for cu in (8, 64, 256, 304) for occ in range(1, 9) for cap in (0, 1, 2)}
    assert set(col["n_frames"].tolist()) >= {1, 2, 15, 16, 31, 32, 37, 255, 256, 257, 300, 520, 523, 1000, 1250, 1251,
                                             5000, 2 ** 28 - 1, 2 ** 28}
    assert set(col["pin"].tolist()) >= {0, 1, 16, 2048, 2049}
    huge = col["width"] * col["height"] * col["C"] >= 2 ** 31
    assert set(col["C"][huge].tolist()) == {1, 3, 4} and not outputs[huge, 0].any()


def test_every_field_equals_the_recorded_table(program, table):
    inputs, outputs, in_cols, out_cols = table
    assert out_cols == "ok small_tile tiles_per_cell part_frames parts n_tiles n_waves blocks items vec_bytes tail_px0 tail_rows".split()
    got = _run(program, inputs[:, [in_cols.index(c) for c in _IN]])
    recorded = outputs >= 0  # -1: the recorded function had no such field
    bad = np.argwhere((got != outputs) & recorded)
    assert bad.size == 0, [(inputs[i].tolist(), out_cols[j], int(got[i, j]), int(outputs[i, j])) for i, j in bad[:5]]


def _row(prod, C, pf, width, height, n, roi=None, unroll=5, aux=0, res_a=4096, res_b=4096, pin=0):
    x, y, w, h = roi or (0, 0, width, height)
    return [prod, C, pf, width, height, n, x, y, w, h, 1, 1, 4, unroll, aux, res_a, res_b, pin]


def test_recorded_schedules_at_4096_slots(program):
    F = dict(ok=0, part_frames=3, parts=4, n_tiles=5, n_waves=6)
    # 4K RGB8, 5,000 frames, per-frame: L = 1000, 4,050 waves; 1080p RGB8, 523 frames: 4 parts of 131, the last 130
    bench, parity = _run(program, [_row(0, 3, 1, 3840, 2160, 5000), _row(0, 3, 1, 1920, 1080, 523)])
    assert bench[F["ok"]] == 1 and bench[F["part_frames"]] == 1000 and bench[F["n_waves"]] == 4050
    assert parity[F["part_frames"]] == 131 and 523 - 3 * 131 == 130 and -(-523 // 131) == 4
    # a 96x64 region of a 4K frame: 6 to 24 tiles, far fewer than the slots.  The mask (unroll 4), the
    # pixel sums (unroll 2, kPixMaxPart 2048) and the change times (unroll 2, 2^30 bytes of summaries)
    roi = (100, 100, 96, 64)
    for prod, unroll, aux in ((4, 4, 0), (3, 2, 2048), (5, 2, 2 ** 30)):
        n31, n37, n300 = _run(program, [_row(prod, 3, 1, 3840, 2160, n, roi, unroll, aux) for n in (31, 37, 300)])
        assert n31[F["ok"]] == 1 and n31[F["parts"]] == 1 and n31[F["part_frames"]] == 31
        assert n37[F["part_frames"]] == 19 and n37[F["parts"]] == 2  # 19 and 18
        assert n300[F["part_frames"]] == 17 and n300[F["parts"]] == 18 and 300 - 17 * 17 == 11


def test_part_schedule_restatement_agrees_on_the_series_rows(program, table):
    inputs, _, in_cols, _ = table
    col = {c: i for i, c in enumerate(in_cols)}
    rows = inputs[(inputs[:, col["prod"]] <= 1)]
    got = _run(program, rows[:, [col[c] for c in _IN]])
    checked = 0
    for r, g in zip(rows.tolist(), got.tolist()):
        ok, part_frames, n_tiles, n_waves = g[0], g[3], g[5], g[6]
        parts_apply = r[col["C"]] in (3, 4) if r[col["prod"]] == 0 else r[col["per_frame"]] == 1
        if not ok or not parts_apply:
            continue
        sch = part_schedule(n_tiles, r[col["n_frames"]], r[col["res_a"]])
        if sch is None:
            assert part_frames == 0 and n_waves == min(n_tiles * r[col["n_frames"]], r[col["res_a"]])
        else:
            assert (part_frames, n_waves) == (sch[0], sch[2])
            checked += 1
    assert checked > 100
