"""CPU checks of the frame chunks of the two batch kernels
(dips_amd/csrc/batch_chunks.h batch_chunk_plan, called by batch_steady in
compat_abi.hip and run_fast in alt_abi.hip) and of the cases
tests/test_gpu_batch_chunks.py runs at the chunk edges (tests/_batch_chunks.py).

* A stand-alone program that includes only that header, compiled with g++,
  equals the Python restatement over a sweep, and the device-independent
  form wherever its premise holds.
* The plan's properties: the chunks tile [0, n) with none empty, at most
  ceil(n / 16) of them, one for n <= 16.
* The case list meets its coverage conditions, so the GPU file cannot
  quietly lose a combination; every placement yields frames of the launch.
* The oracle alone separates the cases: for every dips_alt placement in a
  launch of 33 frames its output differs from the output with the flag at the
  chunk edge moved by one frame, so a test on that case can see an
  off-by-one."""
import os
import subprocess

import numpy as np
import pytest

import _batch_chunks as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")

# stdin rows: n n_tiles resident; stdout rows: chunk n_chunks
_PROGRAM = r'''
#include "batch_chunks.h"
#include <cstdio>
int main() {
    unsigned long long n, n_tiles, resident;
    while (std::scanf("%llu %llu %llu", &n, &n_tiles, &resident) == 3) {
        const dips_sched::BatchChunks p = dips_sched::batch_chunk_plan(n, n_tiles, resident);
        std::printf("%u %llu\n", p.chunk, (unsigned long long)p.n_chunks);
    }
    return 0;
}
'''

SWEEP_N = range(1, 601)
SWEEP_TILES = (1, 2, 4, 8, 507, 8100)
SWEEP_RESIDENT = (256, 1024, 4096, 16384)


@pytest.fixture(scope="module")
def header_plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_chunks")
    src = d / "plan.cpp"
    src.write_text(_PROGRAM)
    exe = d / "plan"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    rows = [(n, t, r) for n in SWEEP_N for t in SWEEP_TILES for r in SWEEP_RESIDENT]
    txt = "".join(f"{n} {t} {r}\n" for n, t, r in rows)
    res = subprocess.run([str(exe)], input=txt, capture_output=True, text=True, timeout=120, check=True)
    out = [tuple(int(x) for x in line.split()) for line in res.stdout.splitlines()]
    assert len(out) == len(rows)
    return dict(zip(rows, out))


def test_header_equals_the_restatement(header_plan):
    bad = [(k, v, bc.plan(*k)) for k, v in header_plan.items() if v != bc.plan(*k)]
    assert not bad, bad[:5]


def test_header_equals_the_device_independent_form_under_its_premise(header_plan):
    checked = 0
    for (n, n_tiles, resident), v in header_plan.items():
        if n_tiles * bc.ceil_div(n, 16) <= resident:
            assert v == bc.plan_small(n), (n, n_tiles, resident)
            checked += 1
    assert checked > 5000
    # the premise of the GPU tests implies that condition for every kernel form: tiles of 128 vecs or
    # more, 4 or more wave slots per compute unit
    for cus in (8, 64, 256, 304):
        for shape in bc.SHAPES.values():
            n_vec = shape[0] * shape[1] // 4
            for n in SWEEP_N:
                if bc.premise(n, n_vec, cus):
                    for vecs_per_tile, slots_per_cu in ((128, 4), (128, 32), (256, 4), (256, 16)):
                        n_tiles = bc.ceil_div(n_vec, vecs_per_tile)
                        assert bc.plan(n, n_tiles, slots_per_cu * cus) == bc.plan_small(n)


def test_plan_properties(header_plan):
    for (n, n_tiles, resident), (chunk, n_chunks) in header_plan.items():
        assert chunk >= 1 and n_chunks >= 1
        # chunks [c * chunk, min((c + 1) * chunk, n)) tile [0, n), none empty
        assert (n_chunks - 1) * chunk < n <= n_chunks * chunk, (n, n_tiles, resident)
        assert n_chunks <= bc.ceil_div(n, 16)
        if n <= 16:
            assert n_chunks == 1 and chunk == n


def test_launch_lengths_cut_as_documented():
    cuts = {m: [min(s + bc.plan_small(m)[0], m) - s for s in bc.chunk_starts(m)] for m in bc.LENGTHS}
    assert cuts == {16: [16], 17: [9, 8], 33: [11, 11, 11], 49: [13, 13, 13, 10], 100: [15] * 6 + [10]}
    # the host feeds of the GPU file: 34 frames of a 136-frame call, 29 and 36 of a 143-frame one
    assert [bc.plan_small(n) for n in (34, 29, 36, 35, 20, 9)] == [(12, 3), (15, 2), (12, 3), (12, 3), (10, 2), (9, 1)]
    for shape, n_vec in (("whole", 512), ("ragged", 253)):
        w, h = bc.SHAPES[shape]
        assert w * h % 4 == 0 and w * h // 4 == n_vec and w * h * 4 % 16 == 0 and w * h * 4 <= 8192
    assert 253 % 128 != 0 and 253 < 256 and 512 % 256 == 0


def test_case_list_meets_the_coverage_conditions():
    assert len(set(bc.CASES)) == len(bc.CASES) and len({bc.case_id(c) for c in bc.CASES}) == len(bc.CASES)
    for family in ("alt", "compat"):
        rows = [c for c in bc.CASES if c[0] == family]
        assert 30 <= len(rows) <= 90
        for (_, shape, m, form, chroma, filt, k, colorize, pl, content) in rows:
            assert shape in bc.SHAPES and m in bc.LENGTHS and chroma in range(4) and content in bc.CONTENTS
            # the form the row names is the one the library picks for its parameters
            assert form == "table" or bc.form_of(True, filt, k) == form
            assert (pl in bc.PLACEMENTS) if family == "alt" else pl is None
            if m == 16:
                assert pl not in bc.EDGE_PLACEMENTS and content != "still"
        # every kernel form x chroma 0..3 at some m >= 33
        assert {(c[3], c[4]) for c in rows if c[2] >= 33} == {(f, ch) for f in bc.FORMS for ch in range(4)}
        # both shapes on every kernel form at m = 49
        assert {(c[1], c[3]) for c in rows if c[2] == 49} == {(s, f) for s in bc.SHAPES for f in bc.FORMS}
        # every content at every m >= 17; the control at m = 16 on every form
        assert {(c[2], c[9]) for c in rows if c[2] >= 17} == {(m, co) for m in bc.LENGTHS[1:] for co in bc.CONTENTS}
        assert {c[3] for c in rows if c[2] == 16} == set(bc.FORMS)
        # both filters of each arithmetic epilogue, colour and gray on every form
        assert {(c[3], c[5], c[6]) for c in rows} >= {(f, *v) for f in ("fast", "spec") for v in bc.FORM_VARIANTS[f]}
        assert {(c[3], c[7]) for c in rows} == {(f, col) for f in bc.FORMS for col in (False, True)}
    # dips_alt: every placement at every m >= 17, each of them on every kernel form somewhere
    alt = [c for c in bc.CASES if c[0] == "alt"]
    assert {(c[2], c[8]) for c in alt if c[2] >= 17} == {(m, p) for m in bc.LENGTHS[1:] for p in bc.PLACEMENTS}
    assert {c[3] for c in alt if c[8] in bc.EDGE_PLACEMENTS} == set(bc.FORMS)


def test_placements_yield_frames_of_the_launch():
    for m in bc.LENGTHS:
        starts = bc.chunk_starts(m)
        for name in bc.PLACEMENTS:
            if m == 16 and name in bc.EDGE_PLACEMENTS:
                with pytest.raises(ValueError):
                    bc.placement(name, m)
                continue
            at = bc.placement(name, m)
            assert at == sorted(set(at)) and all(0 <= t < m for t in at), (m, name, at)
            moved = bc.moved_by_one(name, m)
            assert moved != at and all(0 <= t < m for t in moved)
        if m == 16:
            continue
        t0 = bc.middle_start(m)
        assert t0 in starts[1:]
        assert bc.placement("before_edge", m) == [t0 - 1] and bc.placement("on_edge", m) == [t0]
        assert bc.placement("both_edge", m) == [t0 - 1, t0] and bc.placement("last_chunk_start", m) == [starts[-1]]
        assert len(bc.placement("random", m)) >= 1
        # the held frame of the `still` clips lies inside the launch
        f = bc.make_frames("ragged", m, "still", 1, still_at=t0)
        assert all(np.array_equal(f[t], f[t0]) for t in range(t0 - 2, t0 + 2))
        assert not np.array_equal(f[t0 - 3], f[t0]) and not np.array_equal(f[t0 + 2], f[t0])
    ties = bc.make_frames("whole", 3, "ties", 2)
    assert set(np.unique(ties).tolist()) == {0, 1, 2, 128, 255}


@pytest.mark.parametrize("content", bc.CONTENTS)
@pytest.mark.parametrize("name", bc.PLACEMENTS)
def test_oracle_separates_a_flag_moved_by_one_frame(name, content):
    """The launch of 33 frames and the 5 unflagged frames after it (they show
    the snapshot the launch left)."""
    from oracle import oracle
    m, tail = 33, 5
    frames = bc.make_frames("ragged", m + tail, content, 77, still_at=bc.middle_start(m))
    outs = []
    for at in (bc.placement(name, m), bc.moved_by_one(name, m)):
        flags = np.concatenate([bc.flags_of(at, m), np.zeros(tail, dtype=bool)])
        outs.append(bc.oracle_alt(oracle, "ragged", True, 1, 5.0, 0, 0, frames, flags))
    assert not np.array_equal(outs[0], outs[1])
