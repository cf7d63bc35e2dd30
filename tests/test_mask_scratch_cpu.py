"""CPU checks of the labelling family's scratch plan (dips_amd/csrc/
mask_scratch.h label_scratch): the frames a round takes and the byte offset of
every plane, for components / select / shapes (K = 0) and for tracks (K =
max_boxes).

A stand-alone program that includes only that header, compiled with g++, must
give on every case what run_components_device, run_select_device and
run_tracks_device of mask_abi.hip computed before the plan existed; those
formulae are restated here in Python as they stood (a chain of typed
pointers), not taken from the header.  Two layouts worked by hand pin the
formulae themselves.  No GPU."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")

PLANES = ("sum_i sum_j label0 area min_x max_x max_y parent0 parent block_count ov cprev hrank heads base next_id "
          "prev_count carry0 carry1").split()

# stdin rows: npx nslots bpf n_frames chunk K; stdout rows: F bytes and the offsets in PLANES order
_PROGRAM = r'''
#include "mask_scratch.h"
#include <cstdio>
int main() {
    long long v[6];
    for (;;) {
        for (int i = 0; i < 6; ++i)
            if (std::scanf("%lld", &v[i]) != 1) return 0;
        const dips_sched::LabelScratch p = dips_sched::label_scratch((uint64_t)v[0], (uint64_t)v[1], (uint64_t)v[2],
                                                                     (uint32_t)v[3], (uint32_t)v[4], (uint64_t)v[5]);
        const uint64_t o[] = {p.sum_i, p.sum_j, p.label0, p.area, p.min_x, p.max_x, p.max_y, p.parent0, p.parent,
                              p.block_count, p.ov, p.cprev, p.hrank, p.heads, p.base, p.next_id, p.prev_count,
                              p.carry[0], p.carry[1]};
        std::printf("%u %llu", p.F, (unsigned long long)p.bytes);
        for (uint64_t x : o) std::printf(" %llu", (unsigned long long)x);
        std::printf("\n");
    }
}
'''


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("mask_scratch")
    src = d / "mask_scratch.cpp"
    src.write_text(_PROGRAM)
    exe = d / "mask_scratch"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return exe


def geometry(w, h):
    """npx, nslots, bpf of a w x h mask (components_args of mask_abi.hip)."""
    wpf = ((w + 31) // 32) * h
    return w * h, ((w + 1) // 2) * h, (wpf + 255) // 256


def plan(exe, cases):
    """F, bytes and the offsets by plane name for cases (w, h, n_frames, chunk, K)."""
    txt = "".join(" ".join(str(x) for x in (*geometry(w, h), n, chunk, K)) + "\n" for w, h, n, chunk, K in cases)
    r = subprocess.run([str(exe)], input=txt, capture_output=True, text=True, timeout=60, check=True)
    rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return [(row[0], row[1], dict(zip(PLANES, row[2:]))) for row in rows]


SCRATCH = 1 << 30  # the budget of chunk_frames = 0
TRACKS_CHUNK = 256


def parent_layout(w, h, n, chunk, K):
    """F, bytes, {plane: (offset, size)} as the three run_*_device functions computed them."""
    npx, nslots, bpf = geometry(w, h)
    if K == 0:  # run_components_device and run_select_device, line for line alike
        per_frame = 4 * npx + 32 * nslots + 4 * bpf
        frames = chunk if chunk else max(1, SCRATCH // per_frame)
        frames = min(frames, n)
        frames = min(frames, max(1, (1 << 25) // bpf))
        F = frames
        total = per_frame * F
        sum_i = 0
        sum_j = sum_i + 8 * F * nslots
        area = sum_j + 8 * F * nslots
        min_x = area + 4 * F * nslots
        max_x = min_x + 4 * F * nslots
        max_y = max_x + 4 * F * nslots
        parent = max_y + 4 * F * nslots
        block_count = parent + 4 * F * npx
        end = block_count + 4 * F * bpf
        assert end == total
        sized = dict(sum_i=(sum_i, 8 * F * nslots), sum_j=(sum_j, 8 * F * nslots), label0=(area, 0),
                     area=(area, 4 * F * nslots), min_x=(min_x, 4 * F * nslots), max_x=(max_x, 4 * F * nslots),
                     max_y=(max_y, 4 * F * nslots), parent0=(parent, 0), parent=(parent, 4 * F * npx),
                     block_count=(block_count, 4 * F * bpf))
        # the tracks' planes: empty, at the end
        sized.update({k: (total, 0) for k in PLANES[10:]})
        return F, total, sized
    # run_tracks_device
    per_frame = 4 * npx + 32 * nslots + 4 * bpf + 4 * K * K + 8 * K + 8
    fixed = 4 * npx + 4 * nslots + 16 * K + 8
    frames = chunk if chunk else max(1, (SCRATCH - min(fixed, SCRATCH)) // per_frame)
    frames = min(frames, n)
    frames = min(frames, max(1, (1 << 25) // bpf))
    frames = min(frames, TRACKS_CHUNK)
    F = frames
    total = per_frame * F + fixed
    sum_i = 0
    sum_j = sum_i + 8 * F * nslots
    label0 = sum_j + 8 * F * nslots
    area = label0 + 4 * nslots
    min_x = area + 4 * F * nslots
    max_x = min_x + 4 * F * nslots
    max_y = max_x + 4 * F * nslots
    parent0 = max_y + 4 * F * nslots
    parent = parent0 + 4 * npx
    block_count = parent + 4 * F * npx
    ov = block_count + 4 * F * bpf
    cprev = ov + 4 * F * K * K
    hrank = cprev + 4 * F * K
    heads = hrank + 4 * F * K
    base = heads + 4 * F
    next_id = base + 4 * F
    prev_count = next_id + 4
    carry0 = prev_count + 4
    carry1 = carry0 + 4 * 2 * K
    assert carry1 + 4 * 2 * K == total
    sized = dict(sum_i=(sum_i, 8 * F * nslots), sum_j=(sum_j, 8 * F * nslots), label0=(label0, 4 * nslots),
                 area=(area, 4 * F * nslots), min_x=(min_x, 4 * F * nslots), max_x=(max_x, 4 * F * nslots),
                 max_y=(max_y, 4 * F * nslots), parent0=(parent0, 4 * npx), parent=(parent, 4 * F * npx),
                 block_count=(block_count, 4 * F * bpf), ov=(ov, 4 * F * K * K), cprev=(cprev, 4 * F * K),
                 hrank=(hrank, 4 * F * K), heads=(heads, 4 * F), base=(base, 4 * F), next_id=(next_id, 4),
                 prev_count=(prev_count, 4), carry0=(carry0, 8 * K), carry1=(carry1, 8 * K))
    return F, total, sized


REGIONS = ((1, 1), (37, 5), (64, 3), (65, 2))
CASES = [(w, h, n, chunk, K) for (w, h), n, chunk, K in
         itertools.product(REGIONS, (1, 3, 300), (0, 1, 2, 1000), (0, 1, 4, 256))]
BIG = (32767, 16384)  # wpr 1024, bpf 65536, over 2 GiB of scratch per frame
CLAMPS = [(*BIG, 1000, 1000, 0), (*BIG, 1000, 1000, 4), (*BIG, 1000, 0, 0), (*BIG, 1000, 0, 4), (37, 5, 300, 0, 1)]


def test_plan_equals_the_three_former_layouts(program):
    cases = CASES + CLAMPS
    for case, (F, total, off) in zip(cases, plan(program, cases)):
        want_F, want_total, sized = parent_layout(*case)
        assert (F, total) == (want_F, want_total), case
        assert off == {k: v[0] for k, v in sized.items()}, case
        # pairwise disjoint and inside the total
        spans = sorted((off[k], off[k] + sized[k][1]) for k in PLANES if sized[k][1])
        assert spans[0][0] == 0 and spans[-1][1] <= total, case
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), case
        assert off["sum_i"] % 8 == 0 and off["sum_j"] % 8 == 0 and all(off[k] % 4 == 0 for k in PLANES), case
        if case[4] == 0:
            # no front planes, and the layout of the components
            assert off["label0"] == off["area"] and off["parent0"] == off["parent"], case
            assert all(off[k] == total for k in PLANES[10:]), case
            npx, nslots, bpf = geometry(case[0], case[1])
            assert total == F * (4 * npx + 32 * nslots + 4 * bpf), case


def test_every_clamp_binds(program):
    got = [p[0] for p in plan(program, CLAMPS)]
    assert geometry(*BIG)[2] == 65536
    assert got[0] == 512   # the launches' block counts: 2^25 / bpf
    assert got[1] == 256   # the tracks' cap
    assert got[2] == 1 and got[3] == 1  # the 1 GiB budget holds less than one frame
    assert got[4] == 256   # the tracks' cap under the automatic budget
    # and what binds in the small cases: the clip, the chunk, the tracks' cap
    small = [(37, 5, 3, 0, 0), (37, 5, 300, 2, 4), (37, 5, 300, 1000, 0), (37, 5, 300, 1000, 256)]
    assert [p[0] for p in plan(program, small)] == [3, 2, 300, 256]


def test_two_layouts_worked_by_hand(program):
    """37 x 5: npx 185, nslots 19 * 5 = 95, bpf 1; two frames per round."""
    assert geometry(37, 5) == (185, 95, 1)
    (F0, total0, off0), (F4, total4, off4) = plan(program, [(37, 5, 6, 2, 0), (37, 5, 6, 2, 4)])
    assert (F0, total0) == (2, 7568)
    assert off0 == dict(sum_i=0, sum_j=1520, label0=3040, area=3040, min_x=3800, max_x=4560, max_y=5320, parent0=6080,
                        parent=6080, block_count=7560, ov=7568, cprev=7568, hrank=7568, heads=7568, base=7568,
                        next_id=7568, prev_count=7568, carry0=7568, carry1=7568)
    assert (F4, total4) == (2, 8968)
    assert off4 == dict(sum_i=0, sum_j=1520, label0=3040, area=3420, min_x=4180, max_x=4940, max_y=5700, parent0=6460,
                        parent=7200, block_count=8680, ov=8688, cprev=8816, hrank=8848, heads=8880, base=8888,
                        next_id=8896, prev_count=8900, carry0=8904, carry1=8936)
