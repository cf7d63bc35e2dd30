"""CPU checks of the slot geometry the regional kernels and their host walks
share (dips_amd/csrc/series_slots.h, series_sched.h).  region_slot is what
the grid, pixel-sums and change-times kernels call, region_word_slot what the
background and Sigma-Delta kernels call, with the arguments used here; the
mask kernel has region_word_slot's arithmetic written out and calls only
vec_crosses_frame_end and slot_word_bits ("The regional skeleton").
A stand-alone program that includes only those HIP-free headers, compiled with
g++, enumerates the slots of every tile as the kernels do -- flat vec
v0 + 64 u + lane of tile v0 / (64 U) -- exhaustively over frames 1..12 x 1..5,
every region inside the frame, C in {3, 4} and U in {1, 2, 4}, in the flat and
in the word-padded layout, and checks

1. coverage: every region pixel lies in exactly one slot's `left` pixels and
   no pixel outside the region is counted;
2. frame end: every `ok` slot has off + 4 C <= frame bytes;
3. the `in && !ok` slots are exactly the (row, i0) pairs
   for_frame_end_tail_rows visits;
4. for grids of up to 3 x 3 cells over the region, the left-out slots of the
   cells are exactly the tails for_grid_frame_end_tails visits;
5. padded layout: the 8 slots of a group are lanes 8 g .. 8 g + 7 of one slot
   index u, their word is idx >> 3, words x 4 = row bytes x h, and the pad
   bits of the slots' word bits beyond w are 0.

The program prints the number of cases it checked, or the first failure."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")

_PROGRAM = r'''
#include "series_sched.h"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
using namespace dips_sched;

struct Rect { uint32_t x, y, w, h; };
typedef std::set<std::pair<uint32_t, uint32_t>> Pairs;

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::printf("FAIL %s line %d: W %u H %u roi %u %u %u %u C %u U %u\n", #cond, __LINE__, W, \
                        H, rc.x, rc.y, rc.w, rc.h, C, U);                                             \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

// the split grid_cell_rect (dips_kernels.h) makes of a region
static uint32_t edge(uint32_t x0, uint32_t extent, uint32_t n, uint32_t i) {
    return x0 + (uint32_t)((uint64_t)i * extent / n);
}
static Rect cell_of(const Rect& g, uint32_t rows, uint32_t cols, uint32_t r, uint32_t c) {
    Rect q;
    q.x = edge(g.x, g.w, cols, c);
    q.y = edge(g.y, g.h, rows, r);
    q.w = edge(g.x, g.w, cols, c + 1) - q.x;
    q.h = edge(g.y, g.h, rows, r + 1) - q.y;
    return q;
}

// The slots of every tile of `rc`, flat (padded false) or word-padded, as the
// kernels enumerate them; fills the per-pixel counts and the left-out set.
static void walk(uint32_t W, uint32_t H, const Rect& rc, uint32_t C, uint32_t U, bool padded,
                 std::vector<int>& count, Pairs& left_out) {
    const uint32_t fb = W * H * C;
    const uint32_t vpr = padded ? word_vpr(rc.w) : flat_vpr(rc.w);
    const uint32_t nvec = vpr * rc.h;
    const uint32_t n_tiles = (nvec + 64 * U - 1) / (64 * U);
    if (padded) CHECK((uint64_t)(nvec >> 3) * 4u == mask_words_per_row(rc.w) * 4u * rc.h && nvec % 8u == 0u);
    for (uint32_t tile = 0; tile < n_tiles; ++tile) {
        for (uint32_t u = 0; u < U; ++u) {
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t idx = tile * 64 * U + u * 64 + lane;
                Slot s;
                if (padded) {
                    const WordSlot q = region_word_slot(rc, vpr, nvec, W, C, fb, idx);
                    s = q;
                    // the group's 8 lanes share one slot index u and one word
                    const uint32_t word = idx >> 3;  // what the kernels store to
                    CHECK((idx & 7u) == (lane & 7u) && ((idx & ~7u) >> 3) == word && ((idx | 7u) >> 3) == word);
                    if (q.in) CHECK(q.r * (vpr >> 3) + (q.x4 >> 5) == word && idx < nvec);
                    // the slot's bits of its word: inside the region's columns only
                    const uint32_t bits = slot_word_bits(q.left, 4u * (lane & 7u));
                    for (uint32_t b = 0; b < 32; ++b) {
                        const uint32_t col = (q.x4 & ~31u) + b;
                        if ((bits >> b) & 1u) CHECK(q.in && col < rc.w && col >= q.x4 && col < q.x4 + 4u);
                    }
                } else {
                    s = region_slot(rc, vpr, nvec, W, C, fb, idx);
                    CHECK(s.in == (idx < nvec));
                }
                CHECK(s.voff == (s.ok ? s.off : kNoSlot));
                if (!s.in) {
                    CHECK(s.left == 0u && !s.ok);
                    continue;
                }
                CHECK(s.r < rc.h && s.x4 < rc.w && s.left >= 1u && s.left <= 4u && s.left == vec_px_inside(rc.w, s.x4));
                CHECK(s.off == ((rc.y + s.r) * W + rc.x + s.x4) * C);
                if (s.ok) CHECK(s.off + 4u * C <= fb);
                else CHECK(s.off + 4u * C > fb);
                if (!s.ok) CHECK(left_out.insert({s.r, s.x4}).second);
                for (uint32_t p = 0; p < s.left; ++p) ++count[(rc.y + s.r) * W + rc.x + s.x4 + p];
            }
        }
    }
}

int main() {
    unsigned long long cases = 0;
    for (uint32_t W = 1; W <= 12; ++W)
    for (uint32_t H = 1; H <= 5; ++H)
    for (uint32_t x = 0; x < W; ++x)
    for (uint32_t y = 0; y < H; ++y)
    for (uint32_t w = 1; x + w <= W; ++w)
    for (uint32_t h = 1; y + h <= H; ++h)
    for (uint32_t C = 3; C <= 4; ++C)
    for (uint32_t U = 1; U <= 4; U *= 2) {
        const Rect rc{x, y, w, h};
        // what the host hands to the generic kernel for one region
        Pairs tails;
        for_frame_end_tail_rows(W, H, x, y, w, h, [&](uint32_t r, uint32_t i0) { tails.insert({r, i0}); return 0; });
        for (int padded = 0; padded < 2; ++padded) {
            std::vector<int> count(W * H, 0);
            Pairs left_out;
            walk(W, H, rc, C, U, padded != 0, count, left_out);
            for (uint32_t py = 0; py < H; ++py)
                for (uint32_t px = 0; px < W; ++px)
                    CHECK(count[py * W + px] == (px >= x && px < x + w && py >= y && py < y + h ? 1 : 0));
            CHECK(left_out == tails);
            ++cases;
        }
        // grids of cells over the region: every cell is a flat region of its own
        if (U != 1) continue;  // the cells' left-out vecs do not depend on the tile size
        for (uint32_t rows = 1; rows <= 3 && rows <= h; ++rows)
        for (uint32_t cols = 1; cols <= 3 && cols <= w; ++cols) {
            std::set<std::vector<uint32_t>> want, got;  // {cell, frame column, frame row, pixels}
            std::vector<int> count(W * H, 0);
            for (uint32_t r = 0; r < rows; ++r)
                for (uint32_t c = 0; c < cols; ++c) {
                    const Rect cell = cell_of(rc, rows, cols, r, c);
                    Pairs left_out;
                    walk(W, H, cell, C, 4u, false, count, left_out);
                    for (const auto& q : left_out)
                        want.insert({r * cols + c, cell.x + q.second, cell.y + q.first, cell.w - q.second});
                }
            for_grid_frame_end_tails(
                W, H, y, h, rows, cols, [&](uint32_t r, uint32_t c) { return cell_of(rc, rows, cols, r, c); },
                [&](uint32_t r, uint32_t c, uint32_t x0, uint32_t fy, uint32_t n) {
                    CHECK(got.insert({r * cols + c, x0, fy, n}).second);
                    return 0;
                });
            CHECK(got == want);
            for (uint32_t py = 0; py < H; ++py)
                for (uint32_t px = 0; px < W; ++px)
                    CHECK(count[py * W + px] == (px >= x && px < x + w && py >= y && py < y + h ? 1 : 0));
            ++cases;
        }
    }
    std::printf("OK %llu\n", cases);
    return 0;
}
'''


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    d = tmp_path_factory.mktemp("slots")
    src = d / "slots.cpp"
    src.write_text(_PROGRAM)
    exe = d / "slots"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)


def test_slots_cover_regions_and_agree_with_the_host_walks(result):
    assert result.returncode == 0, result.stdout + result.stderr
    tag, cases = result.stdout.split()
    # 2 layouts x 3 U x 2 C per (frame, region), plus the grids: far more than 100,000 cases
    assert tag == "OK" and int(cases) > 100000
