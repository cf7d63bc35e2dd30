"""The bound the screened RGB8 series kernel rests on
(dips_amd/csrc/series_v2_screen.h): with J = max + min of a pixel's channels,
two pixels whose J differ by at most s(tau) are never selected (|dI| > tau),
for the screen level s(tau) of dips_amd/csrc/series_screen_rule.h.

The rule itself is compiled from that header (a stand-alone g++ program, as
tests/test_sched_cpu.py does for the schedules) and pinned against its
restatement here; the bound is then checked EXHAUSTIVELY: every pair of the
distinct f32 intensities of the 32,896 (max, min) byte pairs, for every tau of
the list, the subtraction and the comparison in f32 as the oracle makes them."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import np_restatement as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")
F32 = np.float32

TAUS = [2.0 ** -5, 8 / 255, 0.05, 0.1, 0.5, 0.999, 1.0]

# stdin: f32 bit patterns of tau; stdout: series_screen_level(tau)
_PROGRAM = r'''
#include "series_screen_rule.h"
#include <cstdio>
#include <cstring>
int main() {
    unsigned bits;
    while (std::scanf("%u", &bits) == 1) {
        float tau;
        std::memcpy(&tau, &bits, 4);
        std::printf("%d\n", dips::series_screen_level(tau));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("screen")
    src = d / "rule.cpp"
    src.write_text(_PROGRAM)
    exe = d / "rule"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def levels(taus):
        bits = np.asarray(taus, dtype=F32).view(np.uint32)
        r = subprocess.run([str(exe)], input="".join(f"{int(b)}\n" for b in bits), capture_output=True, text=True,
                           timeout=60, check=True)
        out = [int(x) for x in r.stdout.split()]
        assert len(out) == bits.size
        return out
    return levels


def screen_level(tau) -> int:
    """The rule restated: the largest integer s with s + 3e-4 < 510 * (double)tau_f32, clamped to [-1, 510]."""
    lim = 510.0 * float(F32(tau)) - 3e-4
    s = math.ceil(lim) - 1  # the largest integer below lim
    return max(-1, min(510, s))


def test_rule_matches_its_restatement(rule):
    taus = list(TAUS) + [0.0, 1e-9, 1 / 510, 2.0, 1e30, float(np.nextafter(F32(2.0 ** -5), F32(0)))]
    for k in range(0, 512):  # the f32 neighbours of every k / 510, where s steps
        t = F32(k / 510)
        taus += [float(np.nextafter(t, F32(-1))), float(t), float(np.nextafter(t, F32(2)))]
    taus = [t for t in taus if t >= 0]
    got = rule(taus)
    want = [screen_level(t) for t in taus]
    assert got == want
    for t, s in zip(taus, got):
        assert -1 <= s <= 510
        assert s == 510 or not (s + 1) + 3e-4 < 510.0 * float(F32(t))  # the largest such s
        assert s == -1 or s == 510 or s + 3e-4 < 510.0 * float(F32(t))
    assert [screen_level(t) for t in TAUS] == [15, 15, 25, 50, 254, 509, 509]
    assert rule([0.0]) == [-1] and rule([2.0]) == [510]


@pytest.fixture(scope="module")
def intensities():
    """(J, I) of every distinct f32 intensity per J = max + min, from the oracle's intensity."""
    mx, mn = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    keep = mx >= mn
    mx, mn = mx[keep].astype(np.uint8), mn[keep].astype(np.uint8)
    assert mx.size == 32896
    px = np.stack([mx, mn, mn], axis=-1)[None, None]  # one row of RGB pixels (max, min, min)
    inten = nr.intensity(px)[0, 0].astype(F32)
    j = mx.astype(np.int64) + mn
    pairs = np.unique(np.stack([j, inten.view(np.uint32).astype(np.int64)], axis=1), axis=0)
    return pairs[:, 0], pairs[:, 1].astype(np.uint32).view(F32)


def _selected_by_dj(j, inten, tau):
    """sel[d], unsel[d]: whether some pair of intensities with |dJ| = d is / is not selected at tau."""
    sel = np.zeros(511, dtype=bool)
    unsel = np.zeros(511, dtype=bool)
    t = F32(tau)
    for s0 in range(0, j.size, 256):
        a = np.abs((inten[s0:s0 + 256, None] - inten[None, :]).astype(F32))
        dj = np.abs(j[s0:s0 + 256, None] - j[None, :])
        hit = a > t
        sel |= np.bincount(dj[hit], minlength=511).astype(bool)
        unsel |= np.bincount(dj[~hit], minlength=511).astype(bool)
    return sel, unsel


@pytest.mark.parametrize("tau", TAUS)
def test_no_pixel_within_the_screen_level_is_selected(rule, intensities, tau):
    j, inten = intensities
    s = rule([tau])[0]
    assert s == screen_level(tau) and s >= 15  # the screened form runs for tau >= 2^-5
    sel, unsel = _selected_by_dj(j, inten, tau)
    assert not sel[:s + 1].any(), (tau, s, np.nonzero(sel[:s + 1])[0])
    if tau == 8 / 255:
        # the edge the exact path is needed for: |dJ| = 16 goes both ways
        assert s == 15 and sel[16] and unsel[16]
        assert not unsel[17:].any()
