"""What test_gpu_regional_fuzz.py rests on, shown without a GPU and on the C
oracle alone: that step_walk content puts a meaningful share of pixel-frames
where the decision |dI| > tau rests on the rounding, that the cases the GPU
test draws reach every kernel form, and that the reference of
tests/_regional_cases.py is consistent with itself.

Rounding-critical share: the share of the pixel-frames of frames 1 .. n - 1
whose oracle bit differs between nextafter(f32(k / 255), 0) and
nextafter(f32(k / 255), 2).  Measured on the clips of the sweep (37x13x9,
3,848 pixel-frames, _regional_cases.edge_frames), overall / per-frame:

  class            k = 4          k = 16          k = 31          k = 64
  GRAY8            1.14 / 4.26    6.00 / 17.00    12.19 / 29.57   23.49 / 49.40
  RGB8  none       0.10 / 0.18    2.10 /  5.43     2.78 /  6.11   15.23 / 41.76
  RGB8  red        2.36 / 5.51    8.19 / 18.24    13.72 / 31.03   21.73 / 48.39
  RGB8  green      1.48 / 3.51    6.29 / 14.45    13.20 / 29.68   21.39 / 46.73
  RGB8  blue       1.90 / 3.72    7.20 / 17.13    13.02 / 28.69   19.96 / 45.30
  RGBA8 none       0.00 / 0.05    2.78 /  5.85     3.53 /  7.41   13.44 / 38.41
  RGBA8 red        1.87 / 4.44    9.10 / 20.74    13.64 / 30.25   19.54 / 45.61
  RGBA8 green      1.77 / 4.42    8.03 / 17.91    14.89 / 32.07   21.73 / 47.66
  RGBA8 blue       1.46 / 4.29    8.60 / 19.96    13.02 / 27.81   19.98 / 45.50

(per cent; the test prints every figure).  The bounds asserted are half the
lowest share an earlier prototype of this content gave per class: 1 % for k in
{16, 31, 64} in every class (at 3,848 pixel-frames about four standard
deviations below a share of 2 %), 0.5 % for k = 4 with GRAY8 or one channel.
With chroma none and k = 4 the reference arithmetic has next to no critical
pixel and nothing is asserted; the case still runs on the GPU."""
import itertools

import numpy as np
import pytest

from _regional_cases import (ISI_TAU, describe, edge_frames, oracle_bits, reference, region_of, region_series,
                             rounding_critical_share, tau_form)
from test_gpu_regional_fuzz import GROUP, GROUPS, N_CASES, SEED, group_cases

F32 = np.float32
CLASSES = [(1, 0)] + [(c, ch) for c in (3, 4) for ch in range(4)]


@pytest.mark.parametrize("k", [4, 16, 31, 64])
@pytest.mark.parametrize("c,chroma", CLASSES)
@pytest.mark.parametrize("mode", [0, 1])
def test_step_walk_is_rounding_critical(c, mode, chroma, k):
    share = rounding_critical_share(edge_frames(c, k), mode, chroma, k)
    print(f"rounding-critical c={c} mode={mode} chroma={chroma} k={k}: {100 * share:.2f} %")
    if k in (16, 31, 64):
        assert share >= 0.01, share
    elif c == 1 or chroma != 0:
        assert share >= 0.005, share


def _all_cases():
    return [case for g in range(GROUPS) for case in group_cases(g)]


def test_drawn_cases_cover_the_forms():
    """The 900 cases of the GPU test's seed, by class; per mode the cases with
    tau = 0, with 0 < tau < 2^-5 (the f64 intensity sum of the grid and sums
    kernels) and with tau >= 2^-5 (their integer sum):

      format chroma   overall      per-frame
      RGB8   none     2  9 35      4 17 36
      RGB8   red      2 15 41      1 16 29
      RGB8   green    4 10 35      3  6 28
      RGB8   blue     3  9 36      4  4 21
      RGBA8  none     1  8 32      3  7 34
      RGBA8  red      3 12 31      1  7 27
      RGBA8  green    4 10 34      1 10 34
      RGBA8  blue     4 10 33      2 14 32

    and 176 GRAY8 cases; 462 through the device entry points, 418 in two
    chunks, 95 of 33 frames or more.  tau = 0 is one draw in twenty of
    _draw_tau, so its 16 classes set the case count: with 200 cases they
    cannot all occur (8 such cases are expected), with this seed the first 881
    cases hold them all."""
    cases = _all_cases()
    # nothing is skipped or filtered: the groups are the drawn cases, each once, in order
    assert GROUPS * GROUP == N_CASES and [case["case"] for case in cases] == list(range(N_CASES))
    seen = {(case["c"], case["chroma"], case["mode"], tau_form(case["tau"])) for case in cases if case["c"] != 1}
    missing = set(itertools.product((3, 4), range(4), (0, 1), (0, 1, 2))) - seen
    assert not missing, (SEED, N_CASES, sorted(missing))
    below = float(np.nextafter(F32(ISI_TAU), F32(0)))
    assert any(case["tau"] == ISI_TAU for case in cases) and any(case["tau"] == below for case in cases)
    # the threshold decides something: both a set and a clear bit
    informative = [case for case in cases if 0 < case["tau"] < 1 and case["n"] >= 2]
    both = 0
    for case in informative:
        bits = oracle_bits(case)
        both += bool(bits.any() and not bits.all())
    print(f"{both} of {len(informative)} cases with 0 < tau < 1 and n >= 2 have a set and a clear bit")
    assert both >= 0.6 * len(informative), (both, len(informative))
    # every drawn alternative of the other arguments occurs
    for key, values in (("content", 5), ("t0", 3), ("connectivity", 2), ("min_area", 3), ("max_boxes", 4),
                        ("labels", 2), ("device", 2), ("explicit_ref", 2)):
        assert len({case[key] for case in cases}) == values, key
    assert any(case["split"] is not None for case in cases)
    long = [case for case in cases if case["n"] >= 33]
    assert {None, 16, 17} <= {case["part_frames"] for case in long}
    assert any(case["part_frames"] == case["n"] for case in long)


def test_reference_identities():
    """The sum over the pixels of the per-pixel series is the series of the
    region's crop in all four fields: SAD, SJ and count are sums over pixels,
    and the oracle defines SI_fixed as the sum over the counted pixels of the
    integer dI * 2^32 (o_series_frame of oracle/dips_oracle.c), so it is
    additive too.  The one-cell grid is that crop's series."""
    for case in group_cases(0)[:20]:
        want = reference(dict(case, rows=1, cols=1))
        region = region_series(case["frames"], case["mode"], case["tau"], case["chroma"], case["ref"], region_of(case))
        what = describe(case)
        assert np.array_equal(want["per_pixel"].sum(axis=(1, 2), dtype=np.uint64), region), what
        assert np.array_equal(want["grid"][:, 0, 0], region), what
        assert np.array_equal(want["sums"].sum(axis=(0, 1), dtype=np.uint64), region.sum(axis=0, dtype=np.uint64)), what
        assert np.array_equal(want["bits"].sum(axis=(1, 2), dtype=np.uint64), region[:, 2]), what
