"""dips_diff_sigma_delta_mask on drawn cases against the definition
(tests/_sigma_delta_ref.py): shape up to 70 x 70, up to 40 frames, a drawn
region, format, n_amp, v_min <= v_max, chroma, an optional ref, and for half
of the cases a split into chunks continued with state=.  Every array of a
case comes from its own generator, so case i is the same whichever cases run.
Every comparison is np.array_equal on the whole mask and the whole state."""
import numpy as np
import pytest

from _sigma_delta_ref import sigma_delta_fold
from test_gpu_change_mask import make_op

pytestmark = pytest.mark.gpu

SEED, N_CASES, GROUP = 20262, 36, 12


def draw_case(i):
    rng = np.random.default_rng([SEED, i])
    c = int(rng.choice([1, 3, 4]))
    w, h = int(rng.integers(1, 71)), int(rng.integers(1, 71))
    if rng.random() < 0.15:
        w = int(rng.integers(1, 4))  # narrow frames: vecs that would cross the frame's end in several rows
    n = int(rng.integers(1, 12)) if rng.random() < 0.8 else int(rng.integers(12, 41))
    roi = None
    if rng.random() < 0.6:
        rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        roi = (int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh)
    shape = (h, w) if c == 1 else (h, w, c)
    base = rng.integers(0, 256, shape, dtype=np.int16)
    amp = int(rng.choice([1, 4, 12, 255]))
    clip = np.clip(base[None] + rng.integers(-amp, amp + 1, (n + 1,) + shape, dtype=np.int16)
                   + (np.arange(n + 1).reshape((-1,) + (1,) * len(shape)) // 2), 0, 255).astype(np.uint8)
    with_ref = bool(rng.random() < 0.5)
    cuts = sorted(set(int(v) for v in rng.integers(0, n + 1, int(rng.integers(1, 4))))) if rng.random() < 0.5 else []
    v_min = int(rng.choice([0, 1, 2, 7, 510]))
    v_max = int(rng.choice([v_min, min(v_min + 4, 510), 255, 510]))
    n_amp = int(rng.choice([1, 2, 4, 15])) if rng.random() < 0.6 else int(rng.integers(1, 16))
    return dict(case=i, c=c, w=w, h=h, n=n, roi=roi, frames=np.ascontiguousarray(clip[1:]),
                ref=np.ascontiguousarray(clip[0]) if with_ref else None, n_amp=n_amp, v_min=v_min,
                v_max=max(v_min, v_max), chroma=int(rng.integers(0, 4)) if c != 1 else 0, cuts=cuts)


def test_the_draw_covers_the_ground():
    cases = [draw_case(i) for i in range(N_CASES)]
    assert {case["c"] for case in cases} == {1, 3, 4}
    assert {1, 15} <= {case["n_amp"] for case in cases}
    assert {(case["ref"] is not None, bool(case["cuts"]), case["roi"] is not None)
            for case in cases if case["c"] != 1} == {(b, x, y) for b in (0, 1) for x in (0, 1) for y in (0, 1)}
    assert {case["chroma"] for case in cases if case["c"] != 1} == {0, 1, 2, 3}
    assert any(case["v_min"] == case["v_max"] for case in cases) and any(case["v_min"] < case["v_max"] < 510 for case in cases)
    assert any(case["w"] < 3 for case in cases) and any(case["n"] > 12 for case in cases)


@pytest.mark.parametrize("group", range(N_CASES // GROUP))
def test_drawn_cases(group):
    for i in range(group * GROUP, (group + 1) * GROUP):
        case = draw_case(i)
        frames, ref, roi = case["frames"], case["ref"], case["roi"]
        kw = dict(n_amp=case["n_amp"], v_min=case["v_min"], v_max=case["v_max"])
        want = sigma_delta_fold(frames, kw["n_amp"], kw["v_min"], kw["v_max"], case["chroma"], ref, roi)
        op = make_op(case["c"], int(i & 1), 8 / 255, case["chroma"])
        try:
            m, s = op.sigma_delta_mask(frames, roi=roi, ref=ref, **kw)
            label = {key: case[key] for key in ("case", "c", "w", "h", "n", "roi", "n_amp", "v_min", "v_max", "chroma", "cuts")}
            assert np.array_equal(m.bits, want[0]), label
            assert np.array_equal(s.state, want[1]), label
            if case["cuts"]:
                bits, state = [], None
                edges = [0] + case["cuts"] + [case["n"]]
                for j, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
                    if j == 0:
                        if hi == 0 and ref is None:
                            continue  # an empty first chunk without ref has nothing to start from
                        mm, state = op.sigma_delta_mask(frames[lo:hi], roi=roi, ref=ref, **kw)
                    elif state is None:
                        mm, state = op.sigma_delta_mask(frames[lo:hi], roi=roi, **kw)
                    else:
                        mm, state = op.sigma_delta_mask(frames[lo:hi], roi=roi, state=state, **kw)
                    bits.append(mm.bits)
                assert np.array_equal(np.concatenate(bits), want[0]), label
                assert np.array_equal(state.state, want[1]), label
        finally:
            op.close()
