"""The persistent kernels where a wave takes several items: every case of
tests/_round_cases.py on the GPU under DIPS_SERIES_WAVES_PER_SIMD = 1, which
leaves a device 4 wave slots per CU (1,024 on 256 CUs) against the 1,100 to
2,200 items of these shapes.  What then runs for the first time in the suite:
the slot offsets derived again for a wave's next tile, the accumulators reset,
the reference state and the frame ring set up again between items, a next
item in another part and another tile, a ragged last round, a partial last
tile behind a whole one, the atomics of several parts from waves on different
trips, the times summaries and their combine, and the state planes of the two
background models loaded and stored tile after tile by one wave.

Every test
 1. reads the device's CU count (torch's multi_processor_count is
    hipDeviceAttributeMultiprocessorCount, which dips_create stores in
    dips_handle::cu_count, dips_handle.h) and asserts on the schedule header
    that at 4 slots per CU the case does take several items per wave
    (_round_cases.check_schedule): on a device with another CU count the test
    fails with the schedule in its message, it never passes single-trip;
 2. runs the product through its device entry point onto outputs filled with
    0xA5 bytes (an item that is skipped shows), the accumulating forms onto a
    random earlier map or state;
 3. compares every word of every output, np.array_equal, with the suite's
    references: py_change_mask, py_pixel_sums, fold_times, oracle_grid,
    background_fold, sigma_delta_fold, _vote_ref and _mask_stats_ref;
 4. runs the same calls without the cap (one item per wave) and with
    DIPS_FLAG_FORCE_GENERIC: all three must give the reference, and the
    message of a failure says which of them do, so that it points at the trip
    count and not at the shape.  The vote and the mask statistics have no
    generic kernel; the flag leaves them as they are.

The references are computed once per (case, format, mode, chroma) and shared
between the forms of a test.  Each asserts on itself that 5-95 % of the bits
behind it are set from frame 1 on."""
import functools

import numpy as np
import pytest

import _components_ref as cref
import _mask_stats_ref as sref
import _round_cases as rc
import _vote_ref as vref
from _background_ref import background_fold
from _sigma_delta_ref import sigma_delta_fold
from test_change_mask_cpu import py_change_mask, unpack_mask
from test_gpu_grid import oracle_grid
from test_gpu_mask_stats import random_bits
from test_pixel_sums_cpu import py_pixel_sums
from test_pixel_times_cpu import crossing_share, fold_times

pytestmark = pytest.mark.gpu

WAYS = ("capped", "uncapped", "generic")
HEAD = 3  # frames of the earlier call behind an accumulated state


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return rc.build_geometry(tmp_path_factory.mktemp("persistent_rounds"))


@pytest.fixture(scope="module", autouse=True)
def _drop_the_clips():
    yield
    rc.clear_caches()
    for f in (mask_want, sums_want, times_want, grid_want, background_want, sigma_delta_want, vote_want,
              mask_times_want):
        f.cache_clear()


def assert_several_items_on_this_device(program, case, c):
    import torch
    slots = 4 * torch.cuda.get_device_properties(0).multi_processor_count  # series_host.h resident_at under the cap
    rc.check_schedule(case, c, rc.schedule(program, case, c, slots), slots)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def make_op(c, mode, chroma, **kw):
    from dips_amd import ChromaFilter, DiffSeriesOperator, Mode, PixelFormat
    fmt = {3: PixelFormat.RGB8, 4: PixelFormat.RGBA8}[c]
    return DiffSeriesOperator(fmt, Mode(mode), rc.TAU, ChromaFilter(chroma), **kw)


def to_device(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached arrays are read-only


def poisoned(shape, dtype):
    """A device tensor of `shape` whose every byte is 0xA5."""
    import torch
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda").view(dtype).view(*shape)


def words(t, np_dtype):
    return t.cpu().numpy().view(np_dtype)


def three_ways(monkeypatch, case, c, mode, chroma, run):
    """{way: run(op)} under the cap, without it and with the generic kernel;
    the case's DIPS_PIXEL_PART_FRAMES holds for all three."""
    import torch
    out = {}
    for way in WAYS:
        with monkeypatch.context() as m:
            if way == "capped":
                m.setenv(rc.CAP_ENV, "1")
            else:
                m.delenv(rc.CAP_ENV, raising=False)
            if case.pin:
                m.setenv(rc.PIN_ENV, str(case.pin))
            else:
                m.delenv(rc.PIN_ENV, raising=False)
            op = make_op(c or 3, mode, chroma, force_generic=way == "generic")
            try:
                out[way] = run(op)
                torch.cuda.synchronize()
            finally:
                op.close()
    return out


def check(out, want, what):
    """Every output of every way equals the reference; the capped run first,
    with the other ways' verdict in its message."""
    for way in WAYS:
        for name, w in want.items():
            got = out[way][name]
            assert got.dtype == w.dtype and got.shape == w.shape, (what, way, name, got.dtype, got.shape, w.shape)
            if np.array_equal(got, w):
                continue
            bad = np.argwhere(got != w)
            others = {o: bool(np.array_equal(out[o][name], w)) for o in WAYS}
            raise AssertionError(f"{what}: {name} ({way}) differs from the reference in {len(bad)} of {w.size} values, "
                                 f"first at {bad[:4].tolist()}; equal to the reference: {others}")


def _params(product):
    """(case name, format) of a product's cases."""
    return [(case.name, c) for case in rc.CASES if case.product == product for c in case.fmts]


def frame_side(product):
    def deco(f):
        for args in (("chroma", rc.CHROMAS), ("mode", rc.MODES), ("name,c", _params(product))):
            f = pytest.mark.parametrize(*args)(f)
        return f
    return deco


def cropped(case, c):
    return rc.crop(rc.frames_of(case, c), rc.region(case))


# -- the change mask ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mask_want(name, c, mode, chroma):
    case = rc.BY_NAME[name]
    want = py_change_mask(cropped(case, c), mode, rc.TAU, chroma)  # the decision is per pixel: the crop's mask
    rc.check_share(unpack_mask(want, rc.region(case)[2])[1:], (name, c, mode, chroma))
    return frozen(want)


@frame_side("mask")
def test_change_mask(program, monkeypatch, name, c, mode, chroma):
    import torch
    case = rc.BY_NAME[name]
    assert_several_items_on_this_device(program, case, c)
    want = mask_want(name, c, mode, chroma)
    dev = to_device(rc.frames_of(case, c))

    def run(op):
        out = poisoned(want.shape, torch.uint8)
        op.run_change_mask_device(dev, out, roi=case.roi)
        return dict(mask=words(out, np.uint8))

    check(three_ways(monkeypatch, case, c, mode, chroma, run), dict(mask=want), (name, c, mode, chroma))


# -- the per-pixel sums ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sums_want(name, c, mode, chroma):
    case = rc.BY_NAME[name]
    _, _, rw, rh = rc.region(case)
    want = py_pixel_sums(cropped(case, c), mode, rc.TAU, chroma)
    share = float(want[..., 2].sum()) / ((case.n - 1) * rw * rh)  # frame 0 meets itself
    assert 0.05 < share < 0.95, (name, c, mode, chroma, share)
    earlier = np.random.default_rng([53, rw, rh]).integers(1, 1 << 40, want.shape, dtype=np.uint64)
    return frozen(want, earlier, earlier + want)


@frame_side("sums")
def test_pixel_sums(program, monkeypatch, name, c, mode, chroma):
    """Plain stores (one part) or the atomics of six parts onto the cleared
    map, then the same onto a random earlier map."""
    import torch
    case = rc.BY_NAME[name]
    assert_several_items_on_this_device(program, case, c)
    want, earlier, summed = sums_want(name, c, mode, chroma)
    dev = to_device(rc.frames_of(case, c))

    def run(op):
        plain = poisoned(want.shape, torch.int64)
        onto = to_device(earlier.view(np.int64))
        op.run_pixel_sums_device(dev, plain, roi=case.roi)
        op.run_pixel_sums_device(dev, onto, roi=case.roi, accumulate=True)
        return dict(sums=words(plain, np.uint64), accumulated=words(onto, np.uint64))

    check(three_ways(monkeypatch, case, c, mode, chroma, run), dict(sums=want, accumulated=summed),
          (name, c, mode, chroma))


# -- the change times --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def times_want(name, c, mode, chroma):
    case = rc.BY_NAME[name]
    rect = rc.region(case)
    ref = rc.crop(rc.ref_of(case, c), rect, lead=0)
    bits = unpack_mask(py_change_mask(cropped(case, c), mode, rc.TAU, chroma, ref), rect[2])
    rc.check_share(bits[1:], (name, c, mode, chroma))
    if case.parts:
        assert crossing_share(bits, case.pin) >= 0.10
    head = fold_times(random_bits(HEAD, rect[3], rect[2], 0.5, seed=41), rc.TIMES_T0 - HEAD)
    assert ((head[3] > 0) & bits[0]).mean() >= 0.10  # runs of the earlier state that go on into the call
    return frozen(fold_times(bits, rc.TIMES_T0), head, fold_times(bits, rc.TIMES_T0, head))


@frame_side("times")
def test_pixel_times(program, monkeypatch, name, c, mode, chroma):
    """From t0 = 7 against an explicit reference: the one-part form, or six
    parts with their summaries and the combine; then the same folded onto the
    state of three earlier frames."""
    import torch
    case = rc.BY_NAME[name]
    assert_several_items_on_this_device(program, case, c)
    want, head, onto_head = times_want(name, c, mode, chroma)
    dev, rdev = to_device(rc.frames_of(case, c)), to_device(rc.ref_of(case, c))

    def run(op):
        plain = poisoned(want.shape, torch.int32)
        onto = to_device(head.view(np.int32))
        op.run_pixel_times_device(dev, plain, roi=case.roi, ref=rdev, t0=rc.TIMES_T0)
        op.run_pixel_times_device(dev, onto, roi=case.roi, ref=rdev, t0=rc.TIMES_T0, accumulate=True)
        return dict(times=words(plain, np.uint32), accumulated=words(onto, np.uint32))

    check(three_ways(monkeypatch, case, c, mode, chroma, run), dict(times=want, accumulated=onto_head),
          (name, c, mode, chroma))


# -- the grid ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid_want(name, c, mode, chroma):
    case = rc.BY_NAME[name]
    want, area = oracle_grid(rc.frames_of(case, c), case.rows, case.cols, case.roi, mode, rc.TAU, chroma)
    share = float(want[1:, ..., 2].sum()) / ((case.n - 1) * float(area.sum()))
    assert 0.05 < share < 0.95, (name, c, mode, chroma, share)
    return frozen(want)


@frame_side("grid")
def test_grid(program, monkeypatch, name, c, mode, chroma):
    import torch
    case = rc.BY_NAME[name]
    assert_several_items_on_this_device(program, case, c)
    want = grid_want(name, c, mode, chroma)
    dev = to_device(rc.frames_of(case, c))

    def run(op):
        cells = poisoned(want.shape, torch.int64)
        op.run_grid_device(dev, cells, case.rows, case.cols, roi=case.roi)
        return dict(cells=words(cells, np.uint64))

    check(three_ways(monkeypatch, case, c, mode, chroma, run), dict(cells=want), (name, c, mode, chroma))


# -- the two background models -----------------------------------------------------------------

RATE_SHIFT = 3
SD_PARAMS = (2, 2, 510)
CUT = 2  # the clip again as 2 + 3 frames with the state carried


def model_want(case, c, chroma, mask, state):
    rc.check_share(unpack_mask(mask, rc.region(case)[2])[1:], (case.name, c, chroma))
    frozen(mask, state)
    return dict(mask=mask, state=state, mask_in_two_calls=mask, state_after_two_calls=state)


@functools.lru_cache(maxsize=None)
def background_want(name, c, chroma, selective):
    case = rc.BY_NAME[name]
    mask, state = background_fold(rc.frames_of(case, c), RATE_SHIFT, selective, rc.TAU, chroma, None, case.roi)
    return model_want(case, c, chroma, mask, state)


@functools.lru_cache(maxsize=None)
def sigma_delta_want(name, c, chroma):
    case = rc.BY_NAME[name]
    mask, state = sigma_delta_fold(rc.frames_of(case, c), *SD_PARAMS, chroma, None, case.roi)
    assert len(np.unique(state[1])) >= 3
    return model_want(case, c, chroma, mask, state)


def run_model(case, want, dev, launch):
    """launch(frames, state, mask, accumulate) in one call and as CUT + the rest."""
    import torch

    def run(op):
        state, mask = poisoned(want["state"].shape, torch.int16), poisoned(want["mask"].shape, torch.uint8)
        launch(op, dev, state, mask, False)
        state2, mask2 = poisoned(want["state"].shape, torch.int16), poisoned(want["mask"].shape, torch.uint8)
        launch(op, dev[:CUT], state2, mask2[:CUT], False)
        launch(op, dev[CUT:], state2, mask2[CUT:], True)
        return dict(mask=words(mask, np.uint8), state=words(state, np.uint16),
                    mask_in_two_calls=words(mask2, np.uint8), state_after_two_calls=words(state2, np.uint16))
    return run


@pytest.mark.parametrize("selective", [False, True])
@frame_side("background")
def test_background(program, monkeypatch, name, c, mode, chroma, selective):
    """The operator's mode is not consulted: both give the one reference."""
    case = rc.BY_NAME[name]
    assert_several_items_on_this_device(program, case, c)
    want = background_want(name, c, chroma, selective)

    def launch(op, frames, state, mask, accumulate):
        op.run_background_mask_device(frames, state, mask, roi=case.roi, rate_shift=RATE_SHIFT, selective=selective,
                                      accumulate=accumulate)

    run = run_model(case, want, to_device(rc.frames_of(case, c)), launch)
    check(three_ways(monkeypatch, case, c, mode, chroma, run), want, (name, c, mode, chroma, selective))


@frame_side("sigma_delta")
def test_sigma_delta(program, monkeypatch, name, c, mode, chroma):
    """Large tiles on the whole frame, tiles of 64 vecs on the region; the
    operator's mode and tau are not consulted."""
    case = rc.BY_NAME[name]
    assert_several_items_on_this_device(program, case, c)
    want = sigma_delta_want(name, c, chroma)

    def launch(op, frames, state, mask, accumulate):
        op.run_sigma_delta_mask_device(frames, state, mask, roi=case.roi, n_amp=SD_PARAMS[0], v_min=SD_PARAMS[1],
                                       v_max=SD_PARAMS[2], accumulate=accumulate)

    run = run_model(case, want, to_device(rc.frames_of(case, c)), launch)
    check(three_ways(monkeypatch, case, c, mode, chroma, run), want, (name, c, mode, chroma))


# -- the mask side -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def vote_want(name):
    case = rc.BY_NAME[name]
    hist = None if case.parts else random_bits(case.window - 1, case.h, case.w, 0.5, seed=43)
    voted, nxt = vref.vote_bits(rc.bits_of(case), case.window, case.votes, hist)
    rc.check_share(voted[case.window:], (name, "voted"))
    return hist, dict(voted=frozen(cref.pack(voted)), history=frozen(cref.pack(nxt)))


@pytest.mark.parametrize("name", [n for n, _ in _params("vote")])
def test_mask_vote(program, monkeypatch, name):
    """3 of 5: the counters primed again for every item, from the history
    (one part) or from the input frames before the part (two parts); the pad
    bits of the inputs are set."""
    import torch
    case = rc.BY_NAME[name]
    assert_several_items_on_this_device(program, case, 0)
    hist, want = vote_want(name)
    mask = to_device(cref.pack(rc.bits_of(case), 1))
    hdev = None if hist is None else to_device(cref.pack(hist, 1))

    def run(op):
        out, nxt = poisoned(want["voted"].shape, torch.uint8), poisoned(want["history"].shape, torch.uint8)
        op.run_mask_vote_device(mask, case.w, out, case.window, case.votes, history=hdev, history_out=nxt)
        return dict(voted=words(out, np.uint8), history=words(nxt, np.uint8))

    check(three_ways(monkeypatch, case, 0, 1, 0, run), want, name)


@functools.lru_cache(maxsize=None)
def mask_times_want(name):
    case = rc.BY_NAME[name]
    bits, head = rc.bits_of(case), random_bits(HEAD, case.h, case.w, 0.5, seed=47)
    head_t, head_s = sref.times_bits(head, rc.TIMES_T0 - HEAD), sref.sums_bits(head)
    assert ((head_t[3] > 0) & bits[0]).mean() >= 0.10
    return frozen(head_t, head_s), dict(times=frozen(sref.times_bits(bits, rc.TIMES_T0)), sums=frozen(sref.sums_bits(bits)),
                                        times_onto=frozen(sref.times_bits(bits, rc.TIMES_T0, head_t)),
                                        sums_onto=frozen(sref.sums_bits(bits, head_s)))


@pytest.mark.parametrize("name", [n for n, _ in _params("mask_times")])
def test_mask_times_and_sums(program, monkeypatch, name):
    """Times and sums in one launch from t0 = 7, one part or two with their
    summaries and the combine; then folded onto the state of three earlier
    frames."""
    import torch
    case = rc.BY_NAME[name]
    assert_several_items_on_this_device(program, case, 0)
    (head_t, head_s), want = mask_times_want(name)
    mask = to_device(cref.pack(rc.bits_of(case), 1))

    def run(op):
        t, s = poisoned(want["times"].shape, torch.int32), poisoned(want["sums"].shape, torch.int32)
        op.run_mask_times_device(mask, case.w, t, s, t0=rc.TIMES_T0)
        t2, s2 = to_device(head_t.view(np.int32)), to_device(head_s.view(np.int32))
        op.run_mask_times_device(mask, case.w, t2, s2, t0=rc.TIMES_T0, accumulate=True)
        return dict(times=words(t, np.uint32), sums=words(s, np.uint32), times_onto=words(t2, np.uint32),
                    sums_onto=words(s2, np.uint32))

    check(three_ways(monkeypatch, case, 0, 1, 0, run), want, name)
