"""Seeded randomized parity test of the regional products of the difference
series -- dips_diff_series_grid, dips_diff_pixel_sums, dips_diff_change_mask,
dips_diff_pixel_times and dips_mask_components (HIP, through the C ABI) --
against the CPU oracle, and a deterministic sweep of the threshold cases that
rest on the rounding.

The hand-listed files of these products (test_gpu_grid.py, _pixel_sums.py,
_change_mask.py, _pixel_times.py, _mask_components.py) pin the geometry at
tau in {0, 4/255, 8/255} and five (tau, chroma) pairs on content with next to
no pixels at the threshold.  Here the parameters are drawn
(tests/_regional_cases.py: every chroma filter, tau at 0, k/255, 2^-5 and 1
with their f32 neighbours, host and device entry points, clips in two chunks,
pinned frame parts), all five products run on the same input, and the
reference of every output is the C oracle on crops (_regional_cases.reference),
not a vectorised twin.  Every comparison is np.array_equal on the whole
output: the pad bits of the mask, the zero-filled box records, the labels and,
on the device path, the words around every output.

test_threshold_edges runs step_walk content -- every pixel moves by exactly
+-k bytes per frame -- at the f32 neighbour below f32(k / 255), at it and at
the neighbour above it: the share of pixel-frames whose bit differs between
the two neighbours is asserted on the oracle alone in
test_regional_edges_cpu.py (1-50 % by class).  A compare that became >=, a
threshold scaled for the other intensity form or a compare in the wrong domain
changes these bits.

N_CASES / SEED: test_regional_edges_cpu.py asserts, on the drawn cases and
the oracle alone, that every (RGB8 / RGBA8, chroma, mode, form of tau) occurs;
tau = 0 is 5 % of _draw_tau's draws, so the 48 classes need several hundred
cases: with this seed the first 881 cover them, run here in 36 groups of 25."""
import numpy as np
import pytest

from _regional_cases import describe, drawn_cases, edge_case, grid_reference, reference, region_of
from test_change_mask_cpu import unpack_mask
from test_pixel_times_cpu import fold_times

pytestmark = pytest.mark.gpu

SEED = 0xD1FC
N_CASES = 900
GROUP = 25
GROUPS = N_CASES // GROUP

POISON64 = -1
POISON32 = 0x5A5A5A5A  # not a value of any u32 output of these shapes
TAIL = 16              # words checked after a device output


def group_cases(g):
    """Cases GROUP * g .. GROUP * g + GROUP - 1 of the seed, whichever groups run."""
    return drawn_cases(SEED, N_CASES)[GROUP * g:GROUP * (g + 1)]


def _fmt(c):
    from dips_amd import PixelFormat
    return {1: PixelFormat.Gray8, 3: PixelFormat.RGB8, 4: PixelFormat.RGBA8}[c]


def make_op(case, **kw):
    from dips_amd import ChromaFilter, DiffSeriesOperator, Mode
    return DiffSeriesOperator(_fmt(case["c"]), Mode(case["mode"]), case["tau"], ChromaFilter(case["chroma"]), **kw)


def _second_ref(case, frames, ref, k):
    """The reference of frames[k:]: the frame before them in per-frame mode, the same reference overall."""
    if case["mode"] == 1:
        return frames[k - 1]
    return ref if ref is not None else frames[0]


def run_host(op, case):
    from dips_amd import ChangeMask
    frames, ref, roi, t0, k = case["frames"], case["ref"], case["roi"], case["t0"], case["split"]
    out = {"grid": op.grid(frames, case["rows"], case["cols"], roi=roi, ref=ref).as_array(),
           "one_cell": op.grid(frames, 1, 1, roi=roi, ref=ref).as_array()[:, 0, 0]}
    if k is None:
        out["sums"] = op.pixel_sums(frames, roi=roi, ref=ref).as_array()
        mask = op.change_mask(frames, roi=roi, ref=ref)
        out["times"] = op.pixel_times(frames, roi=roi, ref=ref, t0=t0).as_array()
    else:
        ref2 = _second_ref(case, frames, ref, k)
        head = op.pixel_sums(frames[:k], roi=roi, ref=ref)
        out["sums"] = op.pixel_sums(frames[k:], roi=roi, ref=ref2, into=head).as_array()
        m1 = op.change_mask(frames[:k], roi=roi, ref=ref)
        m2 = op.change_mask(frames[k:], roi=roi, ref=ref2)
        mask = ChangeMask.from_array(np.concatenate([m1.bits, m2.bits]), m1.width)
        head = op.pixel_times(frames[:k], roi=roi, ref=ref, t0=t0)
        out["times"] = op.pixel_times(frames[k:], roi=roi, ref=ref2, t0=t0 + k, into=head).as_array()
    out["mask"] = mask
    found = op.mask_components(mask, case["connectivity"], case["min_area"], case["max_boxes"], case["labels"])
    out["counts"], out["boxes"], out["labels"] = found.as_arrays()
    return out


class _Guarded:
    """A device output inside a larger prefilled buffer: `guard` words before
    it (the ABI's alignment and no more), TAIL words after it."""

    def __init__(self, shape, dtype, guard, poison):
        import torch
        self.words, self.guard, self.poison = int(np.prod(shape)), guard, poison
        self.store = torch.full((guard + self.words + TAIL,), poison, dtype=dtype, device="cuda")
        self.flat = self.store[guard:guard + self.words]
        self.view = self.flat.view(shape)

    def read(self, what, np_dtype):
        """The output's words; asserts the words around it untouched."""
        got = self.store.cpu().numpy()
        assert (got[:self.guard] == self.poison).all() and (got[self.guard + self.words:] == self.poison).all(), what
        return got[self.guard:self.guard + self.words].view(np_dtype)


def run_device(op, case):
    import torch
    from dips_amd import ChangeMask
    frames, ref, roi, t0, k = case["frames"], case["ref"], case["roi"], case["t0"], case["split"]
    n, g, what = frames.shape[0], case["guard"], str(describe(case))
    _, _, rw, rh = region_of(case)
    rb = 4 * ((rw + 31) // 32)

    def upload(a, off):
        buf = torch.zeros(a.nbytes + 8, dtype=torch.uint8, device="cuda")
        v = buf[off:off + a.nbytes].view(a.shape)
        v.copy_(torch.from_numpy(a.copy()))
        return v

    dev = upload(frames, case["offs"][0])
    rdev = upload(ref, case["offs"][1]) if ref is not None else None
    rows, cols = case["rows"], case["cols"]
    grid = _Guarded((n, rows, cols, 4), torch.int64, g, POISON64)
    one = _Guarded((n, 1, 1, 4), torch.int64, g, POISON64)
    sums = _Guarded((rh, rw, 4), torch.int64, g, POISON64)
    mask = _Guarded((n * rh * rb // 4,), torch.int32, g, POISON32)
    mask_bytes = mask.flat.view(torch.uint8).view(n, rh, rb)
    times = _Guarded((4, rh, rw), torch.int32, g, POISON32)
    counts = _Guarded((n,), torch.int32, g, POISON32)
    boxes = _Guarded((n, case["max_boxes"], 8), torch.int32, g, POISON32) if case["max_boxes"] else None
    labels = _Guarded((n, rh, rw), torch.int32, g, POISON32) if case["labels"] else None

    op.run_grid_device(dev, grid.view, rows, cols, roi=roi, ref=rdev)
    op.run_grid_device(dev, one.view, 1, 1, roi=roi, ref=rdev)
    if k is None:
        op.run_pixel_sums_device(dev, sums.view, roi=roi, ref=rdev)
        op.run_change_mask_device(dev, mask_bytes, roi=roi, ref=rdev)
        op.run_pixel_times_device(dev, times.view, roi=roi, ref=rdev, t0=t0)
    else:
        ref2 = _second_ref(case, dev, rdev, k)
        op.run_pixel_sums_device(dev[:k], sums.view, roi=roi, ref=rdev)
        op.run_pixel_sums_device(dev[k:], sums.view, roi=roi, ref=ref2, accumulate=True)
        op.run_change_mask_device(dev[:k], mask_bytes[:k], roi=roi, ref=rdev)
        op.run_change_mask_device(dev[k:], mask_bytes[k:], roi=roi, ref=ref2)
        op.run_pixel_times_device(dev[:k], times.view, roi=roi, ref=rdev, t0=t0)
        op.run_pixel_times_device(dev[k:], times.view, roi=roi, ref=ref2, t0=t0 + k, accumulate=True)
    op.run_mask_components_device(mask_bytes, rw, counts.view, boxes.view if boxes is not None else None,
                                  labels.view if labels is not None else None,
                                  connectivity=case["connectivity"], min_area=case["min_area"])
    torch.cuda.synchronize()
    return {"grid": grid.read(what, np.uint64).reshape(n, rows, cols, 4),
            "one_cell": one.read(what, np.uint64).reshape(n, 4),
            "sums": sums.read(what, np.uint64).reshape(rh, rw, 4),
            "mask": ChangeMask.from_array(mask.read(what, np.uint32).view(np.uint8).reshape(n, rh, rb), rw),
            "times": times.read(what, np.uint32).reshape(4, rh, rw),
            "counts": counts.read(what, np.uint32),
            "boxes": (boxes.read(what, np.uint32).reshape(n, case["max_boxes"], 8) if boxes is not None
                      else np.zeros((n, 0, 8), dtype=np.uint32)),
            "labels": labels.read(what, np.uint32).reshape(n, rh, rw) if labels is not None else None}


def _where(a, b):
    """The first few indices at which two arrays differ, for a message."""
    return np.argwhere(a != b)[:4].tolist() if a.shape == b.shape else (a.shape, b.shape)


def check_against_oracle(got, want, what):
    assert np.array_equal(got["grid"], want["grid"]), f"{what}: grid"
    assert np.array_equal(got["one_cell"], want["region"]), f"{what}: one-cell grid"
    sums, bits = got["sums"], got["mask"].bits
    assert np.array_equal(sums, want["sums"]), f"{what}: pixel sums {_where(sums, want['sums'])}"
    assert bits.dtype == np.uint8 and np.array_equal(bits, want["mask"]), f"{what}: mask {_where(bits, want['mask'])}"
    assert got["times"].dtype == np.uint32 and np.array_equal(got["times"], want["times"]), f"{what}: pixel times"
    assert np.array_equal(got["counts"], want["counts"]), f"{what}: component counts"
    assert got["boxes"].shape == want["boxes"].shape and np.array_equal(got["boxes"], want["boxes"]), f"{what}: boxes"
    assert (got["labels"] is None) == (want["labels"] is None), f"{what}: labels"
    if want["labels"] is not None:
        assert np.array_equal(got["labels"], want["labels"]), f"{what}: labels"


def check_identities(got, case, what):
    """The identities between the products, on the GPU's own outputs."""
    mask = got["mask"]
    bits = mask.unpack()
    assert np.array_equal(mask.counts(), got["one_cell"][:, 2]), f"{what}: mask popcount != one-cell grid count"
    assert np.array_equal(mask.counts(), got["grid"][..., 2].sum(axis=(1, 2), dtype=np.uint64)), \
        f"{what}: mask popcount != sum of the grid's counts"
    assert np.array_equal(bits.sum(axis=0, dtype=np.uint64), got["sums"][..., 2]), f"{what}: mask summed != sums count"
    assert np.array_equal(got["sums"].sum(axis=(0, 1), dtype=np.uint64),
                          got["one_cell"].sum(axis=0, dtype=np.uint64)), f"{what}: sums summed != one-cell grid summed"
    assert np.array_equal(got["times"], fold_times(bits, case["t0"])), f"{what}: times != fold of the mask"
    if case["min_area"] == 1:
        if got["labels"] is not None:
            assert np.array_equal(got["labels"] != 0, bits), f"{what}: labels do not cover the mask"
        if (got["counts"] <= case["max_boxes"]).all():
            assert np.array_equal(got["boxes"][..., 4].sum(axis=1, dtype=np.uint64), mask.counts()), \
                f"{what}: box areas != mask popcount"


def run_case(case, monkeypatch, **kw):
    """One operator, the five products through the drawn entry points."""
    with monkeypatch.context() as m:
        if case["part_frames"] is None:
            m.delenv("DIPS_PIXEL_PART_FRAMES", raising=False)
        else:
            m.setenv("DIPS_PIXEL_PART_FRAMES", str(case["part_frames"]))
        op = make_op(case, **kw)
        try:
            return run_device(op, case) if case["device"] else run_host(op, case)
        finally:
            op.close()


@pytest.mark.parametrize("group", range(GROUPS))
def test_random_regional_cases_match_oracle(group, monkeypatch):
    failures = []
    for case in group_cases(group):
        what = str(describe(case))
        got = run_case(case, monkeypatch)
        try:
            check_against_oracle(got, reference(case), what)
            check_identities(got, case, what)
        except AssertionError as e:  # every case of the group is run; the message names each that fails
            failures.append(str(e).split("\nassert ")[0])
    assert not failures, "\n".join(failures)


NARROW = [(1, (0, 4, 1, 20), 1, 1),  # case 7 of the seed: rows 21 and 22 of the frame were left out
          (1, None, 5, 1), (2, (0, 3, 2, 21), 4, 2), (2, (1, 0, 1, 24), 3, 1), (3, None, 2, 3)]


@pytest.mark.parametrize("w,roi,rows,cols", NARROW)
@pytest.mark.parametrize("c", [3, 4])
def test_grid_of_frames_narrower_than_a_vec(c, w, roi, rows, cols):
    """The fast grid kernel leaves out every partial vec that would read past
    the frame's end: in frames narrower than 3 pixels those of up to three
    rows before the last one too, which the host has to add like the last
    row's (found by case 7 of the random test: RGB8, 1x24, roi (0, 4, 1, 20),
    one cell, two pixels short in every field)."""
    h, n = 24, 8
    frames = np.random.default_rng([0xED6E, c, w]).integers(0, 256, (n, h, w, c), dtype=np.uint8)
    case = dict(c=c, mode=1, chroma=1, tau=8 / 255, w=w, h=h, n=n, roi=roi, rows=rows, cols=cols, frames=frames,
                ref=None)
    op = make_op(case)
    try:
        got = op.grid(frames, rows, cols, roi=roi).as_array()
    finally:
        op.close()
    want = grid_reference(case)
    assert want[1:, ..., 2].min() > 0  # every cell counts pixels in every frame after the first
    assert np.array_equal(got, want), str(describe(case))


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("grid", "sums", "times", "counts", "boxes", "labels")) \
        and np.array_equal(a["mask"].bits, b["mask"].bits)


def run_edge(case, **kw):
    """grid, pixel_sums, change_mask, pixel_times and change_boxes of one operator on host arrays."""
    frames, roi = case["frames"], case["roi"]
    op = make_op(case, **kw)
    try:
        out = {"grid": op.grid(frames, case["rows"], case["cols"], roi=roi).as_array(),
               "sums": op.pixel_sums(frames, roi=roi).as_array(),
               "mask": op.change_mask(frames, roi=roi),
               "times": op.pixel_times(frames, roi=roi, t0=case["t0"]).as_array()}
        found = op.change_boxes(frames.copy(), roi=roi, connectivity=case["connectivity"], min_area=case["min_area"],
                                max_boxes=case["max_boxes"], labels=case["labels"])
    finally:
        op.close()
    out["counts"], out["boxes"], out["labels"] = found.as_arrays()
    return out


def check_edge(got, want, case, what):
    for k in ("grid", "sums", "times", "counts", "boxes", "labels"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} {_where(got[k], want[k])}"
    assert np.array_equal(got["mask"].bits, want["mask"]), f"{what}: mask"
    bits = unpack_mask(got["mask"].bits, case["roi"][2])
    assert np.array_equal(got["mask"].counts(), got["grid"][..., 2].sum(axis=(1, 2), dtype=np.uint64)), what
    assert np.array_equal(bits.sum(axis=0, dtype=np.uint64), got["sums"][..., 2]), what
    assert np.array_equal(got["sums"].sum(axis=(0, 1), dtype=np.uint64),
                          got["grid"].sum(axis=(0, 1, 2), dtype=np.uint64)), what
    assert np.array_equal(got["times"], fold_times(bits, case["t0"])), what
    assert np.array_equal(got["labels"] != 0, bits), what
    if (got["counts"] <= case["max_boxes"]).all():
        assert np.array_equal(got["boxes"][..., 4].sum(axis=1, dtype=np.uint64), got["mask"].counts()), what


@pytest.mark.parametrize("which", ["below", "at", "above"])
@pytest.mark.parametrize("k", [4, 16, 31, 64])
@pytest.mark.parametrize("c,chroma", [(1, 0)] + [(c, ch) for c in (3, 4) for ch in range(4)])
@pytest.mark.parametrize("mode", [0, 1])
def test_threshold_edges(c, mode, chroma, k, which):
    """step_walk(k) at 37x13x9, roi (3, 2, 33, 10), at f32(k / 255) and its
    two f32 neighbours; RGB8 / RGBA8 also through the generic and the
    cross-check paths."""
    case = edge_case(c, mode, chroma, k, which)
    what = str(describe(case))
    want = reference(case)
    got = run_edge(case)
    check_edge(got, want, case, what)
    if c != 1:
        generic = run_edge(case, force_generic=True)
        cross = run_edge(case, crosscheck=True)
        assert _same(generic, got), f"{what}: generic != fast"
        assert _same(cross, got), f"{what}: crosscheck != fast"
