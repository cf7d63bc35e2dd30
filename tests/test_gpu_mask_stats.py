"""dips_mask_counts and dips_mask_pixel_times on the GPU against
tests/_mask_stats_ref.py, every output value.  The shapes are the smallest at
which each mechanism of mask_stats.hip can go wrong: word and pad edges, cells
that share, straddle and span words, column chunks and row bands, more items
than blocks (a block's second trip through its item loop), the seams of
the frame parts (series_sched.h mask_times_geometry, read from the header
itself), a clip fed in chunks, t0 at its limit, the refused arguments, parity
with the fused products on the raw change mask, the one-call pipeline and a 4K
frame."""
import functools
import os

import numpy as np
import pytest

import _components_ref as cref
import _mask_stats_ref as sref
import _morph_ref as mref
import _reuse_cases as rc
import _vote_ref as vref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")
PX, CHUNK_CELLS, MIN_BAND_WORDS = sref.kernel_constants(CSRC)
DENSITIES = (0.0, 0.01, 0.5, 1.0)
POISON = 0xA5A5A5A5


@pytest.fixture(scope="module")
def op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    yield o
    o.close()


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_bits(n, h, w, density, seed=0):
    if density >= 1.0:
        return frozen(np.ones((n, h, w), dtype=bool))
    return frozen(np.random.default_rng([107, seed, n, h, w]).random((n, h, w)) < density)


def mask_of(bits, pad=1):
    """The ChangeMask of bool bits [n, h, w]; pad = 1: every pad bit set."""
    from dips_amd import ChangeMask
    return ChangeMask(cref.pack(bits, pad), bits.shape[2])


def same(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())


def check_all(op, bits, rows=1, cols=1, t0=0):
    """Counts, times and sums of the host path == the reference, pad bits set."""
    m = mask_of(bits)
    same(op.mask_counts(m, rows, cols), sref.counts_bits(bits, rows, cols), "counts")
    same(op.mask_times(m, t0=t0).as_array(), sref.times_bits(bits, t0), "times")
    same(op.mask_sums(m), sref.sums_bits(bits), "sums")


# -- word and pad edges --------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(w, h) for w in (1, 31, 32, 33, 65, 100, 257) for h in (1, 3, 17)])
def test_word_and_pad_edges(op, w, h):
    for n in (0, 1, 2, 7, 40):
        for d, density in enumerate(DENSITIES):
            check_all(op, random_bits(n, h, w, density, seed=d), t0=3)


@pytest.mark.parametrize("w", [1, 33, 63, 97])
def test_garbage_pad_bits_change_nothing(op, w):
    bits = random_bits(7, 3, w, 0.5, seed=1)
    assert not np.array_equal(cref.pack(bits, 1), cref.pack(bits))
    for pad in (0, 1):
        m = mask_of(bits, pad)
        same(op.mask_counts(m), sref.counts_bits(bits), "counts")
        same(op.mask_times(m).as_array(), sref.times_bits(bits), "times")
        same(op.mask_sums(m), sref.sums_bits(bits), "sums")


# -- grids ---------------------------------------------------------------------------------

GRIDS = [(37, 5, 1, 1), (37, 5, 5, 37),      # every cell one pixel, many cells share a word
         (100, 17, 3, 7),                    # cells 14 or 15 wide straddle words; rows do not divide h
         (200, 17, 1, 2), (200, 17, 4, 2),   # cells span several words
         (257, 17, 17, 257), (257, 17, 5, 9),
         (2500, 2, 1, 2500), (2500, 3, 2, 1200),  # more columns than a block's LDS holds: two, three chunks
         (4100, 300, 2, 3), (4100, 300, 1, 1)]    # several bands per grid row: the blocks add with atomics


@pytest.mark.parametrize("w,h,rows,cols", GRIDS)
def test_grids(op, w, h, rows, cols):
    for n, density in ((3, 0.5), (2, 1.0), (1, 0.01)):
        bits = random_bits(n, h, w, density, seed=rows)
        got = op.mask_counts(mask_of(bits), rows, cols)
        same(got, sref.counts_bits(bits, rows, cols), (rows, cols, n))
        assert np.array_equal(got.sum(axis=(1, 2), dtype=np.uint64), bits.sum(axis=(1, 2)))
    if (rows, cols) == (h, w):  # the mask unpacked to u32
        assert np.array_equal(got, bits.astype(np.uint32))


@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    return sref.build_geometry(tmp_path_factory.mktemp("mask_stats_sched"), CSRC)


def test_the_banded_and_chunked_grids_are_what_they_claim(sched):
    """The shapes above reach two or more column chunks and two or more bands
    for any realistic number of resident blocks."""
    for res in (256, 2048, 8192):
        q = sref.counts_geometry(sched, [(2500, 2, 1, 2500, 3, CHUNK_CELLS, MIN_BAND_WORDS, res),
                                         (4100, 300, 2, 3, 3, CHUNK_CELLS, MIN_BAND_WORDS, res)])
        assert q[0]["col_chunks"] >= 2 and q[1]["bands"] >= 2


# -- more items than blocks: the second trip of a block's item loop ------------------------

@pytest.mark.parametrize("case", rc.COUNTS_CASES, ids=lambda c: c[0])
def test_counts_with_more_items_than_blocks(op, sched, case):
    """mask_counts_kernel launches min(items, 2 * resident blocks) blocks and
    a block loops it += gridDim.x, clearing its LDS cells at the top of every
    trip.  A CU holds at most 2,048 threads, eight blocks of 256, so 8 * CUs
    bounds the resident blocks: each case has more items than twice that
    (test_mask_reuse_cpu.py shows it for 256, 2,048 and 8,192 without a GPU)."""
    import torch
    _, w, h, rows, cols, n, _ = case
    resident = 8 * torch.cuda.get_device_properties(op._dev.device).multi_processor_count
    q = sref.counts_geometry(sched, rc.counts_rows([case], CHUNK_CELLS, MIN_BAND_WORDS, resident))[0]
    rc.check_counts_geometry(case, q, resident)
    for density in (0.5, 1.0, 0.01):
        bits = random_bits.__wrapped__(n, h, w, density, seed=rows)  # up to 41 MB: not kept
        got = op.mask_counts(mask_of(bits), rows, cols)
        same(got, sref.counts_bits(bits, rows, cols), (case[0], density))
        assert np.array_equal(got.sum(axis=(1, 2), dtype=np.uint64), bits.sum(axis=(1, 2)))
        assert got.any()


def test_counts_device_path_writes_every_entry_and_nothing_else(op):
    import torch
    for (w, h, rows, cols, n) in ((100, 17, 3, 7, 7), (4100, 300, 2, 3, 2), (37, 5, 5, 37, 3)):
        bits = random_bits(n, h, w, 0.5, seed=9)
        mask = torch.from_numpy(cref.pack(bits, 1)).cuda()
        raw = torch.full((n * rows * cols + 2,), POISON - (1 << 32), dtype=torch.int32, device="cuda")
        out = raw[1:-1].view(n, rows, cols)
        op.run_mask_counts_device(mask, w, out, rows, cols)
        torch.cuda.synchronize()
        got = raw.cpu().numpy().view(np.uint32)
        assert got[0] == POISON and got[-1] == POISON
        same(got[1:-1].reshape(n, rows, cols), sref.counts_bits(bits, rows, cols), (w, h, rows, cols))
    with pytest.raises(ValueError):
        op.run_mask_counts_device(mask, 37, out[:2], 5, 37)
    with pytest.raises(ValueError):
        op.run_mask_counts_device(mask, 37, out, 6, 37)


# -- the seams of the frame parts ----------------------------------------------------------

def test_part_seams(op, sched):
    import torch
    w, h, n = 33, 2, 600
    cuts = set()
    for times, sums in ((True, True), (True, False), (False, True)):
        cuts |= {(q["parts"], q["part_frames"]) for q in sref.times_geometry(
            sched, [(sref.frame_slots(w, h, PX), n, sref.summary_bytes(w, h, times, sums), sref.PARTS_BYTES, res)
                    for res in (256, 1024, 4096, 8192, 16384)])}
    assert len(cuts) == 1  # one tile: the cut does not depend on the device's wave slots
    parts, L = cuts.pop()
    assert parts >= 2 and (parts - 1) * L < n
    bits = np.array(random_bits(n, h, w, 0.5, seed=4))
    bits[:, 0, 0] = True                       # set in every frame: one run across every part boundary
    bits[:, 0, 1] = True
    bits[L, 0, 1] = False                      # ... but a part's first frame
    bits[:, 0, 2] = True
    bits[2 * L - 1, 0, 2] = False              # ... but a part's last frame
    bits[:, 1, 32] = False                     # never set
    bits[:, 1, 3] = False
    bits[L - 3:3 * L + 2, 1, 3] = True         # one run that holds a whole part and ends inside another
    bits[:, 1, 4] = False
    bits[[L - 1, L], 1, 4] = True              # a run of two across one boundary
    want_t, want_s = sref.times_bits(bits, 7), sref.sums_bits(bits)
    assert want_t[2:, 0, 0].tolist() == [n, n] and want_t[2:, 0, 1].tolist() == [n - L - 1, n - L - 1]
    assert want_t[2:, 0, 2].tolist() == [n - 2 * L, n - 2 * L] and want_t[:, 1, 32].tolist() == [sref.NONE, sref.NONE, 0, 0]
    assert want_t[:, 1, 3].tolist() == [7 + L - 3, 7 + 3 * L + 1, 2 * L + 5, 0] and want_t[2, 1, 4] == 2
    m = mask_of(bits)
    same(op.mask_times(m, t0=7).as_array(), want_t, "times")
    same(op.mask_sums(m), want_s, "sums")
    # the device path: times only, sums only, both; then the same folded onto an earlier state
    mask = torch.from_numpy(m.bits).cuda()
    head = random_bits(5, h, w, 0.5, seed=5)
    head_t, head_s = sref.times_bits(head, 2), sref.sums_bits(head)
    for with_t, with_s in ((True, False), (False, True), (True, True)):
        t = torch.full((4, h, w), -1, dtype=torch.int32, device="cuda") if with_t else None
        s = torch.full((h, w), -1, dtype=torch.int32, device="cuda") if with_s else None
        op.run_mask_times_device(mask, w, t, s, t0=7)
        if with_t:
            same(t.cpu().numpy().view(np.uint32), want_t, "times")
            t.copy_(torch.from_numpy(head_t.view(np.int32)))
        if with_s:
            same(s.cpu().numpy().view(np.uint32), want_s, "sums")
            s.copy_(torch.from_numpy(head_s.view(np.int32)))
        op.run_mask_times_device(mask, w, t, s, t0=7, accumulate=True)
        if with_t:
            same(t.cpu().numpy().view(np.uint32), sref.times_bits(bits, 7, head_t), "times onto a state")
        if with_s:
            same(s.cpu().numpy().view(np.uint32), sref.sums_bits(bits, head_s), "sums onto a state")


# -- chunked equals whole ------------------------------------------------------------------

CHUNKS = (1, 7, 0, 32)


@pytest.mark.parametrize("w,h", [(65, 3), (33, 2)])
def test_chunked_equals_whole_host(op, w, h):
    from dips_amd import ChangeMask
    bits = random_bits(40, h, w, 0.6, seed=6)
    m = mask_of(bits)
    want_t, want_s = sref.times_bits(bits, 11), sref.sums_bits(bits)
    same(op.mask_times(m, t0=11).as_array(), want_t, "one call")
    state, s, at = None, None, 0
    for k in CHUNKS:
        part = ChangeMask(m.bits[at:at + k], w)
        state = op.mask_times(part, t0=11 + at, into=state)
        s = op.mask_sums(part, into=s)
        at += k
    assert at == 40
    same(state.as_array(), want_t, "times in chunks")
    same(s, want_s, "sums in chunks")
    # one frame per call
    state, s = None, None
    for t in range(40):
        state = op.mask_times(ChangeMask(m.bits[t:t + 1], w), t0=11 + t, into=state)
        s = op.mask_sums(ChangeMask(m.bits[t:t + 1], w), into=s)
    same(state.as_array(), want_t, "times frame by frame")
    same(s, want_s, "sums frame by frame")


@pytest.mark.parametrize("with_t,with_s", [(True, False), (False, True), (True, True)])
def test_chunked_equals_whole_device(op, with_t, with_s):
    import torch
    w, h = 65, 3
    bits = random_bits(40, h, w, 0.6, seed=6)
    mask = torch.from_numpy(cref.pack(bits, 1)).cuda()
    t = torch.full((4, h, w), -1, dtype=torch.int32, device="cuda") if with_t else None
    s = torch.full((h, w), -1, dtype=torch.int32, device="cuda") if with_s else None
    at = 0
    for i, k in enumerate(CHUNKS):  # the first call overwrites the poison
        op.run_mask_times_device(mask[at:at + k], w, t, s, t0=11 + at, accumulate=i > 0)
        at += k
    torch.cuda.synchronize()
    if with_t:
        same(t.cpu().numpy().view(np.uint32), sref.times_bits(bits, 11), "times")
    if with_s:
        same(s.cpu().numpy().view(np.uint32), sref.sums_bits(bits), "sums")


def test_no_frames_writes_the_initial_state_or_nothing(op):
    import torch
    from dips_amd import ChangeMask
    w, h = 37, 3
    empty = ChangeMask(np.zeros((0, h, 8), dtype=np.uint8), w)
    same(op.mask_times(empty).as_array(), sref.initial_times(h, w), "initial times")
    same(op.mask_sums(empty), np.zeros((h, w), dtype=np.uint32), "initial sums")
    assert op.mask_counts(empty, 2, 3).shape == (0, 2, 3)
    state = sref.times_bits(random_bits(5, h, w, 0.5), 0)
    same(op.mask_times(empty, t0=5, into=op.mask_times(mask_of(random_bits(5, h, w, 0.5)))).as_array(), state, "kept")
    # the device path
    t = torch.full((4, h, w), 77, dtype=torch.int32, device="cuda")
    s = torch.full((h, w), 77, dtype=torch.int32, device="cuda")
    none = torch.zeros((0, h, 8), dtype=torch.uint8, device="cuda")
    op.run_mask_times_device(none, w, t, s, accumulate=True)
    assert (t == 77).all() and (s == 77).all()
    op.run_mask_times_device(none, w, t, s)
    same(t.cpu().numpy().view(np.uint32), sref.initial_times(h, w), "initial times")
    assert (s == 0).all()


# -- t0 ------------------------------------------------------------------------------------

def test_t0_at_its_limit(op):
    from dips_amd import _lib
    w, h, n = 37, 3, 6
    bits = random_bits(n, h, w, 0.5, seed=8)
    m = mask_of(bits)
    t0 = 0xFFFFFFFF - n
    got = op.mask_times(m, t0=t0).as_array()
    same(got, sref.times_bits(bits, t0), "t0 + n = 0xFFFFFFFF")
    assert (got[1] == 0xFFFFFFFE).any()  # the largest index there is
    hd = op._host
    times = np.full((4, h, w), POISON, dtype=np.uint32)
    sums = np.full((h, w), POISON, dtype=np.uint32)
    st = hd._lib.dips_mask_pixel_times(hd.ptr, m.bits.ctypes.data, n, w, h, t0 + 1, 0, times.ctypes.data, sums.ctypes.data)
    assert st == _lib.DIPS_ERR_INVALID and (times == POISON).all() and (sums == POISON).all()
    # the sums alone have no index to overflow
    hd.check(hd._lib.dips_mask_pixel_times(hd.ptr, m.bits.ctypes.data, n, w, h, 0xFFFFFFFF, 0, None, sums.ctypes.data))
    same(sums, sref.sums_bits(bits), "sums at t0 = 0xFFFFFFFF")
    with pytest.raises(ValueError):
        op.mask_times(m, t0=1 << 32)


# -- refusals ------------------------------------------------------------------------------

def test_refused_arguments_leave_the_outputs_untouched(op):
    from dips_amd import DipsError, _lib
    n, h, w = 6, 5, 37
    mask = cref.pack(random_bits(n, h, w, 0.5))
    nm, npx = mask.size, h * w
    # one buffer: mask | times | sums (the counts use the times' range)
    buf = np.full(nm + 4 * 5 * npx, 0xA5, dtype=np.uint8)
    buf[:nm] = mask.reshape(-1)
    before = buf.copy()
    hd = op._host
    M = buf.ctypes.data
    T, S = M + nm, M + nm + 16 * npx
    counts_cases = [(None, n, w, h, 1, 1, T), (M, n, w, h, 1, 1, None), (M, n, 0, h, 1, 1, T), (M, n, w, 0, 1, 1, T),
                    (M, n, 1 << 15, 1 << 15, 1, 1, T), (M, n, w, h, 0, 1, T), (M, n, w, h, 1, 0, T),
                    (M, n, w, h, h + 1, 1, T), (M, n, w, h, 1, w + 1, T), (M, 1 << 28, w, h, 2, 2, T),
                    (M, n, w, h, 1, 1, M), (M, n, w, h, 1, 1, M + nm - 1), (M, n, w, h, h, w, M - 4 * n * npx + 1)]
    for c in counts_cases:
        st = hd._lib.dips_mask_counts(hd.ptr, *c)
        assert st == _lib.DIPS_ERR_INVALID, c[1:6]
        with pytest.raises(DipsError, match="mask_counts:"):
            hd.check(st)
        assert np.array_equal(buf, before)
    assert hd._lib.dips_mask_counts(hd.ptr, M, 0, w, h, 0, 1, T) == _lib.DIPS_ERR_INVALID  # bad scalars, no frames
    assert hd._lib.dips_mask_counts(hd.ptr, None, 0, w, h, 1, 1, None) == 0
    #              mask n  w  h  t0 acc times sums
    times_cases = [(M, n, w, h, 0, 0, None, None), (None, n, w, h, 0, 0, T, S), (M, n, 0, h, 0, 0, T, S),
                   (M, n, w, 0, 0, 0, T, S), (M, n, 1 << 15, 1 << 15, 0, 0, T, S), (M, n, w, h, 0xFFFFFFFF - n + 1, 0, T, S),
                   (M, n, w, h, 0xFFFFFFFF, 1, T, None), (M, n, w, h, 0, 0, M, S), (M, n, w, h, 0, 0, T, M + nm - 1),
                   (M, n, w, h, 0, 1, M + nm - 1, None), (M, n, w, h, 0, 0, T, T), (M, n, w, h, 0, 0, T, S - 1),
                   (M, n, w, h, 0, 0, S - 16 * npx + 1, S), (None, 0, w, h, 0, 0, None, None), (None, 0, w, h, 0, 1, T, T)]
    for c in times_cases:
        st = hd._lib.dips_mask_pixel_times(hd.ptr, *c)
        assert st == _lib.DIPS_ERR_INVALID, c[1:6]
        with pytest.raises(DipsError, match="mask_pixel_times:"):
            hd.check(st)
        assert np.array_equal(buf, before)
    # touching, not overlapping, ranges are fine
    hd.check(hd._lib.dips_mask_pixel_times(hd.ptr, M, n, w, h, 0, 0, T, S))
    same(buf[nm:nm + 16 * npx].view(np.uint32).reshape(4, h, w), sref.times(mask, w), "times")
    same(buf[nm + 16 * npx:].view(np.uint32).reshape(h, w), sref.sums(mask, w), "sums")
    hd.check(hd._lib.dips_mask_counts(hd.ptr, M, n, w, h, 1, 1, T))
    same(buf[nm:nm + 4 * n].view(np.uint32).reshape(n, 1, 1), sref.counts(mask, w), "counts")
    assert np.array_equal(buf[:nm], before[:nm])


def test_misaligned_or_overlapping_device_pointers_are_refused(op):
    import torch
    from dips_amd import _lib
    n, h, w = 4, 5, 37
    mask = cref.pack(random_bits(n, h, w, 0.5))
    npx = h * w
    src = torch.from_numpy(np.concatenate([mask.reshape(-1), np.zeros(8, dtype=np.uint8)])).cuda()
    dst = torch.full((20 * npx + 16,), 7, dtype=torch.uint8, device="cuda")
    hd = op._dev
    S, D = src.data_ptr(), dst.data_ptr()
    T, U = D, D + 16 * npx
    for dm, dt, ds in ((1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2), (3, 3, 3)):
        st = hd._lib.dips_mask_pixel_times(hd.ptr, S + dm, n, w, h, 0, 0, T + dt, U + ds)
        assert st == _lib.DIPS_ERR_INVALID, (dm, dt, ds)
    for dm, dc in ((1, 0), (0, 1), (0, 2), (2, 2)):
        assert hd._lib.dips_mask_counts(hd.ptr, S + dm, n, w, h, 1, 1, D + dc) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_pixel_times(hd.ptr, S, n, w, h, 0, 0, None, U + 2) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_pixel_times(hd.ptr, S, n, w, h, 0, 0, S, U) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_pixel_times(hd.ptr, S, n, w, h, 0, 0, T, S + 4) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_pixel_times(hd.ptr, S, n, w, h, 0, 0, T, T + 4) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_pixel_times(hd.ptr, S, n, w, h, 0, 1, T, U - 4) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_counts(hd.ptr, S, n, w, h, 1, 1, S + 4) == _lib.DIPS_ERR_INVALID
    torch.cuda.synchronize()
    assert (dst == 7).all() and np.array_equal(src.cpu().numpy()[:mask.size], mask.reshape(-1))
    # the operator refuses the same before the library sees them
    m = src[:mask.size].view(n, h, -1)
    t = dst[:16 * npx].view(torch.int32).view(4, h, w)
    s = dst[16 * npx:20 * npx].view(torch.int32).view(h, w)
    for bad in (dict(), dict(times_out=t[:3]), dict(sums_out=t[0, :2]), dict(times_out=t, sums_out=t[0]),
                dict(times_out=t, t0=0xFFFFFFFF), dict(sums_out=s, t0=-1)):
        with pytest.raises(ValueError):
            op.run_mask_times_device(m, w, **bad)
    op.run_mask_times_device(m, w, t, s)
    same(t.cpu().numpy().view(np.uint32), sref.times(mask, w), "times")
    same(s.cpu().numpy().view(np.uint32), sref.sums(mask, w), "sums")


def test_kernel_time_has_one_entry_per_call():
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    w, h = 33, 2
    bits = random_bits(600, h, w, 0.45)
    mask = torch.from_numpy(cref.pack(bits)).cuda()
    t = torch.zeros((4, h, w), dtype=torch.int32, device="cuda")
    s = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    c = torch.zeros((600, 1, 1), dtype=torch.int32, device="cuda")
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255, time_kernel=True)
    try:
        o.run_mask_times_device(mask, w, t, s)        # two launches (parts, combine), one entry
        o.run_mask_times_device(mask[:3], w, t, None)  # one launch
        o.run_mask_counts_device(mask, w, c)
        ms, launches = o.kernel_time()
        each = o.kernel_times()
    finally:
        o.close()
    assert launches == 3 and len(each) == 3 and ms > 0.0 and all(x > 0.0 for x in each)
    same(c.cpu().numpy().view(np.uint32), sref.counts_bits(bits), "counts")
    same(s.cpu().numpy().view(np.uint32), sref.sums_bits(bits), "sums")


# -- parity with the fused products on the raw change mask ---------------------------------

def moving_clip(w, h, n, seed=0):
    """RGB8 frames: a noisy background and two rectangles that move."""
    rng = np.random.default_rng([109, w, h, n, seed])
    base = rng.integers(30, 200, (h, w, 3), dtype=np.uint8)
    frames = np.repeat(base[None], n, axis=0)
    frames = np.clip(frames.astype(np.int16) + rng.integers(-14, 15, frames.shape), 0, 255).astype(np.uint8)
    for t in range(n):
        frames[t, 2 + t // 2:9 + t // 2, 5 + 2 * t:20 + 2 * t] = 250
        frames[t, h - 8:h - 2, max(0, w - 12 - 3 * t):w - 3 * t] = 5
    return frames


@pytest.mark.parametrize("mode_name", ["Overall", "PerFrame"])
@pytest.mark.parametrize("roi", [None, (3, 2, 60, 15)])
def test_parity_with_the_fused_products(mode_name, roi):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    frames = moving_clip(67, 19, 12)
    o = DiffSeriesOperator(PixelFormat.RGB8, getattr(Mode, mode_name), 8 / 255)
    try:
        m = o.change_mask(frames, roi=roi)
        assert m.bits.any()
        for rows, cols in ((1, 1), (3, 5), (4, 7)):
            want = o.grid(frames, rows, cols, roi=roi).count
            got = o.mask_counts(m, rows, cols)
            assert want.any() and np.array_equal(got.astype(np.uint64), want), (rows, cols)
        assert np.array_equal(o.mask_sums(m).astype(np.uint64), o.pixel_sums(frames, roi=roi).count)
        same(o.mask_times(m, t0=100).as_array(), o.pixel_times(frames, roi=roi, t0=100).as_array(), "times")
    finally:
        o.close()


# -- the one-call pipeline -----------------------------------------------------------------

def test_change_activity_equals_the_stages_one_by_one():
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, MorphShape, PixelFormat
    frames = moving_clip(96, 64, 14, seed=1)
    steps = [(MorphOp.Open, MorphShape.Box, 1, 1)]
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.Overall, 8 / 255)
    try:
        for roi in (None, (5, 3, 80, 50)):
            counts, times, sums = o.change_activity(frames, roi=roi, rows=3, cols=4, sigma_delta=True, vote=3, morph=steps)
            raw, _ = o.sigma_delta_mask(frames, roi=roi)
            voted, _ = o.mask_vote(raw, 3)
            final = o.mask_morph(voted, MorphOp.Open, 1, 1)
            # the stages are what their specifications say
            assert np.array_equal(voted.bits, vref.vote(raw.bits, raw.width, 3, 2)[0])
            assert np.array_equal(final.bits, mref.morph(voted.bits, raw.width, int(MorphOp.Open), int(MorphShape.Box), 1, 1))
            bits = sref.unpack(final.bits, final.width)
            assert bits.any() and not np.array_equal(final.bits, raw.bits)
            same(counts, sref.counts_bits(bits, 3, 4), "counts")
            same(times.as_array(), sref.times_bits(bits), "times")
            same(sums, sref.sums_bits(bits), "sums")
            same(counts, o.mask_counts(final, 3, 4), "counts, stage by stage")
            same(times.as_array(), o.mask_times(final).as_array(), "times, stage by stage")
            same(sums, o.mask_sums(final), "sums, stage by stage")
        # the plain change mask, and the refused arguments
        counts, times, sums = o.change_activity(frames[1:], ref=frames[0])
        m = o.change_mask(frames[1:], ref=frames[0])
        assert np.array_equal(counts[:, 0, 0], m.counts()) and np.array_equal(sums, sref.sums(m.bits, m.width))
        same(times.as_array(), o.pixel_times(frames[1:], ref=frames[0]).as_array(), "times")
        for bad in (dict(rows=0), dict(cols=97), dict(rows=65), dict(vote=32), dict(sigma_delta=True, background=3)):
            with pytest.raises(ValueError):
                o.change_activity(frames, **bad)
    finally:
        o.close()


# -- the 4K width --------------------------------------------------------------------------

def test_4k_frames(op):
    w, h, n = 3840, 2160, 6
    bits = np.array(random_bits(n, h, w, 0.3, seed=2))
    bits[:, 5, 3839] = True
    bits[2, 5, 3839] = False
    m = mask_of(bits)
    want_t = sref.times_bits(bits, 1000)
    same(op.mask_times(m, t0=1000).as_array(), want_t, "times")
    assert want_t[:, 5, 3839].tolist() == [1000, 1005, 3, 3]
    same(op.mask_sums(m), sref.sums_bits(bits), "sums")
    for rows, cols in ((1, 1), (9, 16), (7, 11)):
        same(op.mask_counts(m, rows, cols), sref.counts_bits(bits, rows, cols), (rows, cols))
