"""dips_mask_morph on the GPU against tests/_morph_ref.py: every byte of the
output, pad bytes included.  The shapes are the smallest at which each
mechanism of mask_morph.hip can go wrong: word and row edges with radii beyond
the region, the seams of its 32-row x 32-word tiles with features on both
sides of them and within two radii, pad bits, frame ends, unequal radii, more
frames than a 16-bit grid dimension, one 4K frame, the pointer kinds, the
refused arguments, the path through change_boxes and a randomized draw."""
import functools

import numpy as np
import pytest

import _components_ref as cref
import _morph_ref as mref

pytestmark = pytest.mark.gpu

TH, TW = 32, 32  # mask_morph.hip's tile: rows x 32-bit words
OPS = (mref.ERODE, mref.DILATE, mref.OPEN, mref.CLOSE)
SHAPES = (mref.BOX, mref.DIAMOND)


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
    return frozen(np.random.default_rng([59, seed, n, h, w]).random((n, h, w)) < density)


def run(op, mask_bytes, w, mop, shape=mref.BOX, rx=1, ry=None):
    from dips_amd import ChangeMask
    r = op.mask_morph(ChangeMask(np.ascontiguousarray(mask_bytes), w), mop, rx, ry, shape)
    assert r.width == w
    return r.bits


def check(op, bits, mop, shape=mref.BOX, rx=1, ry=None, pad=0):
    """GPU == reference for bool bits [n, h, w], byte for byte; returns the
    reference's bits."""
    bits = np.asarray(bits, dtype=bool)
    w = bits.shape[2]
    want_bits = mref.morph_bits(bits, mop, shape, rx, ry)
    want = cref.pack(want_bits)
    got = run(op, cref.pack(bits, pad), w, mop, shape, rx, ry)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), (mref.OP_NAMES[mop], mref.SHAPE_NAMES[shape], rx, ry,
                                       np.argwhere(got != want)[:5].tolist())
    return want_bits


# -- word and row edges ---------------------------------------------------------

@pytest.mark.parametrize("h", [1, 2, 3, 29])
@pytest.mark.parametrize("w", [1, 2, 31, 32, 33, 63, 64, 65, 97])
def test_word_and_row_edges(op, w, h):
    corners = np.zeros((h, w), dtype=bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    bits = np.stack([random_bits(1, h, w, 0.3)[0], random_bits(1, h, w, 0.8)[0], np.ones((h, w), dtype=bool),
                     np.zeros((h, w), dtype=bool), corners, ~corners])
    for mop in OPS:
        for shape in SHAPES:
            for r in (1, 15):  # 15: beyond the region in at least one direction
                check(op, bits, mop, shape, r, r)


# -- the seams of the kernel's tiles ----------------------------------------------

def _seam_features(h, w, r):
    """A set pixel on both sides of every tile seam, and at distances r and
    2 r (what open and close reach) from it."""
    def near(seams, size):
        out = {0, size - 1}
        for s in seams:
            out |= {s - 1, s, s - r, s + r - 1, s - 2 * r, s + 2 * r - 1, s - 2 * r - 1, s + 2 * r}
        return sorted(v for v in out if 0 <= v < size)

    rows = near(range(TH, h, TH), h)
    cols = near(range(32 * TW, w, 32 * TW), w)
    x = np.zeros((h, w), dtype=bool)
    x[np.ix_(rows, cols)] = True
    return x


@pytest.mark.parametrize("h", [TH - 1, TH, TH + 1, 2 * TH + 1])
@pytest.mark.parametrize("w", [32 * TW - 1, 32 * TW, 32 * TW + 1])
def test_tile_seams(op, w, h):
    for r in (1, 15):
        f = _seam_features(h, w, r)
        blocks = np.zeros((h, w), dtype=bool)  # blocks that open keeps and close joins, across the seams
        blocks[max(0, h - 2 * r - 3):, 32 * TW - 3 * r - 2:32 * TW - r] = True
        blocks[max(0, h - 2 * r - 3):, 32 * TW - r + 1:] = True
        blocks[:TH - 1, :3] = True
        bits = np.stack([f, ~f, blocks, ~blocks, random_bits(1, h, w, 0.5)[0]])
        for mop in OPS:
            for shape in SHAPES:
                got = check(op, bits, mop, shape, r, r)
                assert got.any() and not got.all()
    check(op, bits, mref.CLOSE, mref.BOX, 15, 3)
    check(op, bits, mref.OPEN, mref.BOX, 2, 15)


# -- pad bits, frame ends, radii -----------------------------------------------------

@pytest.mark.parametrize("w", [1, 33, 63, 97])
def test_garbage_pad_bits_change_nothing(op, w):
    bits = random_bits(3, 5, w, 0.5, seed=1)
    mask = cref.pack(bits)
    rng = np.random.default_rng([61, w])
    garbage = mask | (cref.pack(np.zeros_like(bits), pad=1) & rng.integers(0, 256, mask.shape, dtype=np.uint8))
    assert not np.array_equal(garbage, mask) and np.array_equal(cref.unpack(garbage, w), bits)
    for mop in OPS:
        for shape in SHAPES:
            clean = run(op, mask, w, mop, shape, 2, 2)
            assert np.array_equal(run(op, garbage, w, mop, shape, 2, 2), clean)
            assert np.array_equal(clean, mref.morph(mask, w, mop, shape, 2, 2))
            check(op, bits, mop, shape, 2, 2, pad=1)


def test_frames_and_row_ends_are_independent(op):
    bits = np.zeros((3, 4, 33), dtype=bool)
    bits[0, 3, :] = True    # the last row of frame 0
    bits[1, 0, 32] = True   # a row's last pixel: not the next row's first
    bits[2, 0, :] = True    # the first row of frame 2
    for shape in SHAPES:
        got = check(op, bits, mref.DILATE, shape, 2, 2)
        assert not got[1, 3].any() and not got[1, 1:, :30].any() and got[1, 0, 30:].all()
        inv = check(op, ~bits, mref.ERODE, shape, 2, 2)
        assert np.array_equal(inv, ~got)
        check(op, bits, mref.CLOSE, shape, 3, 3)
        check(op, ~bits, mref.OPEN, shape, 3, 3)


@pytest.mark.parametrize("rx,ry", [(0, 0), (0, 1), (1, 0), (0, 15), (15, 0), (3, 1), (1, 3), (5, 15), (15, 2)])
def test_unequal_radii_and_the_identity(op, rx, ry):
    bits = random_bits(2, 70, 130, 0.4, seed=rx * 16 + ry)
    dense = random_bits(2, 70, 130, 0.9, seed=rx * 16 + ry)
    for mop in OPS:
        got = check(op, bits, mop, mref.BOX, rx, ry, pad=1)
        check(op, dense, mop, mref.BOX, rx, ry)
        if (rx, ry) == (0, 0):
            assert np.array_equal(got, bits)
            check(op, bits, mop, mref.DIAMOND, 0, 0, pad=1)


@pytest.mark.parametrize("shape,rx,ry", [(mref.BOX, 1, 1), (mref.BOX, 4, 2), (mref.BOX, 15, 15), (mref.DIAMOND, 1, 1),
                                         (mref.DIAMOND, 6, 6), (mref.DIAMOND, 15, 15)])
def test_algebra_on_the_devices_own_outputs(op, shape, rx, ry):
    w, h = 32 * TW + 33, 2 * TH + 3
    for density in (0.02, 0.5, 0.98):
        x = cref.pack(random_bits(2, h, w, density, seed=3))
        ero, dil, opened, closed = (run(op, x, w, mop, shape, rx, ry) for mop in OPS)
        inside = cref.pack(np.ones((2, h, w), dtype=bool))
        # duality: erode(X) = D \ dilate(D \ X)
        assert np.array_equal(ero, ~run(op, ~x & inside, w, mref.DILATE, shape, rx, ry) & inside)
        # open <= X <= close
        assert not (opened & ~x).any() and not (x & ~closed).any()
        # idempotence
        assert np.array_equal(run(op, opened, w, mref.OPEN, shape, rx, ry), opened)
        assert np.array_equal(run(op, closed, w, mref.CLOSE, shape, rx, ry), closed)
        # open = erode, then dilate, as two calls
        assert np.array_equal(run(op, ero, w, mref.DILATE, shape, rx, ry), opened)


# -- sizes ---------------------------------------------------------------------------

def test_more_frames_than_a_16_bit_grid_dimension(op):
    n, h, w = 70000, 3, 33
    bits = random_bits(n, h, w, 0.15)
    got = check(op, bits, mref.CLOSE, mref.BOX, 2, 1)
    assert mref.nontrivial(bits[-100:], got[-100:]) and not np.array_equal(got[-1], got[0])
    check(op, bits, mref.ERODE, mref.DIAMOND, 1, 1, pad=1)


def test_one_4k_frame(op):
    w, h = 3840, 2160
    check(op, random_bits(1, h, w, 0.3), mref.CLOSE, mref.BOX, 15, 15)
    sparse = random_bits(1, h, w, 0.0005)
    got = check(op, sparse, mref.CLOSE, mref.BOX, 15, 15)  # an output that is neither full nor the input
    assert mref.nontrivial(sparse, got)


# -- pointer kinds -------------------------------------------------------------------

def test_device_pointers_and_every_byte_written(op):
    import torch
    from dips_amd import MorphOp, MorphShape
    n, h, w = 3, 2 * TH + 1, 32 * TW + 1
    bits = random_bits(n, h, w, 0.5, seed=5)
    mask = torch.from_numpy(cref.pack(bits, pad=1)).cuda()
    for mop, shape, rx, ry in ((MorphOp.Open, MorphShape.Box, 1, None), (MorphOp.Close, MorphShape.Diamond, 3, None),
                               (MorphOp.Dilate, MorphShape.Box, 0, 0), (MorphOp.Erode, MorphShape.Box, 15, 2)):
        raw = torch.full((mask.numel() + 8,), 0xA5, dtype=torch.uint8, device="cuda")  # poison
        out = raw[4:4 + mask.numel()].view(mask.shape)
        op.run_mask_morph_device(mask, w, out, mop, rx, ry, shape)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
        assert (got[:4] == 0xA5).all() and (got[-4:] == 0xA5).all()
        assert np.array_equal(got[4:-4].reshape(mask.shape), mref.morph(cref.pack(bits), w, int(mop), int(shape), rx, ry))
    with pytest.raises(ValueError):
        op.run_mask_morph_device(mask, w, mask, MorphOp.Open)  # in place
    with pytest.raises(ValueError):
        op.run_mask_morph_device(mask, w, out[:2], MorphOp.Open)


def test_host_pointers_at_odd_alignment(op):
    n, h, w = 2, 29, 37
    bits = random_bits(n, h, w, 0.5, seed=6)
    mask = cref.pack(bits)
    bufs = []

    def odd(nbytes, fill=None):
        raw = np.full(nbytes + 8, 0xAB, dtype=np.uint8)
        off = 1 - raw.ctypes.data % 2  # to an odd address
        view = raw[off:off + nbytes]
        assert view.ctypes.data % 2 == 1
        if fill is not None:
            view[:] = np.frombuffer(fill, dtype=np.uint8)
        bufs.append(raw)
        return view

    m, o = odd(mask.size, mask.tobytes()), odd(mask.size)
    hd = op._host
    hd.check(hd._lib.dips_mask_morph(hd.ptr, m.ctypes.data, n, w, h, mref.OPEN, mref.DIAMOND, 2, 2, o.ctypes.data))
    assert np.array_equal(o.reshape(mask.shape), mref.morph(mask, w, mref.OPEN, mref.DIAMOND, 2, 2))
    assert (bufs[1][:1 - bufs[1].ctypes.data % 2] == 0xAB).all() and (bufs[1][-7:] == 0xAB).all()


def test_refused_arguments_leave_the_output_untouched(op):
    from dips_amd import DipsError, _lib
    n, h, w = 2, 5, 37
    mask = cref.pack(random_bits(n, h, w, 0.5))
    both = np.full(2 * mask.size, 0xA5, dtype=np.uint8)
    out = both[mask.size:]
    both[:mask.size] = mask.reshape(-1)
    hd = op._host
    M, O = both.ctypes.data, out.ctypes.data
    #        in  n  w  h  op shape rx ry out
    cases = [(None, n, w, h, 0, 0, 1, 1, O),
             (M, n, w, h, 0, 0, 1, 1, None),
             (M, n, w, h, 4, 0, 1, 1, O),
             (M, n, w, h, 0, 2, 1, 1, O),
             (M, n, w, h, 0, 0, 16, 1, O),
             (M, n, w, h, 0, 0, 1, 16, O),
             (M, n, w, h, 0, 1, 2, 1, O),
             (M, n, w, h, 3, 1, 0, 1, O),
             (M, n, 0, h, 0, 0, 1, 1, O),
             (M, n, w, 0, 0, 0, 1, 1, O),
             (M, n, 1 << 15, 1 << 15, 0, 0, 1, 1, O),
             (M, n, w, h, 2, 0, 1, 1, M),                    # in place
             (M, n, w, h, 2, 0, 1, 1, O - 1),                # the output's first byte is the input's last
             (M + 1, n, w, h, 2, 0, 1, 1, M + mask.size)]    # the input's last byte is the output's first
    for m_, n_, w_, h_, mop, shape, rx, ry, o_ in cases:
        st = hd._lib.dips_mask_morph(hd.ptr, m_, n_, w_, h_, mop, shape, rx, ry, o_)
        assert st == _lib.DIPS_ERR_INVALID, (n_, w_, h_, mop, shape, rx, ry)
        with pytest.raises(DipsError):
            hd.check(st)
        assert (out == 0xA5).all() and np.array_equal(both[:mask.size], mask.reshape(-1))
    # n_frames == 0: fine, nothing written
    assert hd._lib.dips_mask_morph(hd.ptr, None, 0, w, h, 0, 0, 1, 1, None) == 0
    assert hd._lib.dips_mask_morph(hd.ptr, M, 0, w, h, 0, 0, 1, 1, O) == 0
    assert (out == 0xA5).all()
    # touching, not overlapping, ranges are fine
    hd.check(hd._lib.dips_mask_morph(hd.ptr, M, n, w, h, 2, 0, 1, 1, O))
    assert np.array_equal(out.reshape(mask.shape), mref.morph(mask, w, mref.OPEN, mref.BOX, 1, 1))


def test_misaligned_or_overlapping_device_pointers_are_refused(op):
    import torch
    from dips_amd import _lib
    n, h, w = 2, 5, 37
    mask = cref.pack(random_bits(n, h, w, 0.5))
    src = torch.from_numpy(np.concatenate([mask.reshape(-1), np.zeros(8, dtype=np.uint8)])).cuda()
    dst = torch.full((mask.size + 8,), 7, dtype=torch.uint8, device="cuda")
    hd = op._dev
    for di, do in ((1, 0), (2, 0), (0, 1), (0, 2), (3, 3)):
        st = hd._lib.dips_mask_morph(hd.ptr, src.data_ptr() + di, n, w, h, 2, 0, 1, 1, dst.data_ptr() + do)
        assert st == _lib.DIPS_ERR_INVALID, (di, do)
    assert hd._lib.dips_mask_morph(hd.ptr, src.data_ptr(), n, w, h, 2, 0, 1, 1, src.data_ptr()) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_morph(hd.ptr, src.data_ptr(), 1, w, h, 2, 0, 1, 1,
                                   src.data_ptr() + 4) == _lib.DIPS_ERR_INVALID
    torch.cuda.synchronize()
    assert (dst == 7).all() and np.array_equal(src.cpu().numpy()[:mask.size], mask.reshape(-1))


def test_kernel_time_has_one_entry_per_call():
    import torch
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, MorphShape, PixelFormat
    bits = random_bits(7, 33, 65, 0.45)
    mask = torch.from_numpy(cref.pack(bits)).cuda()
    out = torch.zeros_like(mask)
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255, time_kernel=True)
    try:
        o.run_mask_morph_device(mask, 65, out, MorphOp.Erode)
        o.run_mask_morph_device(mask, 65, out, MorphOp.Close, 15, shape=MorphShape.Diamond)  # two operations, one entry
        ms, launches = o.kernel_time()
        each = o.kernel_times()
    finally:
        o.close()
    assert launches == 2 and len(each) == 2 and ms > 0.0 and all(t > 0.0 for t in each)
    assert np.array_equal(out.cpu().numpy(), mref.morph(cref.pack(bits), 65, mref.CLOSE, mref.DIAMOND, 15))


# -- end to end ------------------------------------------------------------------------

def _moving_clip(c, w, h, n):
    """Noise-free background with two bright rectangles that move a frame at a
    time, one of them split by a dark one-pixel line, and a few blinking
    single pixels."""
    rng = np.random.default_rng([67, c, w, h, n])
    base = rng.integers(40, 90, (h, w, c) if c != 1 else (h, w), dtype=np.uint8)
    frames = np.repeat(base[None], n, axis=0)
    for t in range(n):
        frames[t, 10 + t:22 + t, 5 + 2 * t:25 + 2 * t] = 230
        frames[t, 40:50, 70 - 3 * t:84 - 3 * t] = 10
        for y, x in rng.integers(0, (h, w), (6, 2)):
            frames[t, y, x] = 255
    return frames


@pytest.mark.parametrize("c", [3, 1])
def test_change_boxes_with_morph(c):
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, MorphShape, PixelFormat
    w, h, n = 96, 64, 6
    frames = _moving_clip(c, w, h, n)
    o = DiffSeriesOperator(PixelFormat(c), Mode.PerFrame, 8 / 255)
    try:
        for roi in ((3, 2, 90, 60), None):
            mask = o.change_mask(frames, roi=roi)
            rw = mask.width
            plain = cref.components(mask.bits, rw, 8, 1, 32)
            for steps in ([(MorphOp.Open, MorphShape.Box, 1, 1)],
                          [(MorphOp.Open, MorphShape.Diamond, 1, 1), (MorphOp.Close, MorphShape.Box, 3, 2)],
                          [(0, 0, 1, 0), (1, 1, 2, 2), (3, 0, 0, 1)]):
                cleaned = mask.bits
                for mop, shape, rx, ry in steps:
                    cleaned = mref.morph(cleaned, rw, int(mop), int(shape), rx, ry)
                ref = cref.components(cleaned, rw, 8, 1, 32)
                got = o.change_boxes(frames, roi=roi, max_boxes=32, labels=True, morph=steps)
                assert ref[0].any() and not np.array_equal(ref[0], plain[0])  # the cleanup changed the components
                assert all(np.array_equal(g, x) for g, x in zip((got.counts, got.boxes, got.labels), ref))
            # without morph: today's result, and an empty list of steps is the same
            for morph in (None, []):
                got = o.change_boxes(frames, roi=roi, max_boxes=32, labels=True, morph=morph)
                assert all(np.array_equal(g, x) for g, x in zip((got.counts, got.boxes, got.labels), plain))
        with pytest.raises(ValueError):
            o.change_boxes(frames, morph=[(MorphOp.Open, MorphShape.Diamond, 2, 1)])
    finally:
        o.close()


# -- the randomized draw -----------------------------------------------------------------

@pytest.mark.parametrize("group", range(6))
def test_randomized_cases(op, group):
    """Cases 50 * group .. 50 * group + 49 of the draw of _morph_ref.draw_case
    (tests/test_mask_morph_cpu.py asserts that most of them are not trivial)."""
    for k in range(50 * group, 50 * group + 50):
        x, mop, shape, rx, ry = mref.draw_case(k)
        check(op, x, mop, shape, rx, ry, pad=k & 1)
