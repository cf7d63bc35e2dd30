"""dips_mask_components on the GPU against tests/_components_ref.py: counts,
every word of boxes (the zero-filled records too) and labels, exactly.  The
shapes are the smallest at which each mechanism of mask_components.hip can go
wrong: word and row edges, pad bits, both connectivities, merges that happen
late and along long chains, more than one block of 256 words per frame,
several frames per chunk and several chunks, the min_area / max_boxes
renumbering, the statistics of a component of 2^20 pixels, the pointer kinds
and the refused arguments."""
import ctypes
import functools

import numpy as np
import pytest

import _components_ref as cref

pytestmark = pytest.mark.gpu

WORDS = cref.X0, cref.Y0, cref.X1, cref.Y1, cref.AREA, cref.ANCHOR, cref.CX256, cref.CY256


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
    return frozen(np.random.default_rng([41, seed, n, h, w]).random((n, h, w)) < density)


@functools.lru_cache(maxsize=None)
def _want_cached(key, w, connectivity, min_area, max_boxes):
    return tuple(frozen(a) for a in cref.components(_BITS[key], w, connectivity, min_area, max_boxes))


_BITS = {}


def want(mask_bytes, w, connectivity=8, min_area=1, max_boxes=64):
    """The reference of a mask, computed once per (mask, arguments)."""
    key = (mask_bytes.shape, mask_bytes.tobytes())
    _BITS.setdefault(key, mask_bytes)
    return _want_cached(key, w, connectivity, min_area, max_boxes)


def run(op, mask_bytes, w, connectivity=8, min_area=1, max_boxes=64, labels=True, chunk_frames=0):
    from dips_amd import ChangeMask
    r = op.mask_components(ChangeMask(np.ascontiguousarray(mask_bytes), w), connectivity, min_area, max_boxes, labels,
                           chunk_frames)
    return r.counts, r.boxes, r.labels


def check(op, bits, connectivity=8, min_area=1, max_boxes=64, pad=0, chunk_frames=0):
    """GPU == reference for bool bits [n, h, w]; returns the reference."""
    bits = np.asarray(bits, dtype=bool)
    w = bits.shape[2]
    ref = want(cref.pack(bits), w, connectivity, min_area, max_boxes)
    got = run(op, cref.pack(bits, pad), w, connectivity, min_area, max_boxes, True, chunk_frames)
    for name, g, r in zip(("counts", "boxes", "labels"), got, ref):
        assert g.dtype == np.uint32 and g.shape == r.shape, name
        assert np.array_equal(g, r), (name, np.argwhere(g != r)[:5].tolist())
    return ref


# -- word and row edges ---------------------------------------------------------

@pytest.mark.parametrize("h", [1, 2, 3, 29])
@pytest.mark.parametrize("w", [1, 2, 31, 32, 33, 63, 64, 65, 97])
def test_word_and_row_edges(op, w, h):
    corners = np.zeros((h, w), dtype=bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    frames = np.stack([random_bits(1, h, w, 0.5)[0], random_bits(1, h, w, 0.2, 1)[0], np.ones((h, w), dtype=bool),
                       np.zeros((h, w), dtype=bool), corners])
    for connectivity in (4, 8):
        counts, boxes, _ = check(op, frames, connectivity, max_boxes=8)
        assert counts[2] == 1 and boxes[2, 0].tolist()[:6] == [0, 0, w, h, w * h, 0]
        assert counts[3] == 0 and not boxes[3].any()


@pytest.mark.parametrize("w", [33, 37])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_garbage_pad_bits_are_ignored(op, w, connectivity):
    bits = np.concatenate([random_bits(3, 29, w, 0.5), np.ones((1, 29, w), dtype=bool)])
    check(op, bits, connectivity, pad=0)
    check(op, bits, connectivity, pad=1)  # the same reference: pad bits all ones


# -- connectivity ------------------------------------------------------------------

def test_diagonal_and_checkerboard_4_against_8(op):
    h, w = 29, 37
    jj, ii = np.mgrid[0:h, 0:w]
    diagonal = ii == jj
    board = (ii + jj) % 2 == 0
    bits = np.stack([diagonal, board])
    n_board = int(board.sum())
    c4, b4, l4 = check(op, bits, 4, max_boxes=n_board)
    assert c4.tolist() == [h, n_board]  # one component per set pixel: the largest count
    assert np.array_equal(b4[1, :, cref.ANCHOR], np.flatnonzero(board)) and (b4[1, :, cref.AREA] == 1).all()
    c8, b8, l8 = check(op, bits, 8, max_boxes=4)
    assert c8.tolist() == [1, 1] and b8[1, 0].tolist()[:6] == [0, 0, w, h, n_board, 0]


# -- late merges and long chains ---------------------------------------------------

def _u_shape(h, w):
    b = np.zeros((h, w), dtype=bool)
    b[:, 0] = b[:, -1] = b[-1, :] = True
    return b


def _w_shape(h, w):
    b = _u_shape(h, w)
    b[:, w // 2] = True
    return b


def _comb(h, w):
    b = np.zeros((h, w), dtype=bool)
    b[:, ::2] = True
    b[-1, :] = True
    return b


def _serpentine(h, w):
    """A one-pixel path that fills the frame: even rows full, odd rows one
    pixel at alternating ends."""
    b = np.zeros((h, w), dtype=bool)
    b[::2, :] = True
    b[1::4, -1] = True
    b[3::4, 0] = True
    return b


def _spiral(h, w):
    """A rectangular spiral of one-pixel lines two pixels apart, from (0, 0)
    inwards."""
    b = np.zeros((h, w), dtype=bool)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    first = True
    while top <= bottom and left <= right:
        b[top, (left if first else max(left - 1, 0)):right + 1] = True
        b[top:bottom + 1, right] = True
        if bottom - top >= 2 and right - left >= 2:
            b[bottom, left:right + 1] = True
            b[top + 2:bottom + 1, left] = True
        first = False
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return b


@pytest.mark.parametrize("name,h,w", [("u", 29, 37), ("w", 29, 37), ("comb", 29, 37), ("u", 65, 129), ("w", 65, 129),
                                      ("comb", 65, 129), ("serpentine", 65, 129), ("spiral", 65, 129),
                                      ("spiral", 64, 97)])
def test_late_merges_and_long_chains_are_one_component(op, name, h, w):
    shape = {"u": _u_shape, "w": _w_shape, "comb": _comb, "serpentine": _serpentine, "spiral": _spiral}[name](h, w)
    assert shape[0, 0]
    for connectivity in (4, 8):
        counts, boxes, labels = check(op, shape[None], connectivity, max_boxes=3)
        assert counts.tolist() == [1], (name, connectivity)
        assert boxes[0, 0, cref.ANCHOR] == 0 and boxes[0, 0, cref.AREA] == int(shape.sum())
        assert np.array_equal(labels[0] != 0, shape)


def test_runs_longer_than_the_walk_back(op):
    """Runs of more than 64 all-ones words (2,048 pixels): cc_rows_kernel
    stops walking back and chains the run through bit 0 of the word reached."""
    h, w = 4, 4161  # 131 words, the last with one valid bit
    bits = np.zeros((2, h, w), dtype=bool)
    bits[0, 0, :] = True              # the whole row, pad word included
    bits[0, 1, :100] = True           # a gap at 100 and 101, then a run to the end
    bits[0, 1, 102:] = True
    bits[0, 3, 37:4130] = True        # starts and ends inside words, touches nothing
    bits[1] = True
    for connectivity in (4, 8):
        counts, boxes, _ = check(op, bits, connectivity, max_boxes=4)
        assert counts.tolist() == [2, 1]
        assert boxes[0, :2, cref.AREA].tolist() == [2 * w - 2, 4130 - 37] and boxes[1, 0, cref.AREA] == h * w


# -- more than one block per frame -------------------------------------------------

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("density", [0.05, 0.5, 0.593, 0.95])
@pytest.mark.parametrize("h,w", [(130, 257), (360, 640)])
def test_random_masks_across_block_edges(op, h, w, density, connectivity):
    check(op, random_bits(1, h, w, density), connectivity, max_boxes=64)


# -- frames are independent --------------------------------------------------------

def test_frames_are_independent(op):
    n, h, w = 5, 33, 65
    bits = np.zeros((n, h, w), dtype=bool)
    # a bar down to the last row of frame t and one from the first row of
    # frame t + 1, in the same columns; a row's last pixel and the next row's first
    bits[0, 20:, 10:14] = True
    bits[1, :9, 10:14] = True
    bits[1, 15, w - 1] = bits[1, 16, 0] = True
    bits[3] = bits[1]            # identical frames, an all-zero one between busy ones
    bits[4] = random_bits(1, h, w, 0.5)[0]
    for connectivity in (4, 8):
        counts, boxes, labels = check(op, bits, connectivity)
        assert counts[:4].tolist() == [1, 3, 0, 3]
        assert np.array_equal(boxes[1], boxes[3]) and np.array_equal(labels[1], labels[3])
        # one frame at a time gives the same
        for t in range(n):
            single = run(op, cref.pack(bits[t:t + 1]), w, connectivity)
            assert all(np.array_equal(s[0], a[t]) for s, a in zip(single, (counts, boxes, labels)))


@pytest.mark.parametrize("chunk_frames", [0, 1, 2, 3, 7, 100])
def test_result_does_not_depend_on_chunk_frames(op, chunk_frames):
    bits = random_bits(7, 33, 65, 0.45)
    for connectivity in (4, 8):
        check(op, bits, connectivity, min_area=2, max_boxes=16, chunk_frames=chunk_frames)


# -- min_area and max_boxes --------------------------------------------------------

def test_min_area_renumbers(op):
    bits = random_bits(2, 33, 65, 0.4)
    _, full, _ = want(cref.pack(bits), 65, 4, 1, 2048)
    largest = int(full[..., cref.AREA].max())
    assert largest > 5
    for min_area in (0, 1, 2, 5, largest, largest + 1):
        counts, boxes, labels = check(op, bits, 4, min_area=min_area, max_boxes=256)
        areas = full[..., cref.AREA]
        assert counts.tolist() == [(int((areas[t] >= max(min_area, 1)).sum())) for t in range(2)]
        if min_area == largest:
            assert counts.sum() >= 1 and (boxes[..., cref.AREA][boxes[..., cref.AREA] != 0] == largest).all()
        if min_area == largest + 1:
            assert not counts.any() and not boxes.any() and not labels.any()


def test_max_boxes_truncates_the_records_only(op):
    bits = random_bits(1, 33, 65, 0.3)
    w = 65
    count = int(want(cref.pack(bits), w, 8, 1, 0)[0][0])
    assert count > 4
    c_all, b_all, l_all = check(op, bits, 8, max_boxes=count)
    for k in (1, count - 1, count, count + 3):
        counts, boxes, labels = check(op, bits, 8, max_boxes=k)
        assert counts.tolist() == [count] and np.array_equal(labels, l_all)
        m = min(k, count)
        assert np.array_equal(boxes[0, :m], b_all[0, :m]) and not boxes[0, m:].any()
    # K = 0 with boxes NULL: counts (and labels) only
    counts, boxes, labels = run(op, cref.pack(bits), w, 8, 1, 0)
    assert counts.tolist() == [count] and boxes.shape == (1, 0, 8) and np.array_equal(labels, l_all)


# -- statistics at scale -----------------------------------------------------------

def test_statistics_of_one_large_component(op):
    """An all-ones 1024 x 1024 frame: area 2^20, the whole frame as the box,
    centroid 511.5 in both axes; 2048 x 8: sum i = 8 * 2047 * 2048 / 2 > 2^24."""
    for connectivity in (4, 8):
        counts, boxes, labels = run(op, cref.pack(np.ones((1, 1024, 1024), dtype=bool)), 1024, connectivity, 1, 2)
        assert counts.tolist() == [1]
        assert boxes[0, 0].tolist() == [0, 0, 1024, 1024, 1 << 20, 0, 511 * 256 + 128, 511 * 256 + 128]
        assert not boxes[0, 1].any() and (labels == 1).all()
    counts, boxes, labels = run(op, cref.pack(np.ones((1, 8, 2048), dtype=bool)), 2048, 8, 1, 2)
    assert counts.tolist() == [1]
    assert boxes[0, 0].tolist() == [0, 0, 2048, 8, 2048 * 8, 0, 1023 * 256 + 128, 3 * 256 + 128]
    assert (labels == 1).all()


# -- pointers ----------------------------------------------------------------------

def test_device_pointers_equal_host_pointers(op):
    import torch
    bits = random_bits(3, 33, 65, 0.5)
    w, k = 65, 16
    ref = check(op, bits, 8, min_area=2, max_boxes=k)
    mask = torch.from_numpy(cref.pack(bits)).cuda()
    # outputs at an offset of 4 bytes inside larger tensors, prefilled
    counts = torch.full((1 + 3,), -1, dtype=torch.int32, device="cuda")
    boxes = torch.full((1 + 3 * k * 8,), -1, dtype=torch.int32, device="cuda")
    labels = torch.full((1 + 3 * 33 * w,), -1, dtype=torch.int32, device="cuda")
    op.run_mask_components_device(mask, w, counts[1:], boxes[1:].view(3, k, 8), labels[1:].view(3, 33, w), min_area=2)
    torch.cuda.synchronize()
    got = [t.cpu().numpy().view(np.uint32) for t in (counts, boxes, labels)]
    assert all(g[0] == 0xFFFFFFFF for g in got)
    assert np.array_equal(got[0][1:], ref[0]) and np.array_equal(got[1][1:].reshape(3, k, 8), ref[1])
    assert np.array_equal(got[2][1:].reshape(3, 33, w), ref[2])
    # counts only
    counts2 = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    op.run_mask_components_device(mask, w, counts2, min_area=2)
    assert np.array_equal(counts2.cpu().numpy().view(np.uint32), ref[0])


def test_host_pointers_at_odd_alignment(op):
    bits = random_bits(2, 29, 37, 0.5)
    w, h, n, k = 37, 29, 2, 8
    ref = want(cref.pack(bits), w, 8, 1, k)
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

    m = odd(mask.size, mask.tobytes())
    c, b, lab = odd(4 * n), odd(4 * n * k * 8), odd(4 * n * h * w)
    hd = op._host
    hd.check(hd._lib.dips_mask_components(hd.ptr, m.ctypes.data, n, w, h, 8, 1, k, 0, c.ctypes.data, b.ctypes.data,
                                          lab.ctypes.data))
    assert np.array_equal(np.frombuffer(c.tobytes(), dtype="<u4"), ref[0])
    assert np.array_equal(np.frombuffer(b.tobytes(), dtype="<u4").reshape(n, k, 8), ref[1])
    assert np.array_equal(np.frombuffer(lab.tobytes(), dtype="<u4").reshape(n, h, w), ref[2])


# -- end to end --------------------------------------------------------------------

def _moving_clip(c, w, h, n):
    """Noise-free background with two bright rectangles that move one pixel a
    frame and a few blinking single pixels."""
    rng = np.random.default_rng([43, c, w, h, n])
    base = rng.integers(40, 90, (h, w, c) if c != 1 else (h, w), dtype=np.uint8)
    frames = np.repeat(base[None], n, axis=0)
    for t in range(n):
        frames[t, 10 + t:22 + t, 5 + 2 * t:25 + 2 * t] = 230
        frames[t, 40:50, 70 - 3 * t:84 - 3 * t] = 10
        for y, x in rng.integers(0, (h, w), (6, 2)):
            frames[t, y, x] = 255
    return frames


@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_change_boxes_end_to_end(c, mode):
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    w, h, n = 96, 64, 6
    roi = (3, 2, 90, 60)
    frames = _moving_clip(c, w, h, n)
    o = DiffSeriesOperator(PixelFormat(c), Mode(mode), 8 / 255)
    try:
        for r in (roi, None):
            mask = o.change_mask(frames, roi=r)
            rw = mask.width
            got = o.change_boxes(frames, roi=r, connectivity=4, min_area=3, max_boxes=32, labels=True)
            ref = cref.components(mask.bits, rw, 4, 3, 32)
            assert ref[0].any()
            assert all(np.array_equal(g, x) for g, x in zip((got.counts, got.boxes, got.labels), ref))
            assert all(np.array_equal(g, x) for g, x in zip(run(o, mask.bits, rw, 4, 3, 32), ref))
            # every changed pixel lies in one component: the areas sum to the series' count
            everything = o.change_boxes(frames, roi=r, connectivity=8, min_area=1, max_boxes=512)
            assert not everything.truncated.any() and everything.labels is None
            assert np.array_equal(everything.boxes[..., cref.AREA].sum(axis=1, dtype=np.uint64), mask.counts())
        series, _ = o(frames)
        assert np.array_equal(everything.boxes[..., cref.AREA].sum(axis=1, dtype=np.uint64), series.as_array()[:, 2])
    finally:
        o.close()


# -- errors ------------------------------------------------------------------------

def test_refused_arguments_leave_the_outputs_untouched(op):
    from dips_amd import DipsError, _lib
    w, h, n, k = 37, 5, 2, 4
    mask = cref.pack(random_bits(n, h, w, 0.5))
    counts = np.full(n, 0xA5A5A5A5, dtype=np.uint32)
    boxes = np.full((n, k, 8), 0xA5A5A5A5, dtype=np.uint32)
    labels = np.full((n, h, w), 0xA5A5A5A5, dtype=np.uint32)
    hd = op._host
    M, C, B, L = mask.ctypes.data, counts.ctypes.data, boxes.ctypes.data, labels.ctypes.data
    #        mask n  w        h        conn min K  counts boxes labels
    cases = [(None, n, w, h, 8, 1, k, C, B, L),
             (M, n, w, h, 8, 1, k, None, B, L),
             (M, n, w, h, 8, 1, k, C, None, L),
             (M, n, w, h, 6, 1, k, C, B, L),
             (M, n, w, h, 0, 1, k, C, B, L),
             (M, n, 0, h, 8, 1, k, C, B, L),
             (M, n, w, 0, 8, 1, k, C, B, L),
             (M, n, 1 << 24, 1, 8, 1, k, C, B, L),
             (M, n, 1, 1 << 24, 8, 1, k, C, B, L),
             (M, n, 1 << 15, 1 << 15, 8, 1, k, C, B, L),
             (M, 1 << 20, w, h, 8, 1, 1 << 9, C, B, L)]
    for m_, n_, w_, h_, conn, area, k_, c_, b_, l_ in cases:
        st = hd._lib.dips_mask_components(hd.ptr, m_, n_, w_, h_, conn, area, k_, 0, c_, b_, l_)
        assert st == _lib.DIPS_ERR_INVALID, (n_, w_, h_, conn, k_)
        with pytest.raises(DipsError):
            hd.check(st)
        assert (counts == 0xA5A5A5A5).all() and (boxes == 0xA5A5A5A5).all() and (labels == 0xA5A5A5A5).all()
    # n_frames == 0: fine, nothing written
    assert hd._lib.dips_mask_components(hd.ptr, None, 0, w, h, 8, 1, k, 0, None, None, None) == 0
    assert hd._lib.dips_mask_components(hd.ptr, M, 0, w, h, 8, 1, k, 0, C, B, L) == 0
    assert (counts == 0xA5A5A5A5).all() and (boxes == 0xA5A5A5A5).all() and (labels == 0xA5A5A5A5).all()


def test_misaligned_device_pointers_are_refused(op):
    import torch
    from dips_amd import _lib
    w, h, n, k = 37, 5, 2, 4
    mask = torch.from_numpy(np.concatenate([cref.pack(random_bits(n, h, w, 0.5)).reshape(-1),
                                            np.zeros(8, dtype=np.uint8)])).cuda()
    counts = torch.full((n + 1,), 7, dtype=torch.int32, device="cuda")
    boxes = torch.full((n * k * 8 + 1,), 7, dtype=torch.int32, device="cuda")
    labels = torch.full((n * h * w + 1,), 7, dtype=torch.int32, device="cuda")
    hd = op._dev
    ptrs = [mask.data_ptr(), counts.data_ptr(), boxes.data_ptr(), labels.data_ptr()]
    for bad in range(4):
        for off in (1, 2):
            p = list(ptrs)
            p[bad] += off
            st = hd._lib.dips_mask_components(hd.ptr, p[0], n, w, h, 8, 1, k, 0, p[1], p[2], p[3])
            assert st == _lib.DIPS_ERR_INVALID, (bad, off)
    torch.cuda.synchronize()
    assert (counts == 7).all() and (boxes == 7).all() and (labels == 7).all()


def test_kernel_time_has_one_entry_per_call():
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    bits = random_bits(7, 33, 65, 0.45)
    mask = torch.from_numpy(cref.pack(bits)).cuda()
    counts = torch.zeros((7,), dtype=torch.int32, device="cuda")
    boxes = torch.zeros((7, 8, 8), dtype=torch.int32, device="cuda")
    labels = torch.zeros((7, 33, 65), dtype=torch.int32, device="cuda")
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255, time_kernel=True)
    try:
        o.run_mask_components_device(mask, 65, counts, boxes, labels)                   # one chunk
        o.run_mask_components_device(mask, 65, counts, boxes, labels, chunk_frames=2)   # four chunks
        o.run_mask_components_device(mask, 65, counts)                                  # counts only
        ms, launches = o.kernel_time()
        each = o.kernel_times()
    finally:
        o.close()
    assert launches == 3 and len(each) == 3 and ms > 0.0 and all(t > 0.0 for t in each)
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want(cref.pack(bits), 65, 8, 1, 64)[0])
