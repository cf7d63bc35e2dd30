"""dips_mask_shapes on the GPU against tests/_shapes_ref.py: every word of
counts, boxes and shapes (the zero-filled records too), exactly.  The regions
are the smallest at which each mechanism of mask_shapes.hip can go wrong: the
carry bits at word and row edges, pad bits, both connectivities, runs longer
than a word, figures with holes, the records dropped by min_area and
max_boxes, several blocks and several chunks, the weight plane at odd widths
and addresses, one 4K frame whose every wave adds to one record, the pointer
kinds and the refused arguments."""
import functools

import numpy as np
import pytest

import _components_ref as cref
import _shapes_ref as sref
from test_mask_shapes_cpu import BLOB_IN_RING, DIAGONAL_HOLES, EIGHT, NESTED, RING

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5


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
    return frozen(np.random.default_rng([43, seed, n, h, w]).random((n, h, w)) < density)


@functools.lru_cache(maxsize=None)
def random_weights(n, h, w, seed=0):
    return frozen(np.random.default_rng([47, seed, n, h, w]).integers(0, 256, (n, h, w), dtype=np.uint8))


_ARRAYS = {}


@functools.lru_cache(maxsize=None)
def _want_cached(key, wkey, w, connectivity, min_area, max_boxes):
    weights = None if wkey is None else _ARRAYS[wkey]
    return tuple(frozen(a) for a in sref.shapes(_ARRAYS[key], w, weights, connectivity, min_area, max_boxes))


def _key(a):
    key = (a.shape, a.tobytes())
    _ARRAYS.setdefault(key, a)
    return key


def want(mask_bytes, w, weights=None, connectivity=8, min_area=1, max_boxes=8):
    """The reference of a mask, computed once per (mask, weights, arguments)."""
    return _want_cached(_key(mask_bytes), None if weights is None else _key(weights), w, connectivity, min_area,
                        max_boxes)


def run(op, mask_bytes, w, weights=None, connectivity=8, min_area=1, max_boxes=8, chunk_frames=0):
    from dips_amd import ChangeMask
    r = op.mask_shapes(ChangeMask(np.ascontiguousarray(mask_bytes), w), weights, connectivity, min_area, max_boxes,
                       chunk_frames)
    return r.as_arrays()


def same(got, ref):
    for name, g, r in zip(("counts", "boxes", "shapes"), got, ref):
        assert g.dtype == np.uint32 and g.shape == r.shape, name
        assert np.array_equal(g, r), (name, np.argwhere(g != r)[:5].tolist())


def check(op, bits, weights=None, connectivity=8, min_area=1, max_boxes=8, pad=0, chunk_frames=0):
    """GPU == reference for bool bits [n, h, w]; returns the reference."""
    bits = np.asarray(bits, dtype=bool)
    w = bits.shape[2]
    ref = want(cref.pack(bits), w, weights, connectivity, min_area, max_boxes)
    same(run(op, cref.pack(bits, pad), w, weights, connectivity, min_area, max_boxes, chunk_frames), ref)
    return ref


def euler(shapes):
    return shapes[..., sref.EULER].view(np.int32)


def place(figure, h, w, y, x):
    out = np.zeros((h, w), dtype=bool)
    out[y:y + figure.shape[0], x:x + figure.shape[1]] = figure
    return out


# -- word and row edges ---------------------------------------------------------

@pytest.mark.parametrize("h", [1, 2, 3, 29])
@pytest.mark.parametrize("w", [1, 2, 31, 32, 33, 63, 64, 65, 97])
def test_word_and_row_edges(op, w, h):
    corners = np.zeros((h, w), dtype=bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    frames = np.stack([random_bits(1, h, w, 0.3)[0], random_bits(1, h, w, 0.8, 1)[0], np.ones((h, w), dtype=bool),
                       np.zeros((h, w), dtype=bool), corners, ~corners])
    for connectivity in (4, 8):
        for pad in (0, 1):  # the same reference: the pad bits are ignored
            counts, boxes, shapes = check(op, frames, None, connectivity, pad=pad)
        assert counts[2] == 1 and boxes[2, 0, cref.AREA] == w * h and euler(shapes)[2, 0] == 1
        assert shapes[2, 0, sref.CRACKS_V:sref.EULER].tolist() == [2 * h, 2 * w]
        assert counts[3] == 0 and not shapes[3].any()


# -- shapes ------------------------------------------------------------------------

def test_runs_across_words_and_a_run_longer_than_the_walk_back(op):
    w = 64 * 32 + 40
    row = np.ones((1, 1, w), dtype=bool)
    broken = row.copy()
    broken[0, 0, [31, 64, 1000, w - 2]] = False
    for bits in (row, broken):
        for connectivity in (4, 8):
            counts, boxes, shapes = check(op, bits, random_weights(1, 1, w), connectivity)
    assert counts.tolist() == [5]
    counts, _, shapes = want(cref.pack(row), w, random_weights(1, 1, w), 8)
    assert int(sref.get64(shapes[0, 0], sref.SXX)) == (w - 1) * w * (2 * w - 1) // 6
    # runs that cross the words of several rows, every carry bit in use
    h, w = 5, 97
    bits = np.zeros((1, h, w), dtype=bool)
    bits[0, 0, 30:34] = bits[0, 1, 33:70] = bits[0, 2, 60:66] = bits[0, 3, 0:97] = bits[0, 4, 95:97] = True
    for connectivity in (4, 8):
        check(op, bits, random_weights(1, h, w), connectivity)


def test_checkerboard_4_against_8(op):
    h, w = 9, 37
    jj, ii = np.mgrid[0:h, 0:w]
    board = ((ii + jj) % 2 == 0)[None]
    n_board = int(board.sum())
    c4, _, s4 = check(op, board, None, 4, max_boxes=n_board)
    assert c4.tolist() == [n_board] and (euler(s4)[0] == 1).all() and (s4[0, :, sref.CRACKS_V] == 2).all()
    c8, _, s8 = check(op, board, None, 8, max_boxes=4)
    assert c8.tolist() == [1] and euler(s8)[0, 0] == 1 - int((~board[0, 1:-1, 1:-1]).sum())


@pytest.mark.parametrize("connectivity", [4, 8])
def test_figures_with_holes(op, connectivity):
    h, w = 12, 70
    border = np.ones((h, w), dtype=bool)
    border[1:-1, 1:-1] = False
    frames = np.stack([place(RING, h, w, 2, 30), place(EIGHT, h, w, 3, 62), place(NESTED, h, w, 4, 29),
                       place(BLOB_IN_RING, h, w, 0, 31), place(DIAGONAL_HOLES, h, w, 8, 30), border,
                       border | place(NESTED, h, w, 2, 30)])
    _, _, shapes = check(op, frames, None, connectivity)
    e = euler(shapes)
    assert e[0, 0] == 0 and shapes[0, 0, sref.CRACKS_V] + shapes[0, 0, sref.CRACKS_H] == 16
    assert e[1, 0] == -1 and e[2, :2].tolist() == [0, 0] and e[3, :2].tolist() == [0, 1]
    assert e[4, 0] == (-1 if connectivity == 8 else 0)
    assert e[5, 0] == 0 and e[6, :3].tolist() == [0, 0, 0]


# -- selection ---------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [4, 8])
def test_min_area_and_truncation(op, connectivity):
    bits = random_bits(3, 29, 97, 0.4)
    weights = random_weights(3, 29, 97)
    full = check(op, bits, weights, connectivity, 1, 8)
    assert (full[0] > 8).all()  # truncated: counts is not capped
    for min_area in (2, 5):
        counts, boxes, shapes = check(op, bits, weights, connectivity, min_area, 8)
        assert (boxes[..., cref.AREA][boxes[..., cref.AREA] != 0] >= min_area).all()
    counts, boxes, shapes = check(op, bits, weights, connectivity, 5, 3)
    assert (counts > 3).all() and shapes[:, :3].any()
    # a frame with fewer records than K: the rest are zeros
    few = check(op, np.stack([place(RING, 9, 40, 1, 30), np.zeros((9, 40), dtype=bool)]), None, connectivity, 1, 5)
    assert few[0].tolist() == [1, 0] and not few[2][0, 1:].any() and not few[2][1].any()


def test_no_records_at_all(op):
    bits = random_bits(2, 9, 40, 0.4)
    hd = op._host
    mask = cref.pack(bits)
    counts = np.full(2, SENTINEL, dtype=np.uint32)
    assert hd._lib.dips_mask_shapes(hd.ptr, mask.ctypes.data, None, 2, 40, 9, 8, 1, 0, 0, counts.ctypes.data, None,
                                    None) == 0
    assert np.array_equal(counts, cref.components(mask, 40, 8, 1, 1, labels=False)[0])
    got = run(op, mask, 40, None, 8, 1, 0)
    assert got[1].shape == (2, 0, 8) and got[2].shape == (2, 0, 16) and np.array_equal(got[0], counts)


# -- chunking ----------------------------------------------------------------------

def test_chunks_and_blocks(op):
    small, wsmall = random_bits(5, 29, 97, 0.5), random_weights(5, 29, 97)  # 116 words: under one block
    for connectivity in (4, 8):
        for chunk in (0, 1, 2):
            check(op, small, wsmall, connectivity, chunk_frames=chunk)
    large, wlarge = random_bits(2, 40, 300, 0.5), random_weights(2, 40, 300)  # 400 words: two blocks
    for chunk in (0, 1):
        check(op, large, wlarge, 8, chunk_frames=chunk)
    # frames must not leak into each other: a full frame between two sparse ones
    mixed = np.stack([small[0], np.ones((29, 97), dtype=bool), small[1]])
    ref = check(op, mixed, wsmall[:3], 8)
    alone = want(cref.pack(mixed[2:]), 97, wsmall[2:3], 8)
    assert np.array_equal(ref[2][2], alone[2][0])


# -- weights -----------------------------------------------------------------------

@pytest.mark.parametrize("w", [29, 30, 31, 32, 97])
def test_weights_at_every_row_alignment(op, w):
    h = 7
    bits = random_bits(2, h, w, 0.7)
    check(op, bits, random_weights(2, h, w), 8)
    full = np.full((2, h, w), 255, dtype=np.uint8)
    counts, boxes, shapes = check(op, np.ones((2, h, w), dtype=bool), full, 4)
    assert int(sref.get64(shapes[0, 0], sref.WSUM)) == 255 * w * h and shapes[0, 0, sref.WMAX] == 255
    none = check(op, bits, None, 8)
    assert not none[2][..., sref.WSUM:sref.WMAX + 1].any()


def test_single_peak_lands_in_its_record(op):
    h, w = 12, 70
    bits = np.stack([place(RING, h, w, 2, 30) | place(RING, h, w, 6, 62) | place(EIGHT, h, w, 1, 5)])
    weights = np.ones((1, h, w), dtype=np.uint8)
    weights[0, 7, 62] = 200   # on the second ring
    weights[0, 3, 31] = 250   # in the first ring's hole: a clear pixel
    counts, boxes, shapes = check(op, bits, weights, 8)
    assert counts.tolist() == [3]
    k = boxes[0, :3, cref.ANCHOR].tolist().index(6 * w + 62)
    assert shapes[0, :3, sref.WMAX].tolist() == [200 if i == k else 1 for i in range(3)]
    assert int(sref.get64(shapes[0, k], sref.WSUM)) == 7 + 200


def test_device_pointers_streams_and_sentinels(op):
    import torch
    n, h, w, k = 3, 33, 65, 8
    bits = random_bits(n, h, w, 0.6)
    weights = random_weights(n, h, w)
    ref = check(op, bits, weights, 8, min_area=2)
    mask = torch.from_numpy(cref.pack(bits)).cuda()
    # the weights at an odd address, the outputs at 8 bytes inside larger sentinel-filled tensors
    wbuf = torch.zeros(weights.size + 1, dtype=torch.uint8, device="cuda")
    wdev = wbuf[1:].view(n, h, w)
    wdev.copy_(torch.from_numpy(weights.copy()))
    assert wdev.data_ptr() % 2 == 1
    for stream in (None, torch.cuda.Stream()):
        counts = torch.full((2 + n,), -1, dtype=torch.int32, device="cuda")
        boxes = torch.full((2 + n * k * 8,), -1, dtype=torch.int32, device="cuda")
        shapes = torch.full((2 + n * k * 16,), -1, dtype=torch.int32, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        op.run_mask_shapes_device(mask, w, counts[2:], boxes[2:].view(n, k, 8), shapes[2:].view(n, k, 16), wdev,
                                  min_area=2, stream=None if stream is None else stream.cuda_stream)
        torch.cuda.synchronize()
        got = [t.cpu().numpy().view(np.uint32) for t in (counts, boxes, shapes)]
        assert all((g[:2] == 0xFFFFFFFF).all() for g in got)
        same((got[0][2:], got[1][2:].reshape(n, k, 8), got[2][2:].reshape(n, k, 16)), ref)
    # counts only
    counts2 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    op.run_mask_shapes_device(mask, w, counts2, None, None, min_area=2)
    assert np.array_equal(counts2.cpu().numpy().view(np.uint32), ref[0])


def test_counts_and_boxes_equal_the_other_calls(op):
    import torch
    n, h, w, k = 4, 29, 97, 8
    bits = random_bits(n, h, w, 0.45)
    mask = torch.from_numpy(cref.pack(bits)).cuda()

    def outs(words):
        return [torch.full(s, -1, dtype=torch.int32, device="cuda") for s in ((n,), (n, k, 8), (n, k, words))]

    for connectivity in (4, 8):
        c_s, b_s, s_s = outs(16)
        op.run_mask_shapes_device(mask, w, c_s, b_s, s_s, connectivity=connectivity, min_area=2)
        c_c, b_c, _ = outs(1)
        op.run_mask_components_device(mask, w, c_c, b_c, connectivity=connectivity, min_area=2)
        c_t, b_t, l_t = outs(4)
        op.run_mask_tracks_device(mask, w, c_t, b_t, l_t, connectivity=connectivity, min_area=2)
        torch.cuda.synchronize()
        assert torch.equal(c_s, c_c) and torch.equal(b_s, b_c) and torch.equal(c_s, c_t) and torch.equal(b_s, b_t)
        assert (c_s > 0).all()


# -- contention --------------------------------------------------------------------

def test_one_4k_frame_of_ones(op):
    w, h = 3840, 2160
    mask = np.full((1, h, w // 8), 0xFF, dtype=np.uint8)
    weights = np.full((1, h, w), 3, dtype=np.uint8)
    weights[0, 1234, 2345] = 77
    for wts in (None, weights):
        counts, boxes, shapes = run(op, mask, w, wts, 8, 1, 2)
        assert counts.tolist() == [1] and boxes[0, 0, :6].tolist() == [0, 0, w, h, w * h, 0]
        rec = shapes[0, 0]
        assert int(sref.get64(rec, sref.SX)) == h * (w * (w - 1) // 2)
        assert int(sref.get64(rec, sref.SY)) == w * (h * (h - 1) // 2)
        assert int(sref.get64(rec, sref.SXX)) == h * ((w - 1) * w * (2 * w - 1) // 6)
        assert int(sref.get64(rec, sref.SYY)) == w * ((h - 1) * h * (2 * h - 1) // 6)
        assert int(sref.get64(rec, sref.SXY)) == (w * (w - 1) // 2) * (h * (h - 1) // 2)
        assert rec[sref.CRACKS_V:].tolist() == [2 * h, 2 * w, 1]
        assert int(sref.get64(rec, sref.WSUM)) == (0 if wts is None else 3 * w * h + 74)
        assert rec[sref.WMAX] == (0 if wts is None else 77)
        assert not shapes[0, 1].any()


# -- pointer kinds and errors --------------------------------------------------------

def test_host_pointers_at_odd_alignment(op):
    n, h, w, k = 2, 29, 37, 8
    bits = random_bits(n, h, w, 0.5)
    weights = random_weights(n, h, w)
    ref = want(cref.pack(bits), w, weights, 8, 1, k)
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

    m, wt = odd(cref.pack(bits).size, cref.pack(bits).tobytes()), odd(weights.size, weights.tobytes())
    c, b, s = odd(4 * n), odd(4 * n * k * 8), odd(4 * n * k * 16)
    hd = op._host
    hd.check(hd._lib.dips_mask_shapes(hd.ptr, m.ctypes.data, wt.ctypes.data, n, w, h, 8, 1, k, 0, c.ctypes.data,
                                      b.ctypes.data, s.ctypes.data))
    same((np.frombuffer(c.tobytes(), dtype="<u4"), np.frombuffer(b.tobytes(), dtype="<u4").reshape(n, k, 8),
          np.frombuffer(s.tobytes(), dtype="<u4").reshape(n, k, 16)), ref)


def test_refused_arguments_leave_the_outputs_untouched(op):
    from dips_amd import DipsError, _lib
    w, h, n, k = 37, 5, 2, 4
    mask = cref.pack(random_bits(n, h, w, 0.5))
    counts = np.full(n, SENTINEL, dtype=np.uint32)
    boxes = np.full((n, k, 8), SENTINEL, dtype=np.uint32)
    shapes = np.full((n, k, 16), SENTINEL, dtype=np.uint32)
    hd = op._host
    M, C, B, S = mask.ctypes.data, counts.ctypes.data, boxes.ctypes.data, shapes.ctypes.data
    #        mask n  w  h  conn min K  counts boxes shapes
    cases = [(None, n, w, h, 8, 1, k, C, B, S),
             (M, n, w, h, 8, 1, k, None, B, S),
             (M, n, w, h, 8, 1, k, C, None, S),
             (M, n, w, h, 8, 1, k, C, B, None),
             (M, n, w, h, 6, 1, k, C, B, S),
             (M, n, w, h, 0, 1, k, C, B, S),
             (M, n, 0, h, 8, 1, k, C, B, S),
             (M, n, w, 0, 8, 1, k, C, B, S),
             (M, n, 1 << 24, 1, 8, 1, k, C, B, S),
             (M, n, 1, 1 << 24, 8, 1, k, C, B, S),
             (M, n, 1 << 15, 1 << 15, 8, 1, k, C, B, S),
             (M, n, 65537, 1, 8, 1, k, C, B, S),
             (M, n, 1, 65537, 8, 1, k, C, B, S),
             (M, 1 << 20, w, h, 8, 1, 1 << 9, C, B, S),   # n * K * 8 = 2^32
             (M, 1 << 20, w, h, 8, 1, 1 << 8, C, B, S)]   # n * K * 16 = 2^32
    for m_, n_, w_, h_, conn, area, k_, c_, b_, s_ in cases:
        st = hd._lib.dips_mask_shapes(hd.ptr, m_, None, n_, w_, h_, conn, area, k_, 0, c_, b_, s_)
        assert st == _lib.DIPS_ERR_INVALID, (n_, w_, h_, conn, k_)
        with pytest.raises(DipsError):
            hd.check(st)
        assert (counts == SENTINEL).all() and (boxes == SENTINEL).all() and (shapes == SENTINEL).all()
    # n_frames == 0: fine, nothing written
    assert hd._lib.dips_mask_shapes(hd.ptr, None, None, 0, w, h, 8, 1, k, 0, None, None, None) == 0
    assert hd._lib.dips_mask_shapes(hd.ptr, M, None, 0, w, h, 8, 1, k, 0, C, B, S) == 0
    assert (counts == SENTINEL).all() and (boxes == SENTINEL).all() and (shapes == SENTINEL).all()


def test_misaligned_device_pointers_are_refused(op):
    import torch
    from dips_amd import _lib
    w, h, n, k = 37, 5, 2, 4
    mask = torch.from_numpy(np.concatenate([cref.pack(random_bits(n, h, w, 0.5)).reshape(-1),
                                            np.zeros(8, dtype=np.uint8)])).cuda()
    counts = torch.full((n + 1,), 7, dtype=torch.int32, device="cuda")
    boxes = torch.full((n * k * 8 + 1,), 7, dtype=torch.int32, device="cuda")
    shapes = torch.full((n * k * 16 + 2,), 7, dtype=torch.int32, device="cuda")
    hd = op._dev
    ptrs = [mask.data_ptr(), counts.data_ptr(), boxes.data_ptr(), shapes.data_ptr()]
    for bad in range(4):
        for off in (1, 2) + ((4,) if bad == 3 else ()):  # shapes needs 8 bytes
            p = list(ptrs)
            p[bad] += off
            st = hd._lib.dips_mask_shapes(hd.ptr, p[0], None, n, w, h, 8, 1, k, 0, p[1], p[2], p[3])
            assert st == _lib.DIPS_ERR_INVALID, (bad, off)
    torch.cuda.synchronize()
    assert (counts == 7).all() and (boxes == 7).all() and (shapes == 7).all()


def test_python_layer_refusals(op):
    from dips_amd import ChangeMask
    mask = ChangeMask(cref.pack(random_bits(2, 5, 37, 0.5)), 37)
    with pytest.raises(ValueError):
        op.mask_shapes(mask, np.zeros((2, 5, 36), dtype=np.uint8))
    with pytest.raises(ValueError):
        op.mask_shapes(mask, np.zeros((2, 5, 37), dtype=np.uint16))
    with pytest.raises(ValueError):
        op.mask_shapes(mask, connectivity=6)


def test_kernel_time_has_one_entry_per_call():
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    bits = random_bits(5, 29, 97, 0.5)
    mask = torch.from_numpy(cref.pack(bits)).cuda()
    counts = torch.zeros((5,), dtype=torch.int32, device="cuda")
    boxes = torch.zeros((5, 8, 8), dtype=torch.int32, device="cuda")
    shapes = torch.zeros((5, 8, 16), dtype=torch.int32, device="cuda")
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255, time_kernel=True)
    try:
        o.run_mask_shapes_device(mask, 97, counts, boxes, shapes)                   # one chunk
        o.run_mask_shapes_device(mask, 97, counts, boxes, shapes, chunk_frames=2)   # three chunks
        ms, launches = o.kernel_time()
        each = o.kernel_times()
    finally:
        o.close()
    assert launches == 2 and len(each) == 2 and ms > 0.0 and all(t > 0.0 for t in each)
    same([t.cpu().numpy().view(np.uint32) for t in (counts, boxes, shapes)], want(cref.pack(bits), 97, None, 8))


# -- end to end --------------------------------------------------------------------

def test_change_boxes_and_tracks_with_shapes():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    from test_gpu_mask_components import _moving_clip
    frames = _moving_clip(3, 96, 64, 4)
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    try:
        mask = o.change_mask(frames)
        plain = o.change_boxes(frames, connectivity=4, min_area=3, max_boxes=8)
        boxes, shapes = o.change_boxes(frames, connectivity=4, min_area=3, max_boxes=8, shapes=True)
        tracks_plain = o.change_tracks(frames, connectivity=4, min_area=3, max_boxes=8)
        tracks, tshapes = o.change_tracks(frames, connectivity=4, min_area=3, max_boxes=8, shapes=True)
        with pytest.raises(ValueError):
            o.change_boxes(frames, labels=True, shapes=True)
    finally:
        o.close()
    ref = want(mask.bits, 96, None, 4, 3, 8)
    assert ref[0].any()
    same(shapes.as_arrays(), ref)
    same(tshapes.as_arrays(), ref)
    assert np.array_equal(boxes.boxes, plain.boxes) and np.array_equal(boxes.counts, plain.counts)
    assert all(np.array_equal(a, b) for a, b in zip(tracks.as_arrays(), tracks_plain.as_arrays()))
    assert np.isfinite(shapes.orientation[shapes.valid]).all() and (shapes.holes >= 0).all()


# -- randomized draw ---------------------------------------------------------------

@pytest.mark.parametrize("seed", range(40))
def test_randomized_draw(op, seed):
    rng = np.random.default_rng([53, seed])
    n, h, w = int(rng.integers(1, 5)), int(rng.integers(1, 21)), int(rng.integers(1, 71))
    density = float(rng.choice([0.1, 0.3, 0.5, 0.7, 0.9, 0.97]))
    bits = rng.random((n, h, w)) < density
    weights = rng.integers(0, 256, (n, h, w), dtype=np.uint8) if rng.random() < 0.6 else None
    connectivity = int(rng.choice([4, 8]))
    min_area = int(rng.choice([0, 1, 2, 5]))
    k = int(rng.choice([1, 2, 5, 12]))
    chunk = int(rng.choice([0, 1, 3]))
    check(op, bits, weights, connectivity, min_area, k, pad=int(rng.integers(0, 2)), chunk_frames=chunk)
