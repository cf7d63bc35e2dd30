"""dips_mask_tracks on the GPU against tests/_tracks_ref.py: counts, every word
of boxes and links, and the state, exactly; counts and boxes also against
dips_mask_components' own output.  The shapes are the smallest at which each
mechanism of mask_tracks.hip can go wrong: word and row edges, pad bits, the
wave sums (one pair over many waves, 256 pairs in one wave, none), K = 1 and
256, records beyond K, the seam between chunks and between calls, chains
longer than a block and the refused arguments."""
import functools

import numpy as np
import pytest

import _components_ref as cref
import _tracks_ref as tref

pytestmark = pytest.mark.gpu

N = tref.NONE


@pytest.fixture(scope="module")
def op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    yield o
    o.close()


def frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


_MASKS = {}


@functools.lru_cache(maxsize=None)
def _want_cached(key, w, connectivity, min_area, max_boxes, with_state):
    state = np.zeros(1 + 2 * max_boxes, dtype=np.uint32) if with_state else None
    return tuple(frozen(a) for a in tref.tracks(_MASKS[key], w, connectivity, min_area, max_boxes, state=state))


def want(mask_bytes, w, connectivity=8, min_area=1, max_boxes=8, with_state=True):
    """The reference of a whole clip from a zero state, computed once per (mask, arguments)."""
    key = (mask_bytes.shape, mask_bytes.tobytes())
    _MASKS.setdefault(key, mask_bytes)
    return _want_cached(key, w, connectivity, min_area, max_boxes, with_state)


def run_host(op, mask_bytes, w, connectivity=8, min_area=1, max_boxes=8, chunk_frames=0, prev=None, state=None):
    from dips_amd import ChangeMask
    r = op.mask_tracks(ChangeMask(np.ascontiguousarray(mask_bytes), w), connectivity, min_area, max_boxes, chunk_frames,
                       prev, state)
    return r.counts, r.boxes, r.links, r.state


def same(got, ref, what=""):
    for name, g, r in zip(("counts", "boxes", "links", "state"), got, ref):
        if r is None:
            assert g is None, name
            continue
        assert g.dtype == np.uint32 and g.shape == r.shape, (what, name)
        assert np.array_equal(g, r), (what, name, np.argwhere(g != r)[:5].tolist())


def check(op, bits, connectivity=8, min_area=1, max_boxes=8, pad=0, chunk_frames=0):
    """GPU == reference (from a zero state) for bool bits [n, h, w], and
    counts / boxes == dips_mask_components'; returns the reference."""
    from dips_amd import ChangeMask
    bits = np.asarray(bits, dtype=bool)
    w = bits.shape[2]
    ref = want(cref.pack(bits), w, connectivity, min_area, max_boxes)
    mask = cref.pack(bits, pad)
    got = run_host(op, mask, w, connectivity, min_area, max_boxes, chunk_frames,
                   state=np.zeros(1 + 2 * max_boxes, dtype=np.uint32))
    same(got, ref)
    own = op.mask_components(ChangeMask(mask, w), connectivity, min_area, max_boxes, False, chunk_frames)
    assert np.array_equal(got[0], own.counts) and np.array_equal(got[1], own.boxes)
    return ref


def random_bits(n, h, w, density, seed=0):
    return np.random.default_rng([43, seed, n, h, w]).random((n, h, w)) < density


# -- word and row edges, pad bits ---------------------------------------------------

@pytest.mark.parametrize("h", [1, 2, 29])
@pytest.mark.parametrize("w", [1, 31, 32, 33, 64, 65, 97])
def test_word_and_row_edges(op, w, h):
    ones, zero = np.ones((1, h, w), dtype=bool), np.zeros((1, h, w), dtype=bool)
    frames = np.concatenate([random_bits(2, h, w, 0.3), zero, random_bits(3, h, w, 0.5, 1), ones, ones, zero,
                             random_bits(1, h, w, 0.3, 2)])
    for connectivity in (4, 8):
        counts, _, links, _ = check(op, frames, connectivity, max_boxes=8)
        assert links[7, 0].tolist()[:2] == [0, w * h] and links[7, 0, tref.AGE] >= 1  # all ones on all ones
        assert counts[2] == 0 and (links[3, :, tref.PREV] == N).all()                  # nothing before frame 3


@pytest.mark.parametrize("w", [33, 37])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_garbage_pad_bits_are_ignored(op, w, connectivity):
    bits = np.concatenate([random_bits(3, 29, w, 0.5), np.ones((2, 29, w), dtype=bool)])
    check(op, bits, connectivity, pad=0)
    check(op, bits, connectivity, pad=1)  # the same reference: pad bits all ones
    # and in prev_mask: the clip's last four frames behind its first, pad bits set in both
    K = 8
    zero = np.zeros(1 + 2 * K, dtype=np.uint32)
    first = tref.tracks(cref.pack(bits[:1]), w, connectivity, 1, K, state=zero)
    ref = tref.tracks(cref.pack(bits[1:]), w, connectivity, 1, K, prev=cref.pack(bits[:1])[0], state=first[3])
    got = run_host(op, cref.pack(bits[1:], 1), w, connectivity, 1, K, prev=cref.pack(bits[:1], 1)[0], state=first[3])
    same(got, ref)


# -- generated clips, the cases worked by hand ----------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("setting", tref.SETTINGS)
def test_moving_rectangles(op, setting, seed):
    n, h, w, nobj, K, min_area, connectivity = setting
    check(op, tref.moving_rectangles(seed, n, h, w, nobj), connectivity, min_area, K)


def test_cases_worked_by_hand(op):
    pad = [N, 0, N, 0]
    links = check(op, tref.square_clip(), max_boxes=2)[2]
    assert links[:, 0].tolist() == [[N, 0, 0, 0], [0, 3, 0, 1], [0, 3, 0, 2], [0, 3, 0, 3]]
    links = check(op, tref.split_merge_clip(), max_boxes=2)[2]
    assert links.tolist() == [[[N, 0, 0, 0], pad], [[0, 3, 1, 0], [0, 5, 0, 1]], [[1, 5, 0, 2], pad]]
    links = check(op, tref.tie_clip(), max_boxes=2)[2]
    assert links[1].tolist() == [[0, 1, 0, 1], [0, 1, 2, 0]]
    links = check(op, tref.gap_clip(), max_boxes=2)[2]
    assert links[:, 0].tolist() == [[N, 0, 0, 0], [0, 6, 0, 1], pad, [N, 0, 1, 0]]


def test_a_component_beyond_k_or_under_min_area_does_not_link(op):
    links = check(op, tref.excluded_clip(), min_area=2, max_boxes=2)[2]
    assert links[1].tolist() == [[0, 1, 0, 1], [N, 0, N, 0]]
    # and as the current frame: component K + 1 of frame 1 lies on record 0 of frame 0
    links = check(op, tref.excluded_clip()[::-1], min_area=2, max_boxes=2)[2]
    assert links[1].tolist() == [[0, 1, 0, 1], [0, 1, 1, 0]]


# -- the wave sums --------------------------------------------------------------------

def test_one_pair_over_many_waves(op):
    links = check(op, np.ones((2, 96, 128), dtype=bool), max_boxes=3)[2]
    assert links[1, 0].tolist() == [0, 128 * 96, 0, 1]


def test_256_pairs_and_none(op):
    jj, ii = np.mgrid[0:16, 0:32]
    board = (ii + jj) % 2 == 0
    counts, _, links, _ = check(op, np.stack([board, board, ~board, ~board]), connectivity=4, max_boxes=256)
    assert counts.tolist() == [256] * 4
    k = np.arange(256)
    assert np.array_equal(links[1, :, tref.PREV], k) and (links[1, :, tref.OVERLAP] == 1).all()
    assert (links[2, :, tref.PREV] == N).all() and np.array_equal(links[2, :, tref.TRACK], 256 + k)
    assert (links[3, :, tref.AGE] == 1).all()


@pytest.mark.parametrize("K", [1, 256])
def test_smallest_and_largest_k(op, K):
    n, h, w, nobj, _, min_area, connectivity = tref.SETTINGS[3]
    counts = check(op, tref.moving_rectangles(5, n, h, w, nobj), connectivity, 1, K)[0]
    assert (counts > 1).any()


# -- chunks, calls --------------------------------------------------------------------

def test_the_result_does_not_depend_on_chunk_frames(op):
    n, h, w, nobj, K, min_area, connectivity = tref.SETTINGS[1]
    bits = tref.moving_rectangles(3, 7, h, w, nobj)
    for chunk in (0, 1, 2, 3, 7, 100):
        check(op, bits, connectivity, min_area, K, chunk_frames=chunk)


def _device_call(op, mask_dev, w, K, connectivity, min_area, prev=None, state=None, chunk_frames=0):
    import torch
    n = mask_dev.shape[0]
    counts = torch.full((n,), -7, dtype=torch.int32, device=mask_dev.device)
    boxes = torch.full((n, K, 8), -7, dtype=torch.int32, device=mask_dev.device)
    links = torch.full((n, K, 4), -7, dtype=torch.int32, device=mask_dev.device)
    op.run_mask_tracks_device(mask_dev, w, counts, boxes, links, prev=prev, state=state, connectivity=connectivity,
                              min_area=min_area, chunk_frames=chunk_frames)
    return [t.cpu().numpy().view(np.uint32) for t in (counts, boxes, links)]


def test_clip_carry_on_the_device(op):
    """A 6-frame clip in two calls split at every position, with a call of
    no frames between them, equals one call; the state after the last too."""
    import torch
    n, h, w, nobj, K, min_area, connectivity = tref.SETTINGS[0]
    bits = tref.moving_rectangles(4, 6, h, w, nobj)
    mask = cref.pack(bits)
    ref = want(mask, w, connectivity, min_area, K)
    dev = torch.device("cuda", op._dev.device)
    mask_dev = torch.from_numpy(mask).to(dev)
    for cut in range(1, 6):
        state = torch.zeros((1 + 2 * K,), dtype=torch.int32, device=dev)
        a = _device_call(op, mask_dev[:cut], w, K, connectivity, min_area, state=state)
        _device_call(op, mask_dev[:0], w, K, connectivity, min_area, prev=mask_dev[cut - 1], state=state)
        b = _device_call(op, mask_dev[cut:], w, K, connectivity, min_area, prev=mask_dev[cut - 1], state=state,
                         chunk_frames=2)
        got = [np.concatenate([x, y]) for x, y in zip(a, b)] + [state.cpu().numpy().view(np.uint32)]
        same(got, ref, cut)


def test_clip_carry_with_host_pointers(op):
    """The same through host pointers, where prev_mask travels behind the
    mask and the state, read and written, behind the outputs: 37 x 5, six
    frames, four boxes, rounds of two frames, cut in the middle of a round."""
    h, w, K = 5, 37, 4
    mask = cref.pack(random_bits(6, h, w, 0.3, 5))
    ref = want(mask, w, 8, 1, K)
    assert ref[0].max() > K and (ref[2][1:, :, tref.PREV] != N).any()  # records beyond K, and links to carry
    one = run_host(op, mask, w, 8, 1, K, chunk_frames=2, state=np.zeros(1 + 2 * K, dtype=np.uint32))
    same(one, ref)
    a = run_host(op, mask[:3], w, 8, 1, K, chunk_frames=2, state=np.zeros(1 + 2 * K, dtype=np.uint32))
    b = run_host(op, mask[3:], w, 8, 1, K, chunk_frames=2, prev=mask[2], state=a[3])
    same([np.concatenate([x, y]) for x, y in zip(a[:3], b[:3])] + [b[3]], ref)


def test_state_without_prev_is_a_scene_cut(op):
    n, h, w, nobj, K, min_area, connectivity = tref.SETTINGS[2]
    mask = cref.pack(tref.moving_rectangles(6, n, h, w, nobj))
    first = tref.tracks(mask[:4], w, connectivity, min_area, K, state=np.zeros(1 + 2 * K, dtype=np.uint32))
    ref = tref.tracks(mask[4:], w, connectivity, min_area, K, state=first[3])
    got = run_host(op, mask[4:], w, connectivity, min_area, K, state=first[3])
    same(got, ref)
    m0 = min(int(ref[0][0]), K)
    assert m0 > 0 and (got[2][0, :m0, tref.PREV] == N).all()
    assert got[2][0, :m0, tref.TRACK].tolist() == list(range(int(first[3][0]), int(first[3][0]) + m0))
    # no state at all: ids from 0, nothing returned
    same(run_host(op, mask[4:], w, connectivity, min_area, K), tref.tracks(mask[4:], w, connectivity, min_area, K))


def test_a_long_chain(op):
    """300 frames: one object throughout, one that is there two frames of
    three, so ages reach 299 and ids about 100 across several rounds of
    every scan; in one chunk and in chunks of 64."""
    bits = np.zeros((300, 8, 8), dtype=bool)
    bits[:, 1:3, 1:4] = True
    bits[np.arange(300) % 3 != 2, 5:7, 4:7] = True
    for chunk in (0, 64):
        _, _, links, state = check(op, bits, max_boxes=2, chunk_frames=chunk)
        assert links[299, 0].tolist() == [0, 6, 0, 299] and state[0] == 101


def test_host_pointers_against_device_pointers(op):
    import torch
    n, h, w, nobj, K, min_area, connectivity = tref.SETTINGS[3]
    mask = cref.pack(tref.moving_rectangles(7, n, h, w, nobj))
    dev = torch.device("cuda", op._dev.device)
    state = torch.zeros((1 + 2 * K,), dtype=torch.int32, device=dev)
    got_dev = _device_call(op, torch.from_numpy(mask).to(dev), w, K, connectivity, min_area, state=state)
    odd = np.zeros(mask.size + 1, dtype=np.uint8)[1:].reshape(mask.shape)  # a host pointer of odd alignment
    odd[...] = mask
    got_host = run_host(op, odd, w, connectivity, min_area, K, state=np.zeros(1 + 2 * K, dtype=np.uint32))
    same(got_dev + [state.cpu().numpy().view(np.uint32)], got_host)
    same(got_host, want(mask, w, connectivity, min_area, K))


def test_kernel_time_has_one_entry_per_call():
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    K = 8
    mask = cref.pack(random_bits(7, 33, 65, 0.45))
    ref_counts = want(mask, 65, max_boxes=K)[0]
    mask_dev = torch.from_numpy(mask).cuda()
    state = torch.zeros((1 + 2 * K,), dtype=torch.int32, device="cuda")
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255, time_kernel=True)
    try:
        one = _device_call(o, mask_dev, 65, K, 8, 1)[0]                                       # one chunk
        four = _device_call(o, mask_dev, 65, K, 8, 1, chunk_frames=2)[0]                      # four chunks
        carried = _device_call(o, mask_dev[1:], 65, K, 8, 1, prev=mask_dev[0], state=state)[0]  # a labelled predecessor
        ms, launches = o.kernel_time()
        each = o.kernel_times()
    finally:
        o.close()
    assert launches == 3 and len(each) == 3 and ms > 0.0 and all(t > 0.0 for t in each)
    assert np.array_equal(one, ref_counts) and np.array_equal(four, ref_counts) and np.array_equal(carried, ref_counts[1:])


# -- refused arguments ----------------------------------------------------------------

def test_refused_arguments_leave_the_outputs_untouched(op):
    from dips_amd import _lib
    lib, h = op._host._lib, op._host.ptr
    w, rh, n, K = 33, 5, 2, 4
    mask = cref.pack(np.ones((n, rh, w), dtype=bool))
    counts = np.full(n, 0xABABABAB, dtype=np.uint32)
    boxes = np.full((n, K, 8), 0xABABABAB, dtype=np.uint32)
    links = np.full((n, K, 4), 0xABABABAB, dtype=np.uint32)
    state = np.full(1 + 2 * K, 0xABABABAB, dtype=np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(mask_p=p(mask), n_=n, w_=w, h_=rh, conn=8, k=K, prev=None, state_p=p(state), counts_p=p(counts),
             boxes_p=p(boxes), links_p=p(links)):
        return lib.dips_mask_tracks(h, mask_p, n_, w_, h_, conn, 1, k, 0, prev, state_p, counts_p, boxes_p, links_p)

    refused = [dict(k=0), dict(k=257), dict(boxes_p=None), dict(links_p=None), dict(counts_p=None), dict(mask_p=None),
               dict(prev=p(mask), state_p=None), dict(conn=6), dict(w_=0), dict(h_=0), dict(w_=1 << 24),
               dict(w_=1 << 15, h_=1 << 15), dict(n_=1 << 22, k=256)]
    for kw in refused:
        assert call(**kw) == _lib.DIPS_ERR_INVALID, kw
        for a in (counts, boxes, links, state):
            assert (a == 0xABABABAB).all(), kw
    assert call(n_=0) == _lib.DIPS_OK
    for a in (counts, boxes, links, state):
        assert (a == 0xABABABAB).all()
    state[:] = 0
    assert call() == _lib.DIPS_OK
    assert counts.tolist() == [1, 1] and links[1, 0].tolist() == [0, w * rh, 0, 1] and state[0] == 1


def test_misaligned_device_pointers_are_refused(op):
    import torch
    from dips_amd import _lib
    dev = torch.device("cuda", op._dev.device)
    raw = torch.zeros(64, dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.int32, device=dev)
    lib, h = op._dev._lib, op._dev.ptr
    args = (1, 8, 2, 8, 1, 1, 0)
    ok = out.data_ptr()
    assert lib.dips_mask_tracks(h, raw.data_ptr() + 1, *args, None, None, ok, ok + 64, ok + 128) == _lib.DIPS_ERR_INVALID
    assert lib.dips_mask_tracks(h, raw.data_ptr(), *args, None, ok + 2, ok, ok + 64, ok + 128) == _lib.DIPS_ERR_INVALID
    assert lib.dips_mask_tracks(h, raw.data_ptr(), *args, None, None, ok, ok + 64, ok + 130) == _lib.DIPS_ERR_INVALID
    torch.cuda.synchronize()
    assert not out.any().item()


# -- end to end -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def overall_op():
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.Overall, 8 / 255)
    yield o
    o.close()


@pytest.mark.parametrize("route", ["plain", "morph", "background"])
def test_change_tracks_end_to_end(overall_op, route):
    """A moving square over noise below tau, every frame against the same
    reference: change_tracks against the specification applied to the
    library's own mask."""
    from dips_amd import MorphOp, MorphShape
    op = overall_op
    n, h, w, K = 6, 24, 45, 4
    rng = np.random.default_rng(59)
    frames = (100 + rng.integers(-2, 3, size=(n, h, w, 3))).astype(np.uint8)
    for t in range(n):
        frames[t, 5 + t:11 + t, 3 + 4 * t:9 + 4 * t] = 200
    ref_frame = np.full((h, w, 3), 100, dtype=np.uint8)
    kw = {}
    if route == "morph":
        kw["morph"] = [(MorphOp.Open, MorphShape.Box, 1, 1)]
    if route == "background":
        kw["background"] = (2, True)
    got = op.change_tracks(frames, ref=ref_frame, connectivity=8, min_area=2, max_boxes=K, **kw)
    if route == "background":
        mask = op.background_mask(frames, ref=ref_frame, rate_shift=2, selective=True)[0]
    else:
        mask = op.change_mask(frames, ref=ref_frame)
    if route == "morph":
        mask = op.mask_morph(mask, MorphOp.Open, 1, 1, MorphShape.Box)
    ref = tref.tracks(mask.bits, w, 8, 2, K, state=np.zeros(1 + 2 * K, dtype=np.uint32))
    same(got.as_arrays(), ref)
    assert (got.counts >= 1).all()
    longest = max(got.tracks().values(), key=len)
    assert len(longest) == n, "the square is one track through the clip"
