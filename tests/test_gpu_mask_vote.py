"""dips_mask_vote on the GPU against tests/_vote_ref.py: every byte of mask_out
and history_out, pad bytes included.  The shapes are the smallest at which each
mechanism of mask_vote.hip can go wrong: word and row edges and a partial last
run of a lane's words, the window's edges against the clip's ends, the history
in all its forms, a clip fed in chunks, the seams of the frame parts
(series_sched.h vote_geometry, read from the header itself), a 4K frame, the
pointer kinds, the refused arguments, the paths through change_boxes and
change_tracks, and a randomized draw."""
import functools
import os

import numpy as np
import pytest

import _components_ref as cref
import _morph_ref as mref
import _tracks_ref as tref
import _vote_ref as vref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dips_amd", "csrc")
WORDS = vref.words_per_lane(CSRC)  # mask words a lane owns: a tile is 64 * WORDS words
WINDOWS = [(1, 1), (2, 1), (2, 2), (3, 2), (5, 3), (16, 8), (31, 1), (31, 16), (31, 31)]
DENSITIES = (0.05, 0.5, 0.95, 1.0, 0.0)


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
    return frozen(np.random.default_rng([89, seed, n, h, w]).random((n, h, w)) < density)


def run(op, mask_bytes, w, k, m, hist_bytes=None):
    """(mask_out, history_out) bytes of the host path."""
    from dips_amd import ChangeMask
    hist = None if hist_bytes is None else ChangeMask(np.ascontiguousarray(hist_bytes), w)
    out, nxt = op.mask_vote(ChangeMask(np.ascontiguousarray(mask_bytes), w), k, m, hist)
    assert out.width == w and nxt.width == w
    return out.bits, nxt.bits


def check(op, bits, k, m, hist=None, pad=0):
    """GPU == reference for bool bits [n, h, w] and history [k - 1, h, w] or
    None, byte for byte, both outputs; returns the reference's bits."""
    bits = np.asarray(bits, dtype=bool)
    w = bits.shape[2]
    want_bits, want_hist = vref.vote_bits(bits, k, m, hist)
    got, got_hist = run(op, cref.pack(bits, pad), w, k, m, None if hist is None else cref.pack(hist, pad))
    want, want_h = cref.pack(want_bits), cref.pack(want_hist)
    assert got.dtype == np.uint8 and got.shape == want.shape and got_hist.shape == want_h.shape
    assert np.array_equal(got, want), (k, m, bits.shape, np.argwhere(got != want)[:5].tolist())
    assert np.array_equal(got_hist, want_h), (k, m, bits.shape, np.argwhere(got_hist != want_h)[:5].tolist())
    return want_bits


# -- word and row edges ------------------------------------------------------------------

# the last two: 65 words and 3 * 129 words, a partial last run for 1, 2 and 4 words per lane
@pytest.mark.parametrize("w,h", [(w, h) for w in (1, 31, 32, 33, 65, 127, 129) for h in (1, 3)]
                         + [(2075, 1), (4125, 3)])
def test_word_and_row_edges(op, w, h):
    assert (vref.frame_words(2075, 1) % (64 * WORDS), vref.frame_words(4125, 3) % (64 * WORDS)) != (0, 0)
    for d, density in enumerate(DENSITIES):
        bits = random_bits(9, h, w, density, seed=d)
        hist = random_bits(4, h, w, density, seed=10 + d)
        for k, m, hi in ((3, 2, None), (3, 2, hist[:2]), (5, 5, hist), (5, 1, hist)):
            check(op, bits, k, m, hi, pad=1)  # 0xFF in the pad bits of input and history


@pytest.mark.parametrize("w", [1, 33, 63, 97])
def test_garbage_pad_bits_change_nothing(op, w):
    bits, hist = random_bits(7, 3, w, 0.5, seed=1), random_bits(4, 3, w, 0.5, seed=2)
    clean = run(op, cref.pack(bits), w, 5, 3, cref.pack(hist))
    dirty = run(op, cref.pack(bits, 1), w, 5, 3, cref.pack(hist, 1))
    assert not np.array_equal(cref.pack(bits, 1), cref.pack(bits))
    for c, d, want in zip(clean, dirty, vref.vote(cref.pack(bits), w, 5, 3, cref.pack(hist))):
        assert np.array_equal(c, d) and np.array_equal(c, want)


# -- the window's edges ------------------------------------------------------------------

@pytest.mark.parametrize("k,m", WINDOWS)
def test_window_edges(op, k, m):
    for n in sorted({1, max(k - 2, 1), max(k - 1, 1), k, k + 1, 3 * k}):
        for d, density in enumerate(DENSITIES):
            bits = random_bits(n, 3, 37, density, seed=k)
            hist = random_bits(k - 1, 3, 37, (0.5, 0.95, 0.05, 0.0, 1.0)[d], seed=100 + k)
            check(op, bits, k, m)
            got = check(op, bits, k, m, hist, pad=1)
            if k == 1:
                assert np.array_equal(got, bits)


def test_null_history_and_all_votes_leaves_the_first_frames_clear(op):
    for k in (2, 5, 31):
        got = check(op, np.ones((k + 2, 2, 33), dtype=bool), k, k)
        assert not got[:k - 1].any() and got[k - 1:].all()


# -- the history -------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(2, 2), (5, 3), (31, 16), (31, 1)])
def test_history_forms(op, k, m):
    h, w = 3, 65
    zeros, ones = np.zeros((k - 1, h, w), dtype=bool), np.ones((k - 1, h, w), dtype=bool)
    for n in sorted({1, max(k - 2, 1), k - 1, k, k + 5}):  # history_out for n < k - 1, n = k - 1, n > k - 1
        bits = random_bits(n, h, w, 0.4, seed=k + n)
        null = check(op, bits, k, m)
        assert np.array_equal(check(op, bits, k, m, zeros), null)  # NULL is a clear history
        full = check(op, bits, k, m, ones, pad=1)
        assert not (null & ~full).any()
        check(op, bits, k, m, random_bits(k - 1, h, w, 0.6, seed=7))
    # a set history carries into the clip exactly while it is in the window
    got = check(op, np.zeros((k + 1, h, w), dtype=bool), k, 1, ones)
    assert got[:k - 1].all() and not got[k - 1:].any()


def test_no_frames_writes_the_history_only(op):
    from dips_amd import _lib
    h, w, k = 3, 37, 5
    hist = cref.pack(random_bits(k - 1, h, w, 0.5), 1)
    hd = op._host
    for given in (hist, None):
        nxt = np.full_like(hist, 0xA5)
        out = np.full(16, 0xA5, dtype=np.uint8)
        for mi, mo in ((None, None), (out.ctypes.data, out.ctypes.data + 8)):
            st = hd._lib.dips_mask_vote(hd.ptr, mi, 0, w, h, k, 3, given.ctypes.data if given is not None else None,
                                        nxt.ctypes.data, mo)
            assert st == 0
            want = cref.pack(cref.unpack(hist, w)) if given is not None else np.zeros_like(hist)
            assert np.array_equal(nxt, want) and (out == 0xA5).all()
    assert hd._lib.dips_mask_vote(hd.ptr, None, 0, w, h, k, 3, None, None, None) == 0
    assert hd._lib.dips_mask_vote(hd.ptr, None, 0, w, h, 0, 3, None, None, None) == _lib.DIPS_ERR_INVALID
    # the same through the operator
    from dips_amd import ChangeMask
    out, nxt = op.mask_vote(ChangeMask(np.zeros((0, h, hist.shape[2]), dtype=np.uint8), w), k, 3, ChangeMask(hist, w))
    assert out.bits.shape == (0, h, hist.shape[2]) and np.array_equal(nxt.bits, cref.pack(cref.unpack(hist, w)))


# -- chunked equals whole ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def clip300(k, m):
    bits = random_bits(300, 3, 65, 0.5 if m > 1 else 0.03, seed=k)
    return bits, tuple(frozen(a) for a in vref.vote(cref.pack(bits), 65, k, m))


@pytest.mark.parametrize("chunk", [1, 7, 30, 31, 100])
@pytest.mark.parametrize("k,m", [(31, 16), (3, 2), (31, 1)])
def test_chunked_equals_whole_host(op, k, m, chunk):
    bits, (want, want_hist) = clip300(k, m)
    mask = cref.pack(bits, 1)
    outs, hist = [], None
    for s in range(0, 300, chunk):
        o, hist = run(op, mask[s:s + chunk], 65, k, m, hist)
        outs.append(o)
    assert np.array_equal(np.concatenate(outs), want) and np.array_equal(hist, want_hist)


@pytest.mark.parametrize("chunk", [1, 7, 30, 31, 100])
@pytest.mark.parametrize("k,m", [(31, 16), (3, 2)])
def test_chunked_equals_whole_device(op, k, m, chunk):
    import torch
    bits, (want, want_hist) = clip300(k, m)
    mask = torch.from_numpy(cref.pack(bits, 1)).cuda()
    out = torch.full_like(mask, 0xA5)
    hist = [torch.full((k - 1,) + tuple(mask.shape[1:]), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    cur = None  # the first call has no history
    for i, s in enumerate(range(0, 300, chunk)):
        nxt = hist[i & 1]  # ping-pong: never the tensor being read
        op.run_mask_vote_device(mask[s:s + chunk], 65, out[s:s + chunk], k, m, history=cur, history_out=nxt)
        cur = nxt
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(cur.cpu().numpy(), want_hist)


# -- the seams of the frame parts --------------------------------------------------------

@pytest.fixture(scope="module")
def sched(tmp_path_factory):
    return vref.build_geometry(tmp_path_factory.mktemp("vote_sched"), CSRC)


@pytest.mark.parametrize("n,k,m", [(300, 3, 2), (600, 5, 3), (600, 31, 16), (600, 31, 31), (600, 3, 1)])
def test_part_seams(op, sched, n, k, m):
    h, w = 3, 40
    # the cut of this region does not depend on the device's wave slots (one tile, parts of the minimum length)
    cuts = {(q["parts"], q["part_frames"]) for q in
            vref.geometry(sched, [(vref.frame_words(w, h), n, k, WORDS, res) for res in (256, 1024, 4096, 8192, 16384)])}
    assert len(cuts) == 1
    parts, L = cuts.pop()
    assert parts >= 2 and L >= k - 1
    bits = np.array(random_bits(n, h, w, 0.3, seed=k * 40 + m))
    bits[:, 1, :8] = False
    firsts = [p * L for p in range(parts)]
    lasts = [min(n, (p + 1) * L) - 1 for p in range(parts)]
    for s in firsts:   # a run of exactly m set frames ending on a part's first frame
        bits[max(0, s - m + 1):s + 1, 1, 2] = True
    for e in lasts:    # and one ending on its last frame
        bits[e - m + 1:e + 1, 1, 5] = True
    got = check(op, bits, k, m, pad=1)
    for s in firsts[1:]:
        assert got[s, 1, 2] and (m == 1 or not got[s - 1, 1, 2])
    for e in lasts:
        assert got[e, 1, 5] and (m == 1 or not got[e - 1, 1, 5])
    check(op, bits, k, m, random_bits(k - 1, h, w, 0.5, seed=3))


# -- many words --------------------------------------------------------------------------

def test_4k_frames(op):
    w, h = 3840, 2160
    pair = random_bits(2, h, w, 0.5)
    got = check(op, pair, 2, 2)
    assert not got[0].any() and np.array_equal(got[1], pair[0] & pair[1])
    check(op, random_bits(8, h, w, 0.5, seed=1), 5, 3, random_bits(4, h, w, 0.5, seed=2))


# -- pointer kinds -----------------------------------------------------------------------

def test_device_pointers_and_every_byte_written(op):
    import torch
    n, h, w = 40, 5, 129
    bits = random_bits(n, h, w, 0.5, seed=5)
    mask = torch.from_numpy(cref.pack(bits, pad=1)).cuda()
    for k, m, with_hist in ((3, 2, True), (31, 16, False), (1, 1, False), (16, 16, True)):
        hist_bits = random_bits(k - 1, h, w, 0.5, seed=6) if with_hist else None
        hist = torch.from_numpy(cref.pack(hist_bits, pad=1)).cuda() if with_hist else None
        nh = (k - 1) * h * mask.shape[2]
        raw = torch.full((mask.numel() + nh + 12,), 0xA5, dtype=torch.uint8, device="cuda")  # poison
        out = raw[4:4 + mask.numel()].view(mask.shape)
        nxt = raw[8 + mask.numel():8 + mask.numel() + nh].view((k - 1,) + tuple(mask.shape[1:]))
        op.run_mask_vote_device(mask, w, out, k, m, history=hist, history_out=nxt)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
        want, want_hist = vref.vote(cref.pack(bits), w, k, m, None if hist_bits is None else cref.pack(hist_bits))
        assert (got[:4] == 0xA5).all() and (got[4 + mask.numel():8 + mask.numel()] == 0xA5).all() and (got[-4:] == 0xA5).all()
        assert np.array_equal(got[4:4 + mask.numel()].reshape(mask.shape), want)
        if k > 1:
            assert np.array_equal(got[8 + mask.numel():-4].reshape(want_hist.shape), want_hist)
    out = torch.empty_like(mask)
    hist = torch.zeros((2,) + tuple(mask.shape[1:]), dtype=torch.uint8, device="cuda")
    for bad in (dict(out=mask), dict(out=out[:2]), dict(out=out, history=hist[:1]), dict(out=out, history=hist, history_out=hist),
                dict(out=out, history_out=out[:2]), dict(out=out, history_out=mask[:2]), dict(out=out, window=32),
                dict(out=out, votes=4)):
        kw = dict(window=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            op.run_mask_vote_device(mask, w, **kw)


def test_host_pointers_at_odd_alignment(op):
    n, h, w, k, m = 9, 5, 37, 4, 2
    bits, hist_bits = random_bits(n, h, w, 0.5, seed=6), random_bits(k - 1, h, w, 0.5, seed=7)
    mask, hist = cref.pack(bits), cref.pack(hist_bits)
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

    mi, hi, mo, ho = odd(mask.size, mask.tobytes()), odd(hist.size, hist.tobytes()), odd(mask.size), odd(hist.size)
    hd = op._host
    hd.check(hd._lib.dips_mask_vote(hd.ptr, mi.ctypes.data, n, w, h, k, m, hi.ctypes.data, ho.ctypes.data, mo.ctypes.data))
    want, want_hist = vref.vote(mask, w, k, m, hist)
    assert np.array_equal(mo.reshape(mask.shape), want) and np.array_equal(ho.reshape(hist.shape), want_hist)
    for raw in bufs[2:]:
        assert (raw[:1 - raw.ctypes.data % 2] == 0xAB).all() and (raw[-7:] == 0xAB).all()


# -- refusals ----------------------------------------------------------------------------

def test_refused_arguments_leave_the_outputs_untouched(op):
    from dips_amd import DipsError, _lib
    n, h, w, k = 6, 5, 37, 3
    mask = cref.pack(random_bits(n, h, w, 0.5))
    hist = cref.pack(random_bits(k - 1, h, w, 0.5, seed=1))
    nm, nh = mask.size, hist.size
    # one buffer: mask_in | history_in | mask_out | history_out
    buf = np.full(2 * (nm + nh), 0xA5, dtype=np.uint8)
    buf[:nm], buf[nm:nm + nh] = mask.reshape(-1), hist.reshape(-1)
    before = buf.copy()
    hd = op._host
    M = buf.ctypes.data
    H, O = M + nm, M + nm + nh
    N = O + nm
    #        in  n  w  h  k  m  hist hist_out out
    cases = [(None, n, w, h, k, 2, H, N, O),
             (M, n, w, h, k, 2, H, N, None),
             (M, n, w, h, 0, 1, H, N, O),
             (M, n, w, h, 32, 16, H, N, O),
             (M, n, w, h, k, 0, H, N, O),
             (M, n, w, h, k, 4, H, N, O),
             (M, n, w, h, 1, 2, H, N, O),
             (M, n, 0, h, k, 2, H, N, O),
             (M, n, w, 0, k, 2, H, N, O),
             (M, n, 1 << 15, 1 << 15, k, 2, H, N, O),
             (M, n, w, h, k, 2, H, N, M),                 # in place
             (M, n, w, h, k, 2, None, None, M + nm - 1),  # the output's first byte is the input's last
             (M, n, w, h, k, 2, H, N, H),                 # mask_out on history_in
             (M, n, w, h, k, 2, H, None, O - 1),          # ... by one byte
             (M, n, w, h, k, 2, H, M, O),                 # history_out on mask_in
             (M, n, w, h, k, 2, H, M + nm - 1, O + nh),   # ... by one byte
             (M, n, w, h, k, 2, H, H, O),                 # history_out on history_in
             (M, n, w, h, k, 2, H, O - 1, O + nh),        # ... by one byte
             (M, n, w, h, k, 2, H, O, O),                 # the two outputs on each other
             (M, n, w, h, k, 2, H, O + nm - 1, O)]        # ... by one byte
    for c in cases:
        m_, n_, w_, h_, k_, v_, hi_, ho_, o_ = c
        st = hd._lib.dips_mask_vote(hd.ptr, m_, n_, w_, h_, k_, v_, hi_, ho_, o_)
        assert st == _lib.DIPS_ERR_INVALID, c[1:6]
        with pytest.raises(DipsError, match="mask_vote:"):
            hd.check(st)
        assert np.array_equal(buf, before)
    # n_frames == 0 with bad scalars is refused too; with good ones mask_out stays untouched
    assert hd._lib.dips_mask_vote(hd.ptr, M, 0, w, h, k, 4, H, N, O) == _lib.DIPS_ERR_INVALID
    assert np.array_equal(buf, before)
    # touching, not overlapping, ranges are fine
    hd.check(hd._lib.dips_mask_vote(hd.ptr, M, n, w, h, k, 2, H, N, O))
    want, want_hist = vref.vote(mask, w, k, 2, hist)
    assert np.array_equal(buf[nm + nh:2 * nm + nh].reshape(mask.shape), want)
    assert np.array_equal(buf[2 * nm + nh:].reshape(hist.shape), want_hist)
    assert np.array_equal(buf[:nm + nh], before[:nm + nh])
    # window 1 ignores both history pointers: overlapping ones are fine and history_out is not written
    keep = buf.copy()
    hd.check(hd._lib.dips_mask_vote(hd.ptr, M, n, w, h, 1, 1, M, M, O))
    assert np.array_equal(buf[nm + nh:2 * nm + nh].reshape(mask.shape), mask)
    assert np.array_equal(buf[:nm + nh], keep[:nm + nh]) and np.array_equal(buf[2 * nm + nh:], keep[2 * nm + nh:])


def test_misaligned_or_overlapping_device_pointers_are_refused(op):
    import torch
    from dips_amd import _lib
    n, h, w, k = 4, 5, 37, 3
    mask = cref.pack(random_bits(n, h, w, 0.5))
    fb = mask.size // n
    src = torch.from_numpy(np.concatenate([mask.reshape(-1), np.zeros(2 * fb + 8, dtype=np.uint8)])).cuda()
    dst = torch.full((mask.size + 2 * fb + 16,), 7, dtype=torch.uint8, device="cuda")
    hd = op._dev
    S, D = src.data_ptr(), dst.data_ptr()
    HI, HO = S + mask.size, D + mask.size + 8
    for di, do, dhi, dho in ((1, 0, 0, 0), (2, 0, 0, 0), (0, 1, 0, 0), (0, 2, 0, 0), (0, 0, 1, 0), (0, 0, 0, 2), (3, 3, 3, 3)):
        st = hd._lib.dips_mask_vote(hd.ptr, S + di, n, w, h, k, 2, HI + dhi, HO + dho, D + do)
        assert st == _lib.DIPS_ERR_INVALID, (di, do, dhi, dho)
    assert hd._lib.dips_mask_vote(hd.ptr, S, n, w, h, k, 2, None, None, S) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_vote(hd.ptr, S, 1, w, h, k, 2, None, None, S + 4) == _lib.DIPS_ERR_INVALID
    assert hd._lib.dips_mask_vote(hd.ptr, S, n, w, h, k, 2, HI, D + 4, D) == _lib.DIPS_ERR_INVALID
    torch.cuda.synchronize()
    assert (dst == 7).all() and np.array_equal(src.cpu().numpy()[:mask.size], mask.reshape(-1))


# -- the algebra on the device's own outputs, the timing ---------------------------------

@pytest.mark.parametrize("k,m", [(2, 1), (3, 2), (5, 4), (16, 8), (31, 1), (31, 31)])
def test_duality_on_the_devices_own_outputs(op, k, m):
    n, h, w = 2 * k + 3, 4, 97
    inside = cref.pack(np.ones((1, h, w), dtype=bool))
    for density in (0.05, 0.5, 0.95):
        x = cref.pack(random_bits(n, h, w, density, seed=3))
        hist = cref.pack(random_bits(k - 1, h, w, density, seed=4))
        # vote(X, k, m) = D \\ vote(D \\ X, k, k - m + 1), the history complemented too
        got, _ = run(op, x, w, k, m, hist)
        dual, _ = run(op, ~x & inside, w, k, k - m + 1, ~hist & inside)
        assert np.array_equal(got, ~dual & inside)
        # a clear history is NULL; its complement is all ones
        got0, _ = run(op, x, w, k, m)
        dual0, _ = run(op, ~x & inside, w, k, k - m + 1, np.broadcast_to(inside, hist.shape))
        assert np.array_equal(got0, ~dual0 & inside)
        # monotone in m on the device
        if m < k:
            assert not (run(op, x, w, k, m + 1, hist)[0] & ~got).any()


def test_kernel_time_has_one_entry_per_call():
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    bits = random_bits(40, 33, 65, 0.45)
    mask = torch.from_numpy(cref.pack(bits)).cuda()
    out = torch.zeros_like(mask)
    nxt = torch.zeros((4,) + tuple(mask.shape[1:]), dtype=torch.uint8, device="cuda")
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255, time_kernel=True)
    try:
        o.run_mask_vote_device(mask, 65, out, 3)
        o.run_mask_vote_device(mask, 65, out, 5, 3, history_out=nxt)  # two launches, one entry
        o.run_mask_vote_device(mask[:0], 65, out[:0], 5, 3, history_out=nxt)  # the history alone
        ms, launches = o.kernel_time()
        each = o.kernel_times()
    finally:
        o.close()
    assert launches == 3 and len(each) == 3 and ms > 0.0 and all(t > 0.0 for t in each)
    assert np.array_equal(out.cpu().numpy(), vref.vote(cref.pack(bits), 65, 5, 3)[0])
    assert not nxt.cpu().numpy().any()


# -- end to end --------------------------------------------------------------------------

def _flicker_clip(w, h, n):
    """A noise-free background with two bright rectangles that move slowly,
    one-frame specks and a one-frame dropout of one rectangle."""
    rng = np.random.default_rng([97, w, h, n])
    base = rng.integers(40, 90, (h, w, 3), dtype=np.uint8)
    frames = np.repeat(base[None], n, axis=0)
    for t in range(n):
        if t != 4:
            frames[t, 10 + t // 2:24 + t // 2, 6 + t:30 + t] = 230
        frames[t, 40:52, 70 - t:88 - t] = 10
        for y, x in rng.integers(0, (h, w), (5, 2)):
            frames[t, y, x] = 255
    return frames


def test_change_boxes_and_tracks_with_vote():
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, MorphShape, PixelFormat
    w, h, n, K = 96, 64, 9, 16
    frames = _flicker_clip(w, h, n)
    o = DiffSeriesOperator(PixelFormat.RGB8, Mode.Overall, 8 / 255)
    steps = [(MorphOp.Open, MorphShape.Box, 1, 1)]
    try:
        for roi in ((3, 2, 90, 60), None):
            mask = o.change_mask(frames[1:], roi=roi, ref=frames[0])
            rw = mask.width
            plain = cref.components(mask.bits, rw, 8, 1, K)
            for vote, morph in (((3, 2), steps), (3, None), ((2, 2), []), ((5, 1), steps)):
                k, m = vote if isinstance(vote, tuple) else (vote, vote // 2 + 1)
                cleaned = vref.vote(mask.bits, rw, k, m)[0]
                for mop, shape, rx, ry in morph or []:
                    cleaned = mref.morph(cleaned, rw, int(mop), int(shape), rx, ry)
                ref = cref.components(cleaned, rw, 8, 1, K)
                got = o.change_boxes(frames[1:], roi=roi, ref=frames[0], max_boxes=K, labels=True, vote=vote, morph=morph)
                assert ref[0].any() and not np.array_equal(ref[0], plain[0])  # the vote changed the components
                assert all(np.array_equal(g, x) for g, x in zip((got.counts, got.boxes, got.labels), ref))
                want = tref.tracks(cleaned, rw, 8, 1, K, state=np.zeros(1 + 2 * K, dtype=np.uint32))
                tr = o.change_tracks(frames[1:], roi=roi, ref=frames[0], max_boxes=K, vote=vote, morph=morph)
                assert all(np.array_equal(g, x) for g, x in zip((tr.counts, tr.boxes, tr.links, tr.state), want))
            # without vote: today's result
            got = o.change_boxes(frames[1:], roi=roi, ref=frames[0], max_boxes=K, labels=True, vote=None)
            assert all(np.array_equal(g, x) for g, x in zip((got.counts, got.boxes, got.labels), plain))
        for bad in (0, 32, (3, 4), (3, 0), (3, 2, 1)):
            with pytest.raises(ValueError):
                o.change_boxes(frames, vote=bad)
            with pytest.raises(ValueError):
                o.change_tracks(frames, vote=bad)
    finally:
        o.close()


# -- the randomized draw -----------------------------------------------------------------

def draw_case(i):
    """Case i: (bits, k, m, history or None, pad)."""
    rng = np.random.default_rng([101, i])
    w, h, n = int(rng.integers(1, 201)), int(rng.integers(1, 9)), int(rng.integers(1, 81))
    k = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 30, 31]))
    m = int(rng.integers(1, k + 1))
    density = float(rng.choice([0.02, 0.3, 0.5, 0.7, 0.98]))
    bits = rng.random((n, h, w)) < density
    hist = rng.random((k - 1, h, w)) < float(rng.choice([0.1, 0.5, 0.9])) if rng.integers(0, 2) else None
    return bits, k, m, hist, int(rng.integers(0, 2))


@pytest.mark.parametrize("group", range(4))
def test_randomized_cases(op, group):
    """Cases 50 * group .. 50 * group + 49 of draw_case: 200 in all."""
    nontrivial = 0
    for i in range(50 * group, 50 * group + 50):
        bits, k, m, hist, pad = draw_case(i)
        got = check(op, bits, k, m, hist, pad)
        nontrivial += got.any() and not got.all() and not np.array_equal(got, bits)
    assert nontrivial >= 25
