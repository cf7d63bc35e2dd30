"""The screened RGB8 series kernel (dips_amd/csrc/series_v2_screen.h: integer
J path for every pixel, frame_v2's exact intensities only for the 256-pixel
vec rows in which some pixel has |dJ| above the screen level) gives, bit for
bit, all four columns of

* the oracle,
* the same call with DIPS_SERIES_SCREEN=0 (the unscreened body), and
* the exact-f64-sum form (DIPS_FLAG_CROSSCHECK, ISI = 0) in SAD, SJ and count.

Segments.  A wave of the kernel works through segments of consecutive frames
of one tile (1280 pixels); a batch with fewer (tile, frame) items than wave
slots gives every wave ONE frame.  The small shapes (less than a tile with
zero-padded vecs, exactly one tile, tiles plus trailing pixels) therefore
check the tile geometry, and the long segments -- ring fill, the four-frame
main loop, its 1-3 frame tails -- run on 2560x512 frames (1,024 tiles) with
DIPS_SERIES_WAVES_PER_SIMD=1 (1,024 slots on a 256-CU device: a wave per tile,
segments of all n frames) and on 2564x515 (ranges that straddle tiles).  The
part-major schedule is the library's own choice from 256 frames on
(series_sched.h part_geometry; DIPS_PIXEL_PART_FRAMES pins the pixel sums'
and change times' parts, not the series'), so it runs on 262 and 258 frames
of 1280x516, which that cap cuts into two parts of 131 and 129 frames:
asserted through the library's geometry; the second part's first frame
references the last frame of the first."""
import functools

import numpy as np
import pytest

from oracle import np_restatement as nr
from oracle import oracle
from _sched import library_schedule

pytestmark = pytest.mark.gpu

F32 = np.float32
TAU = 8 / 255
TAUS = [2.0 ** -5, TAU, 0.1, 1.0]
BELOW_ISI = 0.03  # < 2^-5: the f64-sum kernel (ISI = 0), screened or not
COUNTS = [1, 2, 3, 4, 5, 9]
SMALL = [(64, 4), (1280, 1), (644, 5)]
U, TILE = 5, 1280


# --------------------------------------------------------------------------
# contents
# --------------------------------------------------------------------------
def _quiet(rng, n, h, w):
    """Frames that differ from one base by -1 / 0 / +1 levels per byte: |dJ| <= 4 everywhere, no hit."""
    base = rng.integers(2, 254, (h, w, 3), dtype=np.uint8)
    noise = rng.integers(-1, 2, (n + 1, h, w, 3)).astype(np.int16)
    fr = (base.astype(np.int16)[None] + noise).astype(np.uint8)
    return fr[1:], fr[0]


def _random(rng, n, h, w):
    fr = rng.integers(0, 256, (n + 1, h, w, 3), dtype=np.uint8)
    return fr[1:], fr[0]


def _middle_only(rng, n, h, w):
    """R = max and B = min stay, G moves between them: dJ = 0 with changed bytes."""
    lo = rng.integers(0, 100, (h, w), dtype=np.uint8)
    hi = rng.integers(160, 256, (h, w), dtype=np.uint8)
    fr = np.empty((n + 1, h, w, 3), dtype=np.uint8)
    fr[..., 0], fr[..., 2] = hi, lo
    fr[..., 1] = rng.integers(100, 160, (n + 1, h, w), dtype=np.uint8)
    return fr[1:], fr[0]


@functools.lru_cache(maxsize=None)
def _edge_pairs():
    """By CPU search at tau = 8/255: (a, b, dj, selected) with a, b = (max, min) byte pairs, J(b) - J(a) = dj for
    dj = 15, 16 (one selected pair and one unselected), 17."""
    t = F32(TAU)
    u = nr.U_LUT
    inten = lambda mx, mn: ((u[mx] + u[mn]).astype(F32) / F32(2)).astype(F32)  # noqa: E731
    found = {}
    for mx in range(40, 256, 3):
        for mn in range(0, mx, 5):
            for dj in (15, 16, 17):
                for dmx in range(0, dj + 1):
                    mx2, mn2 = mx + dmx, mn + dj - dmx
                    if mx2 > 255 or mn2 > mx2:
                        continue
                    sel = bool(np.abs((inten(mx2, mn2) - inten(mx, mn)).astype(F32)) > t)
                    found.setdefault((dj, sel), ((mx, mn), (mx2, mn2)))
        if len(found) == 4:
            break
    assert set(found) == {(15, False), (16, False), (16, True), (17, True)}, sorted(found)
    return [(a, b, dj, sel) for (dj, sel), (a, b) in sorted(found.items())]


def _pixel(pair, where):
    """An RGB pixel with the given (max, min), the max in channel `where`, the third channel between them."""
    mx, mn = pair
    px = [0, 0, 0]
    px[where] = mx
    px[(where + 1) % 3] = mn
    px[(where + 2) % 3] = (mx + mn) // 2
    return px


def _edges(rng, n, h, w):
    """A flat frame with scattered pixels that flip between the two ends of every edge pair (dJ = +-15, +-16
    selected and unselected, +-17), the max in R, G and B in turn, half of them starting at the far end."""
    fr = np.full((n + 1, h, w, 3), 90, dtype=np.uint8)
    pairs = _edge_pairs()
    npx = h * w
    spots = rng.choice(npx, size=min(npx // 2, 6 * len(pairs) * 8), replace=False)
    for k, p in enumerate(spots):
        a, b, _, _ = pairs[k % len(pairs)]
        where = (k // len(pairs)) % 3
        flip = (k // (3 * len(pairs))) % 2
        y, x = divmod(int(p), w)
        for t in range(n + 1):
            fr[t, y, x] = _pixel(b if (t + flip) % 2 else a, where)
    return fr[1:], fr[0]


CONTENTS = {"quiet": _quiet, "random": _random, "middle": _middle_only, "edges": _edges}


def _single_hits(n, h, w):
    """Quiet frames of whole tiles with ONE changed pixel per chosen (tile, frame): lanes 0 and 63, vecs 0 and
    U - 1, the first, second and last frame -- each combination in a tile of its own."""
    assert (h * w) % TILE == 0
    fr, ref = _quiet(np.random.default_rng(77), n, h, w)
    flat = fr.reshape(n, h * w, 3)
    tile = 3
    for lane in (0, 63):
        for u in (0, U - 1):
            for t in sorted({0, min(1, n - 1), n - 1}):
                px = tile * TILE + (u * 64 + lane) * 4 + (tile % 4)
                flat[t, px] = 0 if int(flat[t, px].max()) + int(flat[t, px].min()) >= 255 else 255  # |dJ| >= 255
                tile += 7
    assert tile * TILE < h * w
    return fr, ref


# --------------------------------------------------------------------------
# the three forms
# --------------------------------------------------------------------------
class Forms:
    """The screened, unscreened and f64-sum operators of one (mode, tau)."""

    def __init__(self, monkeypatch, mode, tau):
        from dips_amd import DiffSeriesOperator, Mode, PixelFormat
        make = lambda **kw: DiffSeriesOperator(PixelFormat.RGB8, Mode(mode), tau, **kw)  # noqa: E731
        self.mode, self.tau, self.ops = mode, tau, []
        monkeypatch.delenv("DIPS_SERIES_SCREEN", raising=False)
        self.ops.append(make())
        monkeypatch.setenv("DIPS_SERIES_SCREEN", "0")  # read when the handle is created
        self.ops.append(make())
        monkeypatch.delenv("DIPS_SERIES_SCREEN", raising=False)
        self.ops.append(make(crosscheck=True))

    def close(self):
        for op in self.ops:
            op.close()

    def check(self, frames, ref, what, nthreads=1):
        want, _, _ = oracle.series(frames, mode=self.mode, tau=self.tau, ref=ref, nthreads=nthreads)
        screened, plain, f64 = (op(frames, ref=ref)[0].as_array() for op in self.ops)
        bad = np.nonzero(~np.all(screened == want, axis=1))[0]
        assert bad.size == 0, (what, "screened vs oracle, frames", bad[:8], screened[bad[:2]], want[bad[:2]])
        assert np.array_equal(screened, plain), (what, "screened vs DIPS_SERIES_SCREEN=0")
        assert np.array_equal(screened[:, :3], f64[:, :3]), (what, "screened vs the f64-sum form")
        return want


@pytest.fixture
def forms(monkeypatch):
    made = []

    def make(mode, tau):
        made.append(Forms(monkeypatch, mode, tau))
        return made[-1]
    yield make
    for f in made:
        f.close()


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
def test_edge_pairs_go_both_ways():
    pairs = _edge_pairs()
    assert [(dj, sel) for _, _, dj, sel in pairs] == [(15, False), (16, False), (16, True), (17, True)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("w,h", SMALL)
def test_small_shapes_all_contents(forms, mode, w, h):
    assert (w * h * 3) % 4 == 0
    rng = np.random.default_rng(w * 31 + h)
    clips = {name: make(rng, 9, h, w) for name, make in CONTENTS.items()}
    for tau in TAUS + [BELOW_ISI]:
        f = forms(mode, tau)
        for name, (fr, ref) in clips.items():
            for n in COUNTS:
                f.check(fr[:n], ref, (w, h, mode, tau, name, n, "ref"))
            f.check(fr, None, (w, h, mode, tau, name, "no ref"))


def test_contents_are_what_they_claim(forms):
    """At tau = 8/255: quiet frames select nothing, the middle channel alone moves SAD only, every edge pixel
    counts exactly when its pair is selected, and random frames select most pixels."""
    rng = np.random.default_rng(5)
    h, w, n = 5, 644, 4
    f = forms(1, TAU)
    out = f.check(*_quiet(rng, n, h, w), "quiet")
    assert out[:, 0].min() > 0 and not out[:, 2:].any() and out[:, 1].max() <= 4 * h * w
    out = f.check(*_middle_only(rng, n, h, w), "middle")
    assert out[:, 0].min() > 0 and not out[:, 1:].any()
    out = f.check(*_random(rng, n, h, w), "random")
    assert out[:, 2].min() > h * w // 2
    fr, ref = _edges(rng, n, h, w)
    out = f.check(fr, ref, "edges")
    pairs = _edge_pairs()
    spots = min(h * w // 2, 6 * len(pairs) * 8)
    want = sum(1 for k in range(spots) if pairs[k % len(pairs)][3])
    assert 0 < want < spots and (out[:, 2] == want).all(), (out[:, 2], want, spots)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_long_segments_whole_tiles(forms, monkeypatch, mode, n):
    """2560x512 = 1,024 tiles, a wave per tile: every segment is the n frames of its tile.  Rows of quiet,
    random, edge and middle-channel content (every vec row of a tile alike within a band), then the single
    hits."""
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    monkeypatch.setenv("DIPS_SERIES_WAVES_PER_SIMD", "1")
    w, h = 2560, 512
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode(mode), TAU)
    try:
        waves, tiles, _ = op.geometry(w, h, n)
    finally:
        op.close()
    assert tiles == 1024 and waves <= tiles, (waves, tiles)  # no more waves than tiles: whole-tile segments
    rng = np.random.default_rng(100 + n)
    bands = [make(rng, n, h // 4, w) for make in (_quiet, _random, _edges, _middle_only)]
    fr = np.concatenate([b[0] for b in bands], axis=1)
    ref = np.concatenate([b[1] for b in bands], axis=0)
    hits = _single_hits(n, h, w)
    for tau in TAUS:
        f = forms(mode, tau)
        f.check(fr, ref, (mode, n, tau, "bands"), nthreads=8)
        out = f.check(*hits, (mode, n, tau, "single hits"), nthreads=8)
        if mode == 1 and tau == TAU:
            # four hit pixels in each chosen frame; the frame after a hit differs from it as well
            want = np.zeros(n + 1, dtype=np.uint64)
            for t in sorted({0, min(1, n - 1), n - 1}):
                want[t] += 4
                want[t + 1] += 4
            want = want[:n]
            assert np.array_equal(out[:, 2], want), (out[:, 2], want)


@pytest.mark.parametrize("mode", [0, 1])
def test_long_segments_straddling_tiles(forms, monkeypatch, mode):
    """2564x515: 1,031.7 tiles over 1,024 waves -- ranges start and end inside a tile's frames, and the last
    tile is partly past the frame."""
    monkeypatch.setenv("DIPS_SERIES_WAVES_PER_SIMD", "1")
    w, h, n = 2564, 515, 9
    assert (w * h * 3) % 4 == 0
    rng = np.random.default_rng(9)
    edges, eref = _edges(rng, n, h, w)
    rnd, rref = _random(rng, n, h, w)
    half = h // 2
    fr = np.concatenate([edges[:, :half], rnd[:, half:]], axis=1)
    ref = np.concatenate([eref[:half], rref[half:]], axis=0)
    for tau in (TAU, 1.0):
        forms(mode, tau).check(fr, ref, (mode, tau), nthreads=8)


@pytest.mark.parametrize("n", [262, 258])
def test_part_major_schedule(forms, monkeypatch, n):
    """Two parts of 131 (129) frames of 516 tiles: segments of 32 main-loop rounds and a 3 (1) frame tail, the
    second part's reference the first part's last frame."""
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    monkeypatch.setenv("DIPS_SERIES_WAVES_PER_SIMD", "1")
    w, h = 1280, 516
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, TAU)
    try:
        sch = library_schedule(op, w, h, n)
    finally:
        op.close()
    assert sch is not None and sch[0] == (n + 1) // 2 and sch[1] == 2, sch
    rng = np.random.default_rng(n)
    quiet, qref = _quiet(rng, n, h, w)
    # a third of the rows random, a few edge pixels in the quiet rest
    rnd = rng.integers(0, 256, (n, h // 3, w, 3), dtype=np.uint8)
    quiet[:, :h // 3] = rnd
    pairs = _edge_pairs()
    for k in range(64):
        a, b, _, _ = pairs[k % len(pairs)]
        y, x = h // 3 + 1 + (k * 5) % (h - h // 3 - 1), (k * 197) % w
        quiet[(k % 2)::2, y, x] = _pixel(a, k % 3)
        quiet[1 - (k % 2)::2, y, x] = _pixel(b, k % 3)
    forms(1, TAU).check(quiet, qref, ("per-frame", n), nthreads=16)
    if n == 262:
        forms(0, TAU).check(quiet, qref, ("overall", n), nthreads=16)
