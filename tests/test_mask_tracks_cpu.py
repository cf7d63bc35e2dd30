"""dips_mask_tracks without a GPU: the specification code of
tests/_tracks_ref.py on cases worked by hand, its chunk carry, a check that
the generated clips are not trivial, the header's declaration and constants,
the ctypes binding, the ChangeTracks result type and every argument error the
Python layer raises itself."""
import os
import re

import numpy as np
import pytest

import _components_ref as cref
import _tracks_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = tref.NONE
PAD = [N, 0, N, 0]  # the record beyond a frame's components


def _links(bits, connectivity=8, min_area=1, max_boxes=2, **kw):
    return tref.tracks(cref.pack(bits), bits.shape[2], connectivity, min_area, max_boxes, **kw)


def test_a_moving_square_is_one_track():
    counts, _, links, _ = _links(tref.square_clip())
    assert counts.tolist() == [1, 1, 1, 1]
    assert links.tolist() == [[[N, 0, 0, 0], PAD], [[0, 3, 0, 1], PAD], [[0, 3, 0, 2], PAD], [[0, 3, 0, 3], PAD]]


def test_split_and_merge():
    counts, _, links, _ = _links(tref.split_merge_clip())
    assert counts.tolist() == [1, 2, 1]
    assert links[0].tolist() == [[N, 0, 0, 0], PAD]
    # the 3-pixel child is a head that still names its parent, the 5-pixel child continues
    assert links[1].tolist() == [[0, 3, 1, 0], [0, 5, 0, 1]]
    # the merged bar continues the larger child
    assert links[2].tolist() == [[1, 5, 0, 2], PAD]


def test_an_exact_tie_goes_to_the_smaller_index_on_both_sides():
    counts, _, links, _ = _links(tref.tie_clip())
    assert counts.tolist() == [2, 2]
    assert links[0].tolist() == [[N, 0, 0, 0], [N, 0, 1, 0]]
    # every ov is 1: both rows name column 0, column 0 names row 0
    assert links[1].tolist() == [[0, 1, 0, 1], [0, 1, 2, 0]]


def test_a_gap_of_one_frame_gives_a_new_id():
    counts, _, links, state = _links(tref.gap_clip(), state=np.zeros(5, dtype=np.uint32))
    assert counts.tolist() == [1, 1, 0, 1]
    assert links[:, 0].tolist() == [[N, 0, 0, 0], [0, 6, 0, 1], PAD, [N, 0, 1, 0]]
    assert state.tolist() == [2, 1, N, 0, 0]


def test_components_beyond_k_or_under_min_area_do_not_link():
    counts, boxes, links, _ = _links(tref.excluded_clip(), min_area=2, max_boxes=2)
    assert counts.tolist() == [3, 1] and boxes[0, :, cref.AREA].tolist() == [2, 3]
    assert links[0].tolist() == [[N, 0, 0, 0], [N, 0, 1, 0]]
    # the 6-pixel overlap with component 2 and the single pixel do not count: two ties of 1
    assert links[1].tolist() == [[0, 1, 0, 1], PAD]


def test_ids_start_at_state_and_wrap():
    state = np.array([0xFFFFFFFF, 7, 8, 9, 10], dtype=np.uint32)
    _, _, links, out = _links(tref.tie_clip(), state=state)  # no prev: a scene cut, tracks 7 and 8 are not read
    assert links[:, :, tref.TRACK].tolist() == [[0xFFFFFFFF, 0], [0xFFFFFFFF, 1]]
    assert out.tolist() == [2, 0xFFFFFFFF, 1, 1, 0]
    assert state.tolist() == [0xFFFFFFFF, 7, 8, 9, 10]  # the argument is not modified


@pytest.mark.parametrize("setting", tref.SETTINGS[:2])
def test_reference_chunk_carry(setting):
    """A whole clip equals two calls split at every position, n_frames = 0 included."""
    n, h, w, nobj, K, min_area, connectivity = setting
    mask = cref.pack(tref.moving_rectangles(1, n, h, w, nobj))
    zero = np.zeros(1 + 2 * K, dtype=np.uint32)
    whole = tref.tracks(mask, w, connectivity, min_area, K, state=zero)
    for cut in range(n + 1):
        a = tref.tracks(mask[:cut], w, connectivity, min_area, K, state=zero)
        prev = mask[cut - 1] if cut else None
        b = tref.tracks(mask[cut:], w, connectivity, min_area, K, prev=prev, state=a[3])
        for x, y, z in zip(a[:3], b[:3], whole[:3]):
            assert np.array_equal(np.concatenate([x, y]), z), cut
        assert np.array_equal(b[3], whole[3]), cut
        if cut == 0:
            assert np.array_equal(a[3], zero)  # n_frames = 0 leaves the state alone


@pytest.mark.parametrize("setting", tref.SETTINGS)
def test_generated_clips_are_not_trivial(setting):
    n, h, w, nobj, K, min_area, connectivity = setting
    continued = heads_with_prev = truncated = oldest = 0
    for seed in tref.SEEDS:
        mask = cref.pack(tref.moving_rectangles(seed, n, h, w, nobj))
        counts, _, links, _ = tref.tracks(mask, w, connectivity, min_area, K)
        valid = np.arange(K)[None, :] < np.minimum(counts, K)[:, None]
        age, prev = links[:, :, tref.AGE], links[:, :, tref.PREV]
        continued += int((valid & (age > 0)).sum())
        heads_with_prev += int((valid & (age == 0) & (prev != N)).sum())
        truncated += int((counts > K).sum())
        oldest = max(oldest, int(age.max()))
    assert continued > 0 and heads_with_prev > 0 and truncated > 0 and oldest >= 3, (
        continued, heads_with_prev, truncated, oldest)


def test_header_declares_the_function_and_the_constants():
    from dips_amd import _lib
    assert "dips_mask_tracks" in _lib.header_functions()
    with open(os.path.join(ROOT, "include", "dips_hip.h")) as f:
        text = f.read()
    for k, name in enumerate(("PREV", "OVERLAP", "TRACK", "AGE")):
        assert re.search(r"^#define DIPS_LINK_%s %du$" % (name, k), text, flags=re.M), name
    assert re.search(r"^#define DIPS_LINK_WORDS 4u$", text, flags=re.M)
    assert re.search(r"^#define DIPS_LINK_NONE 0xFFFFFFFFu$", text, flags=re.M)
    assert re.search(r"^#define DIPS_TRACK_MAX_BOXES 256u$", text, flags=re.M)
    assert re.search(r"^#define DIPS_ABI_VERSION 3$", text, flags=re.M)  # no new struct: the version stays
    decl = re.search(r"dips_status dips_mask_tracks\((.*?)\);", text, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["dips_handle *h", "const uint8_t *mask", "uint32_t n_frames", "uint32_t roi_w", "uint32_t roi_h",
                    "uint32_t connectivity", "uint32_t min_area", "uint32_t max_boxes", "uint32_t chunk_frames",
                    "const uint8_t *prev_mask", "uint32_t *state", "uint32_t *counts", "uint32_t *boxes",
                    "uint32_t *links"]
    assert _lib.LINK_WORDS == 4 and _lib.LINK_FIELDS == ("prev", "overlap", "track", "age")
    assert _lib.LINK_NONE == N and _lib.TRACK_MAX_BOXES == 256


def test_ctypes_signature_matches():
    import ctypes

    from dips_amd import _lib
    fn = _lib.load().dips_mask_tracks
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    assert list(fn.argtypes) == [vp, vp] + [u32] * 7 + [vp] * 5
    assert fn.restype is ctypes.c_int


def test_change_tracks_round_trips():
    import dips_amd
    n, h, w, nobj, K, min_area, connectivity = tref.SETTINGS[0]
    mask = cref.pack(tref.moving_rectangles(0, n, h, w, nobj))
    counts, boxes, links, state = tref.tracks(mask, w, connectivity, min_area, K, state=np.zeros(1 + 2 * K, np.uint32))
    ct = dips_amd.ChangeTracks.from_arrays(counts, boxes, links, state)
    assert dips_amd.ChangeTracks.FIELDS == ("prev", "overlap", "track", "age") and dips_amd.ChangeTracks.NONE == N
    back = dips_amd.ChangeTracks.from_arrays(*ct.as_arrays())
    for x, y in zip(back.as_arrays(), (counts, boxes, links, state)):
        assert x.dtype == np.uint32 and np.array_equal(x, y)
    for t in range(n):
        m = min(int(counts[t]), K)
        b, l = ct.frame(t)
        assert np.array_equal(b, boxes[t, :m]) and np.array_equal(l, links[t, :m])
    by_id = ct.tracks()
    assert by_id == tref.tracks_by_id(counts, links)
    assert sorted(by_id) == list(range(int(state[0])))  # every id handed out is used, none twice as a head
    for recs in by_id.values():
        assert [t for t, _ in recs] == list(range(recs[0][0], recs[0][0] + len(recs)))  # one record per frame, no gap
        assert [int(links[t, k, tref.AGE]) for t, k in recs] == list(range(len(recs)))
    assert dips_amd.ChangeTracks.from_arrays(counts, boxes, links).state is None
    with pytest.raises(ValueError):
        dips_amd.ChangeTracks.from_arrays(counts, boxes, links[:, :, :3])
    with pytest.raises(ValueError):
        dips_amd.ChangeTracks.from_arrays(counts, boxes, links[:, :K - 1])
    with pytest.raises(ValueError):
        dips_amd.ChangeTracks.from_arrays(counts[:2], boxes, links)
    with pytest.raises(ValueError):
        dips_amd.ChangeTracks.from_arrays(counts, boxes, links, state[:-1])


def test_python_argument_errors():
    """Raised before the library is reached, so an operator without handles will do."""
    import dips_amd
    op = dips_amd.DiffSeriesOperator.__new__(dips_amd.DiffSeriesOperator)
    good = dips_amd.ChangeMask(cref.pack(np.ones((2, 5, 33), dtype=bool)), 33)
    with pytest.raises(ValueError):
        op.mask_tracks(good.bits)                              # not a ChangeMask
    with pytest.raises(ValueError):
        op.mask_tracks(dips_amd.ChangeMask(good.bits, 65))     # width and row bytes disagree
    with pytest.raises(ValueError):
        op.mask_tracks(dips_amd.ChangeMask(good.bits[0], 33))  # not [n, h, row_bytes]
    for kw in ({"connectivity": 6}, {"connectivity": 0}, {"min_area": -1}, {"min_area": 1 << 32}, {"max_boxes": -1},
               {"max_boxes": 1 << 32}, {"chunk_frames": -1}, {"chunk_frames": 1 << 32},
               {"max_boxes": 0}, {"max_boxes": 257}):
        with pytest.raises(ValueError):
            op.mask_tracks(good, **kw)
    state = np.zeros(1 + 2 * 64, dtype=np.uint32)
    with pytest.raises(ValueError):
        op.mask_tracks(good, prev=good.bits[0])                        # prev without state
    with pytest.raises(ValueError):
        op.mask_tracks(good, prev=good.bits[0, :4], state=state)       # prev is not one frame of the mask
    with pytest.raises(ValueError):
        op.mask_tracks(good, state=state[:-1])                         # state is not [1 + 2K]
    with pytest.raises(ValueError):
        op.mask_tracks(good, max_boxes=8, state=state)
