"""The builders of tests/_large_masks.py against the specifications, and the
conditions under which tests/test_gpu_mask_large.py is not vacuous: every
round of the offsets scan holds kept roots in every case, the truncating
max_boxes cuts inside the second round, and the planner of mask_abi.hip takes
the clip in more than one round of unequal length.  No GPU."""
import functools

import numpy as np
import pytest

import _components_ref as cref
import _large_masks as lm
import _select_ref as sref


def same(got, want):
    for name, g, r in zip(("counts", "boxes", "labels"), got, want):
        assert g.dtype == r.dtype and g.shape == r.shape, name
        assert np.array_equal(g, r), (name, np.argwhere(g != r)[:5].tolist())


# -- tiled ----------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [4, 8])
def test_tiled_equals_the_specification(connectivity):
    """2 x 3 copies, the last row and column of them cut by the frame's edge."""
    H, W = 104, 239
    case = lm.tiled(lm.standard_tiles(), 2, 3, H, W, connectivity)
    mask = cref.pack(case.bits[None])
    assert case.bits[:, -1].any() and case.bits[-1].any() and not case.bits[63].any() and not case.bits[:, 95].any()
    full = cref.components(mask, W, connectivity, 1, case.count)
    assert int(full[0][0]) == case.count > 50
    assert np.array_equal(case.records, full[1][0]) and np.array_equal(case.labels, full[2][0])
    for min_area, k in ((1, case.count), (40, 7), (1, 0)):
        want = cref.components(mask, W, connectivity, min_area, k)
        same(case.expect(min_area, k), want)
    assert int(want[0][0]) == case.count and 7 < int(case.expect(40, 7)[0][0]) < case.count


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H", lm.DENSE_HEIGHTS)
def test_tiled_at_full_size_equals_scipy(H, connectivity):
    """scipy numbers the components by their first pixel in row-major order too."""
    ndi = pytest.importorskip("scipy.ndimage")
    case = lm.dense_case(H, connectivity)
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    lab, num = ndi.label(case.bits, structure=structure)
    assert num == case.count and np.array_equal(lab, case.labels)
    assert np.array_equal(np.bincount(lab.ravel())[1:], case.records[:, cref.AREA])
    boxes = np.array([[s[1].start, s[0].start, s[1].stop, s[0].stop] for s in ndi.find_objects(lab)])
    assert np.array_equal(boxes, case.records[:, :4])
    first = np.full(num + 1, lab.size, dtype=np.int64)
    np.minimum.at(first, lab.ravel(), np.arange(lab.size))
    assert np.array_equal(first[1:], case.records[:, cref.ANCHOR])
    # the centroids from the pixel sums, by the specification's own rounding
    jj, ii = np.nonzero(case.bits)
    area = case.records[:, cref.AREA].astype(np.int64)
    for field, coord in ((cref.CX256, ii), (cref.CY256, jj)):
        s = np.bincount(lab[jj, ii], weights=coord, minlength=num + 1)[1:].astype(np.int64)
        assert np.array_equal((s // area) * 256 + ((s % area) * 256) // area, case.records[:, field])


# -- rings ----------------------------------------------------------------------------

def test_rings_equal_the_specification():
    H, W = 3 * lm.CELL_H + 5, 3 * lm.CELL_W + 17
    r = lm.rings(H, W)
    assert r.holes.shape[0] == 9 and set(r.holes[:, 0].tolist()) == {lm.CLOSED, lm.CORNER, lm.SIDE}
    assert not np.array_equal(r.filled4, r.filled8) and (r.filled4 & ~r.bits).any()
    for connectivity, filled in ((4, r.filled4), (8, r.filled8)):
        assert np.array_equal(sref.fill_holes(r.bits[None], connectivity)[0], filled)
        split = r.splitting_hole(connectivity)
        part = r.expect(connectivity, split)
        assert (part & ~r.bits).any() and (filled & ~part).any()
        assert np.array_equal(sref.fill_holes(r.bits[None], connectivity, split)[0], part)


def test_rings_at_full_size_equal_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    r = lm.rings()
    kinds = np.bincount(r.holes[:, 0], minlength=3)
    assert r.holes.shape[0] > 1000 and (kinds > 100).all()
    # scipy fills what the background cannot reach from outside under `structure`
    assert np.array_equal(ndi.binary_fill_holes(r.bits, structure=np.ones((3, 3), dtype=bool)), r.filled4)
    assert np.array_equal(ndi.binary_fill_holes(r.bits), r.filled8)
    for connectivity in (4, 8):
        part = r.expect(connectivity, r.splitting_hole(connectivity))
        assert (part & ~r.bits).any() and (r.expect(connectivity) & ~part).any()


# -- kept roots per scan round --------------------------------------------------------

def check_rounds(records, h, w, min_area, min_rounds=2):
    per = lm.kept_per_round(records, h, w, min_area)
    assert per.shape[0] >= min_rounds and (per >= 1).all() and per[-1] >= 3, per.tolist()
    return per


def test_the_shapes_reach_the_rounds_they_are_meant_for():
    assert [lm.n_rounds(h, lm.DENSE_W) for h in lm.DENSE_HEIGHTS] == [2, 3]
    assert lm.n_rounds(lm.RINGS_H, lm.RINGS_W) == 3
    for h, w in ((lm.SPARSE_H, lm.SPARSE_W), (lm.CLIP_H, lm.CLIP_W)):
        wpf = ((w + 31) // 32) * h
        assert lm.n_rounds(h, w) == 2 and (wpf + 255) // 256 == 257  # one block in the second round
    assert (lm.DENSE_W + 31) // 32 == 64 and lm.DENSE_W % 32 == 15
    assert lm.round_of([65535 * 32, 65536 * 32], 2048).tolist() == [0, 1]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H", lm.DENSE_HEIGHTS)
def test_every_round_of_the_dense_cases_holds_kept_roots(H, connectivity):
    case = lm.dense_case(H, connectivity)
    (a1, k_all), (a40, k_cut), (a0, k0) = lm.dense_arguments(H, connectivity)
    assert (a1, k_all, a40, a0, k0) == (1, case.count, lm.DENSE_MIN_AREA, 1, 0)
    check_rounds(case.records, H, lm.DENSE_W, 1, lm.n_rounds(H, lm.DENSE_W))
    per = check_rounds(case.records, H, lm.DENSE_W, a40)
    assert per[0] < k_cut < per[0] + per[1]  # strictly inside the second round
    # the pixels of the last word are in use: the pad bits beside them matter
    assert case.bits[:, 2016:].any()


@functools.lru_cache(maxsize=None)
def sparse_reference(connectivity):
    bits, _ = lm.sparse_frame()
    return cref.components(cref.pack(bits[None]), lm.SPARSE_W, connectivity, lm.SPARSE_MIN_AREA, lm.SPARSE_K,
                           labels=False)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_every_round_of_the_sparse_case_holds_kept_roots(connectivity):
    bits, info = lm.sparse_frame()
    counts, boxes, _ = sparse_reference(connectivity)
    count = int(counts[0])
    assert 20 < count <= lm.SPARSE_K  # every kept root has a record
    per = check_rounds(boxes[0, :count], lm.SPARSE_H, lm.SPARSE_W, lm.SPARSE_MIN_AREA)
    assert per[1] >= 4  # the three bars and the run
    # the run: one component of the stated area, anchored in the last round
    y, x0, x1 = info["run"]
    assert info["run_area"] == x1 - x0 > 64 * 32 + 16 and x0 % 32 != 0 and x1 % 32 != 0
    rec = boxes[0, count - 1]
    assert rec.tolist()[:6] == [x0, y, x1, y + 1, x1 - x0, y * lm.SPARSE_W + x0]
    assert lm.round_of(rec[cref.ANCHOR], lm.SPARSE_W) == 1
    # the line: anchored in the first round, its far end in the last
    lx, ly0, ly1 = info["line"]
    assert bits[ly0:ly1 + 1, lx].all()
    assert lm.round_of(ly0 * lm.SPARSE_W + lx, lm.SPARSE_W) == 0 and lm.round_of(ly1 * lm.SPARSE_W + lx, lm.SPARSE_W) == 1
    assert 0.003 < bits.mean() < 0.01


def test_every_round_of_every_clip_frame_holds_kept_roots():
    clip = lm.moving_clip()
    assert clip.shape == (lm.CLIP_N, lm.CLIP_H, lm.CLIP_W)
    counts, boxes, _ = cref.components(cref.pack(clip), lm.CLIP_W, 8, lm.CLIP_MIN_AREA, lm.CLIP_K, labels=False)
    assert (counts >= 10).all() and (counts <= lm.CLIP_K).all()  # every kept root has a record
    for t in range(lm.CLIP_N):
        check_rounds(boxes[t, :int(counts[t])], lm.CLIP_H, lm.CLIP_W, lm.CLIP_MIN_AREA)
    assert len(set(counts.tolist())) > 1  # some blink


@pytest.mark.parametrize("connectivity", [4, 8])
def test_shapes_by_box_equal_the_specification(connectivity):
    """Components with holes, off the origin, at several densities, with and
    without weights, some records cut off."""
    import _shapes_ref as shref
    rng = np.random.default_rng([137, connectivity])
    bits = np.stack([rng.random((41, 97)) < d for d in (0.2, 0.45, 0.6)])
    bits[:, :3] = bits[:, :, :5] = False
    weights = rng.integers(0, 256, bits.shape, dtype=np.uint8)
    for wts in (None, weights):
        for min_area, k in ((1, 6), (4, 40)):
            want = shref.shapes(cref.pack(bits), 97, wts, connectivity, min_area, k)
            got = lm.shapes_by_box(cref.pack(bits), 97, wts, connectivity, min_area, k)
            same(got, want)
    assert (want[2][..., shref.EULER].view(np.int32) < 0).any() and (want[1][..., cref.X0] > 5).any()


# -- the planner ----------------------------------------------------------------------

SCRATCH = 1 << 30  # kComponentsScratchBytes


def planner_frames(n, h, w, tracks_k=None):
    """chunk_frames = 0 as run_components_device, run_select_device and (with
    K) run_tracks_device of mask_abi.hip resolve it."""
    npx, nslots = w * h, ((w + 1) // 2) * h
    bpf = (((w + 31) // 32) * h + 255) // 256
    per_frame = 4 * npx + 32 * nslots + 4 * bpf
    fixed = 0
    if tracks_k is not None:
        per_frame += 4 * tracks_k * tracks_k + 8 * tracks_k + 8
        fixed = 4 * npx + 4 * nslots + 16 * tracks_k + 8
    frames = max(1, (SCRATCH - min(fixed, SCRATCH)) // per_frame)
    frames = min(frames, n, max(1, (1 << 25) // bpf))
    return min(frames, 256) if tracks_k is not None else frames


def test_the_planner_takes_the_clip_in_unequal_rounds():
    for k in (None, lm.CLIP_K):
        F = planner_frames(lm.CLIP_N, lm.CLIP_H, lm.CLIP_W, k)
        assert F == 25 and 1 < F < lm.CLIP_N and lm.CLIP_N % F != 0
    # what the suite had: every frame of a chunk_frames = 0 case fits one round
    assert planner_frames(7, 33, 65) == 7 and planner_frames(1, 2160, 3840) == 1
    assert planner_frames(100, 2160, 3840) == 6  # the headline workload
