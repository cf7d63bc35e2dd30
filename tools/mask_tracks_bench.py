#!/usr/bin/env python3
"""mask_tracks_bench.py -- what linking the components of the change mask
across frames (dips_mask_tracks) costs beside labelling alone and beside the
only route to tracks that existed before it.

Workload: a resident 3840x2160 mask of --frames frames, (connectivity 8,
min_area 16, K 64).  --clip synthetic: the change mask of the synthetic RGB8
frames, 'per-frame' mode, tau = 8/255 (nearly empty: the launch floor).
--clip rectangles: a fabricated mask of 32 drifting rectangles of 40 .. 200
pixels a side, some crossing, so that the time depends on real overlaps.
Legs alternated within every repetition:

  1. components    dips_mask_components alone, device events, ms per frame.
                   With --parent-lib it is called in the library of the parent
                   commit (a second libdips_hip.so loaded beside this build's).
  2. label_route   the route before this call, on the first --route-frames
                   frames: dips_mask_components with labels, the overlap
                   tables from the label images in torch on the device (one
                   batched bincount of lab_t * (K + 1) + lab_{t-1}), the
                   tables copied to the host, the argmax, the mutual test and
                   the ids there.  Wall clock, ms per frame.
  3. tracks        dips_mask_tracks on the whole mask, device events
                   (tracks_events, beside leg 1), and on the first
                   --route-frames frames with the copy of counts, boxes and
                   links to the host, wall clock (tracks_route, beside leg 2).
                   change_tracks (synthetic clip only): DiffSeriesOperator.
                   change_tracks end to end, wall clock.

Prints one JSON line (and writes it to --out).  Exits 1 unless tracks_route is
faster than label_route in every repetition and its links equal the links
built from leg 2's tables.
Run on the GPU box:
    python tools/mask_tracks_bench.py --clip rectangles [--parent-lib PATH] [--out profiles/mask_tracks/NAME.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NONE = 0xFFFFFFFF


class ParentComponents:
    """dips_mask_components of another libdips_hip.so (device pointers, the caller's stream)."""

    def __init__(self, path, params, stream):
        from dips_amd._lib import DipsParams
        self.lib = ctypes.CDLL(path)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        self.lib.dips_create.argtypes = [ctypes.POINTER(DipsParams), ctypes.c_int, ctypes.POINTER(vp)]
        self.lib.dips_set_stream.argtypes = [vp, vp]
        self.lib.dips_mask_components.argtypes = [vp, vp] + [u32] * 7 + [vp] * 3
        self.lib.dips_destroy.argtypes = [vp]
        self.lib.dips_destroy.restype = None
        self.h = vp()
        assert self.lib.dips_create(ctypes.byref(params), 0, ctypes.byref(self.h)) == 0
        assert self.lib.dips_set_stream(self.h, vp(stream)) == 0

    def run(self, mask, w, conn, area, counts, boxes):
        n, h = mask.shape[:2]
        st = self.lib.dips_mask_components(self.h, mask.data_ptr(), n, w, h, conn, area, boxes.shape[1], 0,
                                           counts.data_ptr(), boxes.data_ptr(), None)
        assert st == 0, st

    def close(self):
        self.lib.dips_set_stream(self.h, None)
        self.lib.dips_destroy(self.h)


def links_from_tables(counts, ov, K):
    """The links of dips_mask_tracks from counts [n] and the overlap tables
    ov [n, K, K] (ov[0] zeros), on the host."""
    n = counts.shape[0]
    links = np.zeros((n, K, 4), dtype=np.uint32)
    links[:, :, 0] = NONE
    links[:, :, 2] = NONE
    next_id = 0
    trk_p, age_p = None, None
    for t in range(n):
        m = min(int(counts[t]), K)
        o = ov[t]
        prev, best = o.argmax(axis=1), o.max(axis=1)  # the first maximum: the smallest index on a tie
        nxt = np.where(o.max(axis=0) > 0, o.argmax(axis=0), -1)
        trk, age = np.full(K, NONE, dtype=np.uint32), np.zeros(K, dtype=np.uint32)
        for k in range(m):
            if best[k] > 0:
                links[t, k, 0], links[t, k, 1] = prev[k], best[k]
            if best[k] > 0 and nxt[prev[k]] == k:
                trk[k], age[k] = trk_p[prev[k]], age_p[prev[k]] + 1
            else:
                trk[k] = next_id
                next_id += 1
        links[t, :m, 2], links[t, :m, 3] = trk[:m], age[:m]
        trk_p, age_p = trk, age
    return links


def summary(ms):
    return {"ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
            "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}


def timed_events(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rectangles_mask(torch, dev, F, H, W, RB, seed=11, nobj=32):
    """uint8 [F, H, RB]: nobj rectangles of 40 .. 200 pixels a side that drift
    by -6 .. 6 pixels per frame and wrap around the frame."""
    rng = np.random.default_rng(seed)
    sw, sh = rng.integers(40, 201, nobj), rng.integers(40, 201, nobj)
    x0, y0 = rng.integers(0, W - 200, nobj), rng.integers(0, H - 200, nobj)
    vx, vy = rng.integers(-6, 7, nobj), rng.integers(-6, 7, nobj)
    weights = (1 << torch.arange(8, device=dev, dtype=torch.int32))
    mask = torch.empty((F, H, RB), dtype=torch.uint8, device=dev)
    for t in range(F):
        img = torch.zeros((H, RB * 8), dtype=torch.bool, device=dev)
        for i in range(nobj):
            x, y = int(x0[i] + vx[i] * t) % (W - 200), int(y0[i] + vy[i] * t) % (H - 200)
            img[y:y + int(sh[i]), x:x + int(sw[i])] = True
        mask[t] = (img.reshape(H, RB, 8).to(torch.int32) * weights).sum(dim=-1).to(torch.uint8)
    return mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", choices=("synthetic", "rectangles"), default="synthetic")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route-frames", type=int, default=16, help="frames legs 2 and 3 (tracks_route) run per repetition")
    ap.add_argument("--parent-lib", default=None, help="libdips_hip.so of the parent commit for leg 1")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, _lib, mask_row_bytes
    from dips_amd.api import _params

    W, H, F = args.width, args.height, args.frames
    conn, area, K = 8, 16, 64
    tau = 8 / 255
    dev = torch.device("cuda", 0)
    RB = mask_row_bytes(W)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, tau)
    frames = None
    if args.clip == "synthetic":
        frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        op.synth_device(frames, W, H, 0xD1B5, 0)
        mask = torch.empty((F, H, RB), dtype=torch.uint8, device=dev)
        op.run_change_mask_device(frames, mask)
    else:
        mask = rectangles_mask(torch, dev, F, H, W, RB)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    params = _params(fmt=PixelFormat.RGB8, mode=Mode.PerFrame, tau=tau, flags=_lib.FLAG_DEVICE_PTRS)
    parent = ParentComponents(os.path.abspath(args.parent_lib), params, stream) if args.parent_lib else None
    R = min(args.route_frames, F)

    def i32(*shape):
        return torch.full(shape, -1, dtype=torch.int32, device=dev)

    counts1, boxes1 = i32(F), i32(F, K, 8)
    counts2, boxes2, labels2 = i32(R), i32(R, K, 8), i32(R, H, W)
    counts3, boxes3, links3 = i32(F), i32(F, K, 8), i32(F, K, 4)
    counts3r, boxes3r, links3r = i32(R), i32(R, K, 8), i32(R, K, 4)
    kept = {}

    def leg_components():
        if parent is not None:
            parent.run(mask, W, conn, area, counts1, boxes1)
        else:
            op.run_mask_components_device(mask, W, counts1, boxes1, connectivity=conn, min_area=area)

    def leg_label_route():
        op.run_mask_components_device(mask[:R], W, counts2, boxes2, labels2, connectivity=conn, min_area=area)
        lab = torch.where(labels2 <= K, labels2, 0).to(torch.int64).reshape(R, -1)
        cells = (K + 1) * (K + 1)
        key = lab[1:] * (K + 1) + lab[:-1] + torch.arange(R - 1, device=dev)[:, None] * cells
        table = torch.bincount(key.reshape(-1), minlength=(R - 1) * cells).reshape(R - 1, K + 1, K + 1)
        ov = np.zeros((R, K, K), dtype=np.int64)
        ov[1:] = table[:, 1:, 1:].cpu().numpy()
        kept["links2"] = links_from_tables(counts2.cpu().numpy().view(np.uint32), ov, K)
        kept["boxes2"] = boxes2.cpu().numpy()

    def leg_tracks_events():
        op.run_mask_tracks_device(mask, W, counts3, boxes3, links3, connectivity=conn, min_area=area)

    def leg_tracks_route():
        op.run_mask_tracks_device(mask[:R], W, counts3r, boxes3r, links3r, connectivity=conn, min_area=area)
        kept["links3"] = links3r.cpu().numpy().view(np.uint32)
        kept["counts3"], kept["boxes3"] = counts3r.cpu().numpy(), boxes3r.cpu().numpy()

    event_legs = {"components": (leg_components, F), "tracks_events": (leg_tracks_events, F)}
    wall_legs = {"label_route": (leg_label_route, R), "tracks_route": (leg_tracks_route, R)}
    if frames is not None:
        wall_legs["change_tracks"] = (lambda: op.change_tracks(frames, connectivity=conn, min_area=area, max_boxes=K), F)
    for fn, _ in list(event_legs.values()) + list(wall_legs.values()):
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in list(event_legs) + list(wall_legs)}
    for _ in range(args.reps):  # alternated: every repetition runs every leg once
        for name, (fn, per) in event_legs.items():
            ms[name].append(timed_events(torch, fn) / per)
        for name, (fn, per) in wall_legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / per)

    out = {"metric": "dips_mask_tracks vs dips_mask_components alone vs components with labels -> bincount of label pairs in "
                     "torch -> argmax and ids on the host, 4K mask, ms PER FRAME",
           "clip": args.clip, "frames": F, "width": W, "height": H, "reps": args.reps, "route_frames": R,
           "connectivity": conn, "min_area": area, "max_boxes": K,
           "timing": "components, tracks_events: device events around one call over all frames; label_route, tracks_route: "
                     "wall clock around the call on the first route_frames frames, results on the host; change_tracks: wall "
                     "clock end to end; all divided by the frames of the call; legs alternated per repetition",
           "leg1_library": "parent commit" if args.parent_lib else "this build"}
    out.update(summary(ms))
    med = out["median_ms"]
    c3 = counts3.cpu().numpy().view(np.uint32)
    l3 = links3.cpu().numpy().view(np.uint32)
    valid = np.arange(K)[None, :] < np.minimum(c3, K)[:, None]
    out["mask_set_share"] = round(float(np.unpackbits(mask[:R].cpu().numpy()).mean()) * (RB * 8) / W, 5)
    out["components_per_frame_median"] = float(np.median(c3))
    out["continued_records"] = int((valid & (l3[:, :, 3] > 0)).sum())
    out["heads_with_prev"] = int((valid & (l3[:, :, 3] == 0) & (l3[:, :, 0] != NONE)).sum())
    out["oldest_age"] = int(l3[:, :, 3].max())
    out["ratio_tracks_to_components"] = round(med["tracks_events"] / med["components"], 3)
    out["ratio_label_route_to_tracks_route"] = round(med["label_route"] / med["tracks_route"], 1)
    out["links_agree"] = bool(np.array_equal(kept["links2"], kept["links3"]) and np.array_equal(kept["links3"], l3[:R]))
    out["boxes_agree"] = bool(np.array_equal(kept["boxes2"], kept["boxes3"])
                              and np.array_equal(boxes1.cpu().numpy(), boxes3.cpu().numpy())
                              and np.array_equal(counts1.cpu().numpy(), counts3.cpu().numpy()))
    out["tracks_faster_than_label_route_every_rep"] = bool(max(ms["tracks_route"]) < min(ms["label_route"]))
    ok = out["links_agree"] and out["boxes_agree"] and out["tracks_faster_than_label_route_every_rep"]
    if parent is not None:
        parent.close()
    op.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
