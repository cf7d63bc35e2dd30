#!/usr/bin/env python3
"""mask_components_bench.py -- what the connected components of the change
mask (dips_mask_components) cost beside the mask itself and beside the only
route to blobs and boxes that existed before them.

Workload (--legs clip): 3840x2160 RGB8 synthetic frames resident in HBM,
'per-frame' mode, tau = 8/255.  Legs alternated within every repetition:

  1. mask          dips_diff_change_mask alone, device events.  With
                   --parent-lib it is called in the library of the parent
                   commit (a second libdips_hip.so loaded beside this build's).
  2. scipy_route   today's route: the device mask of leg 1 copied to the host,
                   then scipy.ndimage.label + find_objects per frame in a pool
                   of --workers processes (started before the GPU is opened),
                   on the first --route-frames frames; wall clock, ms per
                   frame.  Absent (and said so in the JSON) where scipy is not
                   installed: the pass mark then cannot be applied.
  3. cc8 / cc4     dips_mask_components on the resident mask of leg 1 at
                   (connectivity 8, min_area 16, K 64) and (4, 1, 64), each
                   without and with labels (cc8_labels / cc4_labels); device
                   events, ms per frame.  change_boxes: DiffSeriesOperator.
                   change_boxes end to end (mask + components + the copy of
                   counts and boxes to the host), wall clock.

--legs fabricated: the same call on three fabricated 4K masks of --fab-frames
frames each -- all ones (connectivity 8), a checkerboard at connectivity 4 (one
component per set pixel) and random at density 0.593 (8 and 4) -- because the
call's time depends on the bits.  One call per mask first, reported as it
ends, then the repetitions.

Prints one JSON line (and writes it to --out).  --legs clip exits 1 unless
(leg 2 present) leg 3 is faster per frame than leg 2 in every repetition and
leg 3's counts and records equal leg 2's labelling on the frames leg 2 ran.
Run on the GPU box:
    python tools/mask_components_bench.py --legs clip [--parent-lib PATH] [--out profiles/mask_components/NAME.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def scipy_frame(job):
    """One frame of leg 2 in a worker: (mask bytes [h, row_bytes], w,
    connectivity, full).  full: also the records of dips_mask_components at
    (min_area, K), from scipy's labelling, for the comparison."""
    from scipy import ndimage as ndi
    mask_bytes, w, connectivity, full, min_area, k = job
    bits = np.unpackbits(mask_bytes, axis=-1, bitorder="little")[:, :w]
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else None
    lab, num = ndi.label(bits, structure=structure)
    objs = ndi.find_objects(lab)
    if not full:
        return num, len(objs)
    flat = lab.ravel()
    area = np.bincount(flat, minlength=num + 1)[1:]
    _, first = np.unique(flat, return_index=True)  # labels in raster order of their first pixel
    first = first[1:] if flat[first[0]] == 0 else first
    xs = np.tile(np.arange(w, dtype=np.float64), lab.shape[0])
    ys = np.repeat(np.arange(lab.shape[0], dtype=np.float64), w)
    si = np.bincount(flat, weights=xs, minlength=num + 1)[1:].astype(np.int64)  # exact below 2^53
    sj = np.bincount(flat, weights=ys, minlength=num + 1)[1:].astype(np.int64)
    kept = np.flatnonzero(area >= max(min_area, 1))
    recs = np.zeros((k, 8), dtype=np.uint32)
    for r, c in enumerate(kept[:k].tolist()):
        a = int(area[c])
        recs[r] = [objs[c][1].start, objs[c][0].start, objs[c][1].stop, objs[c][0].stop, a, int(first[c]),
                   (int(si[c]) // a) * 256 + ((int(si[c]) % a) * 256) // a,
                   (int(sj[c]) // a) * 256 + ((int(sj[c]) % a) * 256) // a]
    return int(kept.size), recs


class ParentMask:
    """dips_diff_change_mask of another libdips_hip.so (device pointers, the caller's stream)."""

    def __init__(self, path, params, stream):
        from dips_amd._lib import DipsParams
        self.lib = ctypes.CDLL(path)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        self.lib.dips_create.argtypes = [ctypes.POINTER(DipsParams), ctypes.c_int, ctypes.POINTER(vp)]
        self.lib.dips_set_stream.argtypes = [vp, vp]
        self.lib.dips_diff_change_mask.argtypes = [vp, u32, u32, vp, u32, vp, vp, vp]
        self.lib.dips_destroy.argtypes = [vp]
        self.lib.dips_destroy.restype = None
        self.h = vp()
        assert self.lib.dips_create(ctypes.byref(params), 0, ctypes.byref(self.h)) == 0
        assert self.lib.dips_set_stream(self.h, vp(stream)) == 0

    def run(self, frames, mask):
        n, h, w = frames.shape[:3]
        st = self.lib.dips_diff_change_mask(self.h, w, h, frames.data_ptr(), n, None, None, mask.data_ptr())
        assert st == 0, st

    def close(self):
        self.lib.dips_set_stream(self.h, None)
        self.lib.dips_destroy(self.h)


def summary(ms):
    return {"ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
            "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}


def timed_events(torch, fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def clip_legs(args, pool, have_scipy):
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, _lib, mask_row_bytes
    from dips_amd.api import _params

    W, H, F = args.width, args.height, args.frames
    tau = 8 / 255
    dev = torch.device("cuda", 0)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, tau)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    params = _params(fmt=PixelFormat.RGB8, mode=Mode.PerFrame, tau=tau, flags=_lib.FLAG_DEVICE_PTRS)
    RB = mask_row_bytes(W)
    mask = torch.full((F, H, RB), 0xFF, dtype=torch.uint8, device=dev)
    parent = ParentMask(os.path.abspath(args.parent_lib), params, stream) if args.parent_lib else None
    K = 64
    configs = {"cc8": (8, 16), "cc4": (4, 1)}
    outs = {name: (torch.full((F,), -1, dtype=torch.int32, device=dev),
                   torch.full((F, K, 8), -1, dtype=torch.int32, device=dev)) for name in configs}
    labels = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    R = min(args.route_frames, F)

    def leg_mask():
        if parent is not None:
            parent.run(frames, mask)
        else:
            op.run_change_mask_device(frames, mask)

    def leg_cc(name, with_labels):
        conn, area = configs[name]
        counts, boxes = outs[name]
        op.run_mask_components_device(mask, W, counts, boxes, labels if with_labels else None, connectivity=conn,
                                      min_area=area)

    def scipy_route(conn, full=False, area=1):
        host = mask[:R].cpu().numpy()  # the copy is part of the route
        return pool.map(scipy_frame, [(host[t], W, conn, full, area, K) for t in range(R)])

    event_legs = {"mask": (leg_mask, F * args.inner, args.inner)}
    for name in configs:
        event_legs[name] = (lambda name=name: leg_cc(name, False), F, 1)
        event_legs[name + "_labels"] = (lambda name=name: leg_cc(name, True), F, 1)
    wall_legs = {"change_boxes": (lambda: op.change_boxes(frames, connectivity=8, min_area=16, max_boxes=K), F)}
    if have_scipy:
        wall_legs["scipy_route8"] = (lambda: scipy_route(8), R)
        wall_legs["scipy_route4"] = (lambda: scipy_route(4), R)

    leg_mask()
    for fn, _, _ in event_legs.values():
        fn()
    for fn, _ in wall_legs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in list(event_legs) + list(wall_legs)}
    for _ in range(args.reps):  # alternated: every repetition runs every leg once
        for name, (fn, per, inner) in event_legs.items():
            ms[name].append(timed_events(torch, fn, inner) * inner / per)
        for name, (fn, per) in wall_legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / per)

    out = {"metric": "connected components of the change mask vs the mask alone vs mask -> host -> scipy.ndimage.label + "
                     "find_objects in a process pool, 4K RGB8 per-frame tau=8/255, ms PER FRAME",
           "frames": F, "width": W, "height": H, "reps": args.reps, "inner_mask": args.inner, "route_frames": R,
           "workers": args.workers, "max_boxes": K, "configs": {k: list(v) for k, v in configs.items()},
           "timing": "mask, cc*: device events on one stream; change_boxes, scipy_route*: wall clock around the call; all "
                     "divided by the frames of the call; legs alternated per repetition",
           "leg1_library": "parent commit" if args.parent_lib else "this build",
           "scipy": have_scipy}
    out.update(summary(ms))
    med = out["median_ms"]
    c8 = outs["cc8"][0].cpu().numpy().view(np.uint32)
    c4 = outs["cc4"][0].cpu().numpy().view(np.uint32)
    out["mask_set_share"] = round(float(np.unpackbits(mask[:R].cpu().numpy()).mean()) * (RB * 8) / W, 4)
    out["components_per_frame_median"] = {"cc8": float(np.median(c8)), "cc4": float(np.median(c4))}
    out["ratio_cc8_to_mask"] = round(med["cc8"] / med["mask"], 3)
    out["ratio_cc4_to_mask"] = round(med["cc4"] / med["mask"], 3)
    out["labels_cost_ms"] = {k: round(med[k + "_labels"] - med[k], 4) for k in configs}
    ok = True
    if have_scipy:
        agree = {}
        for name, (conn, area) in configs.items():
            want = scipy_route(conn, True, area)
            counts = outs[name][0][:R].cpu().numpy().view(np.uint32)
            boxes = outs[name][1][:R].cpu().numpy().view(np.uint32)
            agree[name + "_counts"] = bool(all(int(counts[t]) == want[t][0] for t in range(R)))
            agree[name + "_records"] = bool(all(np.array_equal(boxes[t], want[t][1]) for t in range(R)))
        out["agree"] = agree
        out["cc8_faster_than_scipy_every_rep"] = bool(max(ms["cc8"]) < min(ms["scipy_route8"]))
        out["cc4_faster_than_scipy_every_rep"] = bool(max(ms["cc4"]) < min(ms["scipy_route4"]))
        out["ratio_scipy_route8_to_cc8"] = round(med["scipy_route8"] / med["cc8"], 1)
        out["ratio_scipy_route4_to_cc4"] = round(med["scipy_route4"] / med["cc4"], 1)
        ok = all(agree.values()) and out["cc8_faster_than_scipy_every_rep"] and out["cc4_faster_than_scipy_every_rep"]
    else:
        out["note"] = "scipy is not importable here: leg 2 is absent and the pass mark cannot be applied"
    if parent is not None:
        parent.close()
    op.close()
    return out, ok


def fabricated_legs(args):
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes

    W, H, F = args.width, args.height, args.fab_frames
    dev = torch.device("cuda", 0)
    RB = mask_row_bytes(W)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    rows = torch.arange(H, device=dev)[:, None]
    board_row = torch.where(rows % 2 == 0, 0x55, 0xAA).to(torch.uint8)
    rnd = torch.rand((F, H, RB * 8), device=dev, generator=torch.Generator(device=dev).manual_seed(7)) < 0.593
    weights = (1 << torch.arange(8, device=dev, dtype=torch.int32))
    packed = (rnd.reshape(F, H, RB, 8).to(torch.int32) * weights).sum(dim=-1).to(torch.uint8)
    masks = {"all_ones_c8": (torch.full((F, H, RB), 0xFF, dtype=torch.uint8, device=dev), 8),
             "checkerboard_c4": (board_row[None].expand(F, H, RB).contiguous(), 4),
             "random_0593_c8": (packed, 8),
             "random_0593_c4": (packed, 4)}
    counts = torch.zeros((F,), dtype=torch.int32, device=dev)
    boxes = torch.zeros((F, 64, 8), dtype=torch.int32, device=dev)
    first, ms, comps = {}, {k: [] for k in masks}, {}
    for name, (m, conn) in masks.items():  # the first call of each mask, reported as it ends
        first[name] = timed_events(torch, lambda: op.run_mask_components_device(m, W, counts, boxes, connectivity=conn), 1) / F
        comps[name] = int(counts[0].item()) & 0xFFFFFFFF
        print(f"# first call {name}: {first[name]:.3f} ms per frame, {comps[name]} components in frame 0", flush=True)
    for _ in range(args.reps):
        for name, (m, conn) in masks.items():
            ms[name].append(timed_events(
                torch, lambda: op.run_mask_components_device(m, W, counts, boxes, connectivity=conn), 1) / F)
    op.close()
    out = {"metric": "dips_mask_components on fabricated 4K masks (min_area 1, K 64, no labels), ms PER FRAME",
           "frames": F, "width": W, "height": H, "reps": args.reps,
           "timing": "device events around one call; masks alternated per repetition",
           "first_call_ms": {k: round(v, 4) for k, v in first.items()}, "components_frame0": comps}
    out.update(summary(ms))
    return out, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", choices=("clip", "fabricated"), default="clip")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--fab-frames", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back mask calls inside one timed window")
    ap.add_argument("--route-frames", type=int, default=32, help="frames leg 2 labels per repetition")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--parent-lib", default=None, help="libdips_hip.so of the parent commit for leg 1")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = True
    except Exception:
        have_scipy = False
    pool = None
    if args.legs == "clip" and have_scipy:
        # the workers before this process opens the GPU: they never touch it
        pool = multiprocessing.get_context("fork").Pool(args.workers)
    try:
        out, ok = clip_legs(args, pool, have_scipy) if args.legs == "clip" else fabricated_legs(args)
    finally:
        if pool is not None:
            pool.close()
            pool.join()
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
