#!/usr/bin/env python3
"""pixel_sums_bench.py -- what the per-pixel sums over time
(dips_diff_pixel_sums) cost beside the whole-frame series and beside the only
route to a per-pixel answer that existed before them.

Workload: 3840x2160 RGB8 synthetic frames resident in HBM, 'per-frame' mode,
tau = 8/255.  Legs alternated within every repetition, each timed by device
events on one stream around --inner back-to-back calls:

  1. series      dips_diff_series -- the one-pass cost.  With --parent-lib it
                 is called in the library of the parent commit (a second
                 libdips_hip.so loaded beside this build's), otherwise in
                 this build's (the whole-frame kernels are the same code).
  2. map_sum     dips_diff_series with the abs-diff map, then a torch sum of
                 the map over t: reads the batch, writes it once more and
                 reads that again, and yields the SAD per byte only.
  3. pixel_sums  dips_diff_pixel_sums over the whole frame; also over a
                 1920x1080 region at an odd x (pixel_sums_roi).

Prints one JSON line (and writes it to --out).  Run on the GPU box:
    python tools/pixel_sums_bench.py [--parent-lib PATH] [--out profiles/pixel_sums/NAME.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back calls inside one timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libdips_hip.so of the parent commit for leg 1")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    import numpy as np
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat
    from dips_amd.api import _params
    from dips_amd import _lib
    from grid_bench import ParentSeries

    W, H, F = args.width, args.height, args.frames
    tau = 8 / 255
    roi = (W // 4 + 1, H // 4, W // 2, H // 2)  # 1920x1080 at x = 961 for the 4K default
    dev = torch.device("cuda", 0)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    dmap = torch.empty_like(frames)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, tau)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    series = torch.zeros((F, 4), dtype=torch.int64, device=dev)
    series2 = torch.zeros((F, 4), dtype=torch.int64, device=dev)
    sums = torch.full((H, W, 4), -1, dtype=torch.int64, device=dev)
    sums_roi = torch.full((roi[3], roi[2], 4), -1, dtype=torch.int64, device=dev)
    parent = None
    if args.parent_lib:
        parent = ParentSeries(os.path.abspath(args.parent_lib),
                              _params(fmt=PixelFormat.RGB8, mode=Mode.PerFrame, tau=tau, flags=_lib.FLAG_DEVICE_PTRS),
                              stream)
    byte_sad = [None]

    def leg_series():
        if parent is not None:
            parent.run(frames, series)
        else:
            op.run_device(frames, series)

    def leg_map_sum():
        op.run_device(frames, series2, map_out=dmap)
        byte_sad[0] = dmap.sum(dim=0, dtype=torch.int64)

    legs = {"series": leg_series, "map_sum": leg_map_sum,
            "pixel_sums": lambda: op.run_pixel_sums_device(frames, sums),
            "pixel_sums_roi": lambda: op.run_pixel_sums_device(frames, sums_roi, roi=roi)}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():  # alternated: every repetition runs every leg once
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.inner)

    batch_bytes = F * W * H * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {
        "metric": "per-pixel sums over time vs whole-frame series vs map + sum over t, 4K RGB8 per-frame tau=8/255",
        "frames": F, "width": W, "height": H, "roi": list(roi), "reps": args.reps, "inner": args.inner,
        "warmup": args.warmup,
        "timing": "device events around `inner` back-to-back calls on one stream (ms per call), legs alternated "
                  "per repetition",
        "leg1_library": "parent commit" if args.parent_lib else "this build",
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        "batch_read_gbs": {k: round(batch_bytes / (v / 1e3) / 1e9, 1) for k, v in med.items()},
        "batch_read_frac_of_8tbs": {k: round(batch_bytes / (v / 1e3) / 1e9 / HBM_PEAK_GBS, 4) for k, v in med.items()},
    }
    # the legs agree: pixels sum to the series summed over t, leg 2's SAD is leg 3's SAD, the region is a crop
    s = series.cpu().numpy().view(np.uint64)
    p = sums.cpu().numpy().view(np.uint64)
    pr = sums_roi.cpu().numpy().view(np.uint64)
    x, y, w, h = roi
    agree = {
        "pixel_sums_sum_to_series": bool(np.array_equal(p.sum(axis=(0, 1), dtype=np.uint64),
                                                        s.sum(axis=0, dtype=np.uint64))),
        "map_sum_sad_equals_pixel_sums_sad": bool(np.array_equal(
            byte_sad[0].sum(dim=2).cpu().numpy().view(np.uint64), p[..., 0])),
        "map_leg_series_equals_series": bool(np.array_equal(series2.cpu().numpy().view(np.uint64), s)),
        "roi_equals_crop": bool(np.array_equal(pr, p[y:y + h, x:x + w])),
    }
    out.update({
        "ratio_pixel_sums_to_series": round(med["pixel_sums"] / med["series"], 4),
        "ratio_pixel_sums_roi_to_series": round(med["pixel_sums_roi"] / med["series"], 4),
        "ratio_map_sum_to_pixel_sums": round(med["map_sum"] / med["pixel_sums"], 4),
        "pixel_sums_faster_than_map_sum": bool(max(ms["pixel_sums"]) < min(ms["map_sum"])),
        "agree": agree,
    })
    ok = all(agree.values()) and out["pixel_sums_faster_than_map_sum"]
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
