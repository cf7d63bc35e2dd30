#!/usr/bin/env python3
"""grid_bench.py -- what the grid form of the series (dips_diff_series_grid)
costs beside the whole-frame series and beside the only route to a per-cell
answer that existed before it.

Workload: 3840x2160 RGB8 synthetic frames resident in HBM, 'per-frame' mode,
tau = 8/255.  Three legs, alternated within every repetition, each timed by
device events on one stream around --inner back-to-back calls (series kernel +
reduce each):

  1. series      dips_diff_series -- the one-pass cost.  With --parent-lib it
                 is called in the library of the parent commit (a second
                 libdips_hip.so loaded beside this build's), otherwise in
                 this build's (the whole-frame kernels are the same code).
  2. map_reduce  dips_diff_series with the abs-diff map, then a torch
                 reduction of the map to the 16x9 cells: reads the batch,
                 writes it once more and reads that again (>= 3x the bytes),
                 and yields the SAD per cell only.
  3. grid        dips_diff_series_grid 16x9; also 1x1 and 64x36.

Prints one JSON line (and writes it to --out).  Run on the GPU box:
    python tools/grid_bench.py [--parent-lib PATH] [--out profiles/grid/NAME.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0


class ParentSeries:
    """dips_diff_series of another libdips_hip.so (device pointers, the
    caller's stream): the four entry points it needs, bound by hand."""

    def __init__(self, path, params, stream):
        from dips_amd._lib import DipsParams
        self.lib = ctypes.CDLL(path)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        self.lib.dips_create.argtypes = [ctypes.POINTER(DipsParams), ctypes.c_int, ctypes.POINTER(vp)]
        self.lib.dips_set_stream.argtypes = [vp, vp]
        self.lib.dips_diff_series.argtypes = [vp, u32, u32, vp, u32, vp, vp, vp]
        self.lib.dips_destroy.argtypes = [vp]
        self.lib.dips_destroy.restype = None
        self.lib.dips_last_error.argtypes = [vp]
        self.lib.dips_last_error.restype = ctypes.c_char_p
        self.h = vp()
        self._check(self.lib.dips_create(ctypes.byref(params), 0, ctypes.byref(self.h)))
        self._check(self.lib.dips_set_stream(self.h, vp(stream)))

    def _check(self, st):
        if st < 0:
            raise RuntimeError(f"parent library status {st}: {self.lib.dips_last_error(self.h)}")

    def run(self, frames, series):
        n, h, w = frames.shape[:3]
        self._check(self.lib.dips_diff_series(self.h, w, h, frames.data_ptr(), n, None, series.data_ptr(), None))

    def close(self):
        self._check(self.lib.dips_set_stream(self.h, None))
        self.lib.dips_destroy(self.h)


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

    W, H, F = args.width, args.height, args.frames
    tau = 8 / 255
    rows, cols = 9, 16
    if H % rows or W % cols:
        raise SystemExit("leg 2 reshapes the map: height and width must be multiples of 9 and 16")
    dev = torch.device("cuda", 0)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    dmap = torch.empty_like(frames)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, tau)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    series = torch.zeros((F, 4), dtype=torch.int64, device=dev)
    series2 = torch.zeros((F, 4), dtype=torch.int64, device=dev)
    grids = {(r, c): torch.zeros((F, r, c, 4), dtype=torch.int64, device=dev) for r, c in ((9, 16), (1, 1), (36, 64))}
    parent = None
    if args.parent_lib:
        parent = ParentSeries(os.path.abspath(args.parent_lib),
                              _params(fmt=PixelFormat.RGB8, mode=Mode.PerFrame, tau=tau, flags=_lib.FLAG_DEVICE_PTRS),
                              stream)
    cell_sad = [None]

    def leg_series():
        if parent is not None:
            parent.run(frames, series)
        else:
            op.run_device(frames, series)

    def leg_map_reduce():
        op.run_device(frames, series2, map_out=dmap)
        cell_sad[0] = dmap.view(F, rows, H // rows, cols, W // cols, 3).sum(dim=(2, 4, 5), dtype=torch.int64)

    legs = {"series": leg_series, "map_reduce": leg_map_reduce,
            "grid_16x9": lambda: op.run_grid_device(frames, grids[9, 16], 9, 16),
            "grid_1x1": lambda: op.run_grid_device(frames, grids[1, 1], 1, 1),
            "grid_64x36": lambda: op.run_grid_device(frames, grids[36, 64], 36, 64)}
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

    # the legs agree: cells sum to the series, leg 2's SAD is the grid's SAD
    s = series.cpu().numpy()
    g = grids[9, 16].cpu().numpy()
    agree = {
        "grid_16x9_sums_to_series": bool(np.array_equal(g.sum(axis=(1, 2)), s)),
        "grid_64x36_sums_to_series": bool(np.array_equal(grids[36, 64].cpu().numpy().sum(axis=(1, 2)), s)),
        "grid_1x1_equals_series": bool(np.array_equal(grids[1, 1].cpu().numpy()[:, 0, 0], s)),
        "map_reduce_sad_equals_grid_sad": bool(np.array_equal(cell_sad[0].cpu().numpy(), g[..., 0])),
        "map_leg_series_equals_series": bool(np.array_equal(series2.cpu().numpy(), s)),
    }
    if parent is not None:
        parent.close()
    op.close()

    batch_bytes = F * W * H * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {
        "metric": "grid series vs whole-frame series vs map + reduce, 4K RGB8 per-frame tau=8/255",
        "frames": F, "width": W, "height": H, "reps": args.reps, "inner": args.inner, "warmup": args.warmup,
        "timing": "device events around `inner` back-to-back calls on one stream (ms per call), legs alternated "
                  "per repetition",
        "leg1_library": "parent commit" if args.parent_lib else "this build",
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "batch_read_gbs": {k: round(batch_bytes / (v / 1e3) / 1e9, 1) for k, v in med.items()},
        "batch_read_frac_of_8tbs": {k: round(batch_bytes / (v / 1e3) / 1e9 / HBM_PEAK_GBS, 4) for k, v in med.items()},
        "ratio_grid_16x9_to_series": round(med["grid_16x9"] / med["series"], 4),
        "ratio_grid_1x1_to_series": round(med["grid_1x1"] / med["series"], 4),
        "ratio_grid_64x36_to_series": round(med["grid_64x36"] / med["series"], 4),
        "ratio_map_reduce_to_grid_16x9": round(med["map_reduce"] / med["grid_16x9"], 4),
        "grid_faster_than_map_reduce": bool(max(ms["grid_16x9"]) < min(ms["map_reduce"])),
        "agree": agree,
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(agree.values()) or not out["grid_faster_than_map_reduce"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
