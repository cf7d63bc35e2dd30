#!/usr/bin/env python3
"""pixel_times_bench.py -- what the change times per pixel
(dips_diff_pixel_times) cost beside the whole-frame series and beside the only
route to a motion-history image that existed before them.

Workload: 3840x2160 RGB8 synthetic frames resident in HBM, 'per-frame' mode,
tau = 8/255.  Legs alternated within every repetition, each timed by device
events on one stream around --inner back-to-back calls:

  1. series        dips_diff_series -- the one-pass cost.  With --parent-lib it
                   is called in the library of the parent commit (a second
                   libdips_hip.so loaded beside this build's), otherwise in
                   this build's (the whole-frame kernels are the same code).
  2. mask_route_*  today's route to the `last` plane alone:
                   dips_diff_change_mask on the device, then torch operations
                   on the device mask.  Two formulations, both timed (one call
                   per window), the faster one is the yardstick:
                     amax    frames in chunks of --route-chunk: unpack the
                             chunk's bits, multiply by the 1-based frame
                             index, amax over the chunk, running maximum;
                     argmax  per bit position of the mask bytes: (mask >> b)
                             & 1 over all frames, argmax over the reversed
                             time axis, amax for "ever set".
                   mask is the dips_diff_change_mask call alone.
  3. times         dips_diff_pixel_times over the whole frame; also over a
                   1920x1080 region at an odd x (times_roi).
  NAME=PATH ...    the times leg again in variant libraries built with another
                   DIPS_UNROLL_TIMES (the vecs-per-lane comparison):
    make -C dips_amd/csrc HIPFLAGS="<the Makefile's HIPFLAGS> -DDIPS_UNROLL_TIMES=U" \
         OUTDIR=$PWD/build/times_uU OBJDIR=$PWD/build/obj_times_uU BIN=$PWD/build/obj_times_uU/dips_raw

Prints one JSON line (and writes it to --out); exits 1 unless leg 3 is faster
than the faster formulation of leg 2, its `last` plane equals leg 2's and its
whole-frame planes cropped equal the region's.  Run on the GPU box:
    python tools/pixel_times_bench.py [u1=PATH ...] [--parent-lib PATH] [--out profiles/pixel_times/NAME.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK_GBS = 8000.0
NONE = 0xFFFFFFFF


class VariantTimes:
    """dips_diff_pixel_times of another libdips_hip.so (device pointers, the caller's stream)."""

    def __init__(self, path, params, stream):
        from dips_amd._lib import DipsParams
        self.lib = ctypes.CDLL(path)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        self.lib.dips_create.argtypes = [ctypes.POINTER(DipsParams), ctypes.c_int, ctypes.POINTER(vp)]
        self.lib.dips_set_stream.argtypes = [vp, vp]
        self.lib.dips_diff_pixel_times.argtypes = [vp, u32, u32, vp, u32, vp, vp, u32, u32, vp]
        self.lib.dips_destroy.argtypes = [vp]
        self.lib.dips_destroy.restype = None
        self.h = vp()
        assert self.lib.dips_create(ctypes.byref(params), 0, ctypes.byref(self.h)) == 0
        assert self.lib.dips_set_stream(self.h, vp(stream)) == 0

    def run(self, frames, times):
        n, h, w = frames.shape[:3]
        st = self.lib.dips_diff_pixel_times(self.h, w, h, frames.data_ptr(), n, None, None, 0, 0, times.data_ptr())
        assert st == 0, st

    def close(self):
        self.lib.dips_set_stream(self.h, None)
        self.lib.dips_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="*", help="NAME=PATH of a variant libdips_hip.so (another DIPS_UNROLL_TIMES)")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back calls inside one timed window")
    ap.add_argument("--route-chunk", type=int, default=20, help="frames per chunk of leg 2's amax formulation")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libdips_hip.so of the parent commit for leg 1")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes
    from dips_amd.api import _params
    from dips_amd import _lib
    from grid_bench import ParentSeries

    W, H, F = args.width, args.height, args.frames
    tau = 8 / 255
    roi = (W // 4 + 1, H // 4, W // 2, H // 2)  # 1920x1080 at x = 961 for the 4K default
    dev = torch.device("cuda", 0)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, tau)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    params = _params(fmt=PixelFormat.RGB8, mode=Mode.PerFrame, tau=tau, flags=_lib.FLAG_DEVICE_PTRS)
    series = torch.zeros((F, 4), dtype=torch.int64, device=dev)
    RB = mask_row_bytes(W)
    mask = torch.full((F, H, RB), 0xFF, dtype=torch.uint8, device=dev)
    times = torch.full((4, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    times_roi = torch.full((4, roi[3], roi[2]), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    parent = ParentSeries(os.path.abspath(args.parent_lib), params, stream) if args.parent_lib else None
    variants, vtimes = {}, {}
    for v in args.variants:
        name, path = v.split("=", 1)
        variants["times_" + name] = VariantTimes(os.path.abspath(path), params, stream)
        vtimes["times_" + name] = torch.full_like(times, 0x5A5A5A5A)

    sh = torch.arange(8, dtype=torch.uint8, device=dev)
    route_last = {}

    def route_amax():
        """`last` (int64 [H, W], NONE where never set) from the device mask, frames in chunks."""
        op.run_change_mask_device(frames, mask)
        best = torch.zeros((H, W), dtype=torch.int32, device=dev)  # 1-based index of the last set frame
        for c0 in range(0, F, args.route_chunk):
            m = mask[c0:c0 + args.route_chunk]
            bits = ((m.unsqueeze(-1) >> sh) & 1).reshape(m.shape[0], H, RB * 8)[..., :W]
            idx = torch.arange(c0 + 1, c0 + m.shape[0] + 1, dtype=torch.int32, device=dev)
            best = torch.maximum(best, (bits.to(torch.int32) * idx[:, None, None]).amax(dim=0))
        route_last["amax"] = torch.where(best > 0, best.to(torch.int64) - 1, torch.full_like(best, NONE, dtype=torch.int64))

    def route_argmax():
        """The same per bit position of the mask bytes, over all frames at once."""
        op.run_change_mask_device(frames, mask)
        out = torch.empty((H, RB, 8), dtype=torch.int64, device=dev)
        for b in range(8):
            x = (mask >> b) & 1
            last = (F - 1) - torch.argmax(x.flip(0), dim=0)
            out[:, :, b] = torch.where(x.amax(dim=0) > 0, last, torch.full_like(last, NONE))
        route_last["argmax"] = out.reshape(H, RB * 8)[:, :W]

    def leg_series():
        if parent is not None:
            parent.run(frames, series)
        else:
            op.run_device(frames, series)

    legs = {"series": leg_series, "mask_route_amax": route_amax, "mask_route_argmax": route_argmax,
            "mask": lambda: op.run_change_mask_device(frames, mask),
            "times": lambda: op.run_pixel_times_device(frames, times),
            "times_roi": lambda: op.run_pixel_times_device(frames, times_roi, roi=roi)}
    for name, lb in variants.items():
        legs[name] = (lambda lb=lb, name=name: lb.run(frames, vtimes[name]))
    routes = ("mask_route_amax", "mask_route_argmax")
    for i in range(args.warmup):
        for name, fn in legs.items():
            if name in routes and i > 0:
                continue  # the routes take seconds: one warm-up call each
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():  # alternated: every repetition runs every leg once
            inner = 1 if name in routes else args.inner
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / inner)

    batch_bytes = F * W * H * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    best_route = min(routes, key=lambda k: med[k])
    out = {
        "metric": "change times per pixel vs whole-frame series vs change mask + torch fold to the last plane, 4K RGB8 "
                  "per-frame tau=8/255",
        "frames": F, "width": W, "height": H, "roi": list(roi), "reps": args.reps, "inner": args.inner,
        "route_chunk": args.route_chunk, "warmup": args.warmup,
        "timing": "device events around `inner` back-to-back calls on one stream (ms per call; the mask routes: one "
                  "call per window), legs alternated per repetition",
        "leg1_library": "parent commit" if args.parent_lib else "this build",
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        "batch_read_frac_of_8tbs": {k: round(batch_bytes / (v / 1e3) / 1e9 / HBM_PEAK_GBS, 4)
                                    for k, v in med.items() if k not in routes and k != "times_roi"},
        "fastest_route": best_route,
    }
    torch.cuda.synchronize()
    t64 = times.to(torch.int64) & NONE
    x, y, w, h = roi
    agree = {
        "last_equals_route_amax": bool(torch.equal(t64[1], route_last["amax"])),
        "last_equals_route_argmax": bool(torch.equal(t64[1], route_last["argmax"])),
        "roi_equals_crop": bool(torch.equal(times_roi, times[:, y:y + h, x:x + w])),
        "planes_consistent": bool(((t64[0] == NONE) == (t64[1] == NONE)).all() and (t64[3] <= t64[2]).all()
                                  and (t64[0] <= t64[1]).all() and (t64[2] <= F).all()),
        "variants_equal": all(bool(torch.equal(vt, times)) for vt in vtimes.values()),
    }
    changed = t64[0] != NONE
    out.update({
        "ratio_times_to_series": round(med["times"] / med["series"], 4),
        "ratio_times_to_series_min_max": [round(min(ms["times"]) / max(ms["series"]), 4),
                                          round(max(ms["times"]) / min(ms["series"]), 4)],
        "ratio_times_to_mask": round(med["times"] / med["mask"], 4),
        "ratio_times_roi_to_series": round(med["times_roi"] / med["series"], 4),
        "ratio_fastest_route_to_times": round(med[best_route] / med["times"], 2),
        "times_faster_than_fastest_route": bool(max(ms["times"]) < min(min(ms[r]) for r in routes)),
        "never_changed_share": round(1.0 - float(changed.float().mean()), 4),
        "max_run_max": int(t64[2].max()),
        "agree": agree,
    })
    ok = all(agree.values()) and out["times_faster_than_fastest_route"]
    if parent is not None:
        parent.close()
    for lb in variants.values():
        lb.close()
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
