#!/usr/bin/env python3
"""mask_bench.py -- what the per-frame change mask (dips_diff_change_mask)
costs beside the whole-frame series and beside the only route to per-frame,
per-pixel decisions that existed before it.

Workload: 3840x2160 RGB8 synthetic frames resident in HBM, 'per-frame' mode,
tau = 8/255.  Legs alternated within every repetition, each timed by device
events on one stream around --inner back-to-back calls:

  1. series        dips_diff_series -- the one-pass cost.  With --parent-lib it
                   is called in the library of the parent commit (a second
                   libdips_hip.so loaded beside this build's), otherwise in
                   this build's (the whole-frame kernels are the same code).
  2. sums_per_frame  one dips_diff_pixel_sums call per frame (n_frames = 1,
                   ref = the previous frame) and its count field: 32 B written
                   per pixel and frame.  Timed over --route-frames frames per
                   window, reported per frame.
  3. mask          dips_diff_change_mask over the whole frame; also over a
                   1920x1080 region at an odd x (mask_roi).  Reported per
                   call and per frame.
  NAME=PATH ...    the mask leg again in variant libraries built with another
                   DIPS_UNROLL_MASK (the vecs-per-lane comparison):
    make -C dips_amd/csrc HIPFLAGS="<the Makefile's HIPFLAGS> -DDIPS_UNROLL_MASK=U" \
         OUTDIR=$PWD/build/mask_uU OBJDIR=$PWD/build/obj_mask_uU BIN=$PWD/build/obj_mask_uU/dips_raw

Prints one JSON line (and writes it to --out); exits 1 unless the mask is
faster per frame than leg 2, its bits equal leg 2's counts and its per-frame
popcounts leg 1's count.  Run on the GPU box:
    python tools/mask_bench.py [u2=PATH ...] [--parent-lib PATH] [--out profiles/mask/NAME.json]
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


class VariantMask:
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="*", help="NAME=PATH of a variant libdips_hip.so (another DIPS_UNROLL_MASK)")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back calls inside one timed window")
    ap.add_argument("--route-frames", type=int, default=20, help="frames of leg 2 inside one timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libdips_hip.so of the parent commit for leg 1")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    import numpy as np
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes
    from dips_amd.api import _params
    from dips_amd import _lib
    from grid_bench import ParentSeries

    W, H, F = args.width, args.height, args.frames
    K = min(args.route_frames, F - 1)
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
    sums = torch.full((K, H, W, 4), -1, dtype=torch.int64, device=dev)  # frames 1 .. K
    mask = torch.full((F, H, mask_row_bytes(W)), 0xFF, dtype=torch.uint8, device=dev)
    mask_roi = torch.full((F, roi[3], mask_row_bytes(roi[2])), 0xFF, dtype=torch.uint8, device=dev)
    parent = ParentSeries(os.path.abspath(args.parent_lib), params, stream) if args.parent_lib else None
    variants, vmasks = {}, {}
    for v in args.variants:
        name, path = v.split("=", 1)
        variants["mask_" + name] = VariantMask(os.path.abspath(path), params, stream)
        vmasks["mask_" + name] = torch.full_like(mask, 0xFF)

    def leg_series():
        if parent is not None:
            parent.run(frames, series)
        else:
            op.run_device(frames, series)

    def leg_route():
        for t in range(1, K + 1):
            op.run_pixel_sums_device(frames[t:t + 1], sums[t - 1], ref=frames[t - 1])

    legs = {"series": leg_series, "sums_per_frame": leg_route,
            "mask": lambda: op.run_change_mask_device(frames, mask),
            "mask_roi": lambda: op.run_change_mask_device(frames, mask_roi, roi=roi)}
    for name, lb in variants.items():
        legs[name] = (lambda lb=lb, name=name: lb.run(frames, vmasks[name]))
    frames_of = {k: (K if k == "sums_per_frame" else F) for k in legs}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():  # alternated: every repetition runs every leg once
            inner = 1 if name == "sums_per_frame" else args.inner
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / inner)

    batch_bytes = F * W * H * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    per_frame = {k: [x / frames_of[k] for x in v] for k, v in ms.items()}
    out = {
        "metric": "per-frame change mask vs whole-frame series vs one pixel-sums call per frame, 4K RGB8 per-frame "
                  "tau=8/255",
        "frames": F, "width": W, "height": H, "roi": list(roi), "reps": args.reps, "inner": args.inner,
        "route_frames": K, "warmup": args.warmup,
        "timing": "device events around `inner` back-to-back calls on one stream (ms per call; sums_per_frame: one "
                  "window of route_frames calls), legs alternated per repetition",
        "leg1_library": "parent commit" if args.parent_lib else "this build",
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        "median_us_per_frame": {k: round(1e3 * statistics.median(v), 3) for k, v in per_frame.items()},
        "min_max_us_per_frame": {k: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in per_frame.items()},
        "batch_read_frac_of_8tbs": {k: round(batch_bytes / (v / 1e3) / 1e9 / HBM_PEAK_GBS, 4)
                                    for k, v in med.items() if k != "sums_per_frame"},
    }

    def unpack(m, w):  # uint8 [..., h, row_bytes] -> bool [..., h, w] on the device
        sh = torch.arange(8, dtype=torch.uint8, device=dev)
        b = (m.unsqueeze(-1) >> sh) & 1
        return b.reshape(*m.shape[:-1], m.shape[-1] * 8)[..., :w].bool()

    s = series.cpu().numpy().view(np.uint64)
    pop = torch.stack([unpack(mask[t], W).sum() for t in range(F)]).cpu().numpy().astype(np.uint64)
    x, y, w, h = roi
    agree = {
        "mask_bits_equal_sums_per_frame_counts": all(
            bool(torch.equal(unpack(mask[t], W), sums[t - 1, :, :, 2] != 0)) and int(sums[t - 1, :, :, 2].max()) <= 1
            for t in range(1, K + 1)),
        "mask_popcounts_equal_series_count": bool(np.array_equal(pop, s[:, 2])),
        "roi_equals_crop": all(bool(torch.equal(unpack(mask_roi[t], w), unpack(mask[t], W)[y:y + h, x:x + w]))
                               for t in range(0, F, max(1, F // 16))),
        "pad_bits_zero": bool((unpack(mask_roi, 8 * mask_roi.shape[-1])[..., w:] == 0).all()),
        "variants_equal": all(bool(torch.equal(vm, mask)) for vm in vmasks.values()),
    }
    out.update({
        "ratio_mask_to_series": round(med["mask"] / med["series"], 4),
        "ratio_mask_to_series_min_max": [round(min(ms["mask"]) / max(ms["series"]), 4),
                                         round(max(ms["mask"]) / min(ms["series"]), 4)],
        "ratio_mask_roi_to_series": round(med["mask_roi"] / med["series"], 4),
        "ratio_sums_per_frame_to_mask_per_frame": round(statistics.median(per_frame["sums_per_frame"])
                                                        / statistics.median(per_frame["mask"]), 2),
        "mask_faster_per_frame_than_sums_per_frame": bool(max(per_frame["mask"]) < min(per_frame["sums_per_frame"])),
        "changed_share": round(float(pop[1:].sum()) / float((F - 1) * W * H), 4),
        "agree": agree,
    })
    ok = all(agree.values()) and out["mask_faster_per_frame_than_sums_per_frame"]
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
