#!/usr/bin/env python3
"""background_bench.py -- what the running-average background and its change
mask (dips_diff_background_mask) cost beside the plain change mask and beside
the only route to an adaptive reference that existed before it.

Workload: 3840x2160 RGB8 synthetic frames resident in HBM, tau = 8/255,
rate_shift 3.  Legs alternated within every repetition, each timed by device
events on one stream around --inner back-to-back calls:

  1. mask          dips_diff_change_mask ('per-frame') -- the fixed-reference
                   cost.  With --parent-lib it is called in the library of the
                   parent commit (a second libdips_hip.so loaded beside this
                   build's), otherwise in this build's (the same code).
  2. route         per frame one dips_diff_change_mask call (n_frames = 1, ref
                   = the background's bytes) and the same integer update of the
                   background in torch on the device.  Timed over
                   --route-frames frames per window, reported per frame.
  3. background    dips_diff_background_mask over the whole frame, selective
                   off and on (background_selective), and over a 1920x1080
                   region at an odd x (background_roi).  Per call and per frame.

Prints one JSON line (and writes it to --out); exits 1 unless leg 3 is faster
per frame than leg 2 in every repetition, its bits and state equal leg 2's on
the frames leg 2 ran and the region equals the crop.  leg 3 / leg 1 is
reported without a pass mark.  Run on the GPU box:
    python tools/background_bench.py [--parent-lib PATH] [--out profiles/background/NAME.json]
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
    ap.add_argument("--rate-shift", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="back-to-back calls inside one timed window")
    ap.add_argument("--route-frames", type=int, default=20, help="frames of leg 2 inside one timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="libdips_hip.so of the parent commit for leg 1")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes
    from dips_amd.api import _params
    from dips_amd import _lib
    from mask_bench import VariantMask

    W, H, F, k = args.width, args.height, args.frames, args.rate_shift
    K = min(args.route_frames, F)
    tau = 8 / 255
    roi = (W // 4 + 1, H // 4, W // 2, H // 2)  # 1920x1080 at x = 961 for the 4K default
    dev = torch.device("cuda", 0)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, tau)
    # the route's per-frame mask calls are 'overall' against the background's bytes
    op_overall = DiffSeriesOperator(PixelFormat.RGB8, Mode.Overall, tau)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    params = _params(fmt=PixelFormat.RGB8, mode=Mode.PerFrame, tau=tau, flags=_lib.FLAG_DEVICE_PTRS)
    rb = mask_row_bytes(W)
    mask1 = torch.full((F, H, rb), 0xFF, dtype=torch.uint8, device=dev)
    mask2 = torch.full((K, H, rb), 0xFF, dtype=torch.uint8, device=dev)
    mask3 = torch.full((F, H, rb), 0xFF, dtype=torch.uint8, device=dev)
    mask3_roi = torch.full((F, roi[3], mask_row_bytes(roi[2])), 0xFF, dtype=torch.uint8, device=dev)
    bg3 = torch.full((3, H, W), -1, dtype=torch.int16, device=dev)
    bg3_sel = torch.full((3, H, W), -1, dtype=torch.int16, device=dev)
    bg3_roi = torch.full((3, roi[3], roi[2]), -1, dtype=torch.int16, device=dev)
    route_state = {}
    parent = VariantMask(os.path.abspath(args.parent_lib), params, stream) if args.parent_lib else None

    def leg_mask():
        if parent is not None:
            parent.run(frames, mask1)
        else:
            op.run_change_mask_device(frames, mask1)

    def leg_route():
        B = frames[0].to(torch.int32) << 8
        half = (1 << k) >> 1
        for t in range(K):
            R = ((B + 128) >> 8).to(torch.uint8)
            op_overall.run_change_mask_device(frames[t:t + 1], mask2[t:t + 1], ref=R)
            B = B - ((B + half) >> k) + (frames[t].to(torch.int32) << (8 - k))
        route_state["B"] = B

    legs = {
        "mask": leg_mask,
        "route": leg_route,
        "background": lambda: op.run_background_mask_device(frames, bg3, mask3, rate_shift=k),
        "background_selective": lambda: op.run_background_mask_device(frames, bg3_sel, mask3, rate_shift=k, selective=True),
        "background_roi": lambda: op.run_background_mask_device(frames, bg3_roi, mask3_roi, roi=roi, rate_shift=k),
    }
    frames_of = {name: (K if name == "route" else F) for name in legs}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():  # alternated: every repetition runs every leg once
            inner = 1 if name == "route" else args.inner
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / inner)

    # agreement: the background leg on the frames the route ran, and the region against the crop
    op.run_background_mask_device(frames, bg3, mask3, rate_shift=k)
    op.run_background_mask_device(frames, bg3_roi, mask3_roi, roi=roi, rate_shift=k)
    maskK = torch.full((K, H, rb), 0xFF, dtype=torch.uint8, device=dev)
    bgK = torch.full((3, H, W), -1, dtype=torch.int16, device=dev)
    op.run_background_mask_device(frames[:K], bgK, maskK, rate_shift=k)
    torch.cuda.synchronize()

    def unpack(m, w):  # uint8 [..., h, row_bytes] -> bool [..., h, w] on the device
        sh = torch.arange(8, dtype=torch.uint8, device=dev)
        b = (m.unsqueeze(-1) >> sh) & 1
        return b.reshape(*m.shape[:-1], m.shape[-1] * 8)[..., :w].bool()

    x, y, w, h = roi
    B = route_state["B"].permute(2, 0, 1)
    agree = {
        "bits_equal_route": bool(torch.equal(maskK, mask2)),
        "state_equal_route": bool(torch.equal(bgK.to(torch.int32) & 0xFFFF, B)),
        "prefix_of_whole_clip": bool(torch.equal(mask3[:K], maskK)),
        "roi_mask_equals_crop": all(bool(torch.equal(unpack(mask3_roi[t], w), unpack(mask3[t], W)[y:y + h, x:x + w]))
                                    for t in range(0, F, max(1, F // 16))),
        "roi_state_equals_crop": bool(torch.equal(bg3_roi, bg3[:, y:y + h, x:x + w])),
        "pad_bits_zero": bool((unpack(mask3_roi, 8 * mask3_roi.shape[-1])[..., w:] == 0).all()),
    }
    pop = sum(int(unpack(mask3[t], W).sum()) for t in range(1, F, max(1, F // 16)))
    share = pop / float(len(range(1, F, max(1, F // 16))) * W * H)

    batch_bytes = F * W * H * 3
    med = {name: statistics.median(v) for name, v in ms.items()}
    per_frame = {name: [v_ / frames_of[name] for v_ in v] for name, v in ms.items()}
    faster = all(b < r for b, r in zip(per_frame["background"], per_frame["route"])) and \
        max(per_frame["background"]) < min(per_frame["route"])
    out = {
        "metric": "running-average background + mask vs the plain change mask vs one mask call and a torch update per "
                  "frame, 4K RGB8 tau=8/255",
        "frames": F, "width": W, "height": H, "roi": list(roi), "rate_shift": k, "reps": args.reps, "inner": args.inner,
        "route_frames": K, "warmup": args.warmup,
        "timing": "device events around `inner` back-to-back calls on one stream (ms per call; route: one window of "
                  "route_frames frames), legs alternated per repetition",
        "leg1_library": "parent commit" if args.parent_lib else "this build",
        "ms": {name: [round(v_, 3) for v_ in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 3) for name, v in med.items()},
        "min_max_ms": {name: [round(min(v), 3), round(max(v), 3)] for name, v in ms.items()},
        "median_us_per_frame": {name: round(1e3 * statistics.median(v), 3) for name, v in per_frame.items()},
        "min_max_us_per_frame": {name: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for name, v in per_frame.items()},
        "batch_read_frac_of_8tbs": {name: round(batch_bytes / (v / 1e3) / 1e9 / HBM_PEAK_GBS, 4)
                                    for name, v in med.items() if name not in ("route", "background_roi")},
        "ratio_background_to_mask": round(med["background"] / med["mask"], 4),
        "ratio_background_to_mask_min_max": [round(min(ms["background"]) / max(ms["mask"]), 4),
                                             round(max(ms["background"]) / min(ms["mask"]), 4)],
        "ratio_background_selective_to_mask": round(med["background_selective"] / med["mask"], 4),
        "ratio_route_to_background_per_frame": round(statistics.median(per_frame["route"])
                                                     / statistics.median(per_frame["background"]), 2),
        "background_faster_per_frame_than_route_in_every_rep": bool(faster),
        "changed_share_sampled": round(share, 4),
        "agree": agree,
    }
    ok = all(agree.values()) and faster
    if parent is not None:
        parent.close()
    op.close()
    op_overall.close()
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
