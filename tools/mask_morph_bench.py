#!/usr/bin/env python3
"""mask_morph_bench.py -- what the binary morphology of the change mask
(dips_mask_morph) costs beside the stage before it, beside the traffic floor
and beside the two other routes to the same bits.

Workload (--legs clip): 3840x2160 RGB8 synthetic frames resident in HBM,
'per-frame' mode, tau = 8/255, and their change mask.  Every operation (erode,
dilate, open, close) at box 1x1, box 15x15 and diamond 15.  Legs alternated
within every repetition, ms PER FRAME:

  1. mask          dips_diff_change_mask on the clip: the stage before.
  2. copy          a plain device copy of the mask bytes: one read plus one
                   write, the traffic floor.
  3. morph         dips_mask_morph on the resident mask, device events.
  4. torch         the same operation in torch on the unpacked mask of the
                   first --route-frames frames (max_pool2d and its negation on
                   a float16 image; the diamond as rounds of the 3x1 / 1x3
                   cross), same GPU, device events; the unpacking and packing
                   a caller would also need are left out, in torch's favour.
  5. scipy         the mask of those frames copied to the host (part of the
                   route), scipy.ndimage binary_erosion / binary_dilation with
                   the border values of the definition in a pool of --workers
                   processes started before the GPU is opened; wall clock, once
                   per configuration.  Absent where scipy is not installed.
  6. change_boxes  DiffSeriesOperator.change_boxes end to end without and with
                   morph=[(Open, Box, 1, 1)], wall clock, and the components
                   call alone on the raw and on the opened mask, device events.

Legs 4 and 5 are compared with leg 3 bit for bit on the frames they ran.

--legs fabricated: leg 3 alone on fabricated 4K masks of --fab-frames frames
-- random at densities 0.05 and 0.5, all ones -- and on the clip's mask,
because the claim is that the time does not depend on the bits.

Prints one JSON line (and writes it to --out); exits 1 if a comparison fails.
Run on the GPU box:
    python tools/mask_morph_bench.py --legs clip [--out profiles/mask_morph/NAME.json]
"""
from __future__ import annotations

import argparse
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

from mask_components_bench import summary, timed_events  # noqa: E402  (the timing conventions)

OPS = ("erode", "dilate", "open", "close")
CONFIGS = {"box1": (0, 1, 1), "box15": (0, 15, 15), "diamond15": (1, 15, 15)}  # shape, rx, ry


def scipy_frame(job):
    """One frame of leg 5 in a worker: the packed rows of the result."""
    from scipy import ndimage as ndi
    mask_bytes, w, op, shape, rx, ry = job
    bits = np.unpackbits(mask_bytes, axis=-1, bitorder="little")[:, :w].astype(bool)
    if shape == 0:
        st = np.ones((2 * ry + 1, 2 * rx + 1), dtype=bool)
    else:
        yy, xx = np.mgrid[-rx:rx + 1, -rx:rx + 1]
        st = np.abs(yy) + np.abs(xx) <= rx

    def dil(x):
        return ndi.binary_dilation(x, structure=st, border_value=0)

    def ero(x):
        return ndi.binary_erosion(x, structure=st, border_value=1)

    out = {0: lambda: ero(bits), 1: lambda: dil(bits), 2: lambda: dil(ero(bits)), 3: lambda: ero(dil(bits))}[op]()
    full = np.zeros((bits.shape[0], mask_bytes.shape[1] * 8), dtype=bool)
    full[:, :w] = out
    return np.packbits(full, axis=-1, bitorder="little")


def torch_morph(torch, x, op, shape, rx, ry):
    """x float16 [n, 1, h, w] of 0 / 1 -> the same, by max_pool2d."""
    F = torch.nn.functional

    def dil(y):
        if shape == 0:
            return F.max_pool2d(y, (2 * ry + 1, 2 * rx + 1), stride=1, padding=(ry, rx))
        for _ in range(rx):
            y = torch.maximum(F.max_pool2d(y, (3, 1), stride=1, padding=(1, 0)),
                              F.max_pool2d(y, (1, 3), stride=1, padding=(0, 1)))
        return y

    def ero(y):
        return 1 - dil(1 - y)

    return {0: lambda: ero(x), 1: lambda: dil(x), 2: lambda: dil(ero(x)), 3: lambda: ero(dil(x))}[op]()


def unpack_device(torch, mask, w):
    """uint8 [n, h, row_bytes] -> bool [n, h, w] on the device."""
    shifts = torch.arange(8, device=mask.device, dtype=torch.int32)
    bits = (mask[..., None].to(torch.int32) >> shifts) & 1
    return bits.reshape(mask.shape[0], mask.shape[1], -1)[..., :w].bool()


def clip_legs(args, pool, have_scipy):
    import torch
    from dips_amd import DiffSeriesOperator, Mode, MorphOp, MorphShape, PixelFormat, mask_row_bytes

    W, H, F = args.width, args.height, args.frames
    dev = torch.device("cuda", 0)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    torch.cuda.synchronize()
    RB = mask_row_bytes(W)
    mask = torch.full((F, H, RB), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.empty_like(mask)
    op.run_change_mask_device(frames, mask)
    R = min(args.route_frames, F)
    K = 64
    counts = torch.zeros((F,), dtype=torch.int32, device=dev)
    boxes = torch.zeros((F, K, 8), dtype=torch.int32, device=dev)
    opened = torch.empty_like(mask)
    op.run_mask_morph_device(mask, W, opened, MorphOp.Open, 1)
    image = unpack_device(torch, mask[:R], W).to(torch.float16)[:, None]

    def leg_morph(o, cfg, dst=out):
        shape, rx, ry = CONFIGS[cfg]
        op.run_mask_morph_device(mask, W, dst, o, rx, ry, shape)

    event_legs = {"mask": (lambda: op.run_change_mask_device(frames, mask), F),
                  "copy": (lambda: out.copy_(mask), F)}
    for o, name in enumerate(OPS):
        for cfg in CONFIGS:
            event_legs[f"morph_{name}_{cfg}"] = (lambda o=o, cfg=cfg: leg_morph(o, cfg), F)
            event_legs[f"torch_{name}_{cfg}"] = (lambda o=o, cfg=cfg: torch_morph(torch, image, o, *CONFIGS[cfg]), R)
    event_legs["components_raw"] = (lambda: op.run_mask_components_device(mask, W, counts, boxes, min_area=1), F)
    event_legs["components_opened"] = (lambda: op.run_mask_components_device(opened, W, counts, boxes, min_area=1), F)
    steps = [(MorphOp.Open, MorphShape.Box, 1, 1)]
    wall_legs = {"change_boxes": (lambda: op.change_boxes(frames, min_area=1, max_boxes=K), F),
                 "change_boxes_open1": (lambda: op.change_boxes(frames, min_area=1, max_boxes=K, morph=steps), F)}

    for fn, _ in list(event_legs.values()) + list(wall_legs.values()):
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in list(event_legs) + list(wall_legs)}
    for _ in range(args.reps):  # alternated: every repetition runs every leg once
        for name, (fn, per) in event_legs.items():
            ms[name].append(timed_events(torch, fn, 1) / per)
        for name, (fn, per) in wall_legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / per)

    res = {"metric": "binary morphology of the change mask vs the mask stage, a device copy, torch max_pool2d and "
                     "scipy.ndimage in a process pool, 4K RGB8 per-frame tau=8/255, ms PER FRAME",
           "frames": F, "width": W, "height": H, "reps": args.reps, "route_frames": R, "workers": args.workers,
           "timing": "mask, copy, morph_*, torch_*, components_*: device events around one call on one stream; "
                     "change_boxes*, scipy_*: wall clock around the call; all divided by the frames of the call; legs "
                     "alternated per repetition, scipy once per configuration",
           "scipy": have_scipy}
    res.update(summary(ms))
    res["mask_set_share"] = round(float(unpack_device(torch, mask[:R], W).float().mean().item()), 5)
    op.run_mask_components_device(mask, W, counts, boxes, min_area=1)
    raw_counts = counts.cpu().numpy().view(np.uint32).copy()
    op.run_mask_components_device(opened, W, counts, boxes, min_area=1)
    res["components_per_frame_median"] = {"raw": float(np.median(raw_counts)),
                                          "opened": float(np.median(counts.cpu().numpy().view(np.uint32)))}

    # the comparisons, bit for bit on the first R frames
    agree, scipy_ms = {}, {}
    valid = torch.from_numpy(np.packbits(np.arange(RB * 8) < W, bitorder="little")).to(dev)
    for o, name in enumerate(OPS):
        for cfg, (shape, rx, ry) in CONFIGS.items():
            leg_morph(o, cfg)
            ours = out[:R].clone()
            got = torch_morph(torch, image, o, shape, rx, ry)[:, 0] > 0.5
            agree[f"torch_{name}_{cfg}"] = bool(torch.equal(unpack_device(torch, ours, W), got))
            agree[f"pad_zero_{name}_{cfg}"] = bool(((ours & ~valid) == 0).all().item())
            if have_scipy and cfg in args.scipy_configs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = mask[:R].cpu().numpy()  # the copy is part of the route
                want = pool.map(scipy_frame, [(host[t], W, o, shape, rx, ry) for t in range(R)])
                scipy_ms[f"scipy_{name}_{cfg}"] = round((time.perf_counter() - t0) * 1e3 / R, 3)
                agree[f"scipy_{name}_{cfg}"] = bool(np.array_equal(np.stack(want), ours.cpu().numpy()))
    res["scipy_ms"] = scipy_ms
    res["agree"] = agree
    med = res["median_ms"]
    res["ratio_morph_to_copy"] = {k[6:]: round(med[k] / med["copy"], 2) for k in med if k.startswith("morph_")}
    res["ratio_torch_to_morph"] = {k[6:]: round(med["torch_" + k[6:]] / med[k], 1) for k in med if k.startswith("morph_")}
    res["ratio_scipy_to_morph"] = {k[6:]: round(v / med["morph_" + k[6:]], 0) for k, v in scipy_ms.items()}
    op.close()
    return res, all(agree.values())


def fabricated_legs(args):
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes

    W, H, F = args.width, args.height, args.fab_frames
    dev = torch.device("cuda", 0)
    RB = mask_row_bytes(W)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    gen = torch.Generator(device=dev).manual_seed(7)
    weights = (1 << torch.arange(8, device=dev, dtype=torch.int32))

    def random_mask(p):
        rnd = torch.rand((F, H, RB * 8), device=dev, generator=gen) < p
        return (rnd.reshape(F, H, RB, 8).to(torch.int32) * weights).sum(dim=-1).to(torch.uint8)

    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    clip = torch.empty((F, H, RB), dtype=torch.uint8, device=dev)
    op.run_change_mask_device(frames, clip)
    del frames
    masks = {"clip": clip, "random_005": random_mask(0.05), "random_05": random_mask(0.5),
             "all_ones": torch.full((F, H, RB), 0xFF, dtype=torch.uint8, device=dev)}
    out = torch.empty_like(clip)
    legs = {}
    for o, name in enumerate(OPS):
        for cfg, (shape, rx, ry) in CONFIGS.items():
            for mname, m in masks.items():
                legs[f"{name}_{cfg}/{mname}"] = lambda m=m, o=o, shape=shape, rx=rx, ry=ry: \
                    op.run_mask_morph_device(m, W, out, o, rx, ry, shape)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            ms[k].append(timed_events(torch, fn, 1) / F)
    op.close()
    res = {"metric": "dips_mask_morph on fabricated 4K masks and on the clip's mask, ms PER FRAME",
           "frames": F, "width": W, "height": H, "reps": args.reps,
           "timing": "device events around one call; legs alternated per repetition"}
    res.update(summary(ms))
    med = res["median_ms"]
    spread = {}
    for name in OPS:
        for cfg in CONFIGS:
            v = [med[f"{name}_{cfg}/{m}"] for m in masks]
            spread[f"{name}_{cfg}"] = round(max(v) / min(v), 3)
    res["max_over_min_across_masks"] = spread
    return res, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", choices=("clip", "fabricated"), default="clip")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--fab-frames", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route-frames", type=int, default=16, help="frames legs 4 and 5 run")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--scipy-configs", default="box1,box15,diamond15",
                    help="the configurations leg 5 runs (comma separated; empty: none)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    args.scipy_configs = [c for c in args.scipy_configs.split(",") if c]

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
        res, ok = clip_legs(args, pool, have_scipy) if args.legs == "clip" else fabricated_legs(args)
    finally:
        if pool is not None:
            pool.close()
            pool.join()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
