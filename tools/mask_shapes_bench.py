#!/usr/bin/env python3
"""mask_shapes_bench.py -- what the shape records of the components of the
packed change mask (dips_mask_shapes) cost beside the traffic floor, beside the
labelling they sit behind and beside today's route to a part of them through
the label image.

Workload: the 'per-frame' change mask (tau = 8/255) of --frames 3840x2160 RGB8
synthetic frames (500 frames: 518 MB of mask) and a random mask of density 0.5
of the same shape, both resident in HBM; K = 64 records per frame,
connectivity 8; the weights are a random u8 plane per frame.  Every leg is
timed with device events around --inner back-to-back calls, the legs
alternated within each of --reps repetitions; ms PER CALL over the whole mask.
Per mask:

  a. copy        a plain device copy of the mask bytes: the floor.
  b. components  dips_mask_components with K records and no labels: what the
                 shapes call contains before its own launch.
  c. shapes      dips_mask_shapes without weights.
  d. shapes_w    dips_mask_shapes with weights.
  e. via_labels  today's route: dips_mask_components with labels (4 bytes per
                 pixel), then torch nonzero and bincount per frame and label for
                 the area, SX, SXX, SXY and WSUM only, in chunks of --chunk frames.
                 No perimeter, no Euler number, no SY, SYY, WMAX: it does less
                 than (c), which makes the comparison conservative.
and once: contention, one all-ones frame (every wave adds to one record).

(c) and (d) are compared with (e) on those fields and with each other on the
rest, on all frames; counts and boxes of (c) with (b)'s.  Prints one JSON line
(and writes it to --out); exits 1 if a comparison fails or (c) is not faster
than (e).
Run on the GPU box:
    python tools/mask_shapes_bench.py [--out profiles/mask_shapes/NAME.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--max-boxes", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=1, help="back-to-back calls inside one pair of events")
    ap.add_argument("--chunk", type=int, default=10, help="frames per chunk of the torch sums")
    ap.add_argument("--masks", default="clip,random_05")
    ap.add_argument("--progress", action="store_true", help="say on stderr what is being run")
    ap.add_argument("--note", default=None, help="what this run compares (kept in the JSON line)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    started = time.monotonic()

    sys.path.insert(0, ROOT)
    import torch

    def progress(what):
        if args.progress:
            torch.cuda.synchronize()
            print(f"[{time.monotonic() - started:7.1f} s] {what}", file=sys.stderr, flush=True)
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, _lib, mask_row_bytes

    W, H, F, K = args.width, args.height, args.frames, args.max_boxes
    dev = torch.device("cuda", 0)
    RB = mask_row_bytes(W)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    masks = {}
    if "clip" in args.masks.split(","):
        frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        op.synth_device(frames, W, H, 0xD1B5, 0)
        masks["clip"] = torch.empty((F, H, RB), dtype=torch.uint8, device=dev)
        op.run_change_mask_device(frames, masks["clip"])
        torch.cuda.synchronize()
        del frames
        torch.cuda.empty_cache()
    if "random_05" in args.masks.split(","):
        gen = torch.Generator(device=dev).manual_seed(7)
        masks["random_05"] = torch.randint(0, 256, (F, H, RB), dtype=torch.uint8, device=dev, generator=gen)
    gen = torch.Generator(device=dev).manual_seed(11)
    weights = torch.randint(0, 256, (F, H, W), dtype=torch.uint8, device=dev, generator=gen)

    progress("masks and weights made")

    def outputs():
        return (torch.empty((F,), dtype=torch.int32, device=dev),
                torch.empty((F, K, _lib.BOX_WORDS), dtype=torch.int32, device=dev),
                torch.empty((F, K, _lib.SHAPE_WORDS), dtype=torch.int32, device=dev))

    out = torch.empty((F, H, RB), dtype=torch.uint8, device=dev)
    counts_b, boxes_b, _ = outputs()
    counts_c, boxes_c, shapes_c = outputs()
    counts_d, boxes_d, shapes_d = outputs()
    labels = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    sums_e = torch.empty((5, F, K + 1), dtype=torch.int64, device=dev)  # area, SX, SXX, SXY, WSUM by label; 0: none
    assert H * W * max(W, H) ** 2 < 1 << 53, "leg (e) sums in float64"

    def via_labels(msk):
        op.run_mask_components_device(msk, W, counts_b, boxes_b, labels)
        for s in range(0, F, args.chunk):
            lab = labels[s:s + args.chunk]
            n = lab.shape[0]
            t, y, x = torch.nonzero((lab > 0) & (lab <= K), as_tuple=True)  # the pixels of the records
            idx = lab[t, y, x].to(torch.int64) + (K + 1) * t
            wts = weights[s:s + n][t, y, x]
            # float64 weights: every sum stays below 2^53 at this size, so they are exact
            for k, v in enumerate((None, x, x * x, x * y, wts)):
                sums_e[k, s:s + n] = torch.bincount(idx, None if v is None else v.to(torch.float64),
                                                    minlength=n * (K + 1)).view(n, K + 1).to(torch.int64)

    def u64(shapes, f):
        lo = shapes[..., f].to(torch.int64) & 0xFFFFFFFF
        return lo | (shapes[..., f + 1].to(torch.int64) << 32)

    off = _lib.SHAPE_OFFSETS
    legs, agree = {}, {}
    for name, msk in masks.items():
        legs[f"copy/{name}"] = lambda msk=msk: out.copy_(msk)
        legs[f"components/{name}"] = lambda msk=msk: op.run_mask_components_device(msk, W, counts_b, boxes_b)
        legs[f"shapes/{name}"] = lambda msk=msk: op.run_mask_shapes_device(msk, W, counts_c, boxes_c, shapes_c)
        legs[f"shapes_w/{name}"] = lambda msk=msk: op.run_mask_shapes_device(msk, W, counts_d, boxes_d, shapes_d, weights)
        legs[f"via_labels/{name}"] = lambda msk=msk: via_labels(msk)

        # the comparisons, on all frames (they warm every leg up too)
        for leg in ("shapes", "shapes_w", "via_labels"):
            legs[f"{leg}/{name}"]()
            progress(f"first {leg}/{name}")
        valid = torch.arange(K, device=dev).view(1, K) < counts_c.view(F, 1)
        agree[f"counts_boxes==components/{name}"] = bool(
            torch.equal(counts_c, counts_b) and torch.equal(boxes_c, boxes_b) and torch.equal(counts_d, counts_b)
            and torch.equal(boxes_d, boxes_b) and bool(valid.any()))
        want = sums_e[:, :, 1:] * valid  # label k + 1 is record k
        area = boxes_c[..., _lib.BOX_FIELDS.index("area")].to(torch.int64)
        agree[f"shapes==via_labels/{name}"] = bool(
            torch.equal(area, want[0]) and torch.equal(u64(shapes_c, off["sx"]), want[1])
            and torch.equal(u64(shapes_c, off["sxx"]), want[2]) and torch.equal(u64(shapes_c, off["sxy"]), want[3]))
        agree[f"shapes_w==via_labels/{name}"] = bool(torch.equal(u64(shapes_d, off["wsum"]), want[4]))
        rest = [i for i in range(_lib.SHAPE_WORDS) if i not in (off["wsum"], off["wsum"] + 1, off["wmax"])]
        agree[f"shapes_w==shapes_but_weights/{name}"] = bool(
            torch.equal(shapes_c[..., rest], shapes_d[..., rest]) and not shapes_c[..., off["wsum"]:off["wmax"] + 1].any()
            and bool((shapes_d[..., off["wmax"]] <= 255).all()))
        agree[f"zero_past_counts/{name}"] = bool(not (shapes_d * ~valid.view(F, K, 1)).any())
        progress(f"compared {name}")

    ones = torch.full((1, H, RB), 0xFF, dtype=torch.uint8, device=dev)
    legs["components/all_ones"] = lambda: op.run_mask_components_device(ones, W, counts_b[:1], boxes_b[:1])
    legs["contention/all_ones"] = lambda: op.run_mask_shapes_device(ones, W, counts_d[:1], boxes_d[:1], shapes_d[:1],
                                                                    weights[:1])
    legs["contention/all_ones"]()
    agree["contention_is_one_record"] = bool(
        int(counts_d[0].item()) == 1 and int(u64(shapes_d[0, 0], off["sx"]).item()) == H * (W * (W - 1) // 2)
        and int(u64(shapes_d[0, 0], off["wsum"]).item()) == int(weights[0].sum(dtype=torch.int64).item())
        and shapes_d[0, 0, off["cracks_v"]:].tolist() == [2 * H, 2 * W, 1])
    for name, fn in legs.items():  # the legs the comparisons have not run yet
        if name.split("/")[0] in ("copy", "components"):
            fn()
    torch.cuda.synchronize()

    ms = {name: [] for name in legs}
    for rep in range(args.reps):  # alternated: every repetition runs every leg once
        for name, fn in legs.items():
            ms[name].append(timed_events(torch, fn, args.inner))
        progress(f"repetition {rep + 1} of {args.reps}")

    res = {"metric": "shape records of the components of the 4K change mask vs a device copy, the components call alone "
                     "and the route through the label image, ms PER CALL over all frames",
           "frames": F, "width": W, "height": H, "mask_bytes": F * H * RB, "max_boxes": K, "connectivity": 8,
           "reps": args.reps, "inner": args.inner, "chunk": args.chunk, "note": args.note,
           "cu_count": torch.cuda.get_device_properties(0).multi_processor_count,
           "timing": "device events around `inner` back-to-back calls on one stream, divided by `inner`; legs alternated "
                     "per repetition"}
    res.update(summary(ms))
    med, span = res["median_ms"], res["min_max_ms"]
    res["agree"] = agree
    res["ratio"] = {}
    for name in masks:
        b = med[f"components/{name}"]
        res["ratio"][name] = {
            "shapes/components": round(med[f"shapes/{name}"] / b, 3),
            "shapes_w/components": round(med[f"shapes_w/{name}"] / b, 3),
            "via_labels/shapes": round(med[f"via_labels/{name}"] / med[f"shapes/{name}"], 2),
            "components_spread": round((span[f"components/{name}"][1] - span[f"components/{name}"][0]) / b, 3)}
        agree[f"shapes_faster_than_via_labels/{name}"] = max(ms[f"shapes/{name}"]) < min(ms[f"via_labels/{name}"])
    res["ratio"]["all_ones"] = {"contention/components": round(med["contention/all_ones"] / med["components/all_ones"], 3)}
    op.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(agree.values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
