#!/usr/bin/env python3
"""mask_stats_bench.py -- what the statistics of the packed change mask
(dips_mask_counts, dips_mask_pixel_times) cost beside the traffic floor, beside
the same results computed by torch on the same device and beside the fused
products that read the frames themselves.

Workload: the 'per-frame' change mask (tau = 8/255) of --frames 3840x2160 RGB8
synthetic frames, resident in HBM (500 frames: 518 MB of mask, 12.4 GB of
frames), and a random mask of density 0.5 of the same shape.  Every leg is
timed with device events around --inner back-to-back calls, the legs alternated
within each of --reps repetitions; ms PER CALL over the whole mask.

  1. copy        a plain device copy of the mask bytes (one read, one write).
     write4      a plain write of four u32 planes of the region (the times'
                 output, 16 B per pixel).
  2. counts      dips_mask_counts at the grids of --grids (1x1, 9x16, 135x240:
                 cells of the whole frame, 240 and 16 pixels wide).
     times, sums, times+sums   dips_mask_pixel_times with either output and
                 with both, each on the clip's mask and on the random mask.
  3. torch_*     the unpacked mask ([chunk, H, W] uint8 from the packed words):
                 counts by a reshaped sum per cell, sums by a sum over t, times
                 by where / min / max for first and last and a cummax fold for
                 the runs; in chunks of --chunk frames, state carried.
  4. fused_*     dips_diff_series_grid, dips_diff_pixel_sums and
                 dips_diff_pixel_times on the frames themselves, which read 24
                 times the bytes of the mask.  Legs 3 and 4 are left out with
                 --no-fused (comparing builds of the kernels).

Legs 3 and 4 are compared with leg 2 value for value on the clip's mask.
Prints one JSON line (and writes it to --out); exits 1 if a comparison fails.
--lib PATH runs another build of the library (a variant of the kernels).
Run on the GPU box:
    python tools/mask_stats_bench.py [--out profiles/mask_stats/NAME.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

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


def unpacked(torch, words, w, shifts):
    """words int32 [c, H, wpr] -> uint8 [c, H, w]."""
    c, h, wpr = words.shape
    return ((words[..., None] >> shifts) & 1).to(torch.uint8).reshape(c, h, wpr * 32)[..., :w]


def torch_counts(torch, words, w, rows, cols, chunk, shifts):
    f, h, _ = words.shape
    out = torch.empty((f, rows, cols), dtype=torch.int32, device=words.device)
    for s in range(0, f, chunk):
        b = unpacked(torch, words[s:s + chunk], w, shifts)
        out[s:s + chunk] = b.reshape(b.shape[0], rows, h // rows, cols, w // cols).sum(dim=(2, 4), dtype=torch.int32)
    return out


def torch_sums(torch, words, w, chunk, shifts):
    f, h, _ = words.shape
    out = torch.zeros((h, w), dtype=torch.int32, device=words.device)
    for s in range(0, f, chunk):
        out += unpacked(torch, words[s:s + chunk], w, shifts).sum(dim=0, dtype=torch.int32)
    return out


def torch_times(torch, words, w, chunk, shifts):
    """int64 [4, H, W]: first, last (0xFFFFFFFF: none), run_max, run_cur."""
    f, h, _ = words.shape
    dev = words.device
    none = 0xFFFFFFFF
    first = torch.full((h, w), none, dtype=torch.int64, device=dev)
    last = torch.full((h, w), -1, dtype=torch.int64, device=dev)
    rmax = torch.zeros((h, w), dtype=torch.int32, device=dev)
    rcur = torch.zeros((h, w), dtype=torch.int32, device=dev)
    for s in range(0, f, chunk):
        b = unpacked(torch, words[s:s + chunk], w, shifts) != 0
        c = b.shape[0]
        g = torch.arange(s, s + c, dtype=torch.int64, device=dev)[:, None, None]
        first = torch.minimum(first, torch.where(b, g, none).amin(dim=0))
        last = torch.maximum(last, torch.where(b, g, -1).amax(dim=0))
        pos = torch.arange(1, c + 1, dtype=torch.int32, device=dev)[:, None, None]
        z = torch.where(b, 0, pos).cummax(dim=0).values   # the last clear frame so far, 1-based (0: none yet)
        run = pos - z + torch.where(z == 0, rcur, 0)       # a run that began before the chunk carries rcur
        rmax = torch.maximum(rmax, run.amax(dim=0))
        rcur = run[-1]
    last = torch.where(last < 0, none, last)
    return torch.stack([first, last, rmax.to(torch.int64), rcur.to(torch.int64)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--grids", default="1x1,9x16,135x240")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="back-to-back calls inside one pair of events")
    ap.add_argument("--chunk", type=int, default=10, help="frames per chunk of the torch legs")
    ap.add_argument("--no-fused", action="store_true", help="leave legs 3 and 4 out (comparing builds of the kernels)")
    ap.add_argument("--lib", default=None, help="another build of libdips_hip.so to run")
    ap.add_argument("--note", default=None, help="what this run compares (kept in the JSON line)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    import torch
    from dips_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes

    W, H, F = args.width, args.height, args.frames
    grids = [tuple(int(v) for v in g.split("x")) for g in args.grids.split(",")]
    dev = torch.device("cuda", 0)
    RB = mask_row_bytes(W)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    clip = torch.empty((F, H, RB), dtype=torch.uint8, device=dev)
    op.run_change_mask_device(frames, clip)
    torch.cuda.synchronize()
    full = not args.no_fused
    if not full:
        del frames
        torch.cuda.empty_cache()
    gen = torch.Generator(device=dev).manual_seed(7)
    valid = torch.from_numpy(np.packbits(np.arange(RB * 8) < W, bitorder="little")).to(dev)
    masks = {"clip": clip,
             "random_05": torch.randint(0, 256, clip.shape, dtype=torch.uint8, device=dev, generator=gen) & valid}
    copy_out = torch.empty_like(clip)
    times = torch.empty((4, H, W), dtype=torch.int32, device=dev)
    sums = torch.empty((H, W), dtype=torch.int32, device=dev)
    counts = {g: torch.empty((F, g[0], g[1]), dtype=torch.int32, device=dev) for g in grids}
    clip_words = clip.view(torch.int32)
    shifts = torch.arange(32, device=dev, dtype=torch.int32)

    legs = {"copy": lambda: copy_out.copy_(clip), "write4": lambda: times.fill_(1)}
    for name, msk in masks.items():
        for g in grids:
            legs[f"counts_{g[0]}x{g[1]}/{name}"] = lambda msk=msk, g=g: op.run_mask_counts_device(msk, W, counts[g], *g)
        legs[f"times/{name}"] = lambda msk=msk: op.run_mask_times_device(msk, W, times, None)
        legs[f"sums/{name}"] = lambda msk=msk: op.run_mask_times_device(msk, W, None, sums)
        legs[f"times+sums/{name}"] = lambda msk=msk: op.run_mask_times_device(msk, W, times, sums)
    agree = {}
    if full:
        divisible = [g for g in grids if H % g[0] == 0 and W % g[1] == 0]
        for g in divisible:
            legs[f"torch_counts_{g[0]}x{g[1]}"] = lambda g=g: torch_counts(torch, clip_words, W, g[0], g[1], args.chunk, shifts)
        legs["torch_sums"] = lambda: torch_sums(torch, clip_words, W, args.chunk, shifts)
        legs["torch_times"] = lambda: torch_times(torch, clip_words, W, args.chunk, shifts)
        cells = {g: torch.empty((F, g[0], g[1], 4), dtype=torch.int64, device=dev) for g in grids}
        psums = torch.empty((H, W, 4), dtype=torch.int64, device=dev)
        ptimes = torch.empty((4, H, W), dtype=torch.int32, device=dev)
        for g in grids:
            legs[f"fused_grid_{g[0]}x{g[1]}"] = lambda g=g: op.run_grid_device(frames, cells[g], *g)
        legs["fused_pixel_sums"] = lambda: op.run_pixel_sums_device(frames, psums)
        legs["fused_pixel_times"] = lambda: op.run_pixel_times_device(frames, ptimes)

        # the comparisons, value for value on the clip's mask (they warm every leg's shapes up too)
        op.run_mask_times_device(clip, W, times, sums)
        op.run_pixel_sums_device(frames, psums)
        op.run_pixel_times_device(frames, ptimes)
        agree["fused_pixel_times"] = bool(torch.equal(times, ptimes))
        agree["fused_pixel_sums"] = bool(torch.equal(sums.to(torch.int64), psums[..., 2]))
        agree["torch_sums"] = bool(torch.equal(torch_sums(torch, clip_words, W, args.chunk, shifts), sums))
        agree["torch_times"] = bool(torch.equal(torch_times(torch, clip_words, W, args.chunk, shifts),
                                                times.to(torch.int64) & 0xFFFFFFFF))
        for g in grids:
            op.run_mask_counts_device(clip, W, counts[g], *g)
            op.run_grid_device(frames, cells[g], *g)
            agree[f"fused_grid_{g[0]}x{g[1]}"] = bool(torch.equal(counts[g].to(torch.int64), cells[g][..., 2]))
            if g in divisible:
                agree[f"torch_counts_{g[0]}x{g[1]}"] = bool(torch.equal(
                    torch_counts(torch, clip_words, W, g[0], g[1], args.chunk, shifts), counts[g]))
        op.run_mask_times_device(clip, W, None, sums)
        clip_share = round(float(sums.sum().item()) / (F * H * W), 5)
        agree["the_mask_is_not_empty"] = clip_share > 0.0
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()

    ms = {name: [] for name in legs}
    for _ in range(args.reps):  # alternated: every repetition runs every leg once
        for name, fn in legs.items():
            ms[name].append(timed_events(torch, fn, args.inner))

    mask_bytes = clip.numel()
    res = {"metric": "statistics of the 4K per-frame change mask vs a device copy, a write of four planes, torch and the "
                     "fused products on the frames, ms PER CALL over all frames",
           "frames": F, "width": W, "height": H, "mask_bytes": mask_bytes, "frame_bytes": F * H * W * 3,
           "reps": args.reps, "inner": args.inner, "chunk": args.chunk, "lib": args.lib or "this build",
           "note": args.note,
           "cu_count": torch.cuda.get_device_properties(0).multi_processor_count,
           "timing": "device events around `inner` back-to-back calls on one stream, divided by `inner`; legs alternated "
                     "per repetition"}
    res.update(summary(ms))
    med = res["median_ms"]
    res["agree"] = agree
    res["mask_set_share"] = {"clip": clip_share, "random_05": 0.5} if full else None
    res["ratio_to_copy"] = {k: round(v / med["copy"], 3) for k, v in med.items() if "/" in k}
    res["ratio_times_to_write4"] = {n: round(med[f"times/{n}"] / med["write4"], 2) for n in masks}
    res["GBps_of_mask_read"] = {k: round(mask_bytes / v / 1e6, 0) for k, v in med.items() if "/" in k}
    if full:
        res["ratio_torch_to_ours"] = {
            "sums": round(med["torch_sums"] / med["sums/clip"], 1), "times": round(med["torch_times"] / med["times/clip"], 1),
            **{f"counts_{g[0]}x{g[1]}": round(med[f"torch_counts_{g[0]}x{g[1]}"] / med[f"counts_{g[0]}x{g[1]}/clip"], 1)
               for g in grids if f"torch_counts_{g[0]}x{g[1]}" in med}}
        res["ratio_fused_to_ours"] = {
            "pixel_sums": round(med["fused_pixel_sums"] / med["sums/clip"], 2),
            "pixel_times": round(med["fused_pixel_times"] / med["times/clip"], 2),
            **{f"grid_{g[0]}x{g[1]}": round(med[f"fused_grid_{g[0]}x{g[1]}"] / med[f"counts_{g[0]}x{g[1]}/clip"], 2)
               for g in grids}}
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
