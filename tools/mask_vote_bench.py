#!/usr/bin/env python3
"""mask_vote_bench.py -- what the temporal m-of-k vote on the change mask
(dips_mask_vote) costs beside the traffic floor, beside the stage before it and
beside the same result computed by torch on the same device.

Workload: the 'per-frame' change mask (tau = 8/255) of --frames 3840x2160 RGB8
synthetic frames, resident in HBM (500 frames: 518 MB of mask).  Every event
leg is timed with device events around --inner back-to-back calls, the legs
alternated within each of --reps repetitions; ms PER CALL over the whole mask.

  1. copy          a plain device copy of the mask bytes: one read plus one
                   write, the traffic floor.
  2. mask          dips_diff_change_mask on the clip, the stage before the vote:
                   from this build and, with --parent-tree DIR, from the library
                   built in DIR, each in a process of its own that runs before
                   this one opens the GPU (same timing, not alternated with the
                   other legs).
  3. vote          dips_mask_vote at (k, m) = (3,2), (5,3), (31,1), (31,16),
                   (31,31) on the clip's mask, on an all-zero mask and on a
                   random mask of density 0.5 (the time must not depend on the
                   bits), no history, no history_out.
  4a. torch_packed the packed words as int32: the OR (m = 1) or the AND (m = k)
                   of the k time-shifted slices, by doubling (5 passes at k =
                   31 instead of 30).  Covers (31,1) and (31,31) only.
  4b. torch_general  unpack to uint8, cumsum over t in int16, difference of the
                   sums k apart, compare, repack; in chunks of --chunk frames.

Legs 4a and 4b are compared with leg 3 bit for bit on the whole mask.  The
share of priming reads comes from the schedule itself (series_sched.h
vote_geometry compiled with g++, the wave slots from the device's CU count and
the kernel's 8 waves per SIMD).

Prints one JSON line (and writes it to --out); exits 1 if a comparison fails or
leg 3 is not faster than leg 4.
Run on the GPU box:
    python tools/mask_vote_bench.py [--parent-tree DIR] [--out profiles/mask_vote/NAME.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ((3, 2), (5, 3), (31, 1), (31, 16), (31, 31))
VOTE_WAVES_PER_SIMD = 8  # mask_vote_kernel's occupancy (__launch_bounds__(256, 8))


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


def mask_stage(args):
    """--legs mask: dips_diff_change_mask of the package in --tree, alone."""
    sys.path.insert(0, args.tree)
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes
    W, H, F = args.width, args.height, args.frames
    dev = torch.device("cuda", 0)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    mask = torch.empty((F, H, mask_row_bytes(W)), dtype=torch.uint8, device=dev)
    op.run_change_mask_device(frames, mask)
    torch.cuda.synchronize()
    ms = {"mask": [timed_events(torch, lambda: op.run_change_mask_device(frames, mask), args.inner)
                   for _ in range(args.reps)]}
    op.close()
    print(json.dumps(summary(ms)), flush=True)


def mask_stage_of(tree, args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--legs", "mask", "--tree", tree, "--frames",
                        str(args.frames), "--width", str(args.width), "--height", str(args.height), "--reps",
                        str(args.reps), "--inner", str(args.inner)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"mask stage of {tree} failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def schedule(frame_words, n, cu_count):
    """parts, part_frames per (k, m) from series_sched.h itself."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pathlib

    import _vote_ref as vref
    csrc = os.path.join(ROOT, "dips_amd", "csrc")
    words = vref.words_per_lane(csrc)
    resident = VOTE_WAVES_PER_SIMD * 4 * cu_count
    with tempfile.TemporaryDirectory() as d:
        exe = vref.build_geometry(pathlib.Path(d), csrc)
        rows = vref.geometry(exe, [(frame_words, n, k, words, resident) for k, _ in PAIRS])
    return words, resident, {f"{k},{m}": q for (k, m), q in zip(PAIRS, rows)}


def torch_packed(torch, words, k, take_or):
    """words int32 [F, n]: the OR / AND over t - k + 1 .. t, clear before the clip, by doubling."""
    F = words.shape[0]
    acc, span = words, 1  # acc[t] covers frames t - span + 1 .. t

    def shifted(x, s):  # x[t - s], clear frames (which an AND must see as clear) before the clip
        return torch.cat([torch.zeros_like(x[:min(s, F)]), x[:F - min(s, F)]])

    while 2 * span <= k:
        sh = shifted(acc, span)
        acc = (acc | sh) if take_or else (acc & sh)
        span *= 2
    if span < k:
        sh = shifted(acc, k - span)
        acc = (acc | sh) if take_or else (acc & sh)
    return acc


def torch_general(torch, words, k, m, chunk):
    """words int32 [F, n]: unpack, windowed sum over t by cumsum, compare, repack."""
    F, n = words.shape
    shifts = torch.arange(32, device=words.device, dtype=torch.int32)
    weights = torch.tensor([1 << i for i in range(31)] + [-(1 << 31)], dtype=torch.int32, device=words.device)
    out = torch.empty_like(words)
    for s in range(0, F, chunk):
        e = min(F, s + chunk)
        lo = max(0, s - (k - 1))
        bits = ((words[lo:e, :, None] >> shifts) & 1).to(torch.uint8).reshape(e - lo, n * 32)
        if s - (k - 1) < 0:  # clear frames before the clip
            bits = torch.cat([torch.zeros((k - 1 - s, n * 32), dtype=torch.uint8, device=words.device), bits])
        cs = torch.cumsum(bits, dim=0, dtype=torch.int16)
        count = cs[k - 1:].clone()
        count[1:] -= cs[:e - s - 1]
        voted = (count >= m).reshape(e - s, n, 32).to(torch.int32)
        out[s:e] = (voted * weights).sum(dim=-1, dtype=torch.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", choices=("all", "mask", "vote"), default="all",
                    help="vote: legs 1 and 3 on the clip's mask alone (comparing builds of the kernel)")
    ap.add_argument("--tree", default=ROOT, help="--legs mask: the tree whose package and library run")
    ap.add_argument("--parent-tree", default=None, help="a built tree of the parent commit, for leg 2")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back calls inside one pair of events")
    ap.add_argument("--chunk", type=int, default=50, help="frames per chunk of leg 4b")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    if args.legs == "mask":
        return mask_stage(args)

    # leg 2 first: each in its own process, before this one opens the GPU
    only_vote = args.legs == "vote"
    stage = {} if only_vote else {"this": mask_stage_of(ROOT, args)}
    if args.parent_tree and not only_vote:
        stage["parent"] = mask_stage_of(os.path.abspath(args.parent_tree), args)

    sys.path.insert(0, ROOT)
    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes

    W, H, F = args.width, args.height, args.frames
    dev = torch.device("cuda", 0)
    RB = mask_row_bytes(W)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, 8 / 255)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    clip = torch.empty((F, H, RB), dtype=torch.uint8, device=dev)
    op.run_change_mask_device(frames, clip)
    torch.cuda.synchronize()
    del frames
    torch.cuda.empty_cache()
    gen = torch.Generator(device=dev).manual_seed(7)
    valid = torch.from_numpy(np.packbits(np.arange(RB * 8) < W, bitorder="little")).to(dev)
    masks = {"clip": clip}
    if not only_vote:
        masks.update({"zeros": torch.zeros_like(clip),
                      "random_05": torch.randint(0, 256, clip.shape, dtype=torch.uint8, device=dev, generator=gen) & valid})
    out = torch.empty_like(clip)
    clip_words = clip.view(torch.int32).reshape(F, -1)

    legs = {"copy": lambda: out.copy_(clip)}
    for k, m in PAIRS:
        for name, msk in masks.items():
            legs[f"vote_{k}_{m}/{name}"] = lambda msk=msk, k=k, m=m: op.run_mask_vote_device(msk, W, out, k, m)
        if only_vote:
            continue
        legs[f"torch_general_{k}_{m}"] = lambda k=k, m=m: torch_general(torch, clip_words, k, m, args.chunk)
        if m in (1, k):
            legs[f"torch_packed_{k}_{m}"] = lambda k=k, m=m: torch_packed(torch, clip_words, k, m == 1)

    # the comparisons, bit for bit on the whole mask (they warm every leg's shapes up too)
    agree = {}
    for k, m in () if only_vote else PAIRS:
        op.run_mask_vote_device(clip, W, out, k, m)
        ours = out.view(torch.int32).reshape(F, -1).clone()
        agree[f"torch_general_{k}_{m}"] = bool(torch.equal(torch_general(torch, clip_words, k, m, args.chunk), ours))
        if m in (1, k):
            agree[f"torch_packed_{k}_{m}"] = bool(torch.equal(torch_packed(torch, clip_words, k, m == 1), ours))
        agree[f"not_the_input_{k}_{m}"] = not bool(torch.equal(ours, clip_words))
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()

    ms = {name: [] for name in legs}
    for _ in range(args.reps):  # alternated: every repetition runs every leg once
        for name, fn in legs.items():
            ms[name].append(timed_events(torch, fn, args.inner))

    mask_bytes = clip.numel()
    cu_count = torch.cuda.get_device_properties(0).multi_processor_count
    words, resident, sched = schedule(RB // 4 * H, F, cu_count)
    res = {"metric": "temporal m-of-k vote on the 4K per-frame change mask vs a device copy, the mask stage and torch, "
                     "ms PER CALL over all frames",
           "frames": F, "width": W, "height": H, "mask_bytes": mask_bytes, "reps": args.reps, "inner": args.inner,
           "chunk": args.chunk, "words_per_lane": words, "cu_count": cu_count, "resident_waves": resident,
           "timing": "device events around `inner` back-to-back calls on one stream, divided by `inner`; legs alternated "
                     "per repetition; mask_stage: the same events in a process of its own per library, run first"}
    res.update(summary(ms))
    res["mask_stage"] = stage
    res["mask_set_share"] = round(float((((clip_words[:, :, None] >> torch.arange(32, device=dev, dtype=torch.int32)) & 1)
                                         .float().mean()).item()), 5)
    med = res["median_ms"]
    res["agree"] = agree
    if only_vote:
        res["ratio_vote_to_copy"] = {f"{k},{m}": round(med[f"vote_{k}_{m}/clip"] / med["copy"], 2) for k, m in PAIRS}
        print(json.dumps(res), flush=True)
        op.close()
        return
    res["ratio_vote_to_copy"] = {f"{k},{m}": round(med[f"vote_{k}_{m}/clip"] / med["copy"], 2) for k, m in PAIRS}
    res["ratio_vote_to_mask_stage"] = {who: {f"{k},{m}": round(med[f"vote_{k}_{m}/clip"] / s["median_ms"]["mask"], 3)
                                             for k, m in PAIRS} for who, s in stage.items()}
    res["ratio_torch_general_to_vote"] = {f"{k},{m}": round(med[f"torch_general_{k}_{m}"] / med[f"vote_{k}_{m}/clip"], 1)
                                          for k, m in PAIRS}
    res["ratio_torch_packed_to_vote"] = {f"{k},{m}": round(med[f"torch_packed_{k}_{m}"] / med[f"vote_{k}_{m}/clip"], 1)
                                         for k, m in PAIRS if m in (1, k)}
    res["max_over_min_across_masks"] = {
        f"{k},{m}": round(max(med[f"vote_{k}_{m}/{n}"] for n in masks) / min(med[f"vote_{k}_{m}/{n}"] for n in masks), 3)
        for k, m in PAIRS}
    res["vote_GBps_read_once_write_once"] = {f"{k},{m}": round(2 * mask_bytes / med[f"vote_{k}_{m}/clip"] / 1e6, 0)
                                             for k, m in PAIRS}
    # priming: every part but the first reads k - 1 frames it does not own (no history: the first reads none)
    res["schedule"] = {key: {"parts": q["parts"], "part_frames": q["part_frames"], "n_waves": q["n_waves"],
                             "priming_frames": (q["parts"] - 1) * (int(key.split(",")[0]) - 1),
                             "priming_share_of_input_reads": round((q["parts"] - 1) * (int(key.split(",")[0]) - 1) / F, 4)}
                       for key, q in sched.items()}
    faster = all(med[f"torch_general_{k}_{m}"] > med[f"vote_{k}_{m}/clip"] for k, m in PAIRS) and \
        all(med[f"torch_packed_{k}_{m}"] > med[f"vote_{k}_{m}/clip"] for k, m in PAIRS if m in (1, k))
    res["vote_faster_than_torch"] = faster
    op.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not (faster and all(agree.values())):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
