#!/usr/bin/env python3
"""mask_select_bench.py -- what the selection of components of the packed
change mask (dips_mask_select), the logic of two masks (dips_mask_logic) and
mask_fill_holes cost beside the traffic floor, beside the labelling they
contain and beside today's route to the same mask through the label image.

Workload: the 'per-frame' change mask (tau = 8/255) of --frames 3840x2160 RGB8
synthetic frames (500 frames: 518 MB of mask) and a random mask of density 0.5
of the same shape, both resident in HBM.  Every leg is timed with device events
around --inner back-to-back calls, the legs alternated within each of --reps
repetitions; ms PER CALL over the whole mask.  Per mask:

  a. copy        a plain device copy of the mask bytes: the floor.
  b. label       dips_mask_components with max_boxes = 0 and no labels: the
                 labelling that select contains, and its three counting launches.
  c. select      dips_mask_select with min_area = 16.
  d. reconstruct the same with a marker, the mask eroded 3 x 3: opening by
                 reconstruction.
  e. via_labels  today's route: dips_mask_components with labels (4 bytes per
                 pixel), then torch labels != 0 and a re-pack to bits, in chunks
                 of --chunk frames.
  f. logic_or    dips_mask_logic OR of the mask and the marker of (d).
  g. fill_holes  run_mask_fill_holes_device (NOT, select, OR).
and once: contention, one all-ones frame under an all-ones marker.

Every output is compared on all frames: (c) with (e); (d), (f) and (g) with
torch's own logic where that is direct ((d) is a subset of the mask that holds
the marker, checked against scipy on --check-frames frames where scipy is
installed; (f) with torch's |; (g) is a superset of the mask whose complement
equals the dropped reconstruction of the complement from the border ring).
Prints one JSON line (and writes it to --out); exits 1 if a comparison fails
or (c) is not faster than (e).
Run on the GPU box:
    python tools/mask_select_bench.py [--out profiles/mask_select/NAME.json]
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


def repack(torch, labels, out_words, chunk, weights):
    """labels int32 [F, H, W] (W a multiple of 32) -> out_words int32 [F, H, W / 32]: the bits labels != 0."""
    f, h, w = labels.shape
    for s in range(0, f, chunk):
        b = (labels[s:s + chunk] != 0).reshape(-1, h, w // 32, 32)
        out_words[s:s + chunk] = (b * weights).sum(dim=-1, dtype=torch.int64).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--min-area", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=1, help="back-to-back calls inside one pair of events")
    ap.add_argument("--chunk", type=int, default=10, help="frames per chunk of the torch re-pack")
    ap.add_argument("--check-frames", type=int, default=2, help="frames of each mask compared with scipy")
    ap.add_argument("--masks", default="clip,random_05")
    ap.add_argument("--note", default=None, help="what this run compares (kept in the JSON line)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    import torch
    from dips_amd import DiffSeriesOperator, MaskLogic, Mode, MorphOp, PixelFormat, mask_row_bytes

    W, H, F, A = args.width, args.height, args.frames, args.min_area
    assert W % 32 == 0, "the torch re-pack of leg (e) takes whole words"
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

    out = torch.empty((F, H, RB), dtype=torch.uint8, device=dev)
    other = torch.empty_like(out)
    scratch = torch.empty_like(out)
    counts = torch.empty((F,), dtype=torch.int32, device=dev)
    counts_e = torch.empty((F,), dtype=torch.int32, device=dev)
    labels = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
    ring = np.zeros((H, W), dtype=bool)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
    ring_t = torch.from_numpy(np.packbits(ring, axis=-1, bitorder="little").reshape(1, H, RB)).to(dev)

    def via_labels(msk):
        op.run_mask_components_device(msk, W, counts_e, None, labels, min_area=A)
        repack(torch, labels, other.view(torch.int32), args.chunk, weights)

    legs, agree, markers = {}, {}, {}
    for name, msk in masks.items():
        markers[name] = torch.empty_like(msk)
        op.run_mask_morph_device(msk, W, markers[name], MorphOp.Erode, 1)
        mk = markers[name]
        legs[f"copy/{name}"] = lambda msk=msk: out.copy_(msk)
        legs[f"label/{name}"] = lambda msk=msk: op.run_mask_components_device(msk, W, counts_e, None, None, min_area=A)
        legs[f"select/{name}"] = lambda msk=msk: op.run_mask_select_device(msk, W, out, counts_out=counts, min_area=A)
        legs[f"reconstruct/{name}"] = lambda msk=msk, mk=mk: op.run_mask_select_device(msk, W, out, marker=mk,
                                                                                       counts_out=counts)
        legs[f"via_labels/{name}"] = lambda msk=msk: via_labels(msk)
        legs[f"logic_or/{name}"] = lambda msk=msk, mk=mk: op.run_mask_logic_device(msk, W, out, MaskLogic.Or, mk)
        legs[f"fill_holes/{name}"] = lambda msk=msk: op.run_mask_fill_holes_device(msk, W, out, scratch)

        # the comparisons, on all frames (they warm every leg up too)
        op.run_mask_select_device(msk, W, out, counts_out=counts, min_area=A)
        via_labels(msk)
        agree[f"select==via_labels/{name}"] = bool(torch.equal(out, other) and torch.equal(counts, counts_e))
        agree[f"select_keeps_and_drops/{name}"] = bool(out.any() and not torch.equal(out, msk))
        op.run_mask_select_device(msk, W, out, marker=mk, counts_out=counts)
        agree[f"marker<=reconstruct<=mask/{name}"] = bool(torch.equal(out & mk, mk) and torch.equal(out & msk, out))
        # opening by reconstruction drops exactly the components the erosion emptied: none of them holds a marker bit
        op.run_mask_select_device(msk, W, other, marker=mk, dropped=True)
        agree[f"reconstruct_partition/{name}"] = bool(torch.equal(out | other, msk) and not (out & other).any()
                                                      and not (other & mk).any())
        try:
            import scipy.ndimage as ndi
            ok = True
            for t in range(min(args.check_frames, F)):
                bits = np.unpackbits(msk[t].cpu().numpy(), axis=-1, bitorder="little")[:, :W].astype(bool)
                mbits = np.unpackbits(mk[t].cpu().numpy(), axis=-1, bitorder="little")[:, :W].astype(bool)
                want = ndi.binary_propagation(mbits, structure=np.ones((3, 3), dtype=bool), mask=bits)
                got = np.unpackbits(out[t].cpu().numpy(), axis=-1, bitorder="little")[:, :W].astype(bool)
                ok = ok and np.array_equal(got, want)
            agree[f"reconstruct==scipy/{name}"] = bool(ok)
        except ImportError:
            pass
        op.run_mask_logic_device(msk, W, out, MaskLogic.Or, mk)
        agree[f"logic_or==torch/{name}"] = bool(torch.equal(out, msk | mk))
        # fill_holes: the complement of the result is the complement's components that touch the border
        op.run_mask_fill_holes_device(msk, W, out, scratch)
        op.run_mask_logic_device(msk, W, other, MaskLogic.Not)
        op.run_mask_select_device(other, W, scratch, marker=ring_t, connectivity=4)
        op.run_mask_logic_device(out, W, other, MaskLogic.Not)
        agree[f"fill_holes==border_reconstruction/{name}"] = bool(torch.equal(other, scratch))

    ones = torch.full((1, H, RB), 0xFF, dtype=torch.uint8, device=dev)
    ones_out = torch.empty_like(ones)
    legs["contention/all_ones_under_all_ones"] = lambda: op.run_mask_select_device(ones, W, ones_out, marker=ones,
                                                                                   counts_out=counts[:1])
    legs["label/all_ones"] = lambda: op.run_mask_components_device(ones, W, counts_e[:1], None, None)
    legs["contention/all_ones_under_all_ones"]()
    agree["contention_keeps_the_frame"] = bool(torch.equal(ones_out, ones) and int(counts[0].item()) == 1)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()

    ms = {name: [] for name in legs}
    for _ in range(args.reps):  # alternated: every repetition runs every leg once
        for name, fn in legs.items():
            ms[name].append(timed_events(torch, fn, args.inner))

    res = {"metric": "selection of components, logic and hole filling of the 4K change mask vs a device copy, the labelling "
                     "alone and the route through the label image, ms PER CALL over all frames",
           "frames": F, "width": W, "height": H, "mask_bytes": F * H * RB, "min_area": A, "reps": args.reps,
           "inner": args.inner, "chunk": args.chunk, "note": args.note,
           "cu_count": torch.cuda.get_device_properties(0).multi_processor_count,
           "timing": "device events around `inner` back-to-back calls on one stream, divided by `inner`; legs alternated "
                     "per repetition"}
    res.update(summary(ms))
    med, span = res["median_ms"], res["min_max_ms"]
    res["agree"] = agree
    res["ratio"] = {}
    for name in masks:
        res["ratio"][name] = {
            "select/label": round(med[f"select/{name}"] / med[f"label/{name}"], 3),
            "reconstruct/label": round(med[f"reconstruct/{name}"] / med[f"label/{name}"], 3),
            "logic_or/copy": round(med[f"logic_or/{name}"] / med[f"copy/{name}"], 3),
            "via_labels/select": round(med[f"via_labels/{name}"] / med[f"select/{name}"], 2),
            "fill_holes/label": round(med[f"fill_holes/{name}"] / med[f"label/{name}"], 3),
            "label_spread": round((span[f"label/{name}"][1] - span[f"label/{name}"][0]) / med[f"label/{name}"], 3)}
        agree[f"select_faster_than_via_labels/{name}"] = max(ms[f"select/{name}"]) < min(ms[f"via_labels/{name}"])
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
