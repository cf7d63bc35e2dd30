#!/usr/bin/env python3
"""sigma_delta_bench.py -- what the Sigma-Delta background and its per-pixel
adaptive threshold mask (dips_diff_sigma_delta_mask) cost beside the plain
change mask, beside the running-average background and beside the same
recurrence restated in torch.

Workload: 3840x2160 RGB8 synthetic frames resident in HBM, (n_amp, v_min,
v_max) = (2, 2, 510).  Legs alternated within every repetition, each timed by
device events on one stream around --inner back-to-back calls:

  1. mask          dips_diff_change_mask ('per-frame', tau = 8/255).
  2. background    dips_diff_background_mask at rate_shift 3.
                   With --parent-lib legs 1 and 2 are called in the library of
                   the parent commit (a second libdips_hip.so loaded beside
                   this build's), otherwise in this build's (the same code).
  3. torch         per frame the recurrence in torch on the device: amax /
                   amin over the channels, sign steps and clamps on int16.
                   Timed over --route-frames frames per window, reported per
                   frame.  The bits stay unpacked (nothing is charged for
                   packing them).
  4. sigma_delta   dips_diff_sigma_delta_mask over the whole frame, and over
                   a 1920x1080 region at an odd x (sigma_delta_roi).

Prints one JSON line (and writes it to --out); exits 1 unless leg 4 is faster
per frame than leg 3 in every repetition, its bits and state equal leg 3's on
the frames leg 3 ran, those frames' mask is the prefix of the whole clip's and
the region equals the crop with pad bits 0.  leg 4 / leg 1 and leg 4 / leg 2
are reported without a pass mark.  NAME=PATH arguments add a whole-frame leg
per variant library (built with another -DDIPS_UNROLL_SIGMA_DELTA), whose mask
and state must equal leg 4's.  Run on the GPU box:
    python tools/sigma_delta_bench.py [NAME=PATH ...] [--parent-lib PATH] [--out profiles/sigma_delta/NAME.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="*", help="NAME=PATH of a variant libdips_hip.so (another DIPS_UNROLL_SIGMA_DELTA): "
                                                 "a further whole-frame leg sigma_delta@NAME, its bits compared with leg 4's")
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--n-amp", type=int, default=2)
    ap.add_argument("--v-min", type=int, default=2)
    ap.add_argument("--v-max", type=int, default=510)
    ap.add_argument("--rate-shift", type=int, default=3, help="of leg 2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="back-to-back calls inside one timed window")
    ap.add_argument("--route-frames", type=int, default=20, help="frames of leg 3 inside one timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="libdips_hip.so of the parent commit for legs 1 and 2")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    import torch
    from dips_amd import DiffSeriesOperator, Mode, PixelFormat, mask_row_bytes
    from dips_amd.api import _params
    from dips_amd import _lib
    from mask_bench import VariantMask

    class ParentLib(VariantMask):
        """dips_diff_change_mask and dips_diff_background_mask of another libdips_hip.so."""

        def __init__(self, path, params, stream):
            super().__init__(path, params, stream)
            vp, u32 = ctypes.c_void_p, ctypes.c_uint32
            self.lib.dips_diff_background_mask.argtypes = [vp, u32, u32, vp, u32, vp, vp, u32, u32, u32, vp, vp]

        def run_background(self, frames, bg, mask, k):
            n, h, w = frames.shape[:3]
            st = self.lib.dips_diff_background_mask(self.h, w, h, frames.data_ptr(), n, None, None, k, 0, 0,
                                                    bg.data_ptr(), mask.data_ptr())
            assert st == 0, st

        def run_sigma_delta(self, frames, state, mask, n_amp, v_min, v_max):
            vp, u32 = ctypes.c_void_p, ctypes.c_uint32
            self.lib.dips_diff_sigma_delta_mask.argtypes = [vp, u32, u32, vp, u32, vp, vp, u32, u32, u32, u32, vp, vp]
            n, h, w = frames.shape[:3]
            st = self.lib.dips_diff_sigma_delta_mask(self.h, w, h, frames.data_ptr(), n, None, None, n_amp, v_min, v_max, 0,
                                                     state.data_ptr(), mask.data_ptr())
            assert st == 0, st

    W, H, F = args.width, args.height, args.frames
    N, vmin, vmax, k = args.n_amp, args.v_min, args.v_max, args.rate_shift
    K = min(args.route_frames, F)
    tau = 8 / 255
    roi = (W // 4 + 1, H // 4, W // 2, H // 2)  # 1920x1080 at x = 961 for the 4K default
    dev = torch.device("cuda", 0)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, tau)
    op.synth_device(frames, W, H, 0xD1B5, 0)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    params = _params(fmt=PixelFormat.RGB8, mode=Mode.PerFrame, tau=tau, flags=_lib.FLAG_DEVICE_PTRS)
    rb = mask_row_bytes(W)
    mask1 = torch.full((F, H, rb), 0xFF, dtype=torch.uint8, device=dev)
    mask4 = torch.full((F, H, rb), 0xFF, dtype=torch.uint8, device=dev)
    mask4_roi = torch.full((F, roi[3], mask_row_bytes(roi[2])), 0xFF, dtype=torch.uint8, device=dev)
    bg2 = torch.full((3, H, W), -1, dtype=torch.int16, device=dev)
    sd4 = torch.full((2, H, W), -1, dtype=torch.int16, device=dev)
    sd4_roi = torch.full((2, roi[3], roi[2]), -1, dtype=torch.int16, device=dev)
    bits3 = torch.zeros((K, H, W), dtype=torch.bool, device=dev)
    torch_state = {}
    parent = ParentLib(os.path.abspath(args.parent_lib), params, stream) if args.parent_lib else None

    def leg_mask():
        if parent is not None:
            parent.run(frames, mask1)
        else:
            op.run_change_mask_device(frames, mask1)

    def leg_background():
        if parent is not None:
            parent.run_background(frames, bg2, mask1, k)
        else:
            op.run_background_mask_device(frames, bg2, mask1, rate_shift=k)

    def intensity_j(f):
        return f.amax(dim=-1).to(torch.int16) + f.amin(dim=-1).to(torch.int16)

    def leg_torch():
        M = intensity_j(frames[0])
        V = torch.full_like(M, vmin)
        for t in range(K):
            J = intensity_j(frames[t])
            M = M + torch.sign(J - M)
            D = (J - M).abs()
            V = torch.where(D != 0, (V + torch.sign(N * D - V)).clamp(vmin, vmax), V)
            bits3[t] = D > V
        torch_state["M"], torch_state["V"] = M, V

    legs = {
        "mask": leg_mask,
        "background": leg_background,
        "torch": leg_torch,
        "sigma_delta": lambda: op.run_sigma_delta_mask_device(frames, sd4, mask4, n_amp=N, v_min=vmin, v_max=vmax),
        "sigma_delta_roi": lambda: op.run_sigma_delta_mask_device(frames, sd4_roi, mask4_roi, roi=roi, n_amp=N, v_min=vmin,
                                                                  v_max=vmax),
    }
    variants = {}
    for spec in args.variants:
        name, path = spec.split("=", 1)
        variants[name] = ParentLib(os.path.abspath(path), params, stream)
        variants[name].state = torch.full((2, H, W), -1, dtype=torch.int16, device=dev)
        variants[name].mask = torch.full((F, H, rb), 0xFF, dtype=torch.uint8, device=dev)
        legs["sigma_delta@" + name] = (lambda v: lambda: v.run_sigma_delta(frames, v.state, v.mask, N, vmin, vmax))(variants[name])
    frames_of = {name: (K if name == "torch" else F) for name in legs}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():  # alternated: every repetition runs every leg once
            inner = 1 if name == "torch" else args.inner
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / inner)

    # agreement: leg 4 on the frames leg 3 ran, and the region against the crop
    maskK = torch.full((K, H, rb), 0xFF, dtype=torch.uint8, device=dev)
    sdK = torch.full((2, H, W), -1, dtype=torch.int16, device=dev)
    op.run_sigma_delta_mask_device(frames[:K], sdK, maskK, n_amp=N, v_min=vmin, v_max=vmax)
    torch.cuda.synchronize()

    def unpack(m, w):  # uint8 [..., h, row_bytes] -> bool [..., h, w] on the device
        sh = torch.arange(8, dtype=torch.uint8, device=dev)
        b = (m.unsqueeze(-1) >> sh) & 1
        return b.reshape(*m.shape[:-1], m.shape[-1] * 8)[..., :w].bool()

    x, y, w, h = roi
    agree = {
        "bits_equal_torch": all(bool(torch.equal(unpack(maskK[t], W), bits3[t])) for t in range(K)),
        "state_equal_torch": bool(torch.equal(sdK[0], torch_state["M"]) and torch.equal(sdK[1], torch_state["V"])),
        "prefix_of_whole_clip": bool(torch.equal(mask4[:K], maskK)),
        "roi_mask_equals_crop": all(bool(torch.equal(unpack(mask4_roi[t], w), unpack(mask4[t], W)[y:y + h, x:x + w]))
                                    for t in range(0, F, max(1, F // 16))),
        "roi_state_equals_crop": bool(torch.equal(sd4_roi, sd4[:, y:y + h, x:x + w])),
        "pad_bits_zero": bool((unpack(mask4_roi, 8 * mask4_roi.shape[-1])[..., w:] == 0).all()),
    }
    for name, v in variants.items():
        agree["variant_equal@" + name] = bool(torch.equal(v.mask, mask4) and torch.equal(v.state, sd4))
    pop = sum(int(unpack(mask4[t], W).sum()) for t in range(1, F, max(1, F // 16)))
    share = pop / float(len(range(1, F, max(1, F // 16))) * W * H)

    batch_bytes = F * W * H * 3
    med = {name: statistics.median(v) for name, v in ms.items()}
    per_frame = {name: [v_ / frames_of[name] for v_ in v] for name, v in ms.items()}
    faster = all(s < r for s, r in zip(per_frame["sigma_delta"], per_frame["torch"])) and \
        max(per_frame["sigma_delta"]) < min(per_frame["torch"])

    def ratio(a, b):
        return {"median": round(med[a] / med[b], 4),
                "min_max": [round(min(ms[a]) / max(ms[b]), 4), round(max(ms[a]) / min(ms[b]), 4)]}

    out = {
        "metric": "Sigma-Delta background + mask vs the plain change mask vs the running-average background vs the "
                  "recurrence in torch per frame, 4K RGB8",
        "frames": F, "width": W, "height": H, "roi": list(roi), "n_amp": N, "v_min": vmin, "v_max": vmax, "rate_shift": k,
        "reps": args.reps, "inner": args.inner, "route_frames": K, "warmup": args.warmup,
        "timing": "device events around `inner` back-to-back calls on one stream (ms per call; torch: one window of "
                  "route_frames frames), legs alternated per repetition",
        "legs_1_2_library": "parent commit" if args.parent_lib else "this build",
        "ms": {name: [round(v_, 3) for v_ in v] for name, v in ms.items()},
        "median_ms": {name: round(v, 3) for name, v in med.items()},
        "min_max_ms": {name: [round(min(v), 3), round(max(v), 3)] for name, v in ms.items()},
        "median_us_per_frame": {name: round(1e3 * statistics.median(v), 3) for name, v in per_frame.items()},
        "min_max_us_per_frame": {name: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for name, v in per_frame.items()},
        "batch_read_frac_of_8tbs": {name: round(batch_bytes / (v / 1e3) / 1e9 / HBM_PEAK_GBS, 4)
                                    for name, v in med.items() if name not in ("torch", "sigma_delta_roi")},
        "variants": {name: os.path.basename(os.path.dirname(os.path.abspath(spec.split("=", 1)[1])))
                     for name, spec in zip(variants, args.variants)},
        "ratio_variant_to_sigma_delta": {name: ratio("sigma_delta@" + name, "sigma_delta") for name in variants},
        "ratio_sigma_delta_to_mask": ratio("sigma_delta", "mask"),
        "ratio_sigma_delta_to_background": ratio("sigma_delta", "background"),
        "ratio_torch_to_sigma_delta_per_frame": round(statistics.median(per_frame["torch"])
                                                      / statistics.median(per_frame["sigma_delta"]), 2),
        "sigma_delta_faster_per_frame_than_torch_in_every_rep": bool(faster),
        "changed_share_sampled": round(share, 4),
        "agree": agree,
    }
    ok = all(agree.values()) and faster
    if parent is not None:
        parent.close()
    for v in variants.values():
        v.close()
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
