#!/usr/bin/env python3
"""pixel_unroll_ab.py -- A/B of dips_diff_pixel_sums built with different
vecs per lane (DIPS_UNROLL_PIX): the libraries loaded side by side in one
process, the legs alternated, device events around 5 back-to-back calls, 5
repetitions.  3840x2160, 500 resident frames; RGB8 per-frame at tau = 8/255
and 0, RGB8 overall, RGBA8 per-frame and overall.

Build a variant library next to the shipped one (U = 1, 3, ...):
    make -C dips_amd/csrc HIPFLAGS="<the Makefile's HIPFLAGS> -DDIPS_UNROLL_PIX=U" \
         OUTDIR=$PWD/build/pix_uU OBJDIR=$PWD/build/obj_uU BIN=$PWD/build/obj_uU/dips_raw
then, on the GPU box:
    python tools/pixel_unroll_ab.py u1=build/pix_u1/libdips_hip.so u3=build/pix_u3/libdips_hip.so \
        [--out profiles/pixel_sums/unroll_ab_4k.jsonl]
The shipped library is always the leg "u<kUnrollPix>" (u2).  Prints one JSON
line per configuration; exits 1 if the libraries' maps differ."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from dips_amd import DiffSeriesOperator, Mode, PixelFormat, _lib  # noqa: E402
from dips_amd._lib import DipsParams  # noqa: E402
from dips_amd.api import _params  # noqa: E402


class Lib:
    def __init__(self, path, params, stream):
        self.lib = ctypes.CDLL(path)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        self.lib.dips_create.argtypes = [ctypes.POINTER(DipsParams), ctypes.c_int, ctypes.POINTER(vp)]
        self.lib.dips_set_stream.argtypes = [vp, vp]
        self.lib.dips_diff_pixel_sums.argtypes = [vp, u32, u32, vp, u32, vp, vp, u32, vp]
        self.lib.dips_destroy.argtypes = [vp]
        self.lib.dips_destroy.restype = None
        self.h = vp()
        assert self.lib.dips_create(ctypes.byref(params), 0, ctypes.byref(self.h)) == 0
        assert self.lib.dips_set_stream(self.h, vp(stream)) == 0

    def run(self, frames, sums):
        n, h, w = frames.shape[:3]
        st = self.lib.dips_diff_pixel_sums(self.h, w, h, frames.data_ptr(), n, None, None, 0, sums.data_ptr())
        assert st == 0, st

    def close(self):
        self.lib.dips_set_stream(self.h, None)
        self.lib.dips_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="+", help="NAME=PATH of a variant libdips_hip.so")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    W, H, F = 3840, 2160, 500
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    paths = {"u2": _lib.LIB_PATH}
    for v in args.variants:
        name, path = v.split("=", 1)
        paths[name] = os.path.abspath(path)
    paths = dict(sorted(paths.items()))
    res = []
    for fmt, c in ((PixelFormat.RGB8, 3), (PixelFormat.RGBA8, 4)):
        frames = torch.empty((F, H, W, c), dtype=torch.uint8, device=dev)
        op = DiffSeriesOperator(fmt, Mode.PerFrame, 8 / 255)
        op.synth_device(frames, W, H, 0xD1B5, 0)
        torch.cuda.synchronize()
        op.close()
        for mode in (Mode.PerFrame, Mode.Overall):
            for tau in (8 / 255, 0.0):
                if tau == 0.0 and (c == 4 or mode == Mode.Overall):
                    continue
                p = _params(fmt=fmt, mode=mode, tau=tau, flags=_lib.FLAG_DEVICE_PTRS)
                libs = {k: Lib(v, p, stream) for k, v in paths.items()}
                outs = {k: torch.full((H, W, 4), -1, dtype=torch.int64, device=dev) for k in libs}
                for _ in range(2):
                    for k, lb in libs.items():
                        lb.run(frames, outs[k])
                torch.cuda.synchronize()
                ms = {k: [] for k in libs}
                for _ in range(5):
                    for k, lb in libs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(5):
                            lb.run(frames, outs[k])
                        e1.record()
                        e1.synchronize()
                        ms[k].append(e0.elapsed_time(e1) / 5)
                same = all(bool(torch.equal(outs["u2"], o)) for o in outs.values())
                for lb in libs.values():
                    lb.close()
                rec = {"format": fmt.name, "mode": mode.name, "tau": round(tau, 5), "frames": F, "width": W, "height": H,
                       "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                       "median_ms": {k: round(statistics.median(v), 3) for k, v in ms.items()},
                       "outputs_equal": same}
                print(json.dumps(rec), flush=True)
                res.append(rec)
                del outs
        del frames
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")
    if not all(r["outputs_equal"] for r in res):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
