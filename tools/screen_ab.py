#!/usr/bin/env python3
"""screen_ab.py -- A/B of the screened RGB8 series kernel
(dips_amd/csrc/series_v2_screen.h) against its unscreened body
(DIPS_SERIES_SCREEN=0) on ONE resident batch in one process: two operators,
one per form, alternated round by round, several launches per round, every
launch's device time from kernel_times().  The placement of a 124 GB batch
alone moves the rate by 2-3 points, so only times on the same buffer compare.

Contents at 3840x2160 RGB8, tau = 8/255:
  synthetic 'per-frame'  the bench's frames and mode;
  synthetic 'overall'    the same frames ('overall' has no screened form: both
                         operators run the same kernel -- the noise floor);
  random 'per-frame'     i.i.d. bytes: every 256-pixel vec row holds a hit, the
                         fast and the exact path both run -- the worst case.

Criterion per content: every screened round faster than every unscreened
round ("separated").  Writes profiles/screen_ab/<name>.json and prints one
JSON line per content; run on the GPU box:
    python tools/screen_ab.py [--frames 5000] [--rounds 5] [--launches 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from dips_amd import DiffSeriesOperator, Mode, PixelFormat  # noqa: E402

W, H, TAU, SEED = 3840, 2160, 8 / 255, 0xD1B5


def make_op(mode, screen):
    """An operator created with DIPS_SERIES_SCREEN=`screen` (the library reads it when a handle is created)."""
    old = os.environ.get("DIPS_SERIES_SCREEN")
    os.environ["DIPS_SERIES_SCREEN"] = "1" if screen else "0"
    try:
        return DiffSeriesOperator(PixelFormat.RGB8, mode, TAU, time_kernel=True)
    finally:
        if old is None:
            del os.environ["DIPS_SERIES_SCREEN"]
        else:
            os.environ["DIPS_SERIES_SCREEN"] = old


def launches(op, frames, series, k):
    op.kernel_time(reset=True)
    for _ in range(k):
        op.run_device(frames, series)
    torch.cuda.synchronize()
    ms = op.kernel_times()
    assert len(ms) == k, (len(ms), k)
    return ms


def ab(name, mode, frames, rounds, n_launch):
    """One operator at a time, created for its round and closed after it: the two forms then write their
    partial records to the same allocation (two live handles have one each, and where the second one's lands
    costs it ~1.4 % -- seen with the SAME kernel on both handles, 'overall').  The order within a round
    alternates (on, off), (off, on), ..."""
    n = frames.shape[0]
    out = torch.zeros((n, 4), dtype=torch.int64, device=frames.device)
    ms = {"on": [], "off": []}
    first = {}
    for r in range(rounds):
        for k in (("on", "off") if r % 2 == 0 else ("off", "on")):
            op = make_op(mode, k == "on")
            try:
                launches(op, frames, out, 1)  # warm-up: the partials' allocation and first touch
                ms[k].append(launches(op, frames, out, n_launch))
            finally:
                op.close()
            first.setdefault(k, out.clone())
    same = bool(torch.equal(first["on"], first["off"]))
    mean = {k: [statistics.fmean(r) for r in v] for k, v in ms.items()}
    gbytes = n * W * H * 3 / 1e9
    on, off = statistics.fmean(mean["on"]), statistics.fmean(mean["off"])
    return {"content": name, "mode": mode.name, "tau": round(TAU, 6), "width": W, "height": H, "frames": n,
            "rounds": rounds, "launches_per_round": n_launch, "order": "one operator at a time; (on, off), (off, on), ... by round",
            "kernel_ms": {k: [[round(x, 4) for x in r] for r in v] for k, v in ms.items()},
            "round_mean_ms": {k: [round(x, 4) for x in v] for k, v in mean.items()},
            "mean_ms": {"on": round(on, 4), "off": round(off, 4)},
            "gb_per_s": {"on": round(gbytes / on * 1e3, 1), "off": round(gbytes / off * 1e3, 1)},
            "speedup_off_over_on": round(off / on, 4),
            "separated": max(mean["on"]) < min(mean["off"]),
            "outputs_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_ab"))
    args = ap.parse_args()
    assert args.rounds >= 5 and args.launches >= 5, "at least 5 alternated rounds of 5 launches"
    dev = torch.device("cuda", 0)
    frames = torch.empty((args.frames, H, W, 3), dtype=torch.uint8, device=dev)
    op = DiffSeriesOperator(PixelFormat.RGB8, Mode.PerFrame, TAU)
    op.synth_device(frames, W, H, SEED, 0)
    torch.cuda.synchronize()
    op.close()
    os.makedirs(args.out, exist_ok=True)
    res = []

    def record(r):
        print(json.dumps({k: v for k, v in r.items() if k != "kernel_ms"}), flush=True)
        with open(os.path.join(args.out, f"{r['content']}_{r['mode'].lower()}.json"), "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
        res.append(r)

    record(ab("synthetic", Mode.PerFrame, frames, args.rounds, args.launches))
    record(ab("synthetic", Mode.Overall, frames, args.rounds, args.launches))
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    flat = frames.view(-1)
    step = 1 << 30
    for s in range(0, flat.numel(), step):  # the same buffer, i.i.d. bytes
        e = min(flat.numel(), s + step)
        flat[s:e] = torch.randint(0, 256, (e - s,), dtype=torch.uint8, device=dev, generator=gen)
    torch.cuda.synchronize()
    record(ab("random", Mode.PerFrame, frames, args.rounds, args.launches))
    if not all(r["outputs_equal"] for r in res):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
