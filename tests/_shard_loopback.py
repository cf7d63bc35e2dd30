"""The loopback drivers of the sharded visual operators, shared by
test_gpu_alt_shard.py, test_gpu_shard_native.py and test_gpu_shard_chunks.py:
every rank of a loopback communicator on its own thread of this process, on
the one device.  The threads are joined with a bound and the transport has its
own deadline: a rank that does not return fails the test."""
import threading

import numpy as np


def alt_sharded(world, frames, props, markers, n_tex, device_ptrs, keep_last=False, crosscheck=False):
    """dips_alt_run_sharded on `world` loopback ranks, one thread each;
    returns the concatenated outputs (and the last rank's runner if asked)."""
    import torch
    from dips_amd.alt import DiPsRunner
    from dips_amd.comm import Comm, shard_range
    n, h, w = frames.shape[:3]
    comms = Comm.loopback(world, 0)
    runners = [DiPsRunner(h, w, props, markers, num_textures=n_tex, crosscheck=crosscheck) for _ in range(world)]
    outs, errs = [None] * world, [None] * world

    def rank(r):
        try:
            s, e = shard_range(n, world, r)
            if device_ptrs:
                dev = torch.from_numpy(frames[s:e].copy()).cuda()
                out = torch.empty_like(dev)
                runners[r].run_sharded_device(comms[r], dev, out, n)
                outs[r] = out.cpu().numpy()
            else:
                outs[r] = runners[r].run_sharded(comms[r], frames[s:e], n)
        except Exception as ex:  # reported below, on the test's thread
            errs[r] = ex

    if device_ptrs:
        torch.cuda.synchronize()
    th = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    try:
        assert not any(t.is_alive() for t in th), "a rank did not return"
        assert errs == [None] * world, errs
        got = np.concatenate(outs) if n else np.empty((0, h, w, 4), dtype=np.uint8)
        if keep_last:
            last = runners.pop()
            return got, last
        return got
    finally:
        for r in runners:
            r.close()
        for c in comms:
            c.close()


def compat_loopback(world, n_total, w, h, props, device_ptrs, frames=None, crosscheck=False, keep=False):
    """dips_frame_callback_batch_sharded on `world` loopback ranks (fresh
    ComputeStates of `props`), one thread each; returns (frames, the
    concatenated outputs), and with `keep` the ranks' ComputeStates as well,
    left open for the caller to read, carry on with and close.  Without
    `frames` the clip is random bytes seeded by the layout."""
    import torch
    from dips_amd import ComputeState
    from dips_amd.comm import Comm, shard_range
    if frames is None:
        frames = np.random.default_rng(world * 100 + n_total).integers(0, 256, (n_total, h, w, 4), dtype=np.uint8)
    comms = Comm.loopback(world, 0)
    states = [ComputeState(*props, crosscheck=crosscheck) for _ in range(world)]
    outs, errors = [None] * world, []
    try:
        ranges = [shard_range(n_total, world, r) for r in range(world)]
        if device_ptrs:
            dev_in = [torch.from_numpy(frames[s:e].copy()).cuda() for s, e in ranges]
            dev_out = [torch.empty_like(t) for t in dev_in]
            torch.cuda.synchronize()

        def rank(r):
            try:
                s, e = ranges[r]
                if device_ptrs:
                    states[r].frame_callback_batch_sharded_device(comms[r], dev_in[r], dev_out[r], n_total)
                else:
                    outs[r] = states[r].frame_callback_batch_sharded(comms[r], w, h, frames[s:e], n_total)
            except Exception as ex:  # reported below
                errors.append((r, repr(ex)))

        threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=180)
        assert not any(t.is_alive() for t in threads) and not errors, errors
        if device_ptrs:
            torch.cuda.synchronize()
            outs = [o.cpu().numpy() for o in dev_out]
        got = np.concatenate(outs)
        if keep:
            kept, states = states, []
            return frames, got, kept
        return frames, got
    finally:
        for c in states:
            c.close()
        for c in comms:
            c.close()
