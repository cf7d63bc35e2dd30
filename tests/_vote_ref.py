"""The specification of dips_mask_vote in plain numpy, written from the
definition in include/dips_hip.h: on unpacked bool arrays [n, h, w], a running
sum over the window of the sequence history ++ input.  Packing is
_components_ref.pack's."""
import numpy as np

import _components_ref as cref

MAX_WINDOW = 31


def vote_bits(bits, window, votes, history=None):
    """bits bool [n, h, w], history None (clear) or bool [window - 1, h, w],
    oldest first -> (voted bool [n, h, w], next history bool [window - 1, h,
    w]): voted[t] = at least `votes` of frames t - window + 1 .. t are set."""
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    k, m = int(window), int(votes)
    assert 1 <= k <= MAX_WINDOW and 1 <= m <= k
    hist = np.zeros((k - 1, h, w), dtype=bool) if history is None else np.asarray(history, dtype=bool)
    assert hist.shape == (k - 1, h, w)
    seq = np.concatenate([hist, bits])  # frame t of the clip is seq[t + k - 1]
    # the running sum modulo 256: a window's count is at most 31, so the
    # difference of two sums, taken modulo 256 again, is the count itself
    csum = np.concatenate([np.zeros((1, h, w), dtype=np.uint8), np.cumsum(seq, axis=0, dtype=np.uint8)])
    count = csum[k:] - csum[:n]  # frames t .. t + k - 1 of seq: the window of clip frame t
    return count >= m, seq[n:]


def vote(mask_bytes, w, window, votes, history_bytes=None):
    """The same on mask bytes [n, h, row_bytes] (pad bits ignored) -> (voted
    bytes, next history bytes), pad bits 0."""
    hist = None if history_bytes is None else cref.unpack(history_bytes, w)
    out, nxt = vote_bits(cref.unpack(mask_bytes, w), window, votes, hist)
    return cref.pack(out), cref.pack(nxt)


def vote_naive(bits, window, votes, history=None):
    """vote_bits' first result by the definition itself: a loop over frames,
    rows and pixels that counts the window."""
    bits = np.asarray(bits, dtype=bool)
    n, h, w = bits.shape
    out = np.zeros((n, h, w), dtype=bool)
    for t in range(n):
        for j in range(h):
            for i in range(w):
                c = 0
                for s in range(t - window + 1, t + 1):
                    if s >= 0:
                        c += int(bits[s, j, i])
                    elif history is not None:
                        c += int(history[s + window - 1, j, i])
                out[t, j, i] = c >= votes
    return out


def chunked(bits, window, votes, chunk, history=None):
    """vote_bits fed `chunk` frames per call with the history carried."""
    outs, hist = [], history
    for s in range(0, bits.shape[0], chunk):
        o, hist = vote_bits(bits[s:s + chunk], window, votes, hist)
        outs.append(o)
    if not outs:
        return vote_bits(bits, window, votes, history)
    return np.concatenate(outs), hist


# The vote_geometry harness: tests compile dips_amd/csrc/series_sched.h alone
# with g++ and read the schedule of a mask from it.
# stdin rows: frame_words n_frames window words resident; stdout rows: ok
# part_frames parts n_tiles n_waves blocks min_part_frames
GEOMETRY_PROGRAM = r'''
#include "series_sched.h"
#include <cstdio>
using namespace dips_sched;
int main() {
    long long v[5];
    for (;;) {
        for (int i = 0; i < 5; ++i)
            if (std::scanf("%lld", &v[i]) != 1) return 0;
        const Geom q = vote_geometry((uint64_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (int)v[3], (uint64_t)v[4]);
        std::printf("%d %u %u %llu %llu %llu %u\n", (int)q.ok, q.part_frames, q.parts, (unsigned long long)q.n_tiles,
                    (unsigned long long)q.n_waves, (unsigned long long)q.blocks, vote_min_part_frames((uint32_t)v[2]));
    }
}
'''


def build_geometry(directory, csrc):
    import subprocess
    src = directory / "vote_sched.cpp"
    src.write_text(GEOMETRY_PROGRAM)
    exe = directory / "vote_sched"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    return exe


def geometry(exe, rows):
    """dicts ok, part_frames, parts, n_tiles, n_waves, blocks, min_part for
    rows (frame_words, n_frames, window, words, resident)."""
    import subprocess
    txt = "".join(" ".join(str(int(x)) for x in r) + "\n" for r in rows)
    r = subprocess.run([str(exe)], input=txt, capture_output=True, text=True, timeout=60, check=True)
    names = "ok part_frames parts n_tiles n_waves blocks min_part".split()
    out = [dict(zip(names, (int(x) for x in line.split()))) for line in r.stdout.splitlines()]
    assert len(out) == len(rows)
    return out


def words_per_lane(csrc):
    """kVoteWords (DIPS_VOTE_WORDS) of dips_kernels.h: the mask words a lane of the kernel owns."""
    import os
    import re
    with open(os.path.join(csrc, "dips_kernels.h")) as f:
        return int(re.search(r"#define DIPS_VOTE_WORDS (\d+)", f.read()).group(1))


def frame_words(w, h):
    return ((w + 31) // 32) * h
