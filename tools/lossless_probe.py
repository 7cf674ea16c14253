#!/usr/bin/env python3
"""What SELA_HIP_ENCODE_LOSSLESS costs: the block kernel of the lossless mode against the plain one on the bench
track (3875 stereo frames of 2048 samples), the two taken in turn in one session, and the same for the any-length route.

    python tools/lossless_probe.py [time] [reps]     k_encode_teams<0,16> / <4,16> by the library's own HIP events
                                                     (sela_hip_kernel_times), the any-length calls by events around the call
    python tools/lossless_probe.py run [reps]        the same launches and nothing else: for rocprofv3 --kernel-trace --stats
                                                     (per-kernel durations) or --pmc SQ_INSTS_VALU --kernel-trace (a run of its own)

Every variant's stream is checked as well: the lossless one verifies clean, the plain one's lossy frames are counted."""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sela_amd import capi, codec  # noqa: E402
from sela_amd.synth import synth_frames_torch  # noqa: E402

FRAMES, CHANNELS, TRACK = 3875, 2, 0


def block_kernel_ms(lib, enc, pcm):
    enc.encode(pcm)
    torch.cuda.synchronize()
    ms = (C.c_float * 8)()
    return ms[0] if lib.sela_hip_kernel_times(ms, 8) else float("nan")


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(name, xs):
    xs = sorted(xs)
    return f"{name}: median {statistics.median(xs):.4f} ms, min {xs[0]:.4f}, max {xs[-1]:.4f} ({len(xs)} runs)"


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else (15 if mode == "time" else 3)
    lib = capi.lib()
    pcm = synth_frames_torch(FRAMES, CHANNELS, TRACK, device="cuda")
    fast = {False: codec.Encoder(FRAMES, CHANNELS), True: codec.Encoder(FRAMES, CHANNELS, lossless=True)}
    slow = {False: codec.Encoder32(FRAMES, CHANNELS, 2048), True: codec.Encoder32(FRAMES, CHANNELS, 2048, lossless=True)}
    lib.sela_hip_debug_encode_teams(16)
    try:
        # what the two modes write, and what comes back
        ver = codec.Verifier(FRAMES, CHANNELS, 2048)
        streams = {}
        for lossless in (False, True):
            out = fast[lossless].encode(pcm)
            torch.cuda.synchronize()
            out.check()
            ver.verify(out.frames, out.offsets, FRAMES, pcm)
            streams[lossless] = (out.frames[: out.total_bytes()].clone(), out.offsets.clone(), ver.lossy_frames())
            frames, offsets, _ = slow[lossless].encode(pcm)
            slow[lossless].check()
            n = slow[lossless].needed_bytes()
            assert n == streams[lossless][0].numel() and torch.equal(frames[:n], streams[lossless][0]), "the any-length route writes another stream"
        assert streams[True][2] == 0, "the lossless stream does not verify clean"
        changed = int((streams[False][1][1:] - streams[False][1][:-1] != streams[True][1][1:] - streams[True][1][:-1]).sum())
        print(f"{FRAMES} stereo frames: plain stream {streams[False][0].numel()} bytes, {streams[False][2]} lossy frames; lossless stream "
              f"{streams[True][0].numel()} bytes, 0 lossy frames, {changed} frames of another size")
        for _ in range(3):  # warm
            for lossless in (False, True):
                fast[lossless].encode(pcm)
                slow[lossless].encode(pcm)
        torch.cuda.synchronize()
        if mode == "run":
            for _ in range(reps):
                for lossless in (False, True):
                    fast[lossless].encode(pcm)
                    torch.cuda.synchronize()
                    slow[lossless].encode(pcm)
                    torch.cuda.synchronize()
            return
        k = {False: [], True: []}
        g = {False: [], True: []}
        lib.sela_hip_enable_kernel_timing(1)
        for _ in range(reps):  # in turn: plain, lossless, plain, ...
            for lossless in (False, True):
                k[lossless].append(block_kernel_ms(lib, fast[lossless], pcm))
        lib.sela_hip_enable_kernel_timing(0)
        for _ in range(reps):
            for lossless in (False, True):
                g[lossless].append(call_ms(lambda: slow[lossless].encode(pcm)))
        print(summary("k_encode_teams<0,16> (plain)   ", k[False]))
        print(summary("k_encode_teams<4,16> (lossless)", k[True]))
        print(f"  lossless / plain, medians: {statistics.median(k[True]) / statistics.median(k[False]):.4f}")
        print(summary("sela_hip_encode_n_device      (analyse + plan + write)", g[False]))
        print(summary("sela_hip_encode_n_device_opt  (analyse + plan + write)", g[True]))
        print(f"  lossless / plain, medians: {statistics.median(g[True]) / statistics.median(g[False]):.4f}")
    finally:
        lib.sela_hip_debug_encode_teams(-1)


if __name__ == "__main__":
    main()
