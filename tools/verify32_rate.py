"""Times verification of 32-bit samples on the device (sela_hip_verify_i32_device) against what a caller did
before it existed.  Input: the bench's shape -- 3875 stereo 2048-sample frames of synth_frames -- as int32 [n, 2, 2048], the
stream from codec.Encoder32, everything resident in device memory.
  (a) verify            codec.Verifier32.verify: the decode kernels into the workspace by position, k_verify32_direct, two words
                        per frame; no decoded sample moved by channel or written a second time;
  (b) decode_compare    codec.Decoder32.decode into a second [n, 2, 2048] buffer, then in torch diff = back != samples, the
                        per-frame count diff.sum(1) and the first index diff.argmax(1) -- calls of the parent commit only.
Both are timed with device events in the same process, in alternating windows of at least --window seconds each after a
warm-up; the figure per version is the median over its windows of (window time / calls).  Run the command twice for the
spread.  Under `rocprofv3 --kernel-trace --stats -- python tools/verify32_rate.py --window 0.1 --rounds 2` the per-kernel times
come out of the same run (no counters with the trace).

  python tools/verify32_rate.py [--frames N] [--track T] [--window S] [--rounds R] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # (appended: a PYTHONPATH that names another build of the package comes first)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sela_amd import codec  # noqa: E402
from sela_amd.synth import synth_frames  # noqa: E402


def _window_ms(fn, calls):
    """`calls` calls of fn between two device events -> milliseconds per call."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3875)
    ap.add_argument("--track", type=int, default=0)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window, at least")
    ap.add_argument("--rounds", type=int, default=7, help="windows per version, alternating")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n = a.frames
    x_host = np.ascontiguousarray(synth_frames(n, 2, a.track).transpose(0, 2, 1)).astype(np.int32)
    x = torch.from_numpy(x_host).cuda()
    enc = codec.Encoder32(n, 2, 2048)
    frames, d_offs, _ = enc.encode(x)
    enc.check()
    ver = codec.Verifier32(n, 2, 2048)
    dec = codec.Decoder32(n, 2, 2048)
    out_b = []

    def verify():
        ver.verify(frames, d_offs, n, x)

    def decode_compare():
        back, _, _ = dec.decode(frames, d_offs, n)
        diff = (back != x).reshape(n, -1)
        counts = diff.sum(1)
        first = torch.where(counts != 0, diff.int().argmax(1), -1)
        out_b.append((counts, first))

    # both give the same answer
    verify()
    decode_compare()
    torch.cuda.synchronize()
    ver.check()
    dec.check()
    counts = ver.diff_counts[:n].cpu().numpy()
    assert np.array_equal(counts, out_b[-1][0].cpu().numpy()), "the two versions disagree on the counts"
    assert np.array_equal(ver.first_diff[:n].cpu().numpy(), out_b[-1][1].cpu().numpy()), "the two versions disagree on the first index"
    assert ver.fallback_frames() == 0
    res = {"frames": n, "track": a.track, "lossy_frames": int((counts != 0).sum()), "window_s": a.window, "rounds": a.rounds}
    fns = {"verify_ms": verify, "decode_compare_ms": decode_compare}
    calls = {}
    for k, fn in fns.items():  # warm-up, and how many calls fill a window
        _window_ms(fn, 20)
        out_b.clear()
        per_call = _window_ms(fn, 50)
        out_b.clear()
        calls[k] = max(1, int(a.window * 1e3 / per_call) + 1)
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():  # (alternating)
            times[k].append(_window_ms(fn, calls[k]))
            out_b.clear()
    for k in fns:
        res[k] = float(np.median(times[k]))
        res[k + "_windows"] = [round(t, 5) for t in times[k]]
        res[k.replace("_ms", "_calls_per_window")] = calls[k]
    res["speedup"] = res["decode_compare_ms"] / res["verify_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
