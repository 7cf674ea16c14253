"""Times verification on the device (sela_hip_verify_device) against what a caller did before it existed.
Input: the bench's shape -- 3875 stereo 2048-sample frames of synth_frames -- and its PCM, both resident in device memory.
  (a) verify            codec.Verifier.verify: k_verify_frames, two words per frame, no PCM written;
  (b) decode_compare    codec.DecoderN.decode into a second PCM buffer, then (back != pcm).reshape(n, -1).any(1) in torch.
Both are timed with device events in the same process, in alternating windows of at least --window seconds each after a
warm-up; the figure per version is the median over its windows of (window time / calls).  Run the command twice for the
spread.  Under `rocprofv3 --kernel-trace --stats -- python tools/verify_rate.py --window 0.1 --rounds 2` the per-kernel times
of k_verify_frames and k_decode_frames come out of the same run (no counters with the trace).

  python tools/verify_rate.py [--frames N] [--track T] [--window S] [--rounds R] [--out FILE]
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
    pcm_host = synth_frames(n, 2, a.track)
    blob, offs = codec.encode_host(pcm_host)
    frames = torch.from_numpy(blob).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    pcm = torch.from_numpy(pcm_host).cuda()
    ver = codec.Verifier(n, 2, 2048)
    dec = codec.DecoderN(n, 2, 2048)
    lossy_b = []

    def verify():
        ver.verify(frames, d_offs, n, pcm)

    def decode_compare():
        back, _ = dec.decode(frames, d_offs, n)
        lossy_b.append((back[: n * 2048].reshape(n, -1) != pcm.reshape(n, -1)).any(1))

    # both give the same answer
    verify()
    decode_compare()
    torch.cuda.synchronize()
    ver.check()
    dec.check()
    counts = ver.diff_counts[:n].cpu().numpy()
    assert np.array_equal(counts != 0, lossy_b[-1].cpu().numpy()), "the two versions disagree"
    assert ver.route() == 1 and dec.route() == 1
    res = {"frames": n, "track": a.track, "lossy_frames": int((counts != 0).sum()), "window_s": a.window, "rounds": a.rounds}
    fns = {"verify_ms": verify, "decode_compare_ms": decode_compare}
    calls = {}
    for k, fn in fns.items():  # warm-up, and how many calls fill a window
        _window_ms(fn, 20)
        lossy_b.clear()
        per_call = _window_ms(fn, 50)
        lossy_b.clear()
        calls[k] = max(1, int(a.window * 1e3 / per_call) + 1)
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():  # (alternating)
            times[k].append(_window_ms(fn, calls[k]))
            lossy_b.clear()
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
