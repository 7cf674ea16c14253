#!/usr/bin/env python3
"""What a window costs against the frames it touches.  On the bench's 3875-frame stereo track, on HIP events:
  (a) sela_hip_decode_windows_device: 256 windows of 16000 samples at seeded random starts;
  (b) sela_hip_decode_device on a table of exactly the frames (a)'s workgroups decode, window by window, duplicates included.
Both are warmed up; then `rounds` rounds alternate (a) and (b), each timing `calls` back-to-back calls between two events.
Prints one JSON line: the median, least and largest time per call of both, and the ratio of the medians.
Run on the GPU box:  python tools/window_bench.py [--rounds 15] [--calls 50]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, WINDOWS, WINDOW_SAMPLES, SEED, BLOCK = 3875, 2, 256, 16000, 20261018, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    import torch

    from sela_amd import codec, synth

    assert torch.cuda.is_available(), "window_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    pcm = synth.synth_frames_torch(FRAMES, CHANNELS, 0, device="cuda")
    enc = codec.Encoder(FRAMES, CHANNELS)
    out = enc.encode(pcm)
    torch.cuda.synchronize()
    out.check()
    stream, offs = out.to_host()

    rng = np.random.default_rng(SEED)
    starts = rng.integers(0, FRAMES * BLOCK - WINDOW_SAMPLES + 1, WINDOWS).astype(np.uint64)
    d_windows = torch.from_numpy(codec.WindowDecoder.pack(starts, 0, FRAMES)).cuda()
    # (b)'s table: the frames every window touches, in the windows' order
    touched = np.concatenate([np.arange(int(s) // BLOCK, (int(s) + WINDOW_SAMPLES - 1) // BLOCK + 1) for s in starts])
    sizes = np.diff(offs.astype(np.int64))
    table = np.concatenate([stream[int(offs[f]): int(offs[f + 1])] for f in touched])
    d_table = torch.from_numpy(table).cuda()
    d_table_offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes[touched])]).astype(np.int64)).cuda()
    n_table = len(touched)

    wd = codec.WindowDecoder(WINDOWS, WINDOW_SAMPLES, CHANNELS)
    dec = codec.Decoder(n_table, CHANNELS)
    call_a = lambda: wd.decode(out.frames, out.offsets, FRAMES, d_windows)  # noqa: E731
    call_b = lambda: dec.decode(d_table, d_table_offs, n_table)  # noqa: E731

    # the same samples: window w of (a) is a slice of its frames in (b)
    got, back = call_a().cpu().numpy(), call_b().cpu().numpy()
    torch.cuda.synchronize()
    wd.check(), dec.check()
    at = 0
    for w, s in enumerate(starts):
        k = (int(s) + WINDOW_SAMPLES - 1) // BLOCK + 1 - int(s) // BLOCK
        flat = back[at: at + k].reshape(k * BLOCK, CHANNELS)
        assert np.array_equal(got[w], flat[int(s) % BLOCK: int(s) % BLOCK + WINDOW_SAMPLES]), w
        at += k

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    for _ in range(3):
        timed(call_a), timed(call_b)
    ms_a, ms_b = [], []
    for _ in range(args.rounds):
        ms_a.append(timed(call_a))
        ms_b.append(timed(call_b))
    stats = lambda v: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(float(min(v)), 5), "max_ms": round(float(max(v)), 5)}  # noqa: E731
    print(json.dumps({
        "track_frames": FRAMES, "channels": CHANNELS, "windows": WINDOWS, "window_samples": WINDOW_SAMPLES, "seed": SEED,
        "frames_decoded": n_table, "launch_workgroups_a": WINDOWS * ((WINDOW_SAMPLES + 2046) // BLOCK + 1), "rounds": args.rounds, "calls_per_round": args.calls,
        "a_decode_windows_device": stats(ms_a), "b_decode_device_same_frames": stats(ms_b),
        "ratio_a_over_b": round(float(np.median(ms_a) / np.median(ms_b)), 4),
        "whole_track_frames_over_decoded": round(FRAMES / n_table, 3),
    }))


if __name__ == "__main__":
    main()
