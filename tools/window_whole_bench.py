#!/usr/bin/env python3
"""What the whole-track window call costs beside the window call it is built on.  tools/window_bench.py's table
(the bench's 3875-frame stereo track), windows (256 of 16000 samples at its seeded starts) and method: HIP events, `calls`
back-to-back calls between two events, the calls alternating round by round, medians with least and largest.
  (a) sela_hip_decode_windows_device of ANOTHER build of the library (--parent-lib: the parent commit's), same buffers;
  (b) this tree's same call;
  (c) sela_hip_decode_windows_whole_device on the same table of 2048-sample frames: the plan kernel and two launches that
      return at once are its excess;
  (d) the whole call on whole-track streams: the track cut into 31 tracks of 124 frames and a last frame of 2048 + 777 samples,
      the same number of windows, `TAIL_SHARE` of them placed so that they reach their track's last frame.
Prints one JSON line.  Run on the GPU box:  python tools/window_whole_bench.py [--parent-lib PATH] [--rounds 15] [--calls 50]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, WINDOWS, WINDOW_SAMPLES, SEED, BLOCK = 3875, 2, 256, 16000, 20261018, 2048
TRACK_FRAMES, TAIL, TAIL_SHARE = 125, 777, 0.25  # a track: 124 frames of 2048 samples and one of 2048 + 777


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "window_whole_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    pcm = synth.synth_frames_torch(FRAMES, CHANNELS, 0, device="cuda")
    enc = codec.Encoder(FRAMES, CHANNELS)
    out = enc.encode(pcm)
    torch.cuda.synchronize()
    out.check()

    rng = np.random.default_rng(SEED)
    starts = rng.integers(0, FRAMES * BLOCK - WINDOW_SAMPLES + 1, WINDOWS).astype(np.uint64)
    d_windows = torch.from_numpy(codec.WindowDecoder.pack(starts, 0, FRAMES)).cuda()
    plain = codec.WindowDecoder(WINDOWS, WINDOW_SAMPLES, CHANNELS)
    whole = codec.WindowDecoder(WINDOWS, WINDOW_SAMPLES, CHANNELS, whole=True)
    call_b = lambda: plain.decode(out.frames, out.offsets, FRAMES, d_windows)  # noqa: E731
    call_c = lambda: whole.decode(out.frames, out.offsets, FRAMES, d_windows)  # noqa: E731

    # (d) whole-track streams: tracks of the same samples, each with a tail, back to back in one table
    flat = pcm.reshape(FRAMES * BLOCK, CHANNELS).cpu().numpy()
    track_samples = TRACK_FRAMES * BLOCK + TAIL
    n_tracks = (FRAMES * BLOCK) // track_samples
    blobs, offs = [], [0]
    for k in range(n_tracks):
        fr, fo = codec.encode_whole_host(flat[k * track_samples: (k + 1) * track_samples])
        assert len(fo) - 1 == TRACK_FRAMES
        at = offs[-1]
        offs += [at + int(x) for x in fo[1:]]
        blobs.append(fr)
    d_tracks = torch.from_numpy(np.concatenate(blobs)).cuda()
    d_track_offs = torch.from_numpy(np.asarray(offs, dtype=np.int64)).cuda()
    n_tail = int(WINDOWS * TAIL_SHARE)
    track_of = rng.integers(0, n_tracks, WINDOWS)
    t_starts = rng.integers(0, (TRACK_FRAMES - 1) * BLOCK - WINDOW_SAMPLES + 1, WINDOWS)          # in front of the last frame
    t_starts[:n_tail] = rng.integers(track_samples - WINDOW_SAMPLES, track_samples - 1, n_tail)   # ... or reaching into it
    order = rng.permutation(WINDOWS)
    track_of, t_starts = track_of[order], t_starts[order]
    d_track_windows = torch.from_numpy(codec.WindowDecoder.pack(t_starts.astype(np.uint64), (track_of * TRACK_FRAMES).astype(np.uint64), TRACK_FRAMES)).cuda()
    tailed = codec.WindowDecoder(WINDOWS, WINDOW_SAMPLES, CHANNELS, whole=True)
    call_d = lambda: tailed.decode(d_tracks, d_track_offs, n_tracks * TRACK_FRAMES, d_track_windows)  # noqa: E731

    # (a) another build's window call, through its own handle, on (b)'s buffers
    call_a = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        vp, u32 = C.c_void_p, C.c_uint32
        parent.sela_hip_decode_windows_device.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, vp, vp, vp, vp, C.c_size_t, vp]
        parent.sela_hip_decode_windows_device.restype = C.c_int
        a_out, a_flags, a_status = torch.empty_like(plain.out), torch.zeros_like(plain.window_flags), torch.zeros_like(plain.status)
        a_ws = torch.empty_like(plain.workspace)

        def call_a():
            rc = parent.sela_hip_decode_windows_device(out.frames.data_ptr(), out.offsets.data_ptr(), FRAMES, CHANNELS, d_windows.data_ptr(), WINDOWS, WINDOW_SAMPLES,
                                                       capi.WINDOW_I16_INTERLEAVED, a_out.data_ptr(), a_flags.data_ptr(), a_status.data_ptr(), a_ws.data_ptr(), a_ws.numel(),
                                                       torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
            return a_out

    # the same samples from (a), (b) and (c); (d) against the any-length decoder on one track
    got_b, got_c = call_b().cpu().numpy(), call_c().cpu().numpy()
    torch.cuda.synchronize()
    plain.check(), whole.check()
    assert np.array_equal(got_b, got_c) and torch.equal(plain.status, whole.status)
    if call_a:
        assert np.array_equal(call_a().cpu().numpy(), got_b)
    got_d = call_d().cpu().numpy()
    tailed.check()
    dn = codec.DecoderN(TRACK_FRAMES, CHANNELS, BLOCK + TAIL)
    w = int(np.flatnonzero(t_starts + WINDOW_SAMPLES > (TRACK_FRAMES - 1) * BLOCK)[0])
    k = int(track_of[w])
    one_frames = d_tracks[int(offs[k * TRACK_FRAMES]): int(offs[(k + 1) * TRACK_FRAMES])].clone()
    one_offs = (d_track_offs[k * TRACK_FRAMES: (k + 1) * TRACK_FRAMES + 1] - d_track_offs[k * TRACK_FRAMES]).contiguous()
    track_pcm, _ = dn.decode(one_frames, one_offs, TRACK_FRAMES)
    torch.cuda.synchronize()
    dn.check()
    want = np.zeros((WINDOW_SAMPLES, CHANNELS), np.int16)
    seg = track_pcm.cpu().numpy()[: track_samples][int(t_starts[w]): int(t_starts[w]) + WINDOW_SAMPLES]
    want[: len(seg)] = seg
    assert np.array_equal(got_d[w], want), w
    reach = int((t_starts + WINDOW_SAMPLES > (TRACK_FRAMES - 1) * BLOCK).sum())

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    calls = [("a_parent_decode_windows_device", call_a), ("b_decode_windows_device", call_b), ("c_whole_on_2048_frames", call_c), ("d_whole_on_tailed_streams", call_d)]
    calls = [(name, call) for name, call in calls if call]
    for _ in range(3):
        for _, call in calls:
            timed(call)
    ms = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, call in calls:
            ms[name].append(timed(call))
    stats = lambda v: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(float(min(v)), 5), "max_ms": round(float(max(v)), 5)}  # noqa: E731
    med = {name: float(np.median(v)) for name, v in ms.items()}
    result = {"track_frames": FRAMES, "channels": CHANNELS, "windows": WINDOWS, "window_samples": WINDOW_SAMPLES, "seed": SEED, "rounds": args.rounds,
              "calls_per_round": args.calls, "tailed_tracks": n_tracks, "tailed_track_frames": TRACK_FRAMES, "tail_samples": TAIL, "windows_reaching_a_tail": reach}
    result.update({name: stats(v) for name, v in ms.items()})
    base = "a_parent_decode_windows_device" if call_a else "b_decode_windows_device"
    result["ratio_c_over_" + base[0]] = round(med["c_whole_on_2048_frames"] / med[base], 4)
    result["excess_c_us"] = round(1000 * (med["c_whole_on_2048_frames"] - med[base]), 2)
    result["ratio_d_over_c"] = round(med["d_whole_on_tailed_streams"] / med["c_whole_on_2048_frames"], 4)
    if call_a:
        result["ratio_b_over_a"] = round(med["b_decode_windows_device"] / med[base], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
