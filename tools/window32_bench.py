#!/usr/bin/env python3
"""What the window call for 24- and 32-bit streams costs beside the any-length decoder it is built on.  The
bench's 3875-frame stereo track widened to 24 bits (shifted left 8, noise in the low byte), encoded on the device; tools/
window_bench.py's method: HIP events, `calls` back-to-back calls between two events, the calls alternating round by round, medians
with least and largest.
  (a) sela_hip_decode_i32_device on the whole table at stride 2048: the decoder alone, int32 planar by frame;
  (b) sela_hip_decode_windows_i32_device, SELA_HIP_WINDOW_I32_PLANAR, one window of 2048 samples per frame (every frame once);
  (c) sela_hip_decode_pcm_device on the whole table, 3 bytes a sample: the decoder and the pack kernel;
  (d) the window call, SELA_HIP_WINDOW_PCM24_INTERLEAVED, on (b)'s windows;
  (e), (f) the window call on 256 random crops of one second (44100 samples), I32_PLANAR and PCM24.
Writes one JSON line to profiles/windows/window32_bench.json and prints it.
Run on the GPU box:  python tools/window32_bench.py [--rounds 15] [--calls 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, CROPS, CROP_SAMPLES, SEED, BLOCK = 3875, 2, 256, 44100, 20261020, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows", "window32_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "window32_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    pcm16 = synth.synth_frames_torch(FRAMES, CHANNELS, 0, device="cuda")  # int16 [frames, 2048, channels]
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    wide = (pcm16.to(torch.int32) << 8) | torch.randint(0, 256, pcm16.shape, generator=gen, device="cuda", dtype=torch.int32)
    planar = wide.permute(0, 2, 1).contiguous()  # int32 [frames, channels, 2048]
    enc = codec.Encoder32(FRAMES, CHANNELS, BLOCK, lossless=True)
    frames, offsets, _ = enc.encode(planar)
    torch.cuda.synchronize()
    enc.check()

    dec32 = codec.Decoder32(FRAMES, CHANNELS, BLOCK)
    decpcm = codec.DecoderPcm(FRAMES, CHANNELS, BLOCK, 3)
    every = torch.from_numpy(codec.WindowDecoder32.pack(np.arange(FRAMES, dtype=np.uint64) * BLOCK, 0, FRAMES)).cuda()
    rng = np.random.default_rng(SEED)
    crops = torch.from_numpy(codec.WindowDecoder32.pack(rng.integers(0, FRAMES * BLOCK - CROP_SAMPLES + 1, CROPS).astype(np.uint64), 0, FRAMES)).cuda()
    win_i32 = codec.WindowDecoder32(FRAMES, BLOCK, CHANNELS, capi.WINDOW_I32_PLANAR)
    win_p24 = codec.WindowDecoder32(FRAMES, BLOCK, CHANNELS, capi.WINDOW_PCM24_INTERLEAVED)
    crop_i32 = codec.WindowDecoder32(CROPS, CROP_SAMPLES, CHANNELS, capi.WINDOW_I32_PLANAR)
    crop_p24 = codec.WindowDecoder32(CROPS, CROP_SAMPLES, CHANNELS, capi.WINDOW_PCM24_INTERLEAVED)
    calls = [("a_decode_i32_device", lambda: dec32.decode(frames, offsets, FRAMES)), ("b_windows_i32_planar", lambda: win_i32.decode(frames, offsets, FRAMES, every)),
             ("c_decode_pcm24_device", lambda: decpcm.decode(frames, offsets, FRAMES)), ("d_windows_pcm24", lambda: win_p24.decode(frames, offsets, FRAMES, every)),
             ("e_crops_i32_planar", lambda: crop_i32.decode(frames, offsets, FRAMES, crops)), ("f_crops_pcm24", lambda: crop_p24.decode(frames, offsets, FRAMES, crops))]

    # the same samples from all of them: the track itself (the encode is lossless)
    got = {name: call() for name, call in calls}
    torch.cuda.synchronize()
    dec32.check(), decpcm.check(), win_i32.check(), win_p24.check(), crop_i32.check(), crop_p24.check()
    assert torch.equal(got["a_decode_i32_device"][0], planar) and torch.equal(got["b_windows_i32_planar"], planar)
    packed = torch.stack([((wide >> (8 * k)) & 0xFF).to(torch.uint8) for k in range(3)], dim=-1)  # [frames, 2048, channels, 3]
    assert torch.equal(got["c_decode_pcm24_device"][0].view(FRAMES, BLOCK, CHANNELS, 3), packed) and torch.equal(got["d_windows_pcm24"], packed)
    flat = wide.reshape(FRAMES * BLOCK, CHANNELS)
    starts = crops.cpu().numpy()[:, 0]
    for w in (0, CROPS // 2, CROPS - 1):
        seg = flat[int(starts[w]): int(starts[w]) + CROP_SAMPLES]
        assert torch.equal(got["e_crops_i32_planar"][w], seg.t()) and torch.equal(got["f_crops_pcm24"][w], torch.stack([((seg >> (8 * k)) & 0xFF).to(torch.uint8) for k in range(3)], dim=-1))
    touched = int(sum((int(s) % BLOCK + CROP_SAMPLES - 1) // BLOCK + 1 for s in starts))

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    for _ in range(3):
        for _, call in calls:
            timed(call)
    ms = {name: [] for name, _ in calls}
    for _ in range(args.rounds):
        for name, call in calls:
            ms[name].append(timed(call))
    stats = lambda v: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(float(min(v)), 5), "max_ms": round(float(max(v)), 5)}  # noqa: E731
    med = {name: float(np.median(v)) for name, v in ms.items()}
    result = {"track_frames": FRAMES, "channels": CHANNELS, "sample_bits": 24, "stream_bytes": int(offsets[FRAMES].item()), "windows_every_frame": FRAMES, "window_samples": BLOCK,
              "crops": CROPS, "crop_samples": CROP_SAMPLES, "crop_frames_touched": touched, "seed": SEED, "rounds": args.rounds, "calls_per_round": args.calls}
    result.update({name: stats(v) for name, v in ms.items()})
    result["ratio_b_over_a"] = round(med["b_windows_i32_planar"] / med["a_decode_i32_device"], 4)
    result["ratio_d_over_c"] = round(med["d_windows_pcm24"] / med["c_decode_pcm24_device"], 4)
    result["ratio_d_over_b"] = round(med["d_windows_pcm24"] / med["b_windows_i32_planar"], 4)
    result["crops_i32_us_per_frame_touched"] = round(1000 * med["e_crops_i32_planar"] / touched, 4)
    result["every_frame_i32_us_per_frame"] = round(1000 * med["b_windows_i32_planar"] / FRAMES, 4)
    result["ratio_f_over_e"] = round(med["f_crops_pcm24"] / med["e_crops_i32_planar"], 4)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
