#!/usr/bin/env python3
"""What whole 24-bit tracks cost.  The bench's 3875-frame stereo track widened to 24 bits (shifted left 8, noise in
the low byte) plus a tail of 777 samples, packed 3 bytes a sample.  tools/pcm_bench.py's and tools/window32_bench.py's method: HIP
events, `calls` back-to-back calls between two events, the calls of a group taking turns round by round, medians with least and largest.
  (a) sela_hip_encode_whole_pcm_device on the whole track, against sela_hip_encode_pcm_device on its 3875 whole frames alone and on
      the last frame (2825 samples) alone -- the tail's four launches.  A whole call that costs what the two cost in series has a
      fork that does not work: "fork_hides_the_tail" says whether it costs less.
  (b) sela_hip_decode_windows_i32_whole_device on the tailed table -- windows covering every frame once, and 256 random crops of one
      second, int32 planar and packed 24-bit -- against sela_hip_decode_windows_i32_device on the cut table (3875 frames of 2048);
      and on the cut table itself, where every word must equal the plain call's.
  (c) sela_hip_decode_pcm_device on the tailed stream (stride 4095) against the cut one (stride 2048): times and workspace bytes.
  (d) the untouched calls against another build of the library (--parent-lib: the parent commit's libsela_hip.so) in this process:
      sela_hip_encode_pcm_device, sela_hip_decode_windows_i32_device, sela_hip_decode_windows_whole_device,
      sela_hip_encode_whole_device.  Each must sit inside the parent's own spread between repeats, (largest - least) / median.
Prints one JSON line and writes it to --out (default profiles/whole/whole_pcm_bench.json).  Without --parent-lib (d) is not measured,
nothing is written and the exit code is 2; a call of (d) slower than the parent's by more than the parent's spread: exit code 1.
Run on the GPU box:  python tools/whole_pcm_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 15] [--calls 10]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, TAIL, CHANNELS, BLOCK, BYTES, TRACK, CROPS, CROP_SAMPLES, SEED = 3875, 777, 2, 2048, 3, 0, 256, 44100, 20261020


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whole", "whole_pcm_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "whole_pcm_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
    n = FRAMES * BLOCK + TAIL
    last = BLOCK + TAIL  # the long last frame: frames 0 .. FRAMES - 2 of 2048 samples in front of it
    pcm16 = synth.synth_pcm_torch(n, CHANNELS, TRACK, device="cuda").contiguous()  # int16 [n, channels]
    gen = torch.Generator(device="cuda").manual_seed(0x5E1A)
    wide = (pcm16.to(torch.int32) << 8) | torch.randint(0, 256, pcm16.shape, generator=gen, device="cuda", dtype=torch.int32)

    def packed_of(x):
        return torch.stack([(x >> (8 * k)) & 0xFF for k in range(BYTES)], dim=-1).to(torch.uint8).reshape(-1).contiguous()

    d_packed = packed_of(wide)
    value = CHANNELS * BYTES
    d_tail_packed = d_packed[(FRAMES - 1) * BLOCK * value:]
    d_cut_packed = d_packed[: FRAMES * BLOCK * value]

    def on_device(frames_offsets):
        """Encoder.to_host()'s pair back on the device, the offsets as the int64 the calls take"""
        frames, offsets = frames_offsets
        return torch.from_numpy(np.ascontiguousarray(frames)).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda()

    # ---- (a) the encodes ---------------------------------------------------------------------------------------------------------
    enc_whole = codec.WholeEncoderPcm(n, CHANNELS, BYTES, lossless=True)
    enc_cut = codec.EncoderPcm(FRAMES, CHANNELS, BLOCK, BYTES, lossless=True)
    enc_tail = codec.EncoderPcm(1, CHANNELS, last, BYTES, lossless=True)
    enc_whole.encode(d_packed)
    tailed, tailed_offs = on_device(enc_whole.to_host())
    enc_cut.encode(d_cut_packed)
    cut, cut_offs = on_device(enc_cut.to_host())
    enc_tail.encode(d_tail_packed)
    tail_frame, _ = enc_tail.to_host()
    at = int(tailed_offs[FRAMES - 1].item())
    assert torch.equal(tailed[:at], cut[:at]) and bytes(tailed[at:].cpu().numpy()) == bytes(tail_frame), "the whole call's stream is not the two calls' frames"
    pad = torch.zeros(8, dtype=torch.uint8, device="cuda")
    tailed, cut = torch.cat([tailed, pad]), torch.cat([cut, pad])

    # ---- (b) the windows ---------------------------------------------------------------------------------------------------------
    pack = codec.WindowDecoder32.pack
    every_tailed = torch.from_numpy(pack(np.arange(FRAMES + 1, dtype=np.uint64) * BLOCK, 0, FRAMES)).cuda()  # the last window: the tail's samples behind 2048
    every_cut = torch.from_numpy(pack(np.arange(FRAMES, dtype=np.uint64) * BLOCK, 0, FRAMES)).cuda()
    rng = np.random.default_rng(SEED)
    crops_tailed = torch.from_numpy(pack(rng.integers(0, n - CROP_SAMPLES + 1, CROPS).astype(np.uint64), 0, FRAMES)).cuda()
    crops_cut = torch.from_numpy(pack(rng.integers(0, FRAMES * BLOCK - CROP_SAMPLES + 1, CROPS).astype(np.uint64), 0, FRAMES)).cuda()
    I32, P24 = capi.WINDOW_I32_PLANAR, capi.WINDOW_PCM24_INTERLEAVED
    calls = {}
    decoders = {}
    for fmt, tag in ((I32, "i32"), (P24, "pcm24")):
        for kind, ws, count, wt, wc in (("every", BLOCK, FRAMES + 1, every_tailed, every_cut), ("crops", CROP_SAMPLES, CROPS, crops_tailed, crops_cut)):
            whole_t = codec.WindowDecoder32(count, ws, CHANNELS, fmt, whole=True)
            whole_c = codec.WindowDecoder32(count, ws, CHANNELS, fmt, whole=True)
            plain_c = codec.WindowDecoder32(count, ws, CHANNELS, fmt)
            decoders["%s_%s" % (kind, tag)] = (whole_t, whole_c, plain_c, wt, wc)
            calls["b_%s_%s_whole_tailed" % (kind, tag)] = lambda d=whole_t, w=wt: d.decode(tailed, tailed_offs, FRAMES, w)
            calls["b_%s_%s_whole_cut" % (kind, tag)] = lambda d=whole_c, w=wc: d.decode(cut, cut_offs, FRAMES, w)
            calls["b_%s_%s_plain_cut" % (kind, tag)] = lambda d=plain_c, w=wc: d.decode(cut, cut_offs, FRAMES, w)

    # ---- (c) the full decodes ------------------------------------------------------------------------------------------------------
    dec_tailed = codec.DecoderPcm(FRAMES, CHANNELS, 4095, BYTES)  # (the stride of a caller that knows the rule and not the track)
    dec_cut = codec.DecoderPcm(FRAMES, CHANNELS, BLOCK, BYTES)
    calls["c_decode_pcm_tailed_stride_4095"] = lambda: dec_tailed.decode(tailed, tailed_offs, FRAMES)
    calls["c_decode_pcm_cut_stride_2048"] = lambda: dec_cut.decode(cut, cut_offs, FRAMES)
    calls["a_encode_whole_pcm"] = lambda: enc_whole.encode(d_packed)
    calls["a_encode_pcm_3875_frames"] = lambda: enc_cut.encode(d_cut_packed)
    calls["a_encode_pcm_tail_alone"] = lambda: enc_tail.encode(d_tail_packed)

    # ---- (d) the untouched calls, this build and the parent's ------------------------------------------------------------------------
    def buffers(n_bytes):
        return torch.empty(n_bytes, dtype=torch.uint8, device="cuda")

    enc16 = codec.WholeEncoder(n, CHANNELS)
    enc16.encode(pcm16)
    stream16, offs16 = on_device(enc16.to_host())
    stream16 = torch.cat([stream16, pad])
    cap = FRAMES * ((BLOCK * CHANNELS * 9) // 2 + CHANNELS * 192 + 64)

    class Untouched:
        """the four calls on one build of the library, each on buffers of its own"""

        def __init__(self, L):
            self.L = L
            for name, argtypes in (("sela_hip_encode_pcm_workspace_bytes", [u32] * 3), ("sela_hip_decode_windows_i32_workspace_bytes", [u32] * 3),
                                   ("sela_hip_decode_windows_whole_workspace_bytes", [u32] * 3), ("sela_hip_encode_whole_workspace_bytes", [u64, u32])):
                getattr(L, name).restype, getattr(L, name).argtypes = sz, argtypes
            self.frames, self.frames16 = buffers(cap), buffers(cap)
            self.offsets, self.offsets16 = (torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda") for _ in range(2))
            self.status = torch.zeros(4, 4, dtype=torch.int32, device="cuda")
            self.flags = torch.zeros(2, CROPS, dtype=torch.int32, device="cuda")
            self.ws = [buffers(int(L.sela_hip_encode_pcm_workspace_bytes(FRAMES, CHANNELS, BLOCK))), buffers(int(L.sela_hip_decode_windows_i32_workspace_bytes(CROPS, CROP_SAMPLES, CHANNELS))),
                       buffers(int(L.sela_hip_decode_windows_whole_workspace_bytes(CROPS, CROP_SAMPLES, CHANNELS))), buffers(int(L.sela_hip_encode_whole_workspace_bytes(n, CHANNELS)))]
            self.out32 = torch.empty((CROPS, CHANNELS, CROP_SAMPLES), dtype=torch.int32, device="cuda")
            self.out16 = torch.empty((CROPS, CROP_SAMPLES, CHANNELS), dtype=torch.int16, device="cuda")

        def encode_pcm(self):
            assert self.L.sela_hip_encode_pcm_device(vp(d_packed.data_ptr()), u32(BYTES), u32(FRAMES), u32(CHANNELS), u32(BLOCK), u32(0), vp(self.frames.data_ptr()), sz(cap),
                                                     vp(self.offsets.data_ptr()), vp(self.status[0].data_ptr()), vp(self.ws[0].data_ptr()), sz(self.ws[0].numel()), vp(stream)) == 0

        def windows_i32(self):
            assert self.L.sela_hip_decode_windows_i32_device(vp(cut.data_ptr()), vp(cut_offs.data_ptr()), u32(FRAMES), u32(CHANNELS), vp(crops_cut.data_ptr()), u32(CROPS),
                                                             u32(CROP_SAMPLES), u32(I32), u32(24), vp(self.out32.data_ptr()), vp(self.flags[0].data_ptr()), vp(self.status[1].data_ptr()),
                                                             vp(self.ws[1].data_ptr()), sz(self.ws[1].numel()), vp(stream)) == 0

        def windows_whole(self):
            assert self.L.sela_hip_decode_windows_whole_device(vp(stream16.data_ptr()), vp(offs16.data_ptr()), u32(FRAMES), u32(CHANNELS), vp(crops_tailed.data_ptr()), u32(CROPS),
                                                               u32(CROP_SAMPLES), u32(0), vp(self.out16.data_ptr()), vp(self.flags[1].data_ptr()), vp(self.status[2].data_ptr()),
                                                               vp(self.ws[2].data_ptr()), sz(self.ws[2].numel()), vp(stream)) == 0

        def encode_whole(self):
            assert self.L.sela_hip_encode_whole_device(vp(pcm16.data_ptr()), u64(n), u32(CHANNELS), vp(self.frames16.data_ptr()), sz(cap), vp(self.offsets16.data_ptr()),
                                                       vp(self.status[3].data_ptr()), vp(self.ws[3].data_ptr()), sz(self.ws[3].numel()), vp(stream), u32(0)) == 0

        def words(self):
            torch.cuda.synchronize()
            return [self.frames[: int(self.offsets[FRAMES].item())].clone(), self.offsets.clone(), self.out32.clone(), self.out16.clone(),
                    self.frames16[: int(self.offsets16[FRAMES].item())].clone(), self.offsets16.clone(), self.status.clone(), self.flags.clone()]

    KINDS = ("encode_pcm", "windows_i32", "windows_whole", "encode_whole")
    builds = {"this": Untouched(lib)}
    if args.parent_lib:
        builds["parent"] = Untouched(C.CDLL(os.path.abspath(args.parent_lib)))
    for who, u in builds.items():
        for kind in KINDS:
            calls["d_%s_%s" % (who, kind)] = getattr(u, kind)

    # ---- everything once, and what it must hold ------------------------------------------------------------------------------------
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    flat = wide  # [n, channels]: the encodes are lossless, so every decode is the track
    for name, (whole_t, whole_c, plain_c, wt, wc) in decoders.items():
        whole_t.check(), whole_c.check(), plain_c.check()
        k = plain_c.n_windows
        assert torch.equal(whole_c.out[:k], plain_c.out[:k]) and torch.equal(whole_c.flags, plain_c.flags) and torch.equal(whole_c.status, plain_c.status), \
            name + ": on the cut table a word differs from the plain call's"
        starts = wt.cpu().numpy()[:, 0]
        ws = whole_t.window_samples
        for w in (0, len(starts) // 2, len(starts) - 1):
            seg = flat[int(starts[w]): int(starts[w]) + ws]
            seg = torch.cat([seg, torch.zeros((ws - seg.shape[0], CHANNELS), dtype=torch.int32, device="cuda")])
            want = seg.t() if whole_t.format == I32 else torch.stack([((seg >> (8 * k)) & 0xFF).to(torch.uint8) for k in range(3)], dim=-1)
            assert torch.equal(whole_t.out[w], want), (name, w)
    dec_tailed.check(), dec_cut.check()
    assert torch.equal(dec_tailed.pcm[: n * value], d_packed) and torch.equal(dec_cut.pcm[: FRAMES * BLOCK * value], d_cut_packed)
    if args.parent_lib:
        for a, b in zip(builds["this"].words(), builds["parent"].words()):
            assert torch.equal(a, b), "an untouched call's words differ from the parent's"

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    groups = [("a_encode_whole_pcm", "a_encode_pcm_3875_frames", "a_encode_pcm_tail_alone"), tuple(k for k in calls if k.startswith("c_"))]
    groups += [tuple(k for k in calls if k.startswith("b_%s_%s_" % (kind, tag))) for tag in ("i32", "pcm24") for kind in ("every", "crops")]
    groups += [tuple("d_%s_%s" % (who, kind) for who in builds) for kind in KINDS]
    ms = {k: [] for k in calls}
    for r in range(args.rounds):  # (the calls of a group take turns at going first)
        for group in groups:
            for k in group[r % len(group):] + group[: r % len(group)]:
                ms[k].append(timed(calls[k]))
    stats = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}  # noqa: E731
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {"frames": FRAMES, "tail_samples": TAIL, "last_frame_samples": last, "channels": CHANNELS, "bytes_per_sample": BYTES, "lossless": True,
            "input": "synth_pcm_torch(3875 * 2048 + 777, 2, track=0) << 8 | noise byte, packed", "rounds": args.rounds, "calls_per_round": args.calls,
            "stream_bytes_tailed": int(tailed.numel() - 8), "stream_bytes_cut": int(cut.numel() - 8), "windows_every_frame": FRAMES + 1, "crops": CROPS, "crop_samples": CROP_SAMPLES}
    line.update({k: stats(v) for k, v in ms.items() if not k.startswith("d_")})
    serial = med["a_encode_pcm_3875_frames"] + med["a_encode_pcm_tail_alone"]
    line["a_whole_over_3875_frames"] = round(med["a_encode_whole_pcm"] / med["a_encode_pcm_3875_frames"], 4)
    line["a_whole_over_the_two_in_series"] = round(med["a_encode_whole_pcm"] / serial, 4)
    line["a_fork_hides_the_tail"] = bool(med["a_encode_whole_pcm"] < serial)
    for tag in ("i32", "pcm24"):
        for kind in ("every", "crops"):
            base = "b_%s_%s_" % (kind, tag)
            line[base + "whole_tailed_over_plain_cut"] = round(med[base + "whole_tailed"] / med[base + "plain_cut"], 4)
            line[base + "whole_cut_over_plain_cut"] = round(med[base + "whole_cut"] / med[base + "plain_cut"], 4)
    line["c_tailed_over_cut"] = round(med["c_decode_pcm_tailed_stride_4095"] / med["c_decode_pcm_cut_stride_2048"], 4)
    line["c_workspace_bytes_tailed"] = int(lib.sela_hip_decode_pcm_workspace_bytes(FRAMES, CHANNELS, 4095))
    line["c_workspace_bytes_cut"] = int(lib.sela_hip_decode_pcm_workspace_bytes(FRAMES, CHANNELS, BLOCK))
    line["c_output_room_bytes_tailed"], line["c_output_room_bytes_cut"] = FRAMES * 4095 * value, FRAMES * BLOCK * value
    slow = []
    for kind in KINDS:
        line["d_this_" + kind] = stats(ms["d_this_" + kind])
        if args.parent_lib:
            p = ms["d_parent_" + kind]
            spread = (max(p) - min(p)) / med["d_parent_" + kind]
            slower = med["d_this_" + kind] / med["d_parent_" + kind] - 1.0
            line["d_parent_" + kind] = stats(p)
            line["d_" + kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread, 4), "within_parent_spread": bool(slower <= spread)}
            if slower > spread:
                slow.append(kind)
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("no --parent-lib: figure (d) was not measured, so this is not the record of DESIGN.md 5.25 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    for k in slow:
        print("REQUIRED CONDITION MISSED: %s: this tree over the parent %.4f, the parent's spread %.4f" % (k, line["d_" + k]["this_over_parent"], line["d_" + k]["parent_spread"]))
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
