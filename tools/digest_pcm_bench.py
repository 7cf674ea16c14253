#!/usr/bin/env python3
"""What the digest of a 24- or 32-bit stream costs on the device, on tools/digest_bench.py's protocol.  The input
is the bench's synthetic track (3875 stereo frames of 2048 samples, track 0) widened to 24 bits (the int16 samples times 256, eight
bits of noise below them), encoded lossless by sela_hip_encode_pcm_device, in device memory.  On HIP events, everything warmed up,
`rounds` rounds that alternate the calls, each timing `calls` back-to-back calls between two events; medians with the least and
the largest:
  (a) sela_hip_digest_pcm_device for a 3- and a 4-byte container (no decoded byte reaches memory) against the parent build's
      sela_hip_decode_pcm_device and sela_hip_levels_i32_device on the same frames, and against the COMPOSITE that was the only way
      to the same number before: sela_hip_decode_pcm_device, then sela_hip_crc32_device over what it wrote.  The condition: the new
      call's median lies at or below the composite's median plus the composite's own least-to-largest spread;
  (b) the calls this change does not touch, or touches only by an argument of the fold kernels -- sela_hip_digest_device (on the
      16-bit track), sela_hip_levels_i32_device, sela_hip_verify_pcm_device, sela_hip_decode_pcm_device -- from this build against
      the parent's (--parent-lib: the parent commit's libsela_hip.so): they must lie within the parent's own spread.
Before anything is timed the records and the track words are held against zlib on the bytes the decode call writes, and the
composite's figure against both.  Prints one JSON line and writes it to --out (default profiles/digest/digest_pcm_bench.json).
Without --parent-lib nothing is written and the exit code is 2; where the condition of (a) or (b) fails the exit code is 1.
Run on the GPU box:  python tools/digest_pcm_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 20] [--calls 10]"""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, BLOCK, TRACK = 3875, 2, 2048, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, help="time this one call and nothing else (for a counter run); nothing is written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest", "digest_pcm_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "digest_pcm_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    nf = args.frames
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t

    # the track: int16, and widened to 24 bits as packed 3-byte samples
    d_pcm16 = synth.synth_frames_torch(nf, CHANNELS, TRACK, device="cuda").contiguous()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(29)
    wide = (d_pcm16.to(torch.int32) << 8) | torch.randint(0, 256, d_pcm16.shape, generator=gen, device="cuda", dtype=torch.int32)
    packed = torch.stack([(wide >> (8 * k)) & 0xFF for k in range(3)], dim=-1).to(torch.uint8).reshape(-1).contiguous()
    enc = codec.EncoderPcm(nf, CHANNELS, BLOCK, 3, lossless=True)
    enc.encode(packed)
    enc.check()
    frames_h, offs_h = enc.to_host()
    d_frames = torch.from_numpy(np.concatenate([frames_h, np.zeros(8, np.uint8)])).cuda()
    d_offs = torch.from_numpy(np.ascontiguousarray(offs_h).view(np.int64).copy()).cuda()
    out16 = codec.Encoder(nf, CHANNELS).encode(d_pcm16)
    torch.cuda.synchronize()
    frames16_h, offs16_h = out16.to_host()
    d_frames16 = torch.from_numpy(np.concatenate([frames16_h, np.zeros(8, np.uint8)])).cuda()
    d_offs16 = torch.from_numpy(offs16_h.view(np.int64).copy()).cuda()

    def buffers(n_bytes):
        return torch.empty(max(n_bytes, 1), dtype=torch.uint8, device="cuda")

    def workspace(L, name):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = sz, [u32] * 3
        return buffers(int(fn(nf, CHANNELS, BLOCK)))

    class DecodePcm:  # sela_hip_decode_pcm_device
        def __init__(self, L, b):
            self.L, self.b = L, b
            self.ws = workspace(L, "sela_hip_decode_pcm_workspace_bytes")
            self.pcm = torch.zeros(nf * BLOCK * CHANNELS * b, dtype=torch.uint8, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_decode_pcm_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), u32(self.b),
                                                   vp(self.pcm.data_ptr()), vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.pcm, self.status

    class Composite:  # sela_hip_decode_pcm_device, then sela_hip_crc32_device over what it wrote
        def __init__(self, L, b):
            self.L, self.decode = L, DecodePcm(L, b)
            L.sela_hip_crc32_workspace_bytes.restype, L.sela_hip_crc32_workspace_bytes.argtypes = sz, [u64]
            self.ws = buffers(int(L.sela_hip_crc32_workspace_bytes(self.decode.pcm.numel())))
            self.out = torch.zeros(2, dtype=torch.int64, device="cuda")

        def __call__(self):
            self.decode()
            rc = self.L.sela_hip_crc32_device(vp(self.decode.pcm.data_ptr()), u64(self.decode.pcm.numel()), vp(self.out.data_ptr()), vp(self.ws.data_ptr()),
                                              sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.out, self.decode.status

    class Levels32:  # sela_hip_levels_i32_device
        def __init__(self, L):
            self.L = L
            self.ws = workspace(L, "sela_hip_levels_i32_workspace_bytes")
            self.levels = torch.zeros((nf, CHANNELS, 4), dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_levels_i32_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(self.levels.data_ptr()),
                                                   vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.levels, self.status

    class VerifyPcm:  # sela_hip_verify_pcm_device against the packed bytes the track was made from
        def __init__(self, L):
            self.L = L
            self.ws = workspace(L, "sela_hip_verify_pcm_workspace_bytes")
            self.counts, self.first = torch.zeros(nf, dtype=torch.int32, device="cuda"), torch.zeros(nf, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_verify_pcm_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(packed.data_ptr()), u32(3),
                                                   u64(nf * BLOCK), vp(self.counts.data_ptr()), vp(self.first.data_ptr()), vp(None), vp(self.status.data_ptr()),
                                                   vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.counts, self.first, self.status

    class Digest16:  # sela_hip_digest_device on the int16 track
        def __init__(self, L):
            self.L = L
            self.ws = workspace(L, "sela_hip_digest_workspace_bytes")
            self.digests = torch.zeros(nf, dtype=torch.int64, device="cuda")
            self.track = torch.zeros(2, dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_digest_device(vp(d_frames16.data_ptr()), vp(d_offs16.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(self.digests.data_ptr()),
                                               vp(self.track.data_ptr()), vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.digests, self.track, self.status

    dig = {b: codec.DigesterPcm(nf, CHANNELS, BLOCK, b) for b in (3, 4)}
    calls = {"digest_pcm_3": lambda: dig[3].digest(d_frames, d_offs, nf), "digest_pcm_4": lambda: dig[4].digest(d_frames, d_offs, nf),
             "composite_3": Composite(lib, 3), "composite_4": Composite(lib, 4),
             "decode_pcm": DecodePcm(lib, 3), "levels_i32": Levels32(lib), "verify_pcm": VerifyPcm(lib), "digest": Digest16(lib)}
    untouched = ("decode_pcm", "levels_i32", "verify_pcm", "digest")
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls.update({"parent_decode_pcm": DecodePcm(parent, 3), "parent_levels_i32": Levels32(parent), "parent_verify_pcm": VerifyPcm(parent),
                      "parent_digest": Digest16(parent), "parent_composite_3": Composite(parent, 3), "parent_composite_4": Composite(parent, 4)})
    if args.only:
        calls = {args.only: calls[args.only]}
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()

    crcs = {}
    if not args.only:
        # the records and the track words against zlib on the bytes the decode call writes, and the composite's figure against both
        for b in (3, 4):
            dig[b].check()
            assert dig[b].fallback_frames() == 0 and dig[b].wide_samples() == 0
            raw = calls["composite_%d" % b].decode.pcm.cpu().numpy()
            if b == 3:
                assert np.array_equal(raw, packed.cpu().numpy()), "the stream is not lossless"
            rec = dig[b].records(dig[b].digests[:nf])
            per_frame = raw.reshape(nf, -1)
            assert all(int(rec["crc32"][f]) == zlib.crc32(per_frame[f].tobytes()) for f in range(nf)), "a record differs from zlib on the decoded bytes"
            assert (rec["samples"] == BLOCK).all()
            crcs[b] = zlib.crc32(raw.tobytes())
            assert dig[b].track_words() == (crcs[b], raw.size), "the track word differs from zlib on the decoded bytes"
            comp = calls["composite_%d" % b].out.cpu().numpy().view(np.uint64)
            assert (int(comp[0]), int(comp[1])) == (crcs[b], raw.size), "the composite differs from zlib"
        if args.parent_lib:
            for kind in untouched + ("composite_3", "composite_4"):
                for mine, theirs in zip(calls[kind].result(), calls["parent_" + kind].result()):
                    assert torch.equal(mine, theirs), "%s: this build's results differ from the parent's" % kind

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    ms = {k: [] for k in calls}
    order = list(calls)
    for r in range(args.rounds):  # (alternating: the calls take turns at going first)
        for k in (order if r % 2 == 0 else order[::-1]):
            ms[k].append(timed(calls[k]))
    stats = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}  # noqa: E731
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    line = {
        "frames": nf, "channels": CHANNELS, "samples_per_channel": BLOCK,
        "input": "synth_frames_torch(frames, 2, track=0) * 256 + 8 bits of noise, as sela_hip_encode_pcm_device codes it lossless from 3-byte samples",
        "rounds": args.rounds, "calls_per_round": args.calls, "stream_bytes": int(len(frames_h)), "track_crc32": {str(b): "%08x" % c for b, c in crcs.items()},
        "bytes_stored_per_frame": {"digest_pcm": 8, "levels_i32": 32 * CHANNELS, "decode_pcm_3": BLOCK * CHANNELS * 3, "decode_pcm_4": BLOCK * CHANNELS * 4},
    }
    for k in calls:
        line[k] = dict(stats(ms[k]), spread=round(spread[k], 4))
    text = json.dumps(line)
    if args.only or not args.parent_lib:
        print(text)
        print("no --parent-lib (or --only): the parent's calls were not measured, so this is not the record of DESIGN.md 5.29 and nothing is written")
        return 2
    failed = []
    for b in (3, 4):
        new, comp = "digest_pcm_%d" % b, "parent_composite_%d" % b
        bound = med[comp] + (max(ms[comp]) - min(ms[comp]))
        line["digest_pcm_%d_against_the_composite" % b] = {"new_over_composite": round(med[new] / med[comp], 4), "bound_ms": round(bound, 4),
                                                           "at_or_below_the_bound": bool(med[new] <= bound)}
        if med[new] > bound:
            failed.append(new)
        line["digest_pcm_%d_over_parent_decode_pcm" % b] = round(med[new] / med["parent_decode_pcm"], 4)
        line["digest_pcm_%d_over_parent_levels_i32" % b] = round(med[new] / med["parent_levels_i32"], 4)
    for kind in untouched:
        slower = med[kind] / med["parent_" + kind] - 1.0
        line["untouched_" + kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread["parent_" + kind], 4),
                                     "within_parent_spread": bool(slower <= spread["parent_" + kind])}
        if not line["untouched_" + kind]["within_parent_spread"]:
            failed.append(kind)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    for k in failed:
        print("NOT WITHIN ITS BOUND: %s" % k)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
