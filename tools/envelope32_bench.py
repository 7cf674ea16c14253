#!/usr/bin/env python3
"""What the envelope of a 24-bit stream costs on the device, on tools/levels32_bench.py's protocol.  The input is
the bench's synthetic track (3875 stereo frames of 2048 samples, track 0) widened to 24 bits -- shifted left 8, the low byte noise
-- as sela_hip_encode_i32_device codes it, in device memory.  On HIP events, everything warmed up, `rounds` rounds that alternate
the calls, each timing `calls` back-to-back calls between two events; medians with the least and the largest:
  (a) sela_hip_envelope_i32_device at buckets 32, 256 and 2048 against sela_hip_levels_i32_device and sela_hip_decode_i32_device on
      the same frames from another build of the library (--parent-lib: the parent commit's libsela_hip.so);
  (b) the untouched neighbours of this build -- sela_hip_decode_i32_device, sela_hip_verify_i32_device, sela_hip_levels_i32_device
      and, on the 16-bit track, sela_hip_envelope_device -- against the parent's, whose results must be theirs: each must sit inside
      the parent's spread of its own repeats, (largest - least) / median.
Before anything is timed the records of every bucket are held against numpy on the samples the decode call writes.
Prints one JSON line and writes it to --out (default profiles/envelope/envelope32_bench.json).  These are costs, not gates: the
exit code is 0 once the record is written; without --parent-lib nothing is written and the exit code is 2.
Run on the GPU box:  python tools/envelope32_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 20] [--calls 10]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, BLOCK, TRACK = 3875, 2, 2048, 0
BUCKETS = (32, 256, 2048)


def expect(dec, bucket):
    """numpy on int32 [frames, channels, 2048] -> (min, max, sum, energy as Python integers), each [frames, 2048 / bucket, channels]"""
    f, ch, n = dec.shape
    v = dec.astype(np.int64).reshape(f, ch, n // bucket, bucket).transpose(0, 2, 1, 3)
    sq = (np.abs(v).astype(np.uint64)) ** 2
    energy = (sq & np.uint64(0xFFFFFFFF)).sum(3, dtype=np.uint64).astype(object) + ((sq >> np.uint64(32)).sum(3, dtype=np.uint64).astype(object) << 32)
    return v.min(3), v.max(3), v.sum(3), energy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envelope", "envelope32_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "envelope32_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    nf = args.frames
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t

    d_pcm16 = synth.synth_frames_torch(nf, CHANNELS, TRACK, device="cuda").contiguous()
    gen = torch.Generator(device="cuda").manual_seed(0x5E1A)
    wide = (d_pcm16.to(torch.int32) << 8) | torch.randint(0, 256, d_pcm16.shape, generator=gen, device="cuda", dtype=torch.int32)
    d_planar = wide.permute(0, 2, 1).contiguous()  # int32 [frames, channels, 2048]
    enc = codec.Encoder32(nf, CHANNELS, BLOCK)
    enc.encode(d_planar)
    enc.check()
    frames_h, offs_h = enc.to_host()
    pad = np.zeros(8, np.uint8)
    d_frames = torch.from_numpy(np.concatenate([frames_h, pad])).cuda()
    d_offs = torch.from_numpy(offs_h.view(np.int64).copy()).cuda()
    # the 16-bit track, for the untouched sela_hip_envelope_device
    enc16 = codec.Encoder(nf, CHANNELS)
    out16 = enc16.encode(d_pcm16)
    torch.cuda.synchronize()
    f16_h, o16_h = out16.to_host()
    d_frames16 = torch.from_numpy(np.concatenate([f16_h, pad])).cuda()
    d_offs16 = torch.from_numpy(o16_h.view(np.int64).copy()).cuda()

    def buffers(n_bytes):
        return torch.empty(max(n_bytes, 1), dtype=torch.uint8, device="cuda")

    def sized(L, name):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = sz, [u32] * 3
        return buffers(int(fn(nf, CHANNELS, BLOCK)))

    class DecodeI32:  # sela_hip_decode_i32_device
        def __init__(self, L):
            self.L, self.ws = L, sized(L, "sela_hip_decode_i32_workspace_bytes")
            self.samples = torch.zeros((nf, CHANNELS, BLOCK), dtype=torch.int32, device="cuda")
            self.counts = torch.zeros(nf * CHANNELS, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_decode_i32_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(self.samples.data_ptr()),
                                                   vp(self.counts.data_ptr()), vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.samples, self.counts, self.status

    class VerifyI32:  # sela_hip_verify_i32_device against the samples the track was made from
        def __init__(self, L):
            self.L, self.ws = L, sized(L, "sela_hip_verify_i32_workspace_bytes")
            self.counts, self.first = torch.zeros(nf, dtype=torch.int32, device="cuda"), torch.zeros(nf, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_verify_i32_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(d_planar.data_ptr()),
                                                   vp(None), vp(self.counts.data_ptr()), vp(self.first.data_ptr()), vp(None), vp(self.status.data_ptr()),
                                                   vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.counts, self.first, self.status

    class LevelsI32:  # sela_hip_levels_i32_device
        def __init__(self, L):
            self.L, self.ws = L, sized(L, "sela_hip_levels_i32_workspace_bytes")
            self.levels = torch.zeros((nf, CHANNELS, 4), dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_levels_i32_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(self.levels.data_ptr()),
                                                   vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.levels, self.status

    class Envelope16:  # sela_hip_envelope_device on the 16-bit track, bucket 256
        def __init__(self, L):
            self.L, self.ws = L, sized(L, "sela_hip_envelope_workspace_bytes")
            self.env = torch.zeros((nf, BLOCK // 256, CHANNELS, 2), dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_envelope_device(vp(d_frames16.data_ptr()), vp(d_offs16.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), u32(256), vp(self.env.data_ptr()),
                                                 vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.env, self.status

    envelopers = {b: codec.Enveloper32(nf, CHANNELS, BLOCK, b) for b in BUCKETS}
    calls = {"envelope_i32_%d" % b: (lambda e=e: e.measure(d_frames, d_offs, nf)) for b, e in envelopers.items()}
    kinds = {"decode_i32": DecodeI32, "verify_i32": VerifyI32, "levels_i32": LevelsI32, "envelope_16bit_256": Envelope16}
    for kind, cls in kinds.items():
        calls[kind] = cls(lib)
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        for kind, cls in kinds.items():
            calls["parent_" + kind] = cls(parent)
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()

    # the records against numpy on the decoded samples
    dec = calls["decode_i32"].samples.cpu().numpy()
    assert (calls["decode_i32"].counts.cpu().numpy() == BLOCK).all()
    for b, e in envelopers.items():
        e.check()
        assert e.fallback_frames() == 0
        rec = e.records(e.envelope)
        energy = rec["sum_squares_lo"].astype(object) + (rec["sum_squares_hi"].astype(object) << 64)
        for name, got, w in zip(("min", "max", "sum", "sum_squares"), (rec["min"], rec["max"], rec["sum"], energy), expect(dec, b)):
            assert (got.astype(object) == w.astype(object)).all(), "bucket %d: %s differs from numpy on the decoded samples" % (b, name)
    if args.parent_lib:
        for kind in kinds:
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

    for c in calls.values():
        c()
    torch.cuda.synchronize()
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
        "input": "synth_frames_torch(frames, 2, track=0) << 8 | noise byte, as sela_hip_encode_i32_device codes it",
        "rounds": args.rounds, "calls_per_round": args.calls, "stream_bytes": int(len(frames_h)),
        "bytes_stored_per_frame": {"envelope_i32_%d" % b: 32 * CHANNELS * (BLOCK // b) for b in BUCKETS},
    }
    for k in calls:
        line[k] = dict(stats(ms[k]), spread=round(spread[k], 4))
    if args.parent_lib:
        for b in BUCKETS:
            line["envelope_i32_%d_over_parent_levels_i32" % b] = round(med["envelope_i32_%d" % b] / med["parent_levels_i32"], 4)
            line["envelope_i32_%d_over_parent_decode_i32" % b] = round(med["envelope_i32_%d" % b] / med["parent_decode_i32"], 4)
        for kind in kinds:
            slower = med[kind] / med["parent_" + kind] - 1.0
            line["untouched_" + kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread["parent_" + kind], 4),
                                         "within_parent_spread": bool(slower <= spread["parent_" + kind])}
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("no --parent-lib: the parent's calls were not measured, so this is not the record of DESIGN.md 5.32 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
