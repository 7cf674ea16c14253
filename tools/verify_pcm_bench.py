#!/usr/bin/env python3
"""What holding a stream against packed 24-bit PCM costs on the device, on tools/pcm_bench.py's protocol.  The input
is the bench's synthetic track (3875 stereo frames of 2048 samples, track 0) widened to 24 bits -- shifted left 8, the low byte
filled with noise -- as packed 3-byte samples, and the stream sela_hip_encode_pcm_device makes of it.  On HIP events, everything
warmed up, `rounds` rounds that alternate the calls, each timing `calls` back-to-back calls between two events; medians with the
least and the largest:
  (a) codec.VerifierPcm.verify: sela_hip_verify_pcm_device, the original read as packed bytes by the compare kernel;
  (b) what a caller composed before: codec.pcm_unpack (sela_hip_pcm_unpack_device into a second buffer of frames x channels x
      stride x 4 bytes) and then codec.Verifier32.verify (sela_hip_verify_i32_device) -- both calls in the timed span;
      (a) and (b) must give the same counts in the same frames ((b) orders its first difference c * stride + i, (a) i * channels + c);
  (c) sela_hip_verify_i32_device and sela_hip_decode_pcm_device of this build against the same calls of another build of the library
      (--parent-lib: the parent commit's libsela_hip.so), whose results must be this build's; each should sit inside the parent's own
      spread between repeats, (largest - least) / median.
Prints one JSON line and writes it to --out (default profiles/verify_pcm/verify_pcm_bench.json).  Without --parent-lib (c) is not
measured, nothing is written and the exit code is 2; where a call of (c) is slower than the parent's by more than the parent's
spread the record is written, the fact is printed, and the exit code is 1.
Run on the GPU box:  python tools/verify_pcm_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 15] [--calls 10]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, BLOCK, TRACK, BYTES = 3875, 2, 2048, 0, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_pcm", "verify_pcm_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "verify_pcm_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    nf = args.frames
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t

    d_pcm16 = synth.synth_frames_torch(nf, CHANNELS, TRACK, device="cuda").contiguous()
    gen = torch.Generator(device="cuda").manual_seed(0x5E1A)
    wide = (d_pcm16.to(torch.int32) << 8) | torch.randint(0, 256, d_pcm16.shape, generator=gen, device="cuda", dtype=torch.int32)
    d_planar = wide.permute(0, 2, 1).contiguous()  # int32 [frames, channels, 2048]
    d_packed = torch.stack([(wide >> (8 * k)) & 0xFF for k in range(BYTES)], dim=-1).to(torch.uint8).reshape(-1).contiguous()

    enc = codec.EncoderPcm(nf, CHANNELS, BLOCK, BYTES)
    frames, offsets, _ = enc.encode(d_packed)
    enc.check()
    stream24 = torch.cat([frames[: enc.needed_bytes()].clone(), torch.zeros(8, dtype=torch.uint8, device="cuda")])
    offsets24 = offsets.clone()

    # ---- (a) and (b) --------------------------------------------------------------------------------------------------------------
    ver_pcm = codec.VerifierPcm(nf, CHANNELS, BLOCK, BYTES)
    ver_i32 = codec.Verifier32(nf, CHANNELS, BLOCK)
    d_unpacked = torch.empty_like(d_planar)

    def verify_pcm():
        ver_pcm.verify(stream24, offsets24, nf, d_packed)

    def unpack_then_verify_i32():
        codec.pcm_unpack(d_packed, nf, CHANNELS, BLOCK, BYTES, out=d_unpacked)
        ver_i32.verify(stream24, offsets24, nf, d_unpacked)

    # ---- (c) the untouched calls, this build and the parent's ---------------------------------------------------------------------
    def buffers(n_bytes):
        return torch.empty(n_bytes, dtype=torch.uint8, device="cuda")

    class VerifyI32:
        def __init__(self, L):
            self.L = L
            L.sela_hip_verify_i32_workspace_bytes.restype, L.sela_hip_verify_i32_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_verify_i32_workspace_bytes(nf, CHANNELS, BLOCK)))
            self.counts, self.first = torch.zeros(nf, dtype=torch.int32, device="cuda"), torch.zeros(nf, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_verify_i32_device(vp(stream24.data_ptr()), vp(offsets24.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(d_planar.data_ptr()),
                                                   vp(None), vp(self.counts.data_ptr()), vp(self.first.data_ptr()), vp(None), vp(self.status.data_ptr()),
                                                   vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.counts, self.first, self.status

    class DecodePcm:
        def __init__(self, L):
            self.L = L
            L.sela_hip_decode_pcm_workspace_bytes.restype, L.sela_hip_decode_pcm_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_decode_pcm_workspace_bytes(nf, CHANNELS, BLOCK)))
            self.pcm = buffers(nf * BLOCK * CHANNELS * BYTES)
            self.so, self.status = torch.zeros(nf + 1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_decode_pcm_device(vp(stream24.data_ptr()), vp(offsets24.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), u32(BYTES),
                                                   vp(self.pcm.data_ptr()), vp(self.so.data_ptr()), vp(self.status.data_ptr()), vp(self.ws.data_ptr()),
                                                   sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.pcm, self.so, self.status

    calls = {"verify_pcm": verify_pcm, "unpack_verify_i32": unpack_then_verify_i32, "verify_i32": VerifyI32(lib), "decode_pcm": DecodePcm(lib)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls["parent_verify_i32"], calls["parent_decode_pcm"] = VerifyI32(parent), DecodePcm(parent)
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    ver_pcm.check(), ver_i32.check()
    assert ver_pcm.fallback_frames() == 0 and ver_i32.fallback_frames() == 0
    a_counts, a_first = ver_pcm.diff_counts.cpu().numpy().view(np.uint32), ver_pcm.first_diff.cpu().numpy().view(np.uint32)
    b_counts, b_first = ver_i32.diff_counts.cpu().numpy().view(np.uint32), ver_i32.first_diff.cpu().numpy().view(np.uint32)
    assert np.array_equal(a_counts, b_counts), "the counts of (a) and (b) differ"
    # (b)'s first is the smallest c * stride + i: the same frames have one, and (a)'s i * channels + c names a differing sample of (b)'s
    assert np.array_equal(a_first == 0xFFFFFFFF, b_first == 0xFFFFFFFF)
    lossy = np.flatnonzero(a_counts)
    for f in lossy:  # ((b)'s sample differs, so the smallest interleaved index is not behind it)
        assert int(a_first[f]) <= (int(b_first[f]) % BLOCK) * CHANNELS + int(b_first[f]) // BLOCK, f
    if args.parent_lib:
        for kind in ("verify_i32", "decode_pcm"):
            for mine, theirs in zip(calls[kind].result(), calls["parent_" + kind].result()):
                assert torch.equal(mine, theirs), "sela_hip_%s_device's results differ from the parent's" % kind

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    ms = {k: [] for k in calls}
    pairs = [("verify_pcm", "unpack_verify_i32")]
    if args.parent_lib:
        pairs += [("verify_i32", "parent_verify_i32"), ("decode_pcm", "parent_decode_pcm")]
    else:
        pairs += [("verify_i32",), ("decode_pcm",)]
    for r in range(args.rounds):  # (alternating: the two of a pair take turns at going first)
        for pair in pairs:
            for k in (pair if r % 2 == 0 else pair[::-1]):
                ms[k].append(timed(calls[k]))
    stats = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}  # noqa: E731
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread_b = (max(ms["unpack_verify_i32"]) - min(ms["unpack_verify_i32"])) / med["unpack_verify_i32"]
    spread_a = (max(ms["verify_pcm"]) - min(ms["verify_pcm"])) / med["verify_pcm"]
    saving = 1.0 - med["verify_pcm"] / med["unpack_verify_i32"]
    line = {
        "frames": nf, "channels": CHANNELS, "samples_per_channel": BLOCK, "bytes_per_sample": BYTES,
        "input": "synth_frames_torch(frames, 2, track=0) << 8 | noise byte, packed; the stream sela_hip_encode_pcm_device makes of it",
        "rounds": args.rounds, "calls_per_round": args.calls, "stream_bytes": int(stream24.numel() - 8), "lossy_frames": int(len(lossy)),
        "a_verify_pcm": stats(ms["verify_pcm"]), "b_unpack_then_verify_i32": stats(ms["unpack_verify_i32"]),
        "a_over_b": round(med["verify_pcm"] / med["unpack_verify_i32"], 4), "a_spread": round(spread_a, 4), "b_spread": round(spread_b, 4),
        "a_beats_b_by_more_than_the_spread": bool(saving > max(spread_a, spread_b)),
        "workspace_bytes_a": int(ver_pcm.workspace.numel()), "workspace_and_second_buffer_bytes_b": int(ver_i32.workspace.numel() + d_unpacked.numel() * 4),
        "c_verify_i32_device": stats(ms["verify_i32"]), "c_decode_pcm_device": stats(ms["decode_pcm"]),
    }
    slow = []
    if args.parent_lib:
        for kind in ("verify_i32", "decode_pcm"):
            p = ms["parent_" + kind]
            spread = (max(p) - min(p)) / med["parent_" + kind]
            slower = med[kind] / med["parent_" + kind] - 1.0
            line["c_parent_%s_device" % kind] = stats(p)
            line["c_%s" % kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread, 4), "within_parent_spread": bool(slower <= spread)}
            if slower > spread:
                slow.append(kind)
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("no --parent-lib: figure (c) was not measured, so this is not the record of DESIGN.md 5.24 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    for k in slow:
        print("OUTSIDE THE PARENT'S SPREAD: %s: this tree over the parent %.4f, the parent's spread %.4f" % (k, line["c_" + k]["this_over_parent"], line["c_" + k]["parent_spread"]))
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
