#!/usr/bin/env python3
"""What packed 24-bit PCM costs on the device.  The input is the bench's synthetic track (3875 stereo frames of
2048 samples, track 0) widened to 24 bits -- shifted left 8, the low byte filled with noise -- as packed 3-byte samples.  On HIP
events, everything warmed up, `rounds` rounds that alternate the calls, each timing `calls` back-to-back calls between two events:
  (a) k_pcm_unpack<3> and k_pcm_pack<3> (sela_hip_pcm_unpack_device / sela_hip_pcm_pack_device), each against a device-to-device
      hipMemcpyAsync that moves the same total of bytes read plus written (a copy of B bytes reads B and writes B: B = that total / 2);
  (b) sela_hip_encode_pcm_device against sela_hip_encode_i32_device on the same samples, and sela_hip_decode_pcm_device against
      sela_hip_decode_i32_device on the stream they make, same build;
  (c) sela_hip_encode_i32_device and sela_hip_decode_n_device (a 16-bit stream of the same track) of this build against the same calls
      of another build of the library (--parent-lib: the parent commit's libsela_hip.so), whose bytes must be this build's; each must
      sit inside the parent's own spread between repeats, (largest - least) / median.
Prints one JSON line and writes it to --out (default profiles/pcm/pcm_bench.json).  Without --parent-lib (c) is not measured, nothing
is written and the exit code is 2; where a call of (c) is slower than the parent's by more than the parent's spread the record is
written, the fact is printed, and the exit code is 1.
Run on the GPU box:  python tools/pcm_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 15] [--calls 10]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm", "pcm_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "pcm_bench needs a GPU: there is no CPU path to time"
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
    values = nf * BLOCK * CHANNELS
    cap = nf * ((BLOCK * CHANNELS * 9) // 2 + CHANNELS * 192 + 64)

    def buffers(n_bytes):
        return torch.empty(n_bytes, dtype=torch.uint8, device="cuda")

    # ---- (a) the kernels and the copy ---------------------------------------------------------------------------------------------
    d_unpacked = torch.empty_like(d_planar)
    d_counts = torch.full((nf, CHANNELS), BLOCK, dtype=torch.int32, device="cuda")
    d_so = torch.arange(nf + 1, dtype=torch.int64, device="cuda") * BLOCK
    d_repacked = buffers(values * BYTES)
    d_pack_status = torch.zeros(4, dtype=torch.int32, device="cuda")
    moved = values * (BYTES + 4)  # bytes read plus written, either kernel
    d_copy_src, d_copy_dst = buffers(moved // 2), buffers(moved // 2)
    # the HIP runtime this process already runs on (torch's, which libsela_hip.so was loaded behind): never a second one
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert loaded, "no HIP runtime is loaded"
    hip = C.CDLL(loaded[0])
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [vp, vp, sz, C.c_int, vp]

    def unpack():
        assert lib.sela_hip_pcm_unpack_device(d_packed.data_ptr(), BYTES, nf, CHANNELS, BLOCK, d_unpacked.data_ptr(), stream) == 0

    def pack():
        assert lib.sela_hip_pcm_pack_device(d_planar.data_ptr(), d_counts.data_ptr(), d_so.data_ptr(), nf, CHANNELS, BLOCK, BYTES, d_repacked.data_ptr(),
                                            d_pack_status.data_ptr(), stream) == 0

    def copy():
        assert hip.hipMemcpyAsync(d_copy_dst.data_ptr(), d_copy_src.data_ptr(), moved // 2, 3, stream) == 0  # hipMemcpyDeviceToDevice

    # ---- (b) the composed calls and the i32 calls, this build ---------------------------------------------------------------------
    class Encode:
        def __init__(self, L, packed):
            self.L, self.packed = L, packed
            self.frames, self.offsets, self.status = buffers(cap), torch.zeros(nf + 1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
            name = "sela_hip_encode_pcm_workspace_bytes" if packed else "sela_hip_encode_i32_workspace_bytes"
            getattr(L, name).restype, getattr(L, name).argtypes = sz, [u32] * 3
            self.ws = buffers(int(getattr(L, name)(nf, CHANNELS, BLOCK)))

        def __call__(self):
            tail = [vp(self.frames.data_ptr()), sz(cap), vp(self.offsets.data_ptr()), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream)]
            if self.packed:
                rc = self.L.sela_hip_encode_pcm_device(vp(d_packed.data_ptr()), u32(BYTES), u32(nf), u32(CHANNELS), u32(BLOCK), u32(0), *tail)
            else:
                rc = self.L.sela_hip_encode_i32_device(vp(d_planar.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), *tail)
            assert rc == 0, rc

        def result(self):
            torch.cuda.synchronize()
            assert codec.encode_status_error(self.status.cpu().numpy()) == 0
            return self.frames[: int(self.offsets[nf].item())].clone(), self.offsets.clone()

    enc_pcm, enc_i32 = Encode(lib, True), Encode(lib, False)
    for e in (enc_pcm, enc_i32):
        e()
    stream24, offsets24 = enc_i32.result()
    got, got_offsets = enc_pcm.result()
    assert torch.equal(got, stream24) and torch.equal(got_offsets, offsets24), "the composed encode's bytes differ from the i32 call's"
    stream24 = torch.cat([stream24, torch.zeros(8, dtype=torch.uint8, device="cuda")])

    dec_pcm = codec.DecoderPcm(nf, CHANNELS, BLOCK, BYTES)
    dec_i32 = codec.Decoder32(nf, CHANNELS, BLOCK)

    def decode_pcm():
        dec_pcm.decode(stream24, offsets24, nf)

    def decode_i32():
        dec_i32.decode(stream24, offsets24, nf)

    # ---- (c) the untouched calls, this build and the parent's ---------------------------------------------------------------------
    enc16 = codec.Encoder(nf, CHANNELS)
    out16 = enc16.encode(d_pcm16)
    torch.cuda.synchronize()
    stream16, offsets16 = out16.frames.clone(), out16.offsets.clone()

    class DecodeN:
        def __init__(self, L):
            self.L = L
            L.sela_hip_decode_n_workspace_bytes.restype, L.sela_hip_decode_n_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_decode_n_workspace_bytes(nf, CHANNELS, BLOCK)))
            self.pcm = torch.empty((nf * BLOCK, CHANNELS), dtype=torch.int16, device="cuda")
            self.so, self.status = torch.zeros(nf + 1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_decode_n_device(vp(stream16.data_ptr()), vp(offsets16.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(self.pcm.data_ptr()),
                                                 vp(self.so.data_ptr()), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

    calls = {"unpack3": unpack, "pack3": pack, "copy": copy, "encode_pcm": enc_pcm, "encode_i32": enc_i32, "decode_pcm": decode_pcm, "decode_i32": decode_i32,
             "decode_n": DecodeN(lib)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls["parent_encode_i32"], calls["parent_decode_n"] = Encode(parent, False), DecodeN(parent)
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    assert torch.equal(d_unpacked, d_planar) and torch.equal(d_repacked, d_packed) and d_pack_status.cpu().tolist() == [0, 0, 0, 0]
    dec_pcm.check()
    assert torch.equal(dec_pcm.pcm, torch.stack([(dec_i32.samples.permute(0, 2, 1) >> (8 * k)) & 0xFF for k in range(BYTES)], dim=-1).to(torch.uint8).reshape(-1))
    if args.parent_lib:
        theirs = calls["parent_encode_i32"].result()
        assert torch.equal(theirs[0], stream24[:-8]) and torch.equal(theirs[1], offsets24), "sela_hip_encode_i32_device's bytes differ from the parent's"
        assert torch.equal(calls["parent_decode_n"].pcm, calls["decode_n"].pcm), "sela_hip_decode_n_device's samples differ from the parent's"

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    ms = {k: [] for k in calls}
    pairs = [("unpack3", "copy"), ("pack3", "copy"), ("encode_pcm", "encode_i32"), ("decode_pcm", "decode_i32")]
    if args.parent_lib:
        pairs += [("encode_i32", "parent_encode_i32"), ("decode_n", "parent_decode_n")]
    else:
        pairs += [("decode_n",)]
    for r in range(args.rounds):  # (alternating: the two of a pair take turns at going first)
        for pair in pairs:
            for k in (pair if r % 2 == 0 else pair[::-1]):
                ms[k].append(timed(calls[k]))
    stats = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}  # noqa: E731
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {
        "frames": nf, "channels": CHANNELS, "samples_per_channel": BLOCK, "bytes_per_sample": BYTES,
        "input": "synth_frames_torch(frames, 2, track=0) << 8 | noise byte, packed", "rounds": args.rounds, "calls_per_round": args.calls,
        "bytes_read_plus_written_per_kernel": moved, "stream_bytes": int(stream24.numel() - 8),
        "a_unpack3": stats(ms["unpack3"]), "a_pack3": stats(ms["pack3"]), "a_copy_same_bytes": stats(ms["copy"]),
        "a_unpack3_over_copy": round(med["unpack3"] / med["copy"], 4), "a_pack3_over_copy": round(med["pack3"] / med["copy"], 4),
        "a_copy_GBps": round(moved / med["copy"] / 1e6, 1), "a_unpack3_GBps": round(moved / med["unpack3"] / 1e6, 1), "a_pack3_GBps": round(moved / med["pack3"] / 1e6, 1),
        "b_encode_pcm_device": stats(ms["encode_pcm"]), "b_encode_i32_device": stats(ms["encode_i32"]),
        "b_encode_pcm_over_i32": round(med["encode_pcm"] / med["encode_i32"], 4),
        "b_decode_pcm_device": stats(ms["decode_pcm"]), "b_decode_i32_device": stats(ms["decode_i32"]),
        "b_decode_pcm_over_i32": round(med["decode_pcm"] / med["decode_i32"], 4),
        "c_decode_n_device": stats(ms["decode_n"]),
    }
    slow = []
    if args.parent_lib:
        for kind in ("encode_i32", "decode_n"):
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
        print("no --parent-lib: figure (c) was not measured, so this is not the record of DESIGN.md 5.22 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    for k in slow:
        print("REQUIRED CONDITION MISSED: %s: this tree over the parent %.4f, the parent's spread %.4f" % (k, line["c_" + k]["this_over_parent"], line["c_" + k]["parent_spread"]))
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
