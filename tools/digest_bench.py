#!/usr/bin/env python3
"""What the digest of a stream costs on the device, on tools/levels_bench.py's protocol.  The input is the bench's
synthetic track (3875 stereo frames of 2048 samples, track 0) as the encoder codes it, in device memory.  On HIP events,
everything warmed up, `rounds` rounds that alternate the calls, each timing `calls` back-to-back calls between two events; medians
with the least and the largest:
  (a) sela_hip_digest_device (k_digest_frames: nothing decoded reaches memory, then the track fold) against sela_hip_levels_device
      and sela_hip_decode_device on the same frames from another build of the library (--parent-lib: the parent commit's
      libsela_hip.so).  The digest does ordered work the levels do not, so a slowdown over them is expected; the record says how much;
  (b) sela_hip_crc32_device on the track's decoded PCM (31.7 MB) against a device-to-device copy of the same bytes;
  (c) the calls this change does not touch -- decode, levels, verify -- from this build against the parent's: they must lie within
      the parent's own spread, (largest - least) / median.
Before anything is timed the records and the track word are held against zlib on the PCM the decode call writes.
Prints one JSON line and writes it to --out (default profiles/digest/digest_bench.json).  Without --parent-lib nothing is written
and the exit code is 2; where an untouched call is slower than the parent's by more than the parent's spread the exit code is 1.
Run on the GPU box:  python tools/digest_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 20] [--calls 10]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest", "digest_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "digest_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    nf = args.frames
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t

    d_pcm = synth.synth_frames_torch(nf, CHANNELS, TRACK, device="cuda").contiguous()
    out = codec.Encoder(nf, CHANNELS).encode(d_pcm)
    torch.cuda.synchronize()
    frames_h, offs_h = out.to_host()
    d_frames = torch.from_numpy(np.concatenate([frames_h, np.zeros(8, np.uint8)])).cuda()
    d_offs = torch.from_numpy(offs_h.view(np.int64).copy()).cuda()

    def buffers(n_bytes):
        return torch.empty(max(n_bytes, 1), dtype=torch.uint8, device="cuda")

    class Decode:  # sela_hip_decode_device
        def __init__(self, L):
            self.L = L
            L.sela_hip_decode_workspace_bytes.restype, L.sela_hip_decode_workspace_bytes.argtypes = sz, [u32] * 2
            self.ws = buffers(int(L.sela_hip_decode_workspace_bytes(nf, CHANNELS)))
            self.pcm = torch.zeros((nf * BLOCK, CHANNELS), dtype=torch.int16, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_decode_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), vp(self.pcm.data_ptr()),
                                               vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.pcm, self.status

    class Verify:  # sela_hip_verify_device against the PCM the track was made from
        def __init__(self, L):
            self.L = L
            L.sela_hip_verify_workspace_bytes.restype, L.sela_hip_verify_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_verify_workspace_bytes(nf, CHANNELS, BLOCK)))
            self.counts, self.first = torch.zeros(nf, dtype=torch.int32, device="cuda"), torch.zeros(nf, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_verify_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(d_pcm.data_ptr()),
                                               vp(self.counts.data_ptr()), vp(self.first.data_ptr()), vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()),
                                               sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.counts, self.first, self.status

    class Levels:  # sela_hip_levels_device
        def __init__(self, L):
            self.L = L
            L.sela_hip_levels_workspace_bytes.restype, L.sela_hip_levels_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_levels_workspace_bytes(nf, CHANNELS, BLOCK)))
            self.levels = torch.zeros((nf, CHANNELS, 3), dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_levels_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(self.levels.data_ptr()),
                                               vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.levels, self.status

    dig = codec.Digester(nf, CHANNELS, BLOCK)
    decode = Decode(lib)
    copy_to = torch.empty_like(decode.pcm)
    crc_ws = buffers(int(lib.sela_hip_crc32_workspace_bytes(decode.pcm.numel() * 2)))
    crc_out = [torch.zeros(2, dtype=torch.int64, device="cuda")]
    calls = {"digest": lambda: dig.digest(d_frames, d_offs, nf), "decode": decode, "levels": Levels(lib), "verify": Verify(lib),
             "crc32_device": lambda: codec.crc32_device(decode.pcm, workspace=crc_ws, out=crc_out[0]),
             "device_copy": lambda: copy_to.copy_(decode.pcm)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls["parent_decode"], calls["parent_levels"], calls["parent_verify"] = Decode(parent), Levels(parent), Verify(parent)
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    dig.check()
    assert dig.route() == 1, dig.route()

    # the records, the track word and the raw-bytes call against zlib on the decoded PCM
    pcm_h = np.ascontiguousarray(decode.pcm.cpu().numpy(), "<i2")
    rec = dig.records(dig.digests[:nf])
    per_frame = pcm_h.reshape(nf, -1)
    assert all(int(rec["crc32"][f]) == zlib.crc32(per_frame[f].tobytes()) for f in range(nf)), "a record differs from zlib on the decoded PCM"
    assert (rec["samples"] == BLOCK).all()
    whole = zlib.crc32(pcm_h.tobytes())
    assert dig.track_words() == (whole, pcm_h.nbytes), "the track word differs from zlib on the decoded PCM"
    raw = crc_out[0].cpu().numpy().view(np.uint64)
    assert (int(raw[0]), int(raw[1])) == (whole, pcm_h.nbytes), "sela_hip_crc32_device differs from zlib"
    if args.parent_lib:
        for kind in ("decode", "levels", "verify"):
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
        "frames": nf, "channels": CHANNELS, "samples_per_channel": BLOCK, "input": "synth_frames_torch(frames, 2, track=0) as sela_hip_encode_device codes it",
        "rounds": args.rounds, "calls_per_round": args.calls, "stream_bytes": int(len(frames_h)), "pcm_bytes": int(pcm_h.nbytes), "track_crc32": "%08x" % whole,
        "bytes_stored_per_frame": {"digest": 8, "levels": 24 * CHANNELS, "decode": BLOCK * CHANNELS * 2},
    }
    for k in calls:
        line[k] = dict(stats(ms[k]), spread=round(spread[k], 4))
    line["crc32_device_over_device_copy"] = round(med["crc32_device"] / med["device_copy"], 4)
    line["crc32_device_gb_per_s"] = round(pcm_h.nbytes / med["crc32_device"] / 1e6, 1)
    slow = []
    if args.parent_lib:
        line["digest_over_parent_levels"] = round(med["digest"] / med["parent_levels"], 4)
        line["digest_over_parent_decode"] = round(med["digest"] / med["parent_decode"], 4)
        for kind in ("decode", "levels", "verify"):
            slower = med[kind] / med["parent_" + kind] - 1.0
            line["untouched_" + kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread["parent_" + kind], 4),
                                         "within_parent_spread": bool(slower <= spread["parent_" + kind])}
            if not line["untouched_" + kind]["within_parent_spread"]:
                slow.append(kind)
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("no --parent-lib: the parent's calls were not measured, so this is not the record of DESIGN.md 5.28 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    for k in slow:
        print("AN UNTOUCHED CALL IS SLOWER THAN THE PARENT'S BY MORE THAN ITS SPREAD: %s" % k)
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
