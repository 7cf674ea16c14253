#!/usr/bin/env python3
"""What a stream's envelope costs on the device, on tools/levels_bench.py's protocol.  The input is the bench's
synthetic track (3875 stereo frames of 2048 samples, track 0) as the encoder codes it, in device memory.  On HIP events,
everything warmed up, `rounds` rounds that alternate the calls, each timing `calls` back-to-back calls between two events; medians
with the least and the largest:
  (a) sela_hip_envelope_device at buckets 32, 256 and 2048 (k_envelope_frames: nothing decoded reaches memory) against
      sela_hip_levels_device and sela_hip_decode_n_device on the same frames from another build of the library (--parent-lib: the
      parent commit's libsela_hip.so);
  (b) the cold route: the same track with one more frame of 777 samples behind it, which sends the whole call through the
      any-length kernels into the workspace and k_envelope_channels over it, against the parent's sela_hip_decode_n_device there;
  (c) the calls this change does not touch -- decode_n, verify, levels, digest -- of this build against the parent's, whose
      results they must give.
Before anything is timed the records of both streams are held against numpy on the PCM the decode calls write.
Prints one JSON line and writes it to --out (default profiles/envelope/envelope_bench.json).  The ratios are costs, none is a
gate; "no dearer than decoding to PCM" holds for a bucket where the envelope's median is at or below the parent's decode_n median
plus that call's own spread (largest - least).  Without --parent-lib nothing is written and the exit code is 2.
Run on the GPU box:  python tools/envelope_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 20] [--calls 10]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, BLOCK, TRACK, TAIL = 3875, 2, 2048, 0, 777
BUCKETS = (32, 256, 2048)
UNTOUCHED = ("decode_n", "verify", "levels", "digest")


def expect(pcm, so, slots, bucket):
    """numpy on int16 PCM [total, channels] -> (min, max, sum, sum_squares), each [frames, slots, channels]"""
    n = len(so) - 1
    out = [np.zeros((n, slots, pcm.shape[1]), np.int64) for _ in range(4)]
    for f in range(n):
        v = pcm[int(so[f]): int(so[f + 1])].astype(np.int64)
        whole = len(v) // bucket
        if whole:
            w = v[: whole * bucket].reshape(whole, bucket, -1)
            out[0][f, :whole], out[1][f, :whole], out[2][f, :whole], out[3][f, :whole] = w.min(1), w.max(1), w.sum(1), (w * w).sum(1)
        if len(v) % bucket:
            w = v[whole * bucket:]
            out[0][f, whole], out[1][f, whole], out[2][f, whole], out[3][f, whole] = w.min(0), w.max(0), w.sum(0), (w * w).sum(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envelope", "envelope_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "envelope_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    nf = args.frames
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t

    d_pcm = synth.synth_frames_torch(nf, CHANNELS, TRACK, device="cuda").contiguous()
    enc = codec.Encoder(nf, CHANNELS)
    out = enc.encode(d_pcm)
    torch.cuda.synchronize()
    frames_h, offs_h = out.to_host()
    pad = np.zeros(8, np.uint8)
    d_frames = torch.from_numpy(np.concatenate([frames_h, pad])).cuda()
    d_offs = torch.from_numpy(offs_h.view(np.int64).copy()).cuda()
    # the cold stream: one more frame, of 777 samples
    tail_pcm = synth.synth_frames(1, CHANNELS, TRACK + 1)[:, :TAIL]
    tail_frames, tail_offs = codec.encode_host(np.ascontiguousarray(tail_pcm))
    cold_h = np.concatenate([frames_h, tail_frames, pad])
    cold_offs_h = np.append(offs_h, offs_h[-1] + tail_offs[-1]).astype(np.uint64)
    d_cold = torch.from_numpy(cold_h).cuda()
    d_cold_offs = torch.from_numpy(cold_offs_h.view(np.int64).copy()).cuda()

    def buffers(n_bytes):
        return torch.empty(max(n_bytes, 1), dtype=torch.uint8, device="cuda")

    class FramesCall:
        """sela_hip_<name>_device of library L on the track (or the cold stream): the outputs as zeroed device words"""

        def __init__(self, L, name, out_words, cold=False):
            self.L, self.cold, self.n = L, cold, nf + (1 if cold else 0)
            size = getattr(L, "sela_hip_%s_workspace_bytes" % name)
            size.restype, size.argtypes = sz, [u32] * 3
            self.fn = getattr(L, "sela_hip_%s_device" % name)
            self.ws = buffers(int(size(self.n, CHANNELS, BLOCK)))
            self.outs = [torch.zeros(max(w, 1), dtype=torch.int64, device="cuda") for w in out_words]
            self.so, self.status = torch.zeros(self.n + 1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")

        def args(self):
            return [vp(o.data_ptr()) for o in self.outs]

        def __call__(self):
            fr, of = (d_cold, d_cold_offs) if self.cold else (d_frames, d_offs)
            rc = self.fn(vp(fr.data_ptr()), vp(of.data_ptr()), u32(self.n), u32(CHANNELS), u32(BLOCK), *self.args(), vp(self.so.data_ptr()),
                         vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.outs + [self.so, self.status]

        def pcm(self):
            return self.outs[0].view(torch.int16).reshape(-1, CHANNELS)

    class VerifyCall(FramesCall):  # (the PCM the track was made from goes in front of the two arrays)
        def args(self):
            return [vp(d_pcm.data_ptr())] + [vp(o.data_ptr()) for o in self.outs]

    def untouched(L):
        return {"decode_n": FramesCall(L, "decode_n", [nf * BLOCK * CHANNELS // 4]), "verify": VerifyCall(L, "verify", [nf // 2 + 1, nf // 2 + 1]),
                "levels": FramesCall(L, "levels", [nf * CHANNELS * 3]), "digest": FramesCall(L, "digest", [nf, 2])}

    env = {b: codec.Enveloper(nf, CHANNELS, BLOCK, b) for b in BUCKETS}
    env_cold = codec.Enveloper(nf + 1, CHANNELS, BLOCK, 256)
    calls = {"envelope_%d" % b: (lambda e=env[b]: e.measure(d_frames, d_offs, nf)) for b in BUCKETS}
    calls["envelope_cold_256"] = lambda: env_cold.measure(d_cold, d_cold_offs, nf + 1)
    calls.update(untouched(lib))
    calls["decode_n_cold"] = FramesCall(lib, "decode_n", [(nf + 1) * BLOCK * CHANNELS // 4], cold=True)
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls.update({"parent_" + k: v for k, v in untouched(parent).items()})
        calls["parent_decode_n_cold"] = FramesCall(parent, "decode_n", [(nf + 1) * BLOCK * CHANNELS // 4], cold=True)
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    for e in list(env.values()) + [env_cold]:
        e.check()
    assert all(e.route() == 1 for e in env.values()) and env_cold.route() == 2

    # the records against numpy on the decoded PCM
    def hold(e, n, pcm, so, what):
        rec = e.records(e.envelope[:n])
        for name, w in zip(("min", "max", "sum", "sum_squares"), expect(pcm, so, e.slots, e.bucket)):
            assert np.array_equal(rec[name].astype(np.int64), w), "%s: %s differs from numpy on the decoded PCM" % (what, name)

    pcm_h = calls["decode_n"].pcm().cpu().numpy()
    for b in BUCKETS:
        hold(env[b], nf, pcm_h, np.arange(nf + 1) * BLOCK, "envelope, bucket %d" % b)
    cold_so = calls["decode_n_cold"].so.cpu().numpy()
    assert int(cold_so[-1]) == nf * BLOCK + TAIL
    hold(env_cold, nf + 1, calls["decode_n_cold"].pcm().cpu().numpy(), cold_so, "envelope (cold route)")
    if args.parent_lib:
        for kind in UNTOUCHED + ("decode_n_cold",):
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
        "rounds": args.rounds, "calls_per_round": args.calls, "stream_bytes": int(len(frames_h)),
        "bytes_stored_per_frame": dict({"envelope_%d" % b: 16 * CHANNELS * (BLOCK // b) for b in BUCKETS}, levels=24 * CHANNELS, decode_n=BLOCK * CHANNELS * 2),
        "cold": "the same track and one frame of %d samples behind it: the any-length kernels into the workspace, then k_envelope_channels" % TAIL,
    }
    for k in calls:
        line[k] = dict(stats(ms[k]), spread=round(spread[k], 4))
    if args.parent_lib:
        for b in BUCKETS:
            k = "envelope_%d" % b
            line[k + "_over_parent_levels"] = round(med[k] / med["parent_levels"], 4)
            line[k + "_over_parent_decode_n"] = round(med[k] / med["parent_decode_n"], 4)
            line[k + "_no_dearer_than_parent_decode_n"] = bool(med[k] / med["parent_decode_n"] - 1.0 <= spread["parent_decode_n"])
        line["envelope_32_over_envelope_256"] = round(med["envelope_32"] / med["envelope_256"], 4)
        line["envelope_cold_256_over_parent_decode_n_cold"] = round(med["envelope_cold_256"] / med["parent_decode_n_cold"], 4)
        for kind in UNTOUCHED + ("decode_n_cold",):
            slower = med[kind] / med["parent_" + kind] - 1.0
            line["untouched_" + kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread["parent_" + kind], 4),
                                         "within_parent_spread": bool(slower <= spread["parent_" + kind])}
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("no --parent-lib: the parent's calls were not measured, so this is not the record of DESIGN.md 5.31 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
