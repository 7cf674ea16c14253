#!/usr/bin/env python3
"""What measuring a stream's levels costs on the device, on tools/verify_pcm_bench.py's protocol.  The input is the
bench's synthetic track (3875 stereo frames of 2048 samples, track 0) as the encoder codes it, in device memory.  On HIP events,
everything warmed up, `rounds` rounds that alternate the calls, each timing `calls` back-to-back calls between two events; medians
with the least and the largest:
  (a) sela_hip_levels_device (k_level_frames: nothing decoded reaches memory) against sela_hip_decode_device and
      sela_hip_verify_device on the same frames from another build of the library (--parent-lib: the parent commit's
      libsela_hip.so), and against the same two calls of this build, whose results must be the parent's;
  (b) the cold route: the same track with one more frame of 777 samples behind it, which sends the whole call through the
      any-length kernels into the workspace and k_level_channels over it, against the parent's sela_hip_decode_n_device there.
Before anything is timed the records of both streams are held against numpy on the PCM the decode calls write.
Prints one JSON line and writes it to --out (default profiles/levels/levels_bench.json).  Without --parent-lib nothing is written
and the exit code is 2; where the level call is slower than the parent's decode call by more than that call's own spread, (largest -
least) / median, the record is written, the fact is printed, and the exit code is 1.
Run on the GPU box:  python tools/levels_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 20] [--calls 10]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, BLOCK, TRACK, TAIL = 3875, 2, 2048, 0, 777


def expect(pcm, so):
    """numpy on int16 PCM [total, channels] -> (peak, samples, sum, sum_squares), each [frames, channels]"""
    n = len(so) - 1
    out = [np.zeros((n, pcm.shape[1]), np.int64) for _ in range(4)]
    for f in range(n):
        v = pcm[int(so[f]): int(so[f + 1])].astype(np.int64)
        out[0][f], out[1][f], out[2][f], out[3][f] = np.abs(v).max(0), len(v), v.sum(0), (v * v).sum(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels", "levels_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "levels_bench needs a GPU: there is no CPU path to time"
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

    cold_stride = BLOCK

    class DecodeN:  # sela_hip_decode_n_device on the cold stream
        def __init__(self, L):
            self.L = L
            L.sela_hip_decode_n_workspace_bytes.restype, L.sela_hip_decode_n_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_decode_n_workspace_bytes(nf + 1, CHANNELS, cold_stride)))
            self.pcm = torch.zeros(((nf + 1) * cold_stride, CHANNELS), dtype=torch.int16, device="cuda")
            self.so, self.status = torch.zeros(nf + 2, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_decode_n_device(vp(d_cold.data_ptr()), vp(d_cold_offs.data_ptr()), u32(nf + 1), u32(CHANNELS), u32(cold_stride),
                                                 vp(self.pcm.data_ptr()), vp(self.so.data_ptr()), vp(self.status.data_ptr()), vp(self.ws.data_ptr()),
                                                 sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.pcm, self.so, self.status

    lev, lev_cold = codec.Leveler(nf, CHANNELS, BLOCK), codec.Leveler(nf + 1, CHANNELS, cold_stride)
    calls = {"levels": lambda: lev.measure(d_frames, d_offs, nf), "levels_cold": lambda: lev_cold.measure(d_cold, d_cold_offs, nf + 1),
             "decode": Decode(lib), "verify": Verify(lib), "decode_n_cold": DecodeN(lib)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls["parent_decode"], calls["parent_verify"], calls["parent_decode_n_cold"] = Decode(parent), Verify(parent), DecodeN(parent)
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    lev.check(), lev_cold.check()
    assert lev.route() == 1 and lev_cold.route() == 2, (lev.route(), lev_cold.route())

    # the records against numpy on the decoded PCM
    def hold(leveler, n, pcm, so, what):
        rec = leveler.records(leveler.levels[:n])
        want = expect(pcm, so)
        for name, w in zip(("peak", "samples", "sum", "sum_squares"), want):
            assert np.array_equal(rec[name].astype(np.int64), w), "%s: %s differs from numpy on the decoded PCM" % (what, name)
        return int((want[0] != 0).any(1).sum())

    loud = hold(lev, nf, calls["decode"].pcm.cpu().numpy(), np.arange(nf + 1) * BLOCK, "levels")
    assert lev.loud_frames() == loud
    cold_so = calls["decode_n_cold"].so.cpu().numpy()
    assert int(cold_so[-1]) == nf * BLOCK + TAIL
    hold(lev_cold, nf + 1, calls["decode_n_cold"].pcm.cpu().numpy(), cold_so, "levels (cold route)")
    if args.parent_lib:
        for kind in ("decode", "verify", "decode_n_cold"):
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
        "rounds": args.rounds, "calls_per_round": args.calls, "stream_bytes": int(len(frames_h)), "loud_frames": loud,
        "bytes_stored_per_frame": {"levels": 24 * CHANNELS, "decode": BLOCK * CHANNELS * 2},
        "cold": "the same track and one frame of %d samples behind it: the any-length kernels into the workspace, then k_level_channels" % TAIL,
    }
    for k in calls:
        line[k] = dict(stats(ms[k]), spread=round(spread[k], 4))
    slow = []
    if args.parent_lib:
        line["levels_over_parent_decode"] = round(med["levels"] / med["parent_decode"], 4)
        line["levels_over_parent_verify"] = round(med["levels"] / med["parent_verify"], 4)
        line["levels_cold_over_parent_decode_n"] = round(med["levels_cold"] / med["parent_decode_n_cold"], 4)
        line["levels_within_parent_decode_spread"] = bool(med["levels"] / med["parent_decode"] - 1.0 <= spread["parent_decode"])
        for kind in ("decode", "verify", "decode_n_cold"):
            slower = med[kind] / med["parent_" + kind] - 1.0
            line["untouched_" + kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread["parent_" + kind], 4),
                                         "within_parent_spread": bool(slower <= spread["parent_" + kind])}
        if not line["levels_within_parent_decode_spread"]:
            slow.append("levels")
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("no --parent-lib: the parent's calls were not measured, so this is not the record of DESIGN.md 5.26 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    for k in slow:
        print("SLOWER THAN THE PARENT'S DECODE CALL BY MORE THAN ITS SPREAD: %s over parent_decode %.4f, spread %.4f" % (k, line["levels_over_parent_decode"], spread["parent_decode"]))
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
