#!/usr/bin/env python3
"""What a full decode of a whole-track stream costs.  The track is the bench track plus a 777-sample tail: 3875 x 2048
+ 777 samples of stereo `synth` audio (track 0), coded by sela_hip_encode_whole_device into 3874 frames of 2048 samples and a last
one of 2825, resident in HBM; "cut" is the same track without its tail, 3875 frames of 2048.  On HIP events, every call warmed up,
`rounds` rounds that alternate the calls, each timing `calls` back-to-back calls between two events; medians with least and largest:
  (a) sela_hip_decode_n_device of ANOTHER build of the library (--parent-lib: the parent commit's libsela_hip.so) on the tailed
      stream: the any-length route (2), what a full decode of such a stream cost;
  (b) the parent's same call on the cut stream: the 2048-sample route (1), the floor;
  (c) sela_hip_decode_whole_device on the tailed stream: the 2048-sample decoder with the last frame beside it (route 3);
  (d) this tree's sela_hip_decode_n_device on both streams: each must lie inside the spread of the parent's rounds
      (`d_tailed_within_a_spread`, `d_cut_within_b_spread`), the existing routes being untouched;
  (e) sela_hip_decode against sela_hip_decode_whole on the tailed stream from page-locked memory, wall clock, `host_rounds` rounds of
      `host_calls` calls each, alternating.
(c) is done when its median lies below (a)'s by more than the spread of (a)'s rounds: `c_beats_a`.  `c_over_b` is stated as measured.
Prints one JSON line and writes it to --out (default profiles/whole/whole_decode_bench.json).  Without --parent-lib the record is
not the required one: nothing is written and the exit code is 2.  Exit code 1: a (d) outside its spread, or (c) does not beat (a).
Run on the GPU box:  python tools/whole_decode_bench.py --parent-lib P/libsela_hip.so [--rounds 15] [--calls 20]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, TAIL, CHANNELS, BLOCK, TRACK = 3875, 777, 2, 2048, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=7)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libsela_hip.so built from the parent commit: figures (a) and (b)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whole", "whole_decode_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "whole_decode_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    n = FRAMES * BLOCK + TAIL
    d_pcm = synth.synth_pcm_torch(n, CHANNELS, TRACK, device="cuda").contiguous()
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t

    # the two streams, coded on the device
    whole = codec.WholeEncoder(n, CHANNELS)
    whole.encode(d_pcm)
    torch.cuda.synchronize()
    assert whole.n_frames == FRAMES
    tailed = (whole.frames[: int(whole.offsets[FRAMES].item())].clone(), whole.offsets[: FRAMES + 1].clone().contiguous())
    plain = codec.Encoder(FRAMES, CHANNELS)
    coded = plain.encode(d_pcm[: FRAMES * BLOCK].reshape(FRAMES, BLOCK, CHANNELS))
    torch.cuda.synchronize()
    cut = (coded.frames[: int(coded.offsets[FRAMES].item())].clone(), coded.offsets[: FRAMES + 1].clone().contiguous())

    class DecodeN:
        """sela_hip_decode_n_device of one library on one stream, with buffers of its own."""

        def __init__(self, L, frames, offsets, stride=2 * BLOCK):
            L.sela_hip_decode_n_workspace_bytes.restype = sz
            L.sela_hip_decode_n_workspace_bytes.argtypes = [u32, u32, u32]
            ws = int(L.sela_hip_decode_n_workspace_bytes(FRAMES, CHANNELS, stride))
            self.fn = L.sela_hip_decode_n_device
            self.fn.restype = C.c_int
            self.pcm = torch.empty((FRAMES * stride, CHANNELS), dtype=torch.int16, device="cuda")
            self.sample_offsets = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")
            self.ws = torch.empty(ws, dtype=torch.uint8, device="cuda")
            self.keep = (frames, offsets)
            self.args = [vp(frames.data_ptr()), vp(offsets.data_ptr()), u32(FRAMES), u32(CHANNELS), u32(stride), vp(self.pcm.data_ptr()), vp(self.sample_offsets.data_ptr()),
                         vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(ws), vp(stream)]

        def __call__(self):
            rc = self.fn(*self.args)
            assert rc == 0, rc

        def result(self):
            torch.cuda.synchronize()
            st = self.status.cpu().numpy()
            assert int(st[0]) == 0 and int(st[1]) == 0, st
            return self.pcm[: int(self.sample_offsets[FRAMES].item())], int(st[3])

    class DecodeWhole:
        """sela_hip_decode_whole_device on one stream, with buffers of its own."""

        def __init__(self, frames, offsets):
            ws = int(lib.sela_hip_decode_whole_workspace_bytes(FRAMES, CHANNELS))
            cap = FRAMES * BLOCK + BLOCK - 1
            self.pcm = torch.empty((cap, CHANNELS), dtype=torch.int16, device="cuda")
            self.n_samples = torch.zeros(1, dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")
            self.ws = torch.empty(ws, dtype=torch.uint8, device="cuda")
            self.keep = (frames, offsets)
            self.args = [frames.data_ptr(), offsets.data_ptr(), FRAMES, CHANNELS, self.pcm.data_ptr(), cap, self.n_samples.data_ptr(), self.status.data_ptr(),
                         self.ws.data_ptr(), ws, stream]

        def __call__(self):
            rc = lib.sela_hip_decode_whole_device(*self.args)
            assert rc == 0, rc

        def result(self):
            torch.cuda.synchronize()
            st = self.status.cpu().numpy()
            assert int(st[0]) == 0 and int(st[1]) == 0, st
            return self.pcm[: int(self.n_samples.item())], int(st[3])

    calls = {"c_whole_tailed": DecodeWhole(*tailed), "d_decode_n_tailed": DecodeN(lib, *tailed), "d_decode_n_cut": DecodeN(lib, *cut)}
    # every call's samples are this tree's sela_hip_decode_n_device's on the same stream, by the route named
    want = {"c_whole_tailed": ("d_decode_n_tailed", 3), "d_decode_n_tailed": ("d_decode_n_tailed", 2), "d_decode_n_cut": ("d_decode_n_cut", 1)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls["a_parent_tailed"], calls["b_parent_cut"] = DecodeN(parent, *tailed), DecodeN(parent, *cut)
        want["a_parent_tailed"], want["b_parent_cut"] = ("d_decode_n_tailed", 2), ("d_decode_n_cut", 1)
    for _ in range(2):
        for c in calls.values():
            c()
    results = {k: c.result() for k, c in calls.items()}
    for k, (pcm, route) in results.items():
        assert route == want[k][1] and torch.equal(pcm, results[want[k][0]][0]), (k, route, tuple(pcm.shape))
    assert results["c_whole_tailed"][0].shape[0] == n and results["d_decode_n_cut"][0].shape[0] == FRAMES * BLOCK

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    ms = {k: [] for k in calls}
    names = list(calls)
    for r in range(args.rounds):
        order = names[r % len(names):] + names[: r % len(names)]  # (alternating: every call takes its turn at every place)
        for k in (order if r % 2 == 0 else order[::-1]):
            ms[k].append(timed(calls[k]))

    # (e) the host calls, from page-locked memory
    lib.sela_hip_host_alloc.restype = vp
    lib.sela_hip_host_alloc.argtypes = [sz]
    h_frames, h_offs = tailed[0].cpu().numpy(), tailed[1].cpu().numpy().view(np.uint64)
    p_frames = lib.sela_hip_host_alloc(len(h_frames))
    cap = FRAMES * BLOCK + BLOCK - 1
    p_pcm = lib.sela_hip_host_alloc(cap * CHANNELS * 2)
    assert p_frames and p_pcm
    C.memmove(p_frames, h_frames.ctypes.data, len(h_frames))
    back = np.ctypeslib.as_array((C.c_int16 * (cap * CHANNELS)).from_address(p_pcm)).reshape(cap, CHANNELS)
    n_samples = np.zeros(1, np.uint64)
    host = {"e_host_decode": lambda: lib.sela_hip_decode(p_frames, h_offs.ctypes.data, FRAMES, CHANNELS, p_pcm),
            "e_host_decode_whole": lambda: lib.sela_hip_decode_whole(p_frames, h_offs.ctypes.data, FRAMES, CHANNELS, p_pcm, cap, n_samples.ctypes.data)}
    expect = results["c_whole_tailed"][0].cpu().numpy()
    for k, call in host.items():
        back[:] = 0
        assert call() == 0, k
        assert np.array_equal(back[:n], expect), k
    assert int(n_samples[0]) == n
    host_ms = {k: [] for k in host}
    for r in range(args.host_rounds):
        for k in (list(host) if r % 2 == 0 else list(host)[::-1]):
            t0 = time.perf_counter()
            for _ in range(args.host_calls):
                host[k]()
            host_ms[k].append((time.perf_counter() - t0) * 1e3 / args.host_calls)
    lib.sela_hip_host_free(vp(p_frames)), lib.sela_hip_host_free(vp(p_pcm))

    stats = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4),  # noqa: E731
                       "spread": round((max(v) - min(v)) / float(np.median(v)), 4)}
    med = {k: float(np.median(v)) for k, v in list(ms.items()) + list(host_ms.items())}
    line = {"frames": FRAMES, "tail_samples": TAIL, "channels": CHANNELS, "input": "synth_pcm_torch(3875 * 2048 + 777, 2, track=0)", "rounds": args.rounds,
            "calls_per_round": args.calls, "host_rounds": args.host_rounds, "host_calls_per_round": args.host_calls, "bytes_tailed": int(tailed[0].numel()),
            "bytes_cut": int(cut[0].numel())}
    for k in names:
        line[k] = stats(ms[k])
    for k in host:
        line[k] = stats(host_ms[k])
    line["e_whole_over_decode"] = round(med["e_host_decode_whole"] / med["e_host_decode"], 4)
    rc = 0
    if args.parent_lib:
        a, b = ms["a_parent_tailed"], ms["b_parent_cut"]
        a_spread_ms, b_spread_ms = max(a) - min(a), max(b) - min(b)
        line["c_over_a"] = round(med["c_whole_tailed"] / med["a_parent_tailed"], 4)
        line["c_over_b"] = round(med["c_whole_tailed"] / med["b_parent_cut"], 4)
        line["a_over_b"] = round(med["a_parent_tailed"] / med["b_parent_cut"], 4)
        line["c_beats_a"] = bool(med["a_parent_tailed"] - med["c_whole_tailed"] > a_spread_ms)
        line["d_tailed_over_a"] = round(med["d_decode_n_tailed"] / med["a_parent_tailed"], 4)
        line["d_cut_over_b"] = round(med["d_decode_n_cut"] / med["b_parent_cut"], 4)
        line["d_tailed_within_a_spread"] = bool(min(a) <= med["d_decode_n_tailed"] <= max(a))
        line["d_cut_within_b_spread"] = bool(min(b) <= med["d_decode_n_cut"] <= max(b))
        rc = 0 if line["c_beats_a"] and line["d_tailed_within_a_spread"] and line["d_cut_within_b_spread"] else 1
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("without --parent-lib this is not the record of DESIGN.md 5.21: nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    if rc:
        print("REQUIRED CONDITION MISSED: c_beats_a %s, d_tailed_within_a_spread %s, d_cut_within_b_spread %s"
              % (line["c_beats_a"], line["d_tailed_within_a_spread"], line["d_cut_within_b_spread"]))
    return rc


if __name__ == "__main__":
    sys.exit(main())
