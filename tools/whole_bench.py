#!/usr/bin/env python3
"""What keeping the tail costs.  The track is the bench track plus a 777-sample tail: 3875 x 2048 + 777 samples of
stereo `synth` audio (track 0), resident in HBM.  On HIP events, every call warmed up, `rounds` rounds that alternate the calls, each
timing `calls` back-to-back calls between two events; medians with least and largest:
  (a) sela_hip_encode_device of ANOTHER build of the library (--parent-lib: the parent commit's libsela_hip.so) on the 3875 whole
      frames -- the baseline;
  (c) sela_hip_encode_whole_device on the whole track: the last frame's chain forked onto a side stream beside the main launch,
      the form the tree holds (the serial form, figure (b), lost to it and was deleted: DESIGN.md 9, profiles/whole/forms_ab.json);
  (d) this tree's sela_hip_encode_device on the 3875 frames: it must sit inside the spread of (a)'s rounds (`d_within_a_spread`);
  (e) sela_hip_decode_n_device on the tailed stream (the any-length route, 2) against the same track without its tail (the
      2048-sample route, 1).
Prints one JSON line and writes it to --out (default profiles/whole/whole_bench.json).  Without --parent-lib the record is not the
required one: nothing is written and the exit code is 2.  Exit code 1: (d) is slower than (a) by more than (a)'s spread.
Run on the GPU box:  python tools/whole_bench.py --parent-lib P/libsela_hip.so [--rounds 15] [--calls 20]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, TAIL, CHANNELS, BLOCK, TRACK = 3875, 777, 2, 2048, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libsela_hip.so built from the parent commit: figure (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whole", "whole_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "whole_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    n = FRAMES * BLOCK + TAIL
    d_pcm = synth.synth_pcm_torch(n, CHANNELS, TRACK, device="cuda").contiguous()
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t

    class Encode:
        """One encode entry of one library with buffers of its own."""

        def __init__(self, L, whole):
            self.whole, self.frames_n = whole, FRAMES
            L.sela_hip_encode_workspace_bytes.restype = sz
            L.sela_hip_encode_workspace_bytes.argtypes = [u32, u32]
            L.sela_hip_encode_bound_bytes.restype = sz
            L.sela_hip_encode_bound_bytes.argtypes = [u32, u32]
            if whole:
                L.sela_hip_encode_whole_workspace_bytes.restype = sz
                L.sela_hip_encode_whole_workspace_bytes.argtypes = [u64, u32]
                L.sela_hip_encode_whole_bound_bytes.restype = sz
                L.sela_hip_encode_whole_bound_bytes.argtypes = [u64, u32]
                ws, cap = int(L.sela_hip_encode_whole_workspace_bytes(n, CHANNELS)), int(L.sela_hip_encode_whole_bound_bytes(n, CHANNELS))
                self.fn = L.sela_hip_encode_whole_device
            else:
                ws, cap = int(L.sela_hip_encode_workspace_bytes(FRAMES, CHANNELS)), int(L.sela_hip_encode_bound_bytes(FRAMES, CHANNELS))
                self.fn = L.sela_hip_encode_device
            self.fn.restype = C.c_int
            self.frames = torch.empty(cap, dtype=torch.uint8, device="cuda")
            self.offsets = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")
            self.ws = torch.empty(ws, dtype=torch.uint8, device="cuda")
            head = [vp(d_pcm.data_ptr()), u64(n) if whole else u32(FRAMES), u32(CHANNELS), vp(self.frames.data_ptr()), sz(cap), vp(self.offsets.data_ptr()),
                    vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(ws)]
            self.args = head + ([vp(stream), u32(0)] if whole else [vp(None), vp(stream)])

        def __call__(self):
            rc = self.fn(*self.args)
            assert rc == 0, rc

        def result(self):
            torch.cuda.synchronize()
            st = self.status.cpu().numpy()
            assert codec.encode_status_error(st) == 0 and int(st[1]) == 0, st
            total = int(self.offsets[FRAMES].item())
            return self.frames[:total].clone(), self.offsets.clone(), total

    calls = {"d_plain": Encode(lib, False), "c_whole": Encode(lib, True)}
    if args.parent_lib:
        calls["a_parent_plain"] = Encode(C.CDLL(os.path.abspath(args.parent_lib)), False)
    for _ in range(2):
        for c in calls.values():
            c()
    out = {k: c.result() for k, c in calls.items()}
    if args.parent_lib:
        assert torch.equal(out["d_plain"][0], out["a_parent_plain"][0]) and torch.equal(out["d_plain"][1], out["a_parent_plain"][1]), "the plain call's bytes differ from the parent's"
    whole_frames, whole_offsets, whole_bytes = out["c_whole"]
    before_last = int(whole_offsets[FRAMES - 1].item())
    assert torch.equal(whole_frames[:before_last], out["d_plain"][0][:before_last]), "frames 0 .. F-2 differ from the plain call's"

    # (e) the decode side: the tailed stream, and the same track without its tail
    plain_frames, plain_offsets, plain_bytes = out["d_plain"]
    decoders = {"e_decode_tailed": (codec.DecoderN(FRAMES, CHANNELS, 2 * BLOCK), whole_frames, whole_offsets.contiguous()),
                "e_decode_cut": (codec.DecoderN(FRAMES, CHANNELS, 2 * BLOCK), plain_frames, plain_offsets.contiguous())}
    routes = {}
    for k, (dec, fr, of) in decoders.items():
        dec.decode(fr, of, FRAMES)
        dec.check()
        routes[k] = dec.route()
        calls[k] = (lambda dec=dec, fr=fr, of=of: dec.decode(fr, of, FRAMES))
    assert routes == {"e_decode_tailed": 2, "e_decode_cut": 1}, routes

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
    stats = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4),  # noqa: E731
                       "spread": round((max(v) - min(v)) / float(np.median(v)), 4)}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {"frames": FRAMES, "tail_samples": TAIL, "channels": CHANNELS, "input": "synth_pcm_torch(3875 * 2048 + 777, 2, track=0)", "rounds": args.rounds,
            "calls_per_round": args.calls, "form": "forked", "bytes_plain_3875_frames": plain_bytes, "bytes_whole": whole_bytes}
    for k in names:
        line[k] = stats(ms[k])
    line["e_tailed_over_cut"] = round(med["e_decode_tailed"] / med["e_decode_cut"], 4)
    rc = 0
    if args.parent_lib:
        a = ms["a_parent_plain"]
        spread = (max(a) - min(a)) / med["a_parent_plain"]
        line["d_over_a"] = round(med["d_plain"] / med["a_parent_plain"], 4)
        line["d_within_a_spread"] = bool(med["d_plain"] / med["a_parent_plain"] - 1.0 <= spread)
        line["c_over_a"] = round(med["c_whole"] / med["a_parent_plain"], 4)
        rc = 0 if line["d_within_a_spread"] else 1
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("without --parent-lib this is not the record of DESIGN.md 5.19: nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    if rc:
        print("REQUIRED CONDITION MISSED: (d) over (a) %.4f beyond (a)'s spread" % line["d_over_a"])
    return rc


if __name__ == "__main__":
    sys.exit(main())
