#!/usr/bin/env python3
"""What the salvage of a payload costs on the device, on tools/digest_bench.py's protocol.  The input is the bench's
synthetic track (3875 stereo frames of 2048 samples, track 0) as sela_hip_encode_device codes it, in device memory, intact and with
1 and with 64 sync words flipped, spread evenly over the track.  On HIP events, everything warmed up, `rounds` rounds that alternate
the calls, each timing `calls` back-to-back calls between two events; medians with the least and the largest:
  (a) sela_hip_salvage_frames_device on the three payloads against the PARENT build's sela_hip_index_frames_device on the intact
      one (--parent-lib: the parent commit's libsela_hip.so).  The salvage does strictly more -- a search, a backward scan, the
      gaps -- so this is a cost to report, not a bar to clear.  With it the frames found in each case;
  (b) sela_hip_salvage_payload_device against the parent's index call followed by a device-to-device copy of the same bytes;
      the device copy's rate (bytes copied per second, counted once) next to the copy kernel's, which comes from --kernel-stats:
      the kernel statistics CSV of one `rocprofv3 --kernel-trace --stats -- python tools/salvage_bench.py --only
      salvage_payload_intact` run of its own;
  (c) the untouched neighbours from this build against the parent's, alternating: sela_hip_index_frames_device and
      sela_hip_decode_payload_device.  They must lie within the parent build's own spread of repeats, which is stated.
Before anything is timed the device's records and totals are held against the host walk's on each payload, the compacted payload
against the frames back to back, and the neighbours' outputs against the parent's.  Prints one JSON line and writes it to --out
(default profiles/salvage/salvage_bench.json).  Without --parent-lib nothing is written and the exit code is 2; where a neighbour
leaves the parent's spread the exit code is 1.
Run on the GPU box:  python tools/salvage_bench.py --parent-lib path/to/parent/libsela_hip.so [--kernel-stats FILE] [--rounds 20] [--calls 10]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, TRACK = 3875, 2, 0


def copy_kernel_us(path):
    """The average time of k_salvage_copy in a rocprofv3 kernel statistics CSV, in microseconds (None: not there)."""
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            if "k_salvage_copy" in row.get("Name", ""):
                if row.get("AverageNs"):
                    return float(row["AverageNs"]) / 1e3
                return float(row["TotalDurationNs"]) / float(row["Calls"]) / 1e3
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's kernel statistics CSV of an --only salvage_payload_intact run")
    ap.add_argument("--only", default=None, help="time this one call and nothing else (for a trace run); nothing is written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "salvage", "salvage_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "salvage_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t

    out = codec.Encoder(FRAMES, CHANNELS).encode(synth.synth_frames_torch(FRAMES, CHANNELS, TRACK, device="cuda").contiguous())
    torch.cuda.synchronize()
    frames_h, offs_h = out.to_host()
    n_bytes = int(len(frames_h))
    payloads_h = {}
    for damaged in (0, 1, 64):
        body = frames_h.copy()
        for k in range(damaged):
            body[int(offs_h[(2 * k + 1) * FRAMES // (2 * damaged)])] ^= 0xFF
        payloads_h[damaged] = body
    payloads = {k: torch.from_numpy(v).cuda() for k, v in payloads_h.items()}
    walks = {k: codec.salvage_frames(v, CHANNELS, FRAMES) for k, v in payloads_h.items()}

    class Salvage:  # sela_hip_salvage_frames_device, or (copy) sela_hip_salvage_payload_device
        def __init__(self, damaged, max_frames=FRAMES, copy=False):
            self.payload, self.max_frames, self.copy = payloads[damaged], max_frames, copy
            self.ws = torch.empty(codec.salvage_workspace_bytes(n_bytes, max_frames), dtype=torch.uint8, device="cuda")
            self.records = torch.zeros((max_frames, 3), dtype=torch.int64, device="cuda")
            self.totals = torch.zeros(4, dtype=torch.int64, device="cuda")
            self.offsets = torch.zeros(max_frames + 1, dtype=torch.int64, device="cuda")
            self.out = torch.zeros(n_bytes if copy else 4, dtype=torch.uint8, device="cuda")

        def __call__(self):
            if self.copy:
                rc = lib.sela_hip_salvage_payload_device(self.payload.data_ptr(), n_bytes, self.max_frames, CHANNELS, self.out.data_ptr(), self.out.numel(),
                                                         self.offsets.data_ptr(), self.records.data_ptr(), self.totals.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream)
            else:
                rc = lib.sela_hip_salvage_frames_device(self.payload.data_ptr(), n_bytes, self.max_frames, CHANNELS, self.records.data_ptr(), self.totals.data_ptr(),
                                                        self.ws.data_ptr(), self.ws.numel(), stream)
            assert rc == 0, rc

    class Index:  # sela_hip_index_frames_device
        def __init__(self, L):
            self.L = L
            L.sela_hip_index_workspace_bytes.restype, L.sela_hip_index_workspace_bytes.argtypes = sz, [sz, u32]
            self.ws = torch.empty(int(L.sela_hip_index_workspace_bytes(n_bytes, FRAMES)), dtype=torch.uint8, device="cuda")
            self.offsets = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
            self.count = torch.zeros(1, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_index_frames_device(vp(payloads[0].data_ptr()), sz(n_bytes), u32(FRAMES), u32(CHANNELS), vp(self.offsets.data_ptr()), vp(self.count.data_ptr()),
                                                     vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.offsets, self.count

    class IndexThenCopy:  # the parent's index call, then a device-to-device copy of the payload's bytes
        def __init__(self, L):
            self.index = Index(L)
            self.out = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")

        def __call__(self):
            self.index()
            self.out.copy_(payloads[0])

    class DeviceCopy:
        def __init__(self):
            self.out = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")

        def __call__(self):
            self.out.copy_(payloads[0])

    class DecodePayload:  # sela_hip_decode_payload_device
        def __init__(self, L):
            self.L = L
            L.sela_hip_index_workspace_bytes.restype, L.sela_hip_index_workspace_bytes.argtypes = sz, [sz, u32]
            L.sela_hip_decode_workspace_bytes.restype, L.sela_hip_decode_workspace_bytes.argtypes = sz, [u32, u32]
            self.ws = torch.empty(int(L.sela_hip_index_workspace_bytes(n_bytes, FRAMES)) + int(L.sela_hip_decode_workspace_bytes(FRAMES, CHANNELS)), dtype=torch.uint8,
                                  device="cuda")
            self.pcm = torch.zeros((FRAMES, 2048, CHANNELS), dtype=torch.int16, device="cuda")
            self.offsets = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
            self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_decode_payload_device(vp(payloads[0].data_ptr()), sz(n_bytes), u32(FRAMES), u32(CHANNELS), vp(self.pcm.data_ptr()), vp(self.offsets.data_ptr()),
                                                       vp(self.count.data_ptr()), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.pcm, self.offsets, self.count, self.status

    calls = {"salvage_frames_intact": Salvage(0), "salvage_frames_1": Salvage(1), "salvage_frames_64": Salvage(64),
             "salvage_payload_intact": Salvage(0, copy=True), "salvage_payload_64": Salvage(64, copy=True),
             "device_copy": DeviceCopy(), "index": Index(lib), "decode_payload": DecodePayload(lib)}
    untouched = ("index", "decode_payload")
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls.update({"parent_index": Index(parent), "parent_decode_payload": DecodePayload(parent), "parent_index_then_copy": IndexThenCopy(parent)})
    if args.only:
        calls = {args.only: calls[args.only]}
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()

    found = {}
    if not args.only:
        for name, c in calls.items():
            if not isinstance(c, Salvage):
                continue
            damaged = [k for k, p in payloads.items() if p is c.payload][0]
            want, want_totals = walks[damaged]
            totals = c.totals.cpu().numpy().view(np.uint64)
            assert totals.tolist() == want_totals.tolist(), "%s: the totals differ from the host walk's" % name
            got = np.ascontiguousarray(c.records[:len(want)].cpu().numpy()).view(codec.SALVAGED_DTYPE).reshape(len(want))
            assert got.tobytes() == want.tobytes(), "%s: the records differ from the host walk's" % name
            if c.copy:
                packed = np.concatenate([payloads_h[damaged][int(r["offset"]):int(r["offset"]) + int(r["bytes"])] for r in want])
                assert c.out[:len(packed)].cpu().numpy().tobytes() == packed.tobytes(), "%s: the compacted payload is not the frames back to back" % name
            found[name] = {"frames": int(totals[0]), "gaps": int(totals[1]), "bytes_kept": int(totals[2])}
        assert found["salvage_frames_intact"]["frames"] == FRAMES and found["salvage_frames_1"]["frames"] == FRAMES - 1 and found["salvage_frames_64"]["frames"] == FRAMES - 64
        if args.parent_lib:
            for kind in untouched:
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
    line = {"frames": FRAMES, "channels": CHANNELS, "payload_bytes": n_bytes, "input": "synth_frames_torch(3875, 2, track=0) as sela_hip_encode_device codes it",
            "damage": "sync words flipped at frames (2 k + 1) * 3875 / (2 n), k < n, for n = 1 and n = 64", "rounds": args.rounds, "calls_per_round": args.calls,
            "workspace_bytes": codec.salvage_workspace_bytes(n_bytes, FRAMES), "found": found}
    for k in calls:
        line[k] = dict(stats(ms[k]), spread=round(spread[k], 4))
    if args.only or not args.parent_lib:
        print(json.dumps(line))
        print("no --parent-lib (or --only): the parent's calls were not measured, so this is not the record of DESIGN.md 5.30 and nothing is written")
        return 2
    for k in ("salvage_frames_intact", "salvage_frames_1", "salvage_frames_64"):
        line[k + "_over_parent_index"] = round(med[k] / med["parent_index"], 4)
    line["salvage_payload_intact_over_parent_index_then_copy"] = round(med["salvage_payload_intact"] / med["parent_index_then_copy"], 4)
    line["device_copy_gb_per_s"] = round(n_bytes / (med["device_copy"] * 1e-3) / 1e9, 1)
    us = copy_kernel_us(args.kernel_stats) if args.kernel_stats else None
    line["copy_kernel"] = {"average_us": round(us, 2), "gb_per_s": round(n_bytes / (us * 1e-6) / 1e9, 1), "from": "rocprofv3 --kernel-trace --stats, a run of its own"} if us \
        else "not measured"
    failed = []
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
        print("NOT WITHIN THE PARENT'S SPREAD: %s" % k)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
