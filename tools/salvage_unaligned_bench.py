#!/usr/bin/env python3
"""What the salvage at any byte costs on the device, on tools/salvage_bench.py's protocol.  The input is the bench's
synthetic track (3875 stereo frames of 2048 samples, track 0) as sela_hip_encode_device codes it, in device memory: intact, with 64
sync words flipped, and with 64 single bytes inserted in front of frames, both spread evenly over the track.  On HIP events,
everything warmed up, `rounds` rounds that alternate the calls, each timing `calls` back-to-back calls between two events; medians
with the least and the largest:
  (a) sela_hip_salvage_frames_unaligned_device and sela_hip_salvage_payload_unaligned_device on the three payloads, each against
      the PARENT build's sela_hip_salvage_frames_device / _payload_device (--parent-lib: the parent commit's libsela_hip.so) on the
      intact and the 64-headers payloads in the same process.  Four phases per word are strictly more work: a cost to report, no bar;
  (b) the copy kernel's rate at shift 0 (the intact payload) and at a shift of 1 byte (the intact payload behind one byte of garbage)
      next to a device-to-device copy's; the kernel's times come from --kernel-stats-0 / --kernel-stats-1: the kernel statistics CSV
      of one `rocprofv3 --kernel-trace --stats -- python tools/salvage_unaligned_bench.py --only payload_intact` (or `--only
      payload_prefix1`) run of its own each;
  (c) the untouched neighbours from this build against the parent's, alternating: sela_hip_index_frames_device,
      sela_hip_salvage_frames_device, sela_hip_salvage_payload_device and sela_hip_decode_payload_device.  They must lie within the
      parent build's own spread of repeats, which is stated.
Before anything is timed the device's records and totals are held against the host walk's on each payload, the compacted payload
against the frames back to back, and the neighbours' outputs against the parent's.  Prints one JSON line and writes it to --out
(default profiles/salvage/salvage_unaligned_bench.json).  Without --parent-lib nothing is written and the exit code is 2; where a
neighbour leaves the parent's spread the exit code is 1.
Run on the GPU box:  python tools/salvage_unaligned_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 20] [--calls 10]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, TRACK, DAMAGED = 3875, 2, 0, 64


def copy_kernel_us(path):
    """The average time of k_salvage_ua_copy in a rocprofv3 kernel statistics CSV, in microseconds (None: not there)."""
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            if "k_salvage_ua_copy" in row.get("Name", ""):
                if row.get("AverageNs"):
                    return float(row["AverageNs"]) / 1e3
                return float(row["TotalDurationNs"]) / float(row["Calls"]) / 1e3
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats-0", default=None, help="rocprofv3's kernel statistics CSV of an --only payload_intact run")
    ap.add_argument("--kernel-stats-1", default=None, help="rocprofv3's kernel statistics CSV of an --only payload_prefix1 run")
    ap.add_argument("--only", default=None, help="time this one call and nothing else (for a trace run); nothing is written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "salvage", "salvage_unaligned_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "salvage_unaligned_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t

    out = codec.Encoder(FRAMES, CHANNELS).encode(synth.synth_frames_torch(FRAMES, CHANNELS, TRACK, device="cuda").contiguous())
    torch.cuda.synchronize()
    frames_h, offs_h = out.to_host()
    spots = [int(offs_h[(2 * k + 1) * FRAMES // (2 * DAMAGED)]) for k in range(DAMAGED)]
    flipped = frames_h.copy()
    flipped[spots] ^= 0xFF
    pieces, last = [], 0
    for at in spots:
        pieces += [frames_h[last:at], np.full(1, 0x11, np.uint8)]
        last = at
    inserted = np.concatenate(pieces + [frames_h[last:]])
    payloads_h = {"intact": frames_h, "headers64": flipped, "inserted64": inserted, "prefix1": np.concatenate([np.full(1, 0x11, np.uint8), frames_h])}
    capacity = max(len(v) for v in payloads_h.values())
    payloads = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in payloads_h.items()}
    n_bytes = len(frames_h)

    class Salvage:  # a salvage call of library L: frames or (copy) payload, at word positions or (unaligned) at any byte
        def __init__(self, L, which, copy=False, unaligned=False):
            self.L, self.which, self.copy, self.unaligned = L, which, copy, unaligned
            self.payload = payloads[which]
            name = "sela_hip_salvage_%s%s_device" % ("payload" if copy else "frames", "_unaligned" if unaligned else "")
            self.fn = getattr(L, name)
            sized = getattr(L, "sela_hip_salvage_unaligned_workspace_bytes" if unaligned else "sela_hip_salvage_workspace_bytes")
            sized.restype, sized.argtypes = sz, [sz, u32]
            self.ws = torch.empty(int(sized(capacity, FRAMES)), dtype=torch.uint8, device="cuda")
            self.records = torch.zeros((FRAMES, 3), dtype=torch.int64, device="cuda")
            self.totals = torch.zeros(4, dtype=torch.int64, device="cuda")
            self.offsets = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
            self.out = torch.zeros(capacity // 4 * 4 if copy else 4, dtype=torch.uint8, device="cuda")

        def __call__(self):
            p = self.payload
            if self.copy:
                rc = self.fn(vp(p.data_ptr()), sz(p.numel()), u32(FRAMES), u32(CHANNELS), vp(self.out.data_ptr()), sz(self.out.numel()), vp(self.offsets.data_ptr()),
                             vp(self.records.data_ptr()), vp(self.totals.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            else:
                rc = self.fn(vp(p.data_ptr()), sz(p.numel()), u32(FRAMES), u32(CHANNELS), vp(self.records.data_ptr()), vp(self.totals.data_ptr()), vp(self.ws.data_ptr()),
                             sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            found = int(self.totals.cpu()[0])
            kept = int(self.totals.cpu()[2])
            return (self.records[:found], self.totals) + ((self.offsets[:found + 1], self.out[:kept]) if self.copy else ())

    class Index:  # sela_hip_index_frames_device
        def __init__(self, L):
            self.L = L
            L.sela_hip_index_workspace_bytes.restype, L.sela_hip_index_workspace_bytes.argtypes = sz, [sz, u32]
            self.ws = torch.empty(int(L.sela_hip_index_workspace_bytes(n_bytes, FRAMES)), dtype=torch.uint8, device="cuda")
            self.offsets = torch.zeros(FRAMES + 1, dtype=torch.int64, device="cuda")
            self.count = torch.zeros(1, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_index_frames_device(vp(payloads["intact"].data_ptr()), sz(n_bytes), u32(FRAMES), u32(CHANNELS), vp(self.offsets.data_ptr()),
                                                     vp(self.count.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.offsets, self.count

    class DeviceCopy:
        def __init__(self):
            self.out = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")

        def __call__(self):
            self.out.copy_(payloads["intact"])

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
            rc = self.L.sela_hip_decode_payload_device(vp(payloads["intact"].data_ptr()), sz(n_bytes), u32(FRAMES), u32(CHANNELS), vp(self.pcm.data_ptr()),
                                                       vp(self.offsets.data_ptr()), vp(self.count.data_ptr()), vp(self.status.data_ptr()), vp(self.ws.data_ptr()),
                                                       sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.pcm, self.offsets, self.count, self.status

    calls = {}
    for which in ("intact", "headers64", "inserted64"):
        calls["frames_" + which] = Salvage(lib, which, unaligned=True)
        calls["payload_" + which] = Salvage(lib, which, copy=True, unaligned=True)
    calls["payload_prefix1"] = Salvage(lib, "prefix1", copy=True, unaligned=True)
    calls.update({"device_copy": DeviceCopy(), "index": Index(lib), "salvage_frames": Salvage(lib, "intact"), "salvage_payload": Salvage(lib, "intact", copy=True),
                  "decode_payload": DecodePayload(lib)})
    untouched = ("index", "salvage_frames", "salvage_payload", "decode_payload")
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls.update({"parent_index": Index(parent), "parent_salvage_frames": Salvage(parent, "intact"), "parent_salvage_payload": Salvage(parent, "intact", copy=True),
                      "parent_decode_payload": DecodePayload(parent), "parent_salvage_frames_headers64": Salvage(parent, "headers64"),
                      "parent_salvage_payload_headers64": Salvage(parent, "headers64", copy=True)})
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
            body = payloads_h[c.which]
            want, want_totals = codec.salvage_frames(body, CHANNELS, FRAMES, unaligned=c.unaligned)
            totals = c.totals.cpu().numpy().view(np.uint64)
            assert totals.tolist() == want_totals.tolist(), "%s: the totals differ from the host walk's" % name
            got = np.ascontiguousarray(c.records[:len(want)].cpu().numpy()).view(codec.SALVAGED_DTYPE).reshape(len(want))
            assert got.tobytes() == want.tobytes(), "%s: the records differ from the host walk's" % name
            if c.copy:
                packed = np.concatenate([body[int(r["offset"]):int(r["offset"]) + int(r["bytes"])] for r in want])
                assert c.out[:len(packed)].cpu().numpy().tobytes() == packed.tobytes(), "%s: the compacted payload is not the frames back to back" % name
            found[name] = {"frames": int(totals[0]), "gaps": int(totals[1]), "bytes_kept": int(totals[2])}
        assert found["frames_intact"]["frames"] == FRAMES and found["frames_headers64"]["frames"] == FRAMES - DAMAGED
        assert found["frames_inserted64"] == {"frames": FRAMES, "gaps": DAMAGED, "bytes_kept": n_bytes}, "every frame behind 64 inserted bytes is taken"
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
            "damage": "at frames (2 k + 1) * 3875 / 128, k < 64: the sync word flipped (headers64), or one byte inserted in front (inserted64); prefix1: one byte in front of all",
            "rounds": args.rounds, "calls_per_round": args.calls, "workspace_bytes": codec.salvage_workspace_bytes(capacity, FRAMES, unaligned=True), "found": found}
    for k in calls:
        line[k] = dict(stats(ms[k]), spread=round(spread[k], 4))
    if args.only or not args.parent_lib:
        print(json.dumps(line))
        print("no --parent-lib (or --only): the parent's calls were not measured, so this is not the record of DESIGN.md 5.33 and nothing is written")
        return 2
    for kind in ("frames", "payload"):
        line[kind + "_intact_over_parent_salvage"] = round(med[kind + "_intact"] / med["parent_salvage_" + kind], 4)
        line[kind + "_headers64_over_parent_salvage"] = round(med[kind + "_headers64"] / med["parent_salvage_%s_headers64" % kind], 4)
        line[kind + "_inserted64_over_parent_salvage_headers64"] = round(med[kind + "_inserted64"] / med["parent_salvage_%s_headers64" % kind], 4)
    line["device_copy_gb_per_s"] = round(n_bytes / (med["device_copy"] * 1e-3) / 1e9, 1)
    for shift, path in ((0, args.kernel_stats_0), (1, args.kernel_stats_1)):
        us = copy_kernel_us(path) if path else None
        line["copy_kernel_shift_%d" % shift] = {"average_us": round(us, 2), "gb_per_s": round(n_bytes / (us * 1e-6) / 1e9, 1),
                                                "from": "rocprofv3 --kernel-trace --stats, a run of its own"} if us else "not measured"
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
