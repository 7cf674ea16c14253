#!/usr/bin/env python3
"""What measuring the levels of a 24-bit stream costs on the device, on tools/levels_bench.py's protocol.  The input
is the bench's synthetic track (3875 stereo frames of 2048 samples, track 0) widened to 24 bits -- shifted left 8, the low byte
noise -- as sela_hip_encode_i32_device codes it, in device memory.  On HIP events, everything warmed up, `rounds` rounds that
alternate the calls, each timing `calls` back-to-back calls between two events; medians with the least and the largest:
  (a) sela_hip_levels_i32_device (k_level32_direct: nothing decoded is stored twice) against sela_hip_decode_i32_device and
      sela_hip_verify_i32_device on the same frames from another build of the library (--parent-lib: the parent commit's
      libsela_hip.so), and against the same two calls of this build and its sela_hip_levels_device on the 16-bit track, whose results
      must be the parent's;
  (b) the tailed track: one more frame of 777 samples behind it, against the parent's sela_hip_decode_i32_device there;
  (c) sela_hip_levels_samples_i32_device over the decoded samples, against a device-to-device copy of the same bytes.
Before anything is timed the records of both streams are held against numpy on the samples the decode call writes.
Prints one JSON line and writes it to --out (default profiles/levels/levels32_bench.json).  Without --parent-lib nothing is written
and the exit code is 2; where the level call is slower than the parent's decode call by more than that call's own spread, (largest -
least) / median, the record is written, the fact is printed, and the exit code is 1.
Run on the GPU box:  python tools/levels32_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 20] [--calls 10]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, BLOCK, TRACK, TAIL = 3875, 2, 2048, 0, 777


def expect(dec, counts):
    """numpy on int32 [frames, channels, stride] and counts -> (peak, samples, sum, energy as Python integers), each [frames, channels]"""
    v = dec.astype(np.int64)
    keep = np.arange(dec.shape[2])[None, None, :] < counts[:, :, None]
    v = np.where(keep, v, 0)
    sq = (np.abs(v).astype(np.uint64)) ** 2
    energy = (sq & np.uint64(0xFFFFFFFF)).sum(2, dtype=np.uint64).astype(object) + ((sq >> np.uint64(32)).sum(2, dtype=np.uint64).astype(object) << 32)
    return np.abs(v).max(2), counts.astype(np.int64), v.sum(2), energy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels", "levels32_bench.json"))
    args = ap.parse_args()
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "levels32_bench needs a GPU: there is no CPU path to time"
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
    frames, offsets, _ = enc.encode(d_planar)
    enc.check()
    frames_h, offs_h = enc.to_host()
    pad = np.zeros(8, np.uint8)
    d_frames = torch.from_numpy(np.concatenate([frames_h, pad])).cuda()
    d_offs = torch.from_numpy(offs_h.view(np.int64).copy()).cuda()
    # the tailed track: one more frame, of 777 samples
    tail = (synth.synth_frames(1, CHANNELS, TRACK + 1)[0, :TAIL].T.astype(np.int32) << 8) | 0x5A
    tail_frames, tail_offs = codec.encode_i32(np.ascontiguousarray(tail)[None])
    d_tailed = torch.from_numpy(np.concatenate([frames_h, tail_frames, pad])).cuda()
    d_tailed_offs = torch.from_numpy(np.append(offs_h, offs_h[-1] + tail_offs[-1]).astype(np.uint64).view(np.int64).copy()).cuda()
    # the 16-bit track, for the untouched sela_hip_levels_device
    enc16 = codec.Encoder(nf, CHANNELS)
    out16 = enc16.encode(d_pcm16)
    torch.cuda.synchronize()
    f16_h, o16_h = out16.to_host()
    d_frames16 = torch.from_numpy(np.concatenate([f16_h, pad])).cuda()
    d_offs16 = torch.from_numpy(o16_h.view(np.int64).copy()).cuda()

    def buffers(n_bytes):
        return torch.empty(max(n_bytes, 1), dtype=torch.uint8, device="cuda")

    class DecodeI32:  # sela_hip_decode_i32_device
        def __init__(self, L, fr, of, n):
            self.L, self.fr, self.of, self.n = L, fr, of, n
            L.sela_hip_decode_i32_workspace_bytes.restype, L.sela_hip_decode_i32_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_decode_i32_workspace_bytes(n, CHANNELS, BLOCK)))
            self.samples = torch.zeros((n, CHANNELS, BLOCK), dtype=torch.int32, device="cuda")
            self.counts = torch.zeros(n * CHANNELS, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_decode_i32_device(vp(self.fr.data_ptr()), vp(self.of.data_ptr()), u32(self.n), u32(CHANNELS), u32(BLOCK), vp(self.samples.data_ptr()),
                                                   vp(self.counts.data_ptr()), vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.samples, self.counts, self.status

    class VerifyI32:  # sela_hip_verify_i32_device against the samples the track was made from
        def __init__(self, L):
            self.L = L
            L.sela_hip_verify_i32_workspace_bytes.restype, L.sela_hip_verify_i32_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_verify_i32_workspace_bytes(nf, CHANNELS, BLOCK)))
            self.counts, self.first = torch.zeros(nf, dtype=torch.int32, device="cuda"), torch.zeros(nf, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_verify_i32_device(vp(d_frames.data_ptr()), vp(d_offs.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(d_planar.data_ptr()),
                                                   vp(None), vp(self.counts.data_ptr()), vp(self.first.data_ptr()), vp(None), vp(self.status.data_ptr()),
                                                   vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.counts, self.first, self.status

    class Levels16:  # sela_hip_levels_device on the 16-bit track
        def __init__(self, L):
            self.L = L
            L.sela_hip_levels_workspace_bytes.restype, L.sela_hip_levels_workspace_bytes.argtypes = sz, [u32] * 3
            self.ws = buffers(int(L.sela_hip_levels_workspace_bytes(nf, CHANNELS, BLOCK)))
            self.levels = torch.zeros((nf, CHANNELS, 3), dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

        def __call__(self):
            rc = self.L.sela_hip_levels_device(vp(d_frames16.data_ptr()), vp(d_offs16.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(self.levels.data_ptr()),
                                               vp(None), vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(self.ws.numel()), vp(stream))
            assert rc == 0, rc

        def result(self):
            return self.levels, self.status

    lev, lev_tailed = codec.Leveler32(nf, CHANNELS, BLOCK), codec.Leveler32(nf + 1, CHANNELS, BLOCK)
    decode = DecodeI32(lib, d_frames, d_offs, nf)
    decode_tailed = DecodeI32(lib, d_tailed, d_tailed_offs, nf + 1)
    copy_to = torch.empty_like(decode.samples)
    calls = {"levels_i32": lambda: lev.measure(d_frames, d_offs, nf), "levels_i32_tailed": lambda: lev_tailed.measure(d_tailed, d_tailed_offs, nf + 1),
             "decode_i32": decode, "decode_i32_tailed": decode_tailed, "verify_i32": VerifyI32(lib), "levels": Levels16(lib)}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        calls["parent_decode_i32"], calls["parent_decode_i32_tailed"] = DecodeI32(parent, d_frames, d_offs, nf), DecodeI32(parent, d_tailed, d_tailed_offs, nf + 1)
        calls["parent_verify_i32"], calls["parent_levels"] = VerifyI32(parent), Levels16(parent)
    for _ in range(2):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    lev.check(), lev_tailed.check()
    assert lev.fallback_frames() == 0 and lev_tailed.fallback_frames() == 0
    s_levels = torch.zeros((nf, CHANNELS, 4), dtype=torch.int64, device="cuda")
    s_status = torch.zeros(4, dtype=torch.int32, device="cuda")
    s_ws = buffers(int(lib.sela_hip_levels_samples_i32_workspace_bytes(nf, CHANNELS, BLOCK)))

    def levels_samples():
        rc = lib.sela_hip_levels_samples_i32_device(vp(decode.samples.data_ptr()), vp(None), u32(nf), u32(CHANNELS), u32(BLOCK), vp(s_levels.data_ptr()),
                                                    vp(s_status.data_ptr()), vp(s_ws.data_ptr()), sz(s_ws.numel()), vp(stream))
        assert rc == 0, rc

    calls["levels_samples_i32"] = levels_samples
    calls["copy_of_the_samples"] = lambda: copy_to.copy_(decode.samples)

    # the records against numpy on the decoded samples
    def hold(leveler, dec, what):
        n = dec.n
        rec = leveler.records(leveler.levels[:n])
        want = expect(dec.samples.cpu().numpy(), dec.counts.cpu().numpy().view(np.uint32).reshape(n, CHANNELS))
        energy = rec["sum_squares_lo"].astype(object) + (rec["sum_squares_hi"].astype(object) << 64)
        for name, got, w in zip(("peak", "samples", "sum", "sum_squares"), (rec["peak"], rec["samples"], rec["sum"], energy), want):
            assert (got.astype(object) == w.astype(object)).all(), "%s: %s differs from numpy on the decoded samples" % (what, name)
        return rec, int((want[0] != 0).any(1).sum())

    rec, loud = hold(lev, decode, "levels_i32")
    assert lev.loud_frames() == loud
    hold(lev_tailed, decode_tailed, "levels_i32 (tailed)")
    assert int(decode_tailed.counts[-1].item()) == TAIL
    got, _ = codec.levels_samples_i32(decode.samples)
    assert np.array_equal(codec.Leveler32.records(got), rec), "levels_samples_i32 differs from the stream's records"
    if args.parent_lib:
        for kind in ("decode_i32", "decode_i32_tailed", "verify_i32", "levels"):
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
        "rounds": args.rounds, "calls_per_round": args.calls, "stream_bytes": int(len(frames_h)), "loud_frames": loud,
        "bytes_stored_per_frame": {"levels_i32": 32 * CHANNELS, "decode_i32": BLOCK * CHANNELS * 4},
        "tailed": "the same track and one frame of %d samples behind it" % TAIL,
        "levels_samples_i32": "over the decode call's [frames][2][2048] int32 output; copy_of_the_samples: a device copy of those bytes",
    }
    for k in calls:
        line[k] = dict(stats(ms[k]), spread=round(spread[k], 4))
    line["levels_samples_over_copy"] = round(med["levels_samples_i32"] / med["copy_of_the_samples"], 4)
    slow = []
    if args.parent_lib:
        line["levels_i32_over_parent_decode_i32"] = round(med["levels_i32"] / med["parent_decode_i32"], 4)
        line["levels_i32_over_parent_verify_i32"] = round(med["levels_i32"] / med["parent_verify_i32"], 4)
        line["levels_i32_tailed_over_parent_decode_i32"] = round(med["levels_i32_tailed"] / med["parent_decode_i32_tailed"], 4)
        line["levels_i32_within_parent_decode_spread"] = bool(med["levels_i32"] / med["parent_decode_i32"] - 1.0 <= spread["parent_decode_i32"])
        for kind in ("decode_i32", "decode_i32_tailed", "verify_i32", "levels"):
            slower = med[kind] / med["parent_" + kind] - 1.0
            line["untouched_" + kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread["parent_" + kind], 4),
                                         "within_parent_spread": bool(slower <= spread["parent_" + kind])}
        if not line["levels_i32_within_parent_decode_spread"]:
            slow.append("levels_i32")
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("no --parent-lib: the parent's calls were not measured, so this is not the record of DESIGN.md 5.27 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    for k in slow:
        print("SLOWER THAN THE PARENT'S DECODE CALL BY MORE THAN ITS SPREAD: %s over parent_decode_i32 %.4f, spread %.4f"
              % (k, line["levels_i32_over_parent_decode_i32"], spread["parent_decode_i32"]))
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
