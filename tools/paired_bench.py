#!/usr/bin/env python3
"""What channel pairs cost and save.  On 3875 frames (the bench's frame count) of 6-channel 2048 x int16 `synth`
audio, on HIP events:
  (a) the bytes of the plain and of the paired stream (both calls' own offsets, both status words clean);
  (b) sela_hip_encode_paired_n_device against sela_hip_encode_n_device of this tree (9 signals analysed against 6);
  (c) sela_hip_encode_n_device and sela_hip_encode_i32_device of this tree against the same calls of another build of the library
      (--parent-lib: the parent commit's libsela_hip.so), whose bytes must be this tree's.
Everything is warmed up; then `rounds` rounds alternate the calls, each timing `calls` back-to-back calls between two events.
The parent's own spread between repeats is (largest - least) / median of its rounds: the plain calls of this tree may be slower
than the parent's by no more than that (`within_parent_spread`).
Prints one JSON line and writes it to --out (default profiles/paired/paired_bench.json), then puts the figures into DESIGN.md 5.18
(between its paired_bench markers).  The record is the required one only with (c) in it: without --parent-lib nothing is written
and the exit code is 2.  Where a plain call of this tree is slower than the parent's by more than the parent's spread the record
is written, the fact is printed, and the exit code is 1.
Run on the GPU box:  python tools/paired_bench.py --parent-lib path/to/parent/libsela_hip.so [--rounds 15] [--calls 20]
Anywhere, no GPU:    python tools/paired_bench.py --from-json profiles/paired/paired_bench.json   (DESIGN.md from a record)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, CHANNELS, BLOCK, TRACK = 3875, 6, 2048, 3
DESIGN, BEGIN, END = os.path.join(ROOT, "DESIGN.md"), "<!-- paired_bench:begin -->", "<!-- paired_bench:end -->"


def design_text(r):
    """The record as DESIGN.md 5.18 states it."""
    t = lambda s: "%.4f ms (%.4f .. %.4f)" % (s["median_ms"], s["min_ms"], s["max_ms"])  # noqa: E731
    a, cn, ci = r["a_bytes"], r["c_n"], r["c_i32"]
    verdict = lambda c: "within" if c["within_parent_spread"] else "**beyond**"  # noqa: E731
    return (
        "%d frames of 6-channel 2048 x int16 `synth` audio (track 3), %d rounds of %d calls, medians with least and largest:\n"
        "(a) %d bytes plain, %d bytes paired, a ratio of %.4f -- the synthetic track's figure and nothing more.\n"
        "(b) `sela_hip_encode_paired_n_device` %s against `sela_hip_encode_n_device` %s: %.4f times (9 signals analysed against 6; recorded, not required).\n"
        "(c) against the parent commit's build in the same process, the same bytes: `sela_hip_encode_n_device` %s here, %s the parent's, %.4f times, the\n"
        "parent's own spread between repeats %.4f: %s it; `sela_hip_encode_i32_device` %s here, %s the parent's, %.4f times, spread %.4f: %s it.\n"
        % (r["frames"], r["rounds"], r["calls_per_round"], a["plain"], a["paired"], a["ratio"], t(r["b_paired_n_device"]), t(r["b_plain_n_device"]),
           r["b_ratio_paired_over_plain"], t(r["b_plain_n_device"]), t(r["c_parent_n_device"]), cn["this_over_parent"], cn["parent_spread"], verdict(cn),
           t(r["c_plain_i32_device"]), t(r["c_parent_i32_device"]), ci["this_over_parent"], ci["parent_spread"], verdict(ci)))


def write_design(record):
    with open(DESIGN) as fh:
        text = fh.read()
    head, rest = text.split(BEGIN, 1)
    _, tail = rest.split(END, 1)
    with open(DESIGN, "w") as fh:
        fh.write(head + BEGIN + "\n" + design_text(record) + END + tail)


def finish(record):
    """DESIGN.md, and the exit code: 1 where a plain call is slower than the parent's by more than the parent's spread."""
    if os.path.exists(DESIGN):
        write_design(record)
    slow = [k for k in ("c_n", "c_i32") if not record[k]["within_parent_spread"]]
    for k in slow:
        print("REQUIRED CONDITION MISSED: %s: this tree over the parent %.4f, the parent's spread %.4f" % (k, record[k]["this_over_parent"], record[k]["parent_spread"]))
    return 1 if slow else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--parent-lib", default=None, help="libsela_hip.so built from the parent commit (figure (c)); without it (c) is not measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paired", "paired_bench.json"))
    ap.add_argument("--from-json", default=None, help="no run: put this record's figures into DESIGN.md and judge it")
    args = ap.parse_args()
    if args.from_json:
        with open(args.from_json) as fh:
            return finish(json.loads(fh.read()))
    import torch

    from sela_amd import capi, codec, synth

    assert torch.cuda.is_available(), "paired_bench needs a GPU: there is no CPU path to time"
    torch.cuda.set_device(0)
    nf = args.frames
    d_pcm = synth.synth_pcm_torch(nf * BLOCK, CHANNELS, TRACK, device="cuda").reshape(nf, BLOCK, CHANNELS).contiguous()
    d_i32 = d_pcm.permute(0, 2, 1).to(torch.int32).contiguous()
    lib = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    cap = int(lib.sela_hip_encode_bound_bytes_n(nf, CHANNELS, BLOCK))

    class Call:
        """One device entry of one library with buffers of its own."""

        def __init__(self, L, name, d_x, ws_bytes, options=None):
            self.fn = getattr(L, name)
            self.fn.restype = C.c_int
            self.d_x = d_x
            self.frames = torch.empty(cap, dtype=torch.uint8, device="cuda")
            self.offsets = torch.zeros(nf + 1, dtype=torch.int64, device="cuda")
            self.status = torch.zeros(4, dtype=torch.int32, device="cuda")
            self.ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
            self.args = [vp(d_x.data_ptr()), u32(nf), u32(CHANNELS), u32(BLOCK), vp(self.frames.data_ptr()), sz(cap), vp(self.offsets.data_ptr()),
                         vp(self.status.data_ptr()), vp(self.ws.data_ptr()), sz(ws_bytes), vp(stream)] + ([u32(options)] if options is not None else [])

        def __call__(self):
            rc = self.fn(*self.args)
            assert rc == 0, rc

        def result(self):
            torch.cuda.synchronize()
            st = self.status.cpu().numpy()
            assert codec.encode_status_error(st) == 0 and int(st[1]) == 0, st
            total = int(self.offsets[nf].item())
            return self.frames[:total].clone(), self.offsets.clone(), total

    ws_plain = int(lib.sela_hip_encode_i32_workspace_bytes(nf, CHANNELS, BLOCK))
    ws_paired = int(lib.sela_hip_encode_paired_workspace_bytes(nf, CHANNELS, BLOCK))
    calls = {
        "paired_n": Call(lib, "sela_hip_encode_paired_n_device", d_pcm, ws_paired, 0),
        "plain_n": Call(lib, "sela_hip_encode_n_device", d_pcm, ws_plain),
        "plain_i32": Call(lib, "sela_hip_encode_i32_device", d_i32, ws_plain),
    }
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.sela_hip_encode_i32_workspace_bytes.restype = C.c_size_t
        parent.sela_hip_encode_i32_workspace_bytes.argtypes = [C.c_uint32] * 3
        assert int(parent.sela_hip_encode_i32_workspace_bytes(nf, CHANNELS, BLOCK)) == ws_plain, "the plain calls' workspace changed size"
        calls["parent_n"] = Call(parent, "sela_hip_encode_n_device", d_pcm, ws_plain)
        calls["parent_i32"] = Call(parent, "sela_hip_encode_i32_device", d_i32, ws_plain)

    # warm-up, and what the calls wrote
    for _ in range(2):
        for c in calls.values():
            c()
    out = {k: c.result() for k, c in calls.items()}
    assert torch.equal(out["plain_n"][0], out["plain_i32"][0]) and torch.equal(out["plain_n"][1], out["plain_i32"][1])
    if args.parent_lib:
        for mine, theirs in (("plain_n", "parent_n"), ("plain_i32", "parent_i32")):
            assert torch.equal(out[mine][0], out[theirs][0]) and torch.equal(out[mine][1], out[theirs][1]), "the plain call's bytes differ from the parent's"
    bytes_plain, bytes_paired = out["plain_n"][2], out["paired_n"][2]

    def timed(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.calls):
            call()
        end.record()
        end.synchronize()
        return begin.elapsed_time(end) / args.calls

    ms = {k: [] for k in calls}
    for r in range(args.rounds):
        # (alternating: this tree's call and the parent's take turns at going first and at following the longer paired call)
        mine, theirs = ["plain_n", "plain_i32"], ["parent_n", "parent_i32"] if args.parent_lib else []
        pairs = list(zip(mine, theirs)) if theirs else [(m,) for m in mine]
        order = [k for pair in pairs for k in (pair if r % 2 == 0 else pair[::-1])] + ["paired_n"]
        for k in order:
            ms[k].append(timed(calls[k]))
    stats = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}  # noqa: E731
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {
        "frames": nf, "channels": CHANNELS, "samples_per_channel": BLOCK, "input": "synth_pcm_torch(frames * 2048, 6, track=3)", "rounds": args.rounds,
        "calls_per_round": args.calls,
        "a_bytes": {"plain": bytes_plain, "paired": bytes_paired, "ratio": round(bytes_paired / bytes_plain, 4)},
        "b_paired_n_device": stats(ms["paired_n"]), "b_plain_n_device": stats(ms["plain_n"]),
        "b_ratio_paired_over_plain": round(med["paired_n"] / med["plain_n"], 4),
        "c_plain_i32_device": stats(ms["plain_i32"]),
    }
    if args.parent_lib:
        line["c_parent_n_device"], line["c_parent_i32_device"] = stats(ms["parent_n"]), stats(ms["parent_i32"])
        for kind in ("n", "i32"):
            p = ms["parent_" + kind]
            spread = (max(p) - min(p)) / med["parent_" + kind]
            slower = med["plain_" + kind] / med["parent_" + kind] - 1.0
            line["c_%s" % kind] = {"this_over_parent": round(1.0 + slower, 4), "parent_spread": round(spread, 4), "within_parent_spread": bool(slower <= spread)}
    text = json.dumps(line)
    print(text)
    if not args.parent_lib:
        print("no --parent-lib: figure (c) was not measured, so this is not the record of DESIGN.md 5.18 and nothing is written")
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return finish(line)


if __name__ == "__main__":
    sys.exit(main())
