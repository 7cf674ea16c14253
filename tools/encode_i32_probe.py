"""Times the any-length / 32-bit encode on device pointers (sela_hip_encode_i32_device) against the host-pointer
sela_hip_encode_i32 on the same data -- alone, and as a device-resident caller had to run it before: copy the samples back, encode
on host pointers, upload the frames.  Inputs (int32, planar):
  track  the bench's 3875 stereo 2048-sample frames;
  mixed  24-bit stereo frames of eight lengths (700 .. 4096), --frames per length, one call per length;
  long   --frames 24-bit stereo frames of 65535 samples.
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times; --device-only / --host-only run one side alone (each
route's kernels in a profile of its own).  End-to-end times are medians of --reps runs, the routes taken in turn.

  python tools/encode_i32_probe.py --input track|mixed|long [--reps R] [--frames F] [--device-only|--host-only] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # (appended: a PYTHONPATH that names another build of the package comes first)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sela_amd import capi, codec  # noqa: E402
from sela_amd.synth import synth_frames  # noqa: E402

MIXED_LENGTHS = (700, 777, 1000, 1500, 2047, 2049, 3000, 4096)


def _inputs(kind, frames):
    """-> list of int32 [n_frames, 2, n] batches (one call each)"""
    if kind == "track":
        return [np.ascontiguousarray(synth_frames(3875, 2, 0).transpose(0, 2, 1)).astype(np.int32)]
    rng = np.random.default_rng(24)
    lengths = MIXED_LENGTHS if kind == "mixed" else (65535,)
    out = []
    for i, n in enumerate(lengths):
        t = np.arange(n)
        ph = rng.uniform(0, 6, (frames, 1))
        a = np.round((1 << 22) * np.sin(t * (0.003 + 0.001 * (i % 7)) + ph) + rng.normal(0, 2000, (frames, n)))
        b = np.round((1 << 21) * np.sin(t * 0.011 + 2 * ph) + rng.normal(0, 500, (frames, n)))
        out.append(np.ascontiguousarray(np.stack([a, b], axis=1).astype(np.int32)))
    return out


def _median_ms(fns, reps):
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():  # (alternating)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: float(np.median(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", choices=("track", "mixed", "long"), default="track")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = capi.lib()
    frames = a.frames or (400 if a.input == "mixed" else 60)
    batches = _inputs(a.input, frames)
    d_batches = [torch.from_numpy(x).cuda() for x in batches]
    res = {"input": a.input, "calls": len(batches), "frames": sum(x.shape[0] for x in batches), "lengths": [int(x.shape[2]) for x in batches],
           "input_bytes": int(sum(x.nbytes for x in batches)), "reps": a.reps}
    fns = {}
    encs = []
    if not a.host_only:
        encs = [codec.Encoder32(x.shape[0], 2, x.shape[2]) for x in batches]

        def device_route():
            for e, d in zip(encs, d_batches):
                e.encode(d)

        fns["encode_i32_device_ms"] = device_route
        device_route()
        torch.cuda.synchronize()
        for e in encs:
            e.check()
        res["workspace_bytes"] = int(sum(e.workspace.numel() for e in encs))
        res["frame_bytes"] = int(sum(e.needed_bytes() for e in encs))
    host_out = []
    if not a.device_only:
        bufs = []
        for x in batches:
            cap = int(lib.sela_hip_encode_bound_bytes_n(x.shape[0], 2, x.shape[2]))
            bufs.append((np.empty(cap, np.uint8), np.zeros(x.shape[0] + 1, np.uint64)))

        def host_call(x, buf):
            capi.check(lib.sela_hip_encode_i32(x.ctypes.data, x.shape[0], 2, x.shape[2], buf[0].ctypes.data, buf[0].nbytes, buf[1].ctypes.data))

        def host_alone():
            for x, buf in zip(batches, bufs):
                host_call(x, buf)

        def host_route():  # what a caller whose samples are in device memory ran before
            for d, buf in zip(d_batches, bufs):
                x = d.cpu().numpy()
                host_call(x, buf)
                torch.from_numpy(buf[0][: int(buf[1][-1])]).cuda()

        fns["encode_i32_host_ms"] = host_alone
        fns["copy_back_encode_i32_upload_ms"] = host_route
        host_alone()
        host_out = bufs
    res.update(_median_ms(fns, a.reps))
    if encs and host_out:
        for e, (fr, offs) in zip(encs, host_out):
            got, o = e.to_host()
            assert np.array_equal(o, offs) and got.tobytes() == fr[: int(offs[-1])].tobytes()
        res["same_as_host"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
