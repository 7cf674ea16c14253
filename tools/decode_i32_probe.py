"""Times the 32-bit decode on device pointers (sela_hip_decode_i32_device / sela_hip_decode_payload_i32_device)
against what a device-resident caller had before it: copy the payload back, walk it on the host (sela_hip_index_frames +
sela_hip_index_samples), sela_hip_decode_i32 on host pointers, upload the samples.  Streams:
  track  the bench's 3875 stereo 2048-sample frames;
  mixed  stereo 24-bit frames of 700 .. 4096 samples, tiled to about --mb MB;
  album  the track tiled --tile times (142: 550,250 frames), device calls only (--host-album adds the host route).
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times; --device-only / --host-only run one side alone (the
kernel sums of the two routes, each in a profile of its own).  End-to-end times are medians of --reps runs, the routes taken in
turn.

  python tools/decode_i32_probe.py --stream track|mixed|album [--reps R] [--mb M] [--tile N] [--device-only|--host-only] [--out FILE]
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


def _stream(kind, mb, tile):
    if kind in ("track", "album"):
        frames, _ = codec.encode_host(synth_frames(3875, 2, 0))
        return np.tile(frames, tile if kind == "album" else 1)
    rng = np.random.default_rng(24)
    blobs = []
    for i in range(96):  # (distinct frames, then tiled: the decode does not care that they repeat)
        n = int(rng.integers(700, 4097))
        t = np.arange(n)
        x = np.stack([np.round((1 << 22) * np.sin(t * (0.003 + 0.001 * (i % 7)) + i) + rng.normal(0, 2000, n)),
                      np.round((1 << 21) * np.sin(t * 0.011 + 2 * i) + rng.normal(0, 500, n))]).astype(np.int32)
        blobs.append(codec.encode_i32(x[None])[0])
    one = np.concatenate(blobs)
    return np.tile(one, max(1, int(mb * (1 << 20)) // one.nbytes))


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
    ap.add_argument("--stream", choices=("track", "mixed", "album"), default="track")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--tile", type=int, default=142)
    ap.add_argument("--host-album", action="store_true")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = capi.lib()
    blob = _stream(a.stream, a.mb, a.tile)
    cap = 1 << 22
    offs = codec.index_frames(blob, cap, 2)
    n = len(offs) - 1
    so, largest = codec.index_samples(blob, offs, 2)
    stride = largest
    payload = torch.from_numpy(blob).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    res = {"stream": a.stream, "frames": n, "payload_bytes": int(blob.nbytes), "stride": stride, "samples_per_channel": int(so[n]), "reps": a.reps}
    fns = {}
    if not a.host_only:
        dec = codec.Decoder32(n, 2, stride)
        fns["decode_i32_device_ms"] = lambda: dec.decode(payload, d_offs, n)
        fns["decode_payload_i32_device_ms"] = lambda: dec.decode_payload(payload)
        dec.decode_payload(payload)  # (the workspace is allocated here)
        torch.cuda.synchronize()
        dec.check()
        res["workspace_bytes"] = int(dec.workspace.numel())
    if not a.device_only and (a.stream != "album" or a.host_album):
        out = np.empty((n, 2, stride), np.int32)
        counts = np.empty((n, 2), np.uint32)
        d_out = torch.empty((n, 2, stride), dtype=torch.int32, device="cuda")

        def host_route():
            src = payload.cpu().numpy()
            o = codec.index_frames(src, cap, 2)
            k = len(o) - 1
            s, big = codec.index_samples(src, o, 2)
            capi.check(lib.sela_hip_decode_i32(src.ctypes.data, o.ctypes.data, k, 2, out.ctypes.data, big, counts.ctypes.data))
            d_out.copy_(torch.from_numpy(out))

        fns["copy_back_host_walk_decode_i32_upload_ms"] = host_route
        host_route()
    res.update(_median_ms(fns, a.reps))
    if not a.host_only and not a.device_only and (a.stream != "album" or a.host_album):
        samples, cnt, sofs, _, count = dec.decode_payload(payload)
        torch.cuda.synchronize()
        dec.check()
        assert int(count.item()) == n and np.array_equal(sofs.cpu().numpy().view(np.uint64), so)
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), counts)
        got = samples.cpu().numpy()
        for f in range(0, n, max(1, n // 64)):
            for c in range(2):
                assert np.array_equal(got[f, c, : counts[f, c]], out[f, c, : counts[f, c]]), (f, c)
        res["same_as_host"] = True
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
