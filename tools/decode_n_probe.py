"""Times the int16 decode of any length on device pointers (sela_hip_decode_n_device / sela_hip_decode_payload_n_device,
DESIGN.md 5.13) against what a device-resident caller has besides it.  Streams:
  track  the bench's 3875 stereo 2048-sample frames: against sela_hip_decode_payload_device (the 2048-sample payload call);
  mixed  stereo 24-bit frames of 700 .. 4096 samples, tiled to about --mb MB (decode_i32_probe.py's shape): against
         sela_hip_decode_payload_i32_device and against copy-back + host sela_hip_decode + upload.
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times (on the mixed stream the host route runs
k_generic_combine<true> on the same decoded subframes the device call hands to k_interleave16).  End-to-end times are medians
of --reps runs, the calls taken in turn; the outputs are checked against each other first.

  python tools/decode_n_probe.py --stream track|mixed [--reps R] [--mb M] [--out FILE]
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


def _stream(kind, mb):
    if kind == "track":
        return codec.encode_host(synth_frames(3875, 2, 0))[0]
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
    ap.add_argument("--stream", choices=("track", "mixed"), default="track")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = capi.lib()
    blob = _stream(a.stream, a.mb)
    offs = codec.index_frames(blob, 1 << 22, 2)
    n = len(offs) - 1
    so, largest = codec.index_samples(blob, offs, 2)
    stride = largest
    payload = torch.from_numpy(blob).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    res = {"stream": a.stream, "frames": n, "payload_bytes": int(blob.nbytes), "stride": stride, "samples_per_channel": int(so[n]), "reps": a.reps}
    dec = codec.DecoderN(n, 2, stride)
    dec.decode_payload(payload)  # (the workspace is allocated here)
    torch.cuda.synchronize()
    dec.check()
    res["route"] = dec.route()
    res["workspace_bytes"] = int(dec.payload_workspace.numel())
    total = int(so[n]) * 2
    got = dec.pcm.reshape(-1)[:total].cpu().numpy()
    fns = {"decode_n_device_ms": lambda: dec.decode(payload, d_offs, n), "decode_payload_n_device_ms": lambda: dec.decode_payload(payload)}
    if a.stream == "track":
        d16 = codec.Decoder(n, 2)
        want, _, _ = d16.decode_payload(payload)
        torch.cuda.synchronize()
        d16.check()
        assert np.array_equal(got, want.reshape(-1).cpu().numpy())
        fns["decode_payload_device_ms"] = lambda: d16.decode_payload(payload)
    else:
        d32 = codec.Decoder32(n, 2, stride)
        d32.decode_payload(payload)
        torch.cuda.synchronize()
        d32.check()
        fns["decode_payload_i32_device_ms"] = lambda: d32.decode_payload(payload)
        out = np.empty(max(n * 2048, int(so[n])) * 2, np.int16)
        d_out = torch.empty(total, dtype=torch.int16, device="cuda")

        def host_route():
            src = payload.cpu().numpy()
            o = codec.index_frames(src, 1 << 22, 2)
            capi.check(lib.sela_hip_decode(src.ctypes.data, o.ctypes.data, len(o) - 1, 2, out.ctypes.data))
            d_out.copy_(torch.from_numpy(out[:total]))

        host_route()
        assert np.array_equal(got, out[:total])
        fns["copy_back_host_decode_upload_ms"] = host_route
    res["same_as_reference_call"] = True
    res.update(_median_ms(fns, a.reps))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
