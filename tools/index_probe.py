"""Times the device frame index (sela_hip_index_frames_device) and the payload decode (sela_hip_decode_payload_device) against
the host route -- walk the payload on the host, upload the offsets, sela_hip_decode_device -- on one payload: the bench's 3875
stereo frames, or that stream tiled (--tile 142: 550,250 frames, the album's size).  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel times.  --decode-only times only sela_hip_decode_device on host-walked
offsets (what a library without the device index can run: the k_decode_frames comparison before / after).

  python tools/index_probe.py [--tile N] [--reps R] [--decode-only] [--out FILE]
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


def _median_ms(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = capi.lib()
    frames, offs = codec.encode_host(synth_frames(3875, 2, 0))
    blob = np.tile(frames, a.tile)
    n = 3875 * a.tile
    host_offs = np.zeros(n + 1, np.uint64)
    assert lib.sela_hip_index_frames(blob.ctypes.data, blob.nbytes, n, 2, host_offs.ctypes.data) == n
    payload = torch.from_numpy(blob).cuda()
    d_offs = torch.from_numpy(host_offs.view(np.int64).copy()).cuda()
    dec = codec.Decoder(n, 2)
    res = {"frames": n, "payload_bytes": int(blob.nbytes), "reps": a.reps}

    res["decode_device_ms"] = _median_ms(lambda: dec.decode(payload, d_offs, n), a.reps)
    dec.check()

    pinned_offs = torch.empty(n + 1, dtype=torch.int64).pin_memory()

    def host_route(copy_payload_back):
        src = payload.cpu().numpy() if copy_payload_back else blob
        o = pinned_offs.numpy().view(np.uint64)
        found = lib.sela_hip_index_frames(src.ctypes.data, src.nbytes, n, 2, o.ctypes.data)
        d_offs.copy_(pinned_offs, non_blocking=True)
        dec.decode(payload, d_offs, found)

    res["host_walk_upload_decode_ms"] = _median_ms(lambda: host_route(False), a.reps)
    res["payload_back_host_walk_upload_decode_ms"] = _median_ms(lambda: host_route(True), max(3, a.reps // 4))
    if not a.decode_only:
        ws = torch.empty(codec.index_workspace_bytes(blob.nbytes, n), dtype=torch.uint8, device="cuda")
        got = {}

        def index():
            got["r"] = codec.index_frames_device(payload, n, 2, ws)

        res["index_device_ms"] = _median_ms(index, a.reps)
        d_o, d_n = got["r"]
        assert int(d_n.item()) == n and np.array_equal(d_o.cpu().numpy().view(np.uint64), host_offs)
        res["decode_payload_device_ms"] = _median_ms(lambda: dec.decode_payload(payload), a.reps)
        pcm, o2, c2 = dec.decode_payload(payload)
        torch.cuda.synchronize()
        dec.check()
        ref = codec.Decoder(n, 2)
        ref.decode(payload, d_offs, n)
        torch.cuda.synchronize()
        assert int(c2.item()) == n and torch.equal(pcm, ref.pcm)
        res["index_workspace_bytes"] = int(ws.numel())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
