"""CPU-only side of the verification calls: what they are expected to find is pinned to the REFERENCE (the
fixture tests/golden/verify_corpus.json, made by tests/golden/make_verify_corpus.py from the unmodified reference), the C ABI
declares and exports them, their sizing needs no GPU, and the host's report has its lines and exit codes."""
import json
import os
import subprocess
import sys

import numpy as np

import corpus
from oracle_lib import oracle
from sela_amd import capi
from test_host_cpp import HOST, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "verify_corpus.json")) as fh:
        return json.load(fh)


def test_the_oracle_loses_the_frames_the_reference_loses():
    """The restatement oracle, asked the generator's question, gives the reference's recorded answer: the same lossy frames,
    the same counts, the same first indices.  (Passes without the feature: it pins what the GPU test expects.)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        from make_verify_corpus import lossy_frames
    finally:
        sys.path.pop(0)
    fx = _fixture()
    assert fx["channels"] == 2 and fx["samples_per_frame"] == 2048
    pcm = corpus.build(fx["frames"], fx["seed"])
    assert pcm.shape == (fx["frames"], 2048, 2)
    assert lossy_frames(oracle(), pcm) == fx["lossy"]
    assert len(fx["lossy"]) >= 3 and all(0 < e["count"] <= 4096 and 0 <= e["first"] < 4096 for e in fx["lossy"])


def test_the_calls_are_declared_and_exported_and_sized_without_a_gpu():
    names = ["sela_hip_verify_workspace_bytes", "sela_hip_verify_device", "sela_hip_verify_payload_device", "sela_hip_verify"]
    assert all(n in capi.EXPORTS for n in names)
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in names)
    ws, dn = lib.sela_hip_verify_workspace_bytes, lib.sela_hip_decode_n_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for frames, ch, stride in [(0, 1, 1), (1, 2, 2048), (3875, 2, 2048), (4097, 3, 777), (5, 8, 4096), (5, 9, 4096), (7, 255, 65535)]:
        slices = (ch * stride + 16383) // 16384
        # the decode call's workspace | the PCM of the routes that are not fused | two words per (frame, slice)
        want = int(dn(frames, ch, stride)) + up(frames * ch * stride * 2) + up(max(frames * slices, 1) * 8)
        assert int(ws(frames, ch, stride)) == want, (frames, ch, stride)
    assert int(ws(0xFFFFFFFF, 255, 0xFFFFFFFF)) == (1 << 64) - 1
    # frames x channels at 2^31 and beyond is refused whatever the stride (also where the product of all three wraps 64 bits)
    assert int(ws(1 << 31, 1, 1)) == (1 << 64) - 1 and int(ws(0x80000000, 2, 0xFFFFFFFF)) == (1 << 64) - 1
    assert int(ws(0xFFFFFFFF, 255, 0x01010102)) == (1 << 64) - 1
    assert int(ws((1 << 31) // 255, 255, 1)) < (1 << 40)
    # argument errors are found before any device is asked for
    assert lib.sela_hip_verify_device(None, None, 1, 0, 2048, None, None, None, None, None, None, 0, None) == -2
    assert lib.sela_hip_verify(None, None, 1, 2, None, None, None, None) == -2
    assert lib.sela_hip_verify(None, None, 1, 0, None, None, None, None) == -2


def test_the_python_layer_has_the_verifier():
    from sela_amd import codec

    for name in ("verify", "verify_payload", "lossy_frames", "route", "check"):
        assert callable(getattr(codec.Verifier, name))
    assert callable(codec.verify_host)


def test_host_selftest_report_case(tmp_path):
    """host_selftest's report section: the lines of `sela_mi355x -v` and its exit codes 0 / 3 / 4, no GPU."""
    _build()
    out = subprocess.run([os.path.join(HOST, "host_selftest"), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    usage = subprocess.run([os.path.join(HOST, "sela_mi355x"), "-v"], capture_output=True, text=True)
    assert usage.returncode == 2 and "-v path/to/input.wav path/to/input.sela" in usage.stdout
