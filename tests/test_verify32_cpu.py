"""CPU-only side of the 32-bit verification calls: what they are expected to find on wide audio is pinned to
the REFERENCE (the fixture tests/golden/verify_wide.json, made by tests/golden/make_verify_wide.py from the unmodified
reference), the C ABI declares and exports them, their sizing follows the formula of include/sela_hip.h piece by piece, and
argument errors need no GPU."""
import json
import os
import sys

from oracle_lib import oracle
from sela_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = (1 << 64) - 1
NAMES = ["sela_hip_verify_i32_workspace_bytes", "sela_hip_verify_i32_device", "sela_hip_verify_payload_i32_device", "sela_hip_verify_i32"]


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "verify_wide.json")) as fh:
        return json.load(fh)


def test_the_oracle_loses_the_wide_frames_the_reference_loses():
    """The restatement oracle, asked the generator's question, gives the reference's recorded answer entry for entry.  (Passes
    without the feature: it pins what the GPU test expects.)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        from make_verify_wide import lossy_frames, wide_frames
    finally:
        sys.path.pop(0)
    fx = _fixture()
    assert (fx["frames"], fx["seed"], fx["noise_seed"], fx["bits"]) == (1500, 20260927, 20261017, 24)
    x = wide_frames(fx["frames"], fx["seed"], fx["noise_seed"], fx["bits"])
    assert x.shape == (1500, 2, 2048) and x.min() >= -(1 << 23) and x.max() < (1 << 23) and abs(x).max() >= 1 << 22
    assert lossy_frames(oracle(), x) == fx["lossy"]


def test_the_fixture_is_neither_empty_nor_the_rule():
    fx = _fixture()
    lossy = fx["lossy"]
    assert len(lossy) >= 3, "the GPU test could pass on 'nothing differs'"
    assert len(lossy) * 100 < fx["frames"], "one frame in a hundred or more is lossy"
    assert [e["frame"] for e in lossy] == sorted({e["frame"] for e in lossy}) and all(0 <= e["frame"] < fx["frames"] for e in lossy)
    assert all(0 < e["count"] <= 4096 and 0 <= e["first"] < 4096 for e in lossy)


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    assert "sela_hip_debug_verify_i32_fallback_frames" in capi.DEBUG_EXPORTS
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES + ["sela_hip_debug_verify_i32_fallback_frames"])
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    assert all(n + "(" in header for n in NAMES)


def test_the_workspace_formula_piece_by_piece():
    lib = capi.lib()
    ws, dec = lib.sela_hip_verify_i32_workspace_bytes, lib.sela_hip_decode_i32_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for frames, ch, stride in [(0, 1, 1), (1, 2, 2048), (1500, 2, 2048), (4097, 3, 777), (2, 255, 65535)]:
        slices = (stride + 4095) // 4096
        want = (int(dec(frames, ch, stride))              # the subframes as decoded, their records, the index
                + up(frames * ch * stride * 4)           # the samples by channel, for frames of any other layout
                + up(frames * ch * 4)                    # ... and their counts
                + up(max(frames, 1) * 4)                 # a mark per frame
                + up(max(frames * slices, 1) * 8)        # two words per (frame, slice)
                + 256)                                   # the control words
        assert int(ws(frames, ch, stride)) == want, (frames, ch, stride)
    # SIZE_MAX where the decode call's is ...
    assert int(dec(1 << 30, 1, 1 << 30)) == SIZE_MAX and int(ws(1 << 30, 1, 1 << 30)) == SIZE_MAX
    assert int(dec(1 << 23, 255, 1 << 30)) == SIZE_MAX and int(ws(1 << 23, 255, 1 << 30)) == SIZE_MAX
    assert int(ws(0xFFFFFFFF, 255, 0xFFFFFFFF)) == SIZE_MAX
    # ... and where frames x channels reaches 2^31, whatever the stride (also where the product of all three wraps 64 bits)
    assert int(ws(1 << 31, 1, 1)) == SIZE_MAX and int(ws(0x80000000, 2, 0xFFFFFFFF)) == SIZE_MAX
    assert int(ws(0xFFFFFFFF, 255, 0x01010102)) == SIZE_MAX
    assert int(ws((1 << 31) // 255 + 1, 255, 1)) == SIZE_MAX
    assert int(ws((1 << 31) // 255, 255, 1)) < (1 << 40)


def test_argument_errors_are_found_before_any_device_is_asked_for():
    lib = capi.lib()
    one = 0x1000  # (never dereferenced: every call below fails on its arguments)
    dev = lib.sela_hip_verify_i32_device
    assert dev(None, None, 1, 0, 2048, None, None, None, None, None, None, None, 0, None) == -2
    assert dev(one, one, 1, 256, 2048, one, None, one, one, None, one, one, 1 << 40, None) == -2       # channels
    assert dev(one, one, 1, 2, 0, one, None, one, one, None, one, one, 1 << 40, None) == -2            # stride
    assert dev(one, one, 1 << 30, 2, 1, one, None, one, one, None, one, one, 1 << 40, None) == -2      # frames x channels
    assert dev(one, one, 1, 2, 2048, None, None, one, one, None, one, one, 1 << 40, None) == -2        # d_samples
    assert dev(one, one, 1, 2, 2048, one, None, None, one, None, one, one, 1 << 40, None) == -2        # d_diff_counts
    assert dev(one, one, 1, 2, 2048, one, None, one, None, None, one, one, 1 << 40, None) == -2        # d_first_diff
    assert dev(one, one, 1, 2, 2048, one + 2, None, one, one, None, one, one, 1 << 40, None) == -2     # misaligned d_samples
    assert dev(one, one, 1, 2, 2048, one, one + 1, one, one, None, one, one, 1 << 40, None) == -2      # misaligned d_lengths
    assert dev(one, one, 1, 2, 2048, one, None, one + 2, one, None, one, one, 1 << 40, None) == -2     # misaligned d_diff_counts
    assert dev(one, one, 1, 2, 2048, one, None, one, one + 1, None, one, one, 1 << 40, None) == -2     # misaligned d_first_diff
    assert dev(one + 1, one, 1, 2, 2048, one, None, one, one, None, one, one, 1 << 40, None) == -2     # misaligned d_frames
    assert dev(one, None, 1, 2, 2048, one, None, one, one, None, one, one, 1 << 40, None) == -2        # d_frame_offsets
    assert dev(one, one, 1, 2, 2048, one, None, one, one, None, None, one, 1 << 40, None) == -2        # d_status
    assert dev(one, one, 1, 2, 2048, one, None, one, one, None, one, None, 1 << 40, None) == -2        # d_workspace
    need = int(lib.sela_hip_verify_i32_workspace_bytes(1, 2, 2048))
    assert dev(one, one, 1, 2, 2048, one, None, one, one, None, one, one, need - 1, None) == -4        # a smaller workspace
    pay = lib.sela_hip_verify_payload_i32_device
    assert pay(None, 0, 1, 2, 2048, None, None, None, None, None, None, None, None, None, 0, None) == -2
    assert pay(one, 64, 1, 2, 2048, None, None, one, one, None, one, one, one, one, 1 << 40, None) == -2
    assert pay(one, 64, 1, 2, 2048, one, None, one, one, None, one, one, one, one, need - 1, None) == -4
    host = lib.sela_hip_verify_i32
    assert host(None, None, 1, 2, 2048, None, None, None, None, None) == -2
    assert host(None, None, 1, 0, 2048, None, None, None, None, None) == -2
    assert host(one, one, 1, 2, 0, one, None, one, one, None) == -2


def test_the_python_layer_has_the_verifier():
    from sela_amd import codec

    for name in ("verify", "verify_payload", "lossy_frames", "check"):
        assert callable(getattr(codec.Verifier32, name))
    assert callable(codec.verify_i32)
