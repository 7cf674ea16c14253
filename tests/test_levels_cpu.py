"""CPU-only side of the level calls: the C ABI declares and exports them, their sizing and their argument
checks need no GPU, the Python layer has its classes, and the fold over records is big-integer arithmetic."""
import os

import numpy as np
import pytest

from sela_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
NAMES = ["sela_hip_levels_workspace_bytes", "sela_hip_levels_device", "sela_hip_levels_payload_device", "sela_hip_levels"]


def test_level_report(tmp_path):
    """tests/c/level_report.cpp: host/include/sela_host/levels.hpp alone under -fsanitize=address,undefined, run directly."""
    import subprocess

    from test_pcm_cpu import _compile

    exe = _compile(tmp_path, "level_report", [os.path.join(ROOT, "tests", "c", "level_report.cpp")], ["-I" + os.path.join(ROOT, "host", "include")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "level_report: 0 failures" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    assert "sela_hip_debug_levels_lds_bytes" in capi.DEBUG_EXPORTS
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES) and hasattr(lib, "sela_hip_debug_levels_lds_bytes")
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert "typedef struct sela_hip_level" in header
    assert "sela_hip_debug_levels_lds_bytes(" in open(os.path.join(ROOT, "include", "sela_hip_debug.h")).read()


def test_the_kernels_have_a_translation_unit_of_their_own():
    import __graft_entry__ as entry

    assert "sela_levels.hip" in entry.HIP_SOURCES
    text = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_levels.hip")).read()
    assert "k_level_frames" in text and "k_level_channels" in text and '#include "sela_decode_core.inc"' in text


def test_the_record_is_24_bytes():
    from sela_amd import codec

    assert codec.LEVEL_DTYPE.itemsize == 24
    assert [(n, codec.LEVEL_DTYPE.fields[n][0].str, codec.LEVEL_DTYPE.fields[n][1]) for n in codec.LEVEL_DTYPE.names] == [
        ("peak", "<u4", 0), ("samples", "<u4", 4), ("sum", "<i8", 8), ("sum_squares", "<u8", 16)]


def test_the_workspace_formula_piece_by_piece():
    lib = capi.lib()
    ws, dn, ver = lib.sela_hip_levels_workspace_bytes, lib.sela_hip_decode_n_workspace_bytes, lib.sela_hip_verify_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for frames, ch, stride in [(0, 1, 1), (1, 2, 2048), (1, 2, 2049), (3875, 2, 2048), (4097, 3, 777), (5, 8, 4096), (5, 9, 4096), (7, 255, 65535), (1, 1, 1)]:
        # the decode call's workspace | the int16 PCM of the routes that are not fused
        want = int(dn(frames, ch, stride)) + up(frames * ch * stride * 2)
        assert int(ws(frames, ch, stride)) == want, (frames, ch, stride)
        assert want < int(ver(frames, ch, stride))  # (the verifier's, without its words per slice)
    # SIZE_MAX where the verifier's is ...
    for shape in [(0xFFFFFFFF, 255, 0xFFFFFFFF), (1 << 31, 1, 1), (0x80000000, 2, 0xFFFFFFFF), (0xFFFFFFFF, 255, 0x01010102), ((1 << 31) // 255 + 1, 255, 1),
                  (1 << 30, 1, 1 << 30)]:
        assert int(ver(*shape)) == SIZE_MAX and int(ws(*shape)) == SIZE_MAX, shape
    assert int(ws((1 << 31) // 255, 255, 1)) < (1 << 40)
    # ... and without channels
    assert int(ws(1, 0, 2048)) == SIZE_MAX and int(ws(0, 0, 1)) == SIZE_MAX


def test_argument_errors_are_found_before_any_device_is_asked_for():
    lib = capi.lib()
    one = 0x1000  # (never dereferenced: every call below fails on its arguments)
    big = 1 << 40
    dev = lib.sela_hip_levels_device
    err = lib.sela_hip_last_error
    # (d_frames, d_frame_offsets, n_frames, channels, stride, d_levels, d_sample_offsets, d_status, d_workspace, bytes, stream)
    assert dev(None, None, 1, 0, 2048, None, None, None, None, 0, None) == EINVAL and b"channels" in err()
    assert dev(one, one, 1, 256, 2048, one, None, one, one, big, None) == EINVAL and b"channels" in err()
    assert dev(one, one, 1, 2, 0, one, None, one, one, big, None) == EINVAL and b"stride" in err()
    assert dev(one, one, 1 << 30, 2, 1, one, None, one, one, big, None) == EINVAL and b"2^31" in err()
    assert dev(one, one, 1, 2, 2048, None, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_levels
    assert dev(one, one, 1, 2, 2048, one, None, None, one, big, None) == EINVAL and b"null device pointer" in err()   # d_status
    assert dev(one, one, 1, 2, 2048, one, None, one, None, big, None) == EINVAL and b"null device pointer" in err()   # d_workspace
    assert dev(one, one, 1, 2, 2048, one + 4, None, one, one, big, None) == EINVAL and b"d_levels must be 8-byte aligned" in err()
    assert dev(one, None, 1, 2, 2048, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_frame_offsets
    assert dev(None, one, 1, 2, 2048, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_frames
    assert dev(one + 1, one, 1, 2, 2048, one, None, one, one, big, None) == EINVAL and b"d_frames must be 4-byte aligned" in err()
    # the order: the shape, the call's pointers, the record's alignment, the form's pointers, the capacity
    assert dev(one + 1, None, 1, 0, 0, one + 4, None, None, one, 0, None) == EINVAL and b"channels" in err()
    assert dev(one + 1, None, 1, 2, 0, one + 4, None, None, one, 0, None) == EINVAL and b"stride" in err()
    assert dev(one + 1, None, 1, 2, 2048, one + 4, None, None, one, 0, None) == EINVAL and b"null device pointer" in err()
    assert dev(one + 1, None, 1, 2, 2048, one + 4, None, one, one, 0, None) == EINVAL and b"d_levels" in err()
    assert dev(one + 1, one, 1, 2, 2048, one, None, one, one, 0, None) == EINVAL and b"d_frames" in err()
    need = int(lib.sela_hip_levels_workspace_bytes(1, 2, 2048))
    assert dev(one, one, 1, 2, 2048, one, None, one, one, need - 1, None) == ECAPACITY and b"sela_hip_levels_workspace_bytes" in err()
    assert dev(one, one, 1 << 20, 255, 65535, one, None, one, one, big, None) == ECAPACITY  # (more than `big`)
    pay = lib.sela_hip_levels_payload_device
    # (d_payload, payload_bytes, max_frames, channels, stride, d_levels, d_sample_offsets, d_frame_offsets, d_n_frames, d_status, ws, bytes, stream)
    assert pay(None, 0, 1, 2, 2048, None, None, None, None, None, None, 0, None) == EINVAL
    assert pay(one, 64, 1, 0, 2048, one, None, one, one, one, one, big, None) == EINVAL and b"channels" in err()
    assert pay(one + 2, 64, 1, 2, 2048, one, None, one, one, one, one, big, None) == EINVAL and b"d_payload" in err()
    assert pay(one, 64, 1, 2, 0, one, None, one, one, one, one, big, None) == EINVAL and b"stride" in err()
    assert pay(one, 64, 1, 2, 2048, None, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one + 4, None, one, one, one, one, big, None) == EINVAL and b"d_levels" in err()
    assert pay(one, 64, 1, 2, 2048, one, None, None, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one, None, one, None, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one, None, one, one, None, one, big, None) == EINVAL
    both = int(lib.sela_hip_index_workspace_bytes(64, 1)) + need
    assert pay(one, 64, 1, 2, 2048, one, None, one, one, one, one, both - 1, None) == ECAPACITY
    host = lib.sela_hip_levels
    # (frames, frame_offsets, n_frames, channels, levels)
    assert host(None, None, 1, 2, None) == EINVAL
    assert host(one, one, 1, 0, one) == EINVAL and b"channels" in err()
    assert host(one, one, 1, 256, one) == EINVAL
    assert host(one, one, 1 << 30, 2, one) == EINVAL and b"2^31" in err()
    assert host(one, one, 1, 2, None) == EINVAL
    assert host(None, one, 1, 2, one) == EINVAL
    assert host(one, None, 0, 2, one) == EINVAL


def test_the_host_call_without_frames_returns_0():
    offs = np.zeros(1, np.uint64)
    assert capi.lib().sela_hip_levels(None, offs.ctypes.data, 0, 2, None) == 0


def test_the_python_layer_has_the_leveler():
    from sela_amd import codec

    for name in ("measure", "measure_payload", "records", "loud_frames", "route", "check"):
        assert callable(getattr(codec.Leveler, name))
    import inspect

    assert "self.status = " in inspect.getsource(codec.Leveler.__init__)  # (.status: the call's four words, a device tensor)
    assert callable(codec.levels_host) and callable(codec.track_levels)


def test_track_levels_matches_big_integer_arithmetic():
    from sela_amd import codec

    rng = np.random.default_rng(5)
    frames, ch = 300, 3
    rec = np.zeros((frames, ch), codec.LEVEL_DTYPE)
    rec["peak"] = rng.integers(0, 32769, (frames, ch))
    rec["samples"] = rng.integers(0, 65536, (frames, ch))
    rec["sum"] = rng.integers(-(1 << 31) + 1, 1 << 31, (frames, ch))
    rec["sum_squares"] = rng.integers(0, 1 << 46, (frames, ch), dtype=np.uint64)
    rec[7, 1] = (32768, 65535, -65535 * 32768, 65535 << 30)   # the extremes of a record
    rec[8, 1] = (32767, 65535, 65535 * 32767, 65535 * 32767 * 32767)
    rec[:, 2]["peak"] = 0                                      # a silent channel
    rec["sum"][:, 2] = 0
    rec["sum_squares"][:, 2] = 0
    got = codec.track_levels(rec)
    assert got.dtype == codec.TRACK_LEVEL_DTYPE and got.shape == (ch,)
    for c in range(ch):
        assert int(got[c]["peak"]) == max(int(x) for x in rec["peak"][:, c])
        assert int(got[c]["samples"]) == sum(int(x) for x in rec["samples"][:, c])
        assert int(got[c]["sum"]) == sum(int(x) for x in rec["sum"][:, c])
        assert int(got[c]["sum_squares"]) == sum(int(x) for x in rec["sum_squares"][:, c])
    assert int(got[1]["peak"]) == 32768 and int(got[2]["sum_squares"]) == 0
    # 2^18 full-scale frames still fit; float64 would have lost the low bits long before
    full = np.zeros((1 << 10, 1), codec.LEVEL_DTYPE)
    full["peak"], full["samples"], full["sum"], full["sum_squares"] = 32768, 65535, -65535 * 32768, (65535 << 30) + 1
    t = codec.track_levels(full)[0]
    assert int(t["sum_squares"]) == ((65535 << 30) + 1) << 10 and int(t["sum"]) == (-65535 * 32768) << 10 and int(t["samples"]) == 65535 << 10
    assert codec.track_levels(np.zeros((0, 2), codec.LEVEL_DTYPE)).tolist() == [(0, 0, 0, 0), (0, 0, 0, 0)]
    with pytest.raises(OverflowError):
        over = np.zeros((2, 1), codec.LEVEL_DTYPE)
        over["sum_squares"] = 1 << 63
        codec.track_levels(over)
