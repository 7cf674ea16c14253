"""CPU-only side of the level calls for 24- and 32-bit streams: the C ABI declares and exports them, their
sizing and every refusal need no GPU, and the record is the numpy dtype's."""
import os
import subprocess

import numpy as np

from sela_amd import capi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
NAMES = ["sela_hip_levels_i32_workspace_bytes", "sela_hip_levels_i32_device", "sela_hip_levels_payload_i32_device",
         "sela_hip_levels_samples_i32_workspace_bytes", "sela_hip_levels_samples_i32_device", "sela_hip_levels_i32"]


def test_level_report32(tmp_path):
    """tests/c/level_report32.cpp: host/include/sela_host/levels.hpp alone under -fsanitize=address,undefined, run directly."""
    from test_pcm_cpu import _compile

    exe = _compile(tmp_path, "level_report32", [os.path.join(ROOT, "tests", "c", "level_report32.cpp")], ["-I" + os.path.join(ROOT, "host", "include")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "level_report32: 0 failures" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    assert "sela_hip_debug_levels_i32_fallback_frames" in capi.DEBUG_EXPORTS
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES) and hasattr(lib, "sela_hip_debug_levels_i32_fallback_frames")
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    assert all(n + "(" in header for n in NAMES) and "typedef struct sela_hip_level32" in header
    assert "sela_hip_debug_levels_i32_fallback_frames(" in open(os.path.join(ROOT, "include", "sela_hip_debug.h")).read()
    import __graft_entry__ as entry

    assert "sela_levels32.hip" in entry.HIP_SOURCES


def test_the_record_is_the_dtype(tmp_path):
    from test_pcm_cpu import _compile

    exe = _compile(tmp_path, "level32_record", [os.path.join(ROOT, "tests", "c", "level32_record.cpp")], ["-I" + os.path.join(ROOT, "include")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    d = codec.LEVEL32_DTYPE
    assert [int(x) for x in out.stdout.split()] == [d.itemsize, 8] + [d.fields[n][1] for n in d.names]
    assert d.itemsize == 32 and d.names == ("peak", "samples", "sum", "sum_squares_lo", "sum_squares_hi")
    assert [d.fields[n][0].str for n in d.names] == ["<u4", "<u4", "<i8", "<u8", "<u8"]


def test_the_workspace_formula_piece_by_piece():
    lib = capi.lib()
    ws, ver, di, smp = (lib.sela_hip_levels_i32_workspace_bytes, lib.sela_hip_verify_i32_workspace_bytes, lib.sela_hip_decode_i32_workspace_bytes,
                        lib.sela_hip_levels_samples_i32_workspace_bytes)
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for frames, ch, stride in [(0, 1, 1), (1, 2, 2048), (1, 2, 2049), (3875, 2, 2048), (4097, 3, 777), (5, 8, 4096), (5, 9, 4097), (7, 255, 65535), (1, 1, 1)]:
        slices = (stride + 4095) // 4096
        # the verify call's pieces, with 32 bytes per (frame, slice, channel) where it has 8 per (frame, slice)
        want = int(ver(frames, ch, stride)) - up(max(frames * slices, 1) * 8) + up(max(frames * slices * ch * 4, 1) * 8)
        assert int(ws(frames, ch, stride)) == want, (frames, ch, stride)
        assert want > int(di(frames, ch, stride))
        assert int(smp(frames, ch, stride)) == up(max(frames * slices * ch * 4, 1) * 8) + 256, (frames, ch, stride)
    # SIZE_MAX where the verify call's is ...
    for shape in [(0xFFFFFFFF, 255, 0xFFFFFFFF), (1 << 31, 1, 1), (0x80000000, 2, 0xFFFFFFFF), (0xFFFFFFFF, 255, 0x01010102), ((1 << 31) // 255 + 1, 255, 1),
                  (1 << 30, 1, 1 << 30)]:
        assert int(ver(*shape)) == SIZE_MAX and int(ws(*shape)) == SIZE_MAX and int(smp(*shape)) == SIZE_MAX, shape
    assert int(ws((1 << 31) // 255, 255, 1)) < (1 << 40)
    # ... and without channels
    assert int(ws(1, 0, 2048)) == SIZE_MAX and int(ws(0, 0, 1)) == SIZE_MAX and int(smp(1, 0, 2048)) == SIZE_MAX


def test_every_refusal_comes_before_any_device_is_asked_for():
    lib = capi.lib()
    one = 0x1000  # (never dereferenced: every call below fails on its arguments)
    big = 1 << 40
    created = int(lib.sela_hip_debug_contexts_created())
    dev = lib.sela_hip_levels_i32_device
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
    # the order, as sela_hip_levels_device's: the shape, the call's pointers, the record's alignment, the form's pointers, the capacity
    assert dev(one + 1, None, 1, 0, 0, one + 4, None, None, one, 0, None) == EINVAL and b"channels" in err()
    assert dev(one + 1, None, 1, 2, 0, one + 4, None, None, one, 0, None) == EINVAL and b"stride" in err()
    assert dev(one + 1, None, 1, 2, 2048, one + 4, None, None, one, 0, None) == EINVAL and b"null device pointer" in err()
    assert dev(one + 1, None, 1, 2, 2048, one + 4, None, one, one, 0, None) == EINVAL and b"d_levels" in err()
    assert dev(one + 1, one, 1, 2, 2048, one, None, one, one, 0, None) == EINVAL and b"d_frames" in err()
    need = int(lib.sela_hip_levels_i32_workspace_bytes(1, 2, 2048))
    assert dev(one, one, 1, 2, 2048, one, None, one, one, need - 1, None) == ECAPACITY and b"sela_hip_levels_i32_workspace_bytes" in err()
    assert dev(one, one, 1 << 20, 255, 65535, one, None, one, one, big, None) == ECAPACITY  # (more than `big`)
    # the same arguments get the same code from the 16-bit call
    lev = lib.sela_hip_levels_device
    for args in [(one, one, 1, 256, 2048, one, None, one, one, big, None), (one, one, 1, 2, 0, one, None, one, one, big, None),
                 (one, one, 1, 2, 2048, one + 4, None, one, one, big, None), (one + 1, one, 1, 2, 2048, one, None, one, one, big, None),
                 (one, one, 1, 2, 2048, one, None, one, one, 16, None)]:
        assert dev(*args) == lev(*args), args
    pay = lib.sela_hip_levels_payload_i32_device
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
    smp = lib.sela_hip_levels_samples_i32_device
    # (d_samples, d_counts, n_frames, channels, stride, d_levels, d_status, d_workspace, bytes, stream)
    assert smp(one, None, 1, 0, 2048, one, one, one, big, None) == EINVAL and b"channels" in err()
    assert smp(one, None, 1, 256, 2048, one, one, one, big, None) == EINVAL and b"channels" in err()
    assert smp(one, None, 1, 2, 0, one, one, one, big, None) == EINVAL and b"stride" in err()
    assert smp(one, None, 1 << 30, 2, 1, one, one, one, big, None) == EINVAL and b"2^31" in err()
    assert smp(one, None, 1, 2, 2048, None, one, one, big, None) == EINVAL and b"null device pointer" in err()
    assert smp(one, None, 1, 2, 2048, one, None, one, big, None) == EINVAL and b"null device pointer" in err()
    assert smp(one, None, 1, 2, 2048, one, one, None, big, None) == EINVAL and b"null device pointer" in err()
    assert smp(one, None, 1, 2, 2048, one + 4, one, one, big, None) == EINVAL and b"d_levels must be 8-byte aligned" in err()
    assert smp(None, None, 1, 2, 2048, one, one, one, big, None) == EINVAL and b"null device pointer" in err()
    assert smp(one + 2, None, 1, 2, 2048, one, one, one, big, None) == EINVAL and b"4-byte aligned" in err()
    assert smp(one, one + 1, 1, 2, 2048, one, one, one, big, None) == EINVAL and b"4-byte aligned" in err()
    small = int(lib.sela_hip_levels_samples_i32_workspace_bytes(1, 2, 2048))
    assert smp(one, None, 1, 2, 2048, one, one, one, small - 1, None) == ECAPACITY and b"sela_hip_levels_samples_i32_workspace_bytes" in err()
    host = lib.sela_hip_levels_i32
    # (frames, frame_offsets, n_frames, channels, levels)
    assert host(None, None, 1, 2, None) == EINVAL
    assert host(one, one, 1, 0, one) == EINVAL and b"channels" in err()
    assert host(one, one, 1, 256, one) == EINVAL
    assert host(one, one, 1 << 30, 2, one) == EINVAL and b"2^31" in err()
    assert host(one, one, 1, 2, None) == EINVAL
    assert host(None, one, 1, 2, one) == EINVAL
    assert host(one, None, 0, 2, one) == EINVAL
    # ... and zero frames ask for no device
    offs = np.zeros(1, np.uint64)
    assert host(None, offs.ctypes.data, 0, 2, None) == 0
    assert int(lib.sela_hip_debug_contexts_created()) == created, "a refusal asked for a device"


def test_the_python_layer_has_the_leveler32():
    for name in ("measure", "measure_payload", "records", "loud_frames", "fallback_frames", "check"):
        assert callable(getattr(codec.Leveler32, name))
    assert callable(codec.levels_i32_host) and callable(codec.levels_samples_i32) and callable(codec.track_levels32)
    rec = np.zeros((2, 1), codec.LEVEL32_DTYPE)
    rec["sum_squares_lo"], rec["sum_squares_hi"], rec["peak"], rec["samples"], rec["sum"] = (1 << 64) - 1, 16383, 1 << 31, 65535, -65535 << 31
    assert codec.track_levels32(rec) == [{"peak": 1 << 31, "samples": 131070, "sum": -131070 << 31, "sum_squares": 2 * (((1 << 64) - 1) + (16383 << 64))}]
    assert codec.track_levels32(np.zeros((0, 2), codec.LEVEL32_DTYPE)) == [{"peak": 0, "samples": 0, "sum": 0, "sum_squares": 0}] * 2
