"""CPU-only: the envelope calls of 24- and 32-bit streams at the boundary -- declared, exported, sized as the
verify_i32 call, and every argument error found before any device is asked for, in the level call's order -- the record's layout,
the Python helpers against big-integer arithmetic, and the header-only host part as a stand-alone program."""
import os

import numpy as np
import pytest

from sela_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
NAMES = ["sela_hip_envelope_i32_workspace_bytes", "sela_hip_envelope_i32_device", "sela_hip_envelope_payload_i32_device",
         "sela_hip_envelope_samples_i32_workspace_bytes", "sela_hip_envelope_samples_i32_device", "sela_hip_envelope_i32"]
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def test_envelope32_report(tmp_path):
    """tests/c/envelope32_report.cpp: host/include/sela_host/envelope.hpp alone under -fsanitize=address,undefined, run directly."""
    import subprocess

    from test_pcm_cpu import _compile

    exe = _compile(tmp_path, "envelope32_report", [os.path.join(ROOT, "tests", "c", "envelope32_report.cpp")], ["-I" + os.path.join(ROOT, "host", "include")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "envelope32_report: 0 failures" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    assert "sela_hip_debug_envelope_i32_fallback_frames" in capi.DEBUG_EXPORTS
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES) and hasattr(lib, "sela_hip_debug_envelope_i32_fallback_frames")
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert "struct sela_hip_envelope32 {" in header and "typedef struct sela_hip_envelope32 sela_hip_envelope32_record;" in header
    assert "2^42" in header and "2^73" in header, "the bounds are written in the header"
    assert "sela_hip_debug_envelope_i32_fallback_frames(" in open(os.path.join(ROOT, "include", "sela_hip_debug.h")).read()


def test_the_kernels_have_a_translation_unit_of_their_own():
    import __graft_entry__ as entry

    assert "sela_envelope32.hip" in entry.HIP_SOURCES
    text = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_envelope32.hip")).read()
    assert "k_envelope32_direct" in text and "k_envelope32_rest" in text and '#include "sela_group_reduce.h"' in text
    # group_reduce has one definition, which both envelope units include
    narrow = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_envelope.hip")).read()
    shared = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_group_reduce.h")).read()
    assert '#include "sela_group_reduce.h"' in narrow and "uint32_t group_reduce(uint32_t v, uint32_t lanes, Op op)" in shared
    assert "uint32_t group_reduce(uint32_t v" not in narrow and "uint32_t group_reduce(uint32_t v" not in text


def test_the_record_is_32_bytes():
    from sela_amd import codec

    assert codec.ENVELOPE32_DTYPE.itemsize == 32
    assert [(n, codec.ENVELOPE32_DTYPE.fields[n][0].str, codec.ENVELOPE32_DTYPE.fields[n][1]) for n in codec.ENVELOPE32_DTYPE.names] == [
        ("min", "<i4", 0), ("max", "<i4", 4), ("sum", "<i8", 8), ("sum_squares_lo", "<u8", 16), ("sum_squares_hi", "<u8", 24)]


def test_the_workspace_is_the_verify_i32_call_s():
    lib = capi.lib()
    ws, ver, tok = lib.sela_hip_envelope_i32_workspace_bytes, lib.sela_hip_verify_i32_workspace_bytes, lib.sela_hip_envelope_samples_i32_workspace_bytes
    for shape in [(0, 1, 1), (1, 2, 2048), (1, 2, 2049), (3875, 2, 2048), (4097, 3, 777), (5, 8, 4096), (5, 9, 4097), (7, 255, 65535), (1, 1, 1),
                  ((1 << 31) // 255, 255, 1), (1, 0, 2048), (0, 0, 1)]:
        assert int(ws(*shape)) == int(ver(*shape)), shape
    for shape in [(0, 1, 1), (1, 2, 2048), (7, 255, 65535)]:
        assert int(ver(*shape)) != SIZE_MAX and 0 < int(tok(*shape)) == int(tok(1, 1, 1)) <= 4096, shape  # (the samples call keeps nothing: a token, whatever the shape)
    for shape in [(0xFFFFFFFF, 255, 0xFFFFFFFF), (1 << 31, 1, 1), (0x80000000, 2, 0xFFFFFFFF), (0xFFFFFFFF, 255, 0x01010102), ((1 << 31) // 255 + 1, 255, 1),
                  (1 << 30, 1, 1 << 30)]:
        assert int(ver(*shape)) == SIZE_MAX and int(ws(*shape)) == SIZE_MAX and int(tok(*shape)) == SIZE_MAX, shape


def test_argument_errors_are_found_before_any_device_is_asked_for():
    lib = capi.lib()
    one = 0x1000  # (never dereferenced: every call below fails on its arguments)
    big = 1 << 40
    dev = lib.sela_hip_envelope_i32_device
    err = lib.sela_hip_last_error
    # (d_frames, d_frame_offsets, n_frames, channels, stride, bucket, d_env, d_sample_offsets, d_status, d_workspace, bytes, stream)
    assert dev(None, None, 1, 0, 2048, 256, None, None, None, None, 0, None) == EINVAL and b"channels" in err()
    assert dev(one, one, 1, 256, 2048, 256, one, None, one, one, big, None) == EINVAL and b"channels" in err()
    assert dev(one, one, 1, 2, 0, 256, one, None, one, one, big, None) == EINVAL and b"stride" in err()
    assert dev(one, one, 1 << 30, 2, 1, 256, one, None, one, one, big, None) == EINVAL and b"2^31" in err()
    for bucket in (0, 16, 48, 4096, 31, 2049):
        assert dev(one, one, 1, 2, 2048, bucket, one, None, one, one, big, None) == EINVAL and b"bucket must be one of 32, 64, 128, 256, 512, 1024, 2048" in err()
    assert dev(one, one, 1, 2, 2048, 256, None, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_env
    assert dev(one, one, 1, 2, 2048, 256, one, None, None, one, big, None) == EINVAL and b"null device pointer" in err()   # d_status
    assert dev(one, one, 1, 2, 2048, 256, one, None, one, None, big, None) == EINVAL and b"null device pointer" in err()   # d_workspace
    assert dev(one, one, 1, 2, 2048, 256, one + 4, None, one, one, big, None) == EINVAL and b"d_env must be 8-byte aligned" in err()
    assert dev(one, None, 1, 2, 2048, 256, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_frame_offsets
    assert dev(None, one, 1, 2, 2048, 256, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_frames
    assert dev(one + 1, one, 1, 2, 2048, 256, one, None, one, one, big, None) == EINVAL and b"d_frames must be 4-byte aligned" in err()
    # the order: the shape with the bucket, the call's pointers, the record's alignment, the form's pointers, the capacity
    assert dev(one + 1, None, 1, 0, 0, 48, one + 4, None, None, one, 0, None) == EINVAL and b"channels" in err()
    assert dev(one + 1, None, 1, 2, 0, 48, one + 4, None, None, one, 0, None) == EINVAL and b"stride" in err()
    assert dev(one + 1, None, 1 << 30, 2, 1, 48, one + 4, None, None, one, 0, None) == EINVAL and b"2^31" in err()
    assert dev(one + 1, None, 1, 2, 2048, 48, one + 4, None, None, one, 0, None) == EINVAL and b"bucket" in err()
    assert dev(one + 1, None, 1, 2, 2048, 64, one + 4, None, None, one, 0, None) == EINVAL and b"null device pointer" in err()
    assert dev(one + 1, None, 1, 2, 2048, 64, one + 4, None, one, one, 0, None) == EINVAL and b"d_env" in err()
    assert dev(one + 1, one, 1, 2, 2048, 64, one, None, one, one, 0, None) == EINVAL and b"d_frames" in err()
    need = int(lib.sela_hip_envelope_i32_workspace_bytes(1, 2, 2048))
    assert dev(one, one, 1, 2, 2048, 64, one, None, one, one, need - 1, None) == ECAPACITY and b"sela_hip_envelope_i32_workspace_bytes" in err()
    assert dev(one, one, 1 << 20, 255, 65535, 64, one, None, one, one, big, None) == ECAPACITY  # (more than `big`)
    # no frames: d_env may be null, the other pointers may not
    assert dev(None, one, 0, 2, 2048, 64, None, None, None, one, big, None) == EINVAL and b"null device pointer" in err()
    pay = lib.sela_hip_envelope_payload_i32_device
    # (d_payload, payload_bytes, max_frames, channels, stride, bucket, d_env, d_sample_offsets, d_frame_offsets, d_n_frames, d_status, ws, bytes, stream)
    assert pay(None, 0, 1, 2, 2048, 256, None, None, None, None, None, None, 0, None) == EINVAL
    assert pay(one, 64, 1, 0, 2048, 256, one, None, one, one, one, one, big, None) == EINVAL and b"channels" in err()
    assert pay(one + 2, 64, 1, 2, 2048, 256, one, None, one, one, one, one, big, None) == EINVAL and b"d_payload" in err()
    assert pay(one, 64, 1, 2, 0, 256, one, None, one, one, one, one, big, None) == EINVAL and b"stride" in err()
    assert pay(one, 64, 1, 2, 2048, 48, one, None, one, one, one, one, big, None) == EINVAL and b"bucket" in err()
    assert pay(one, 64, 1, 2, 2048, 256, None, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, 256, one + 4, None, one, one, one, one, big, None) == EINVAL and b"d_env" in err()
    assert pay(one, 64, 1, 2, 2048, 256, one, None, None, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, 256, one, None, one, None, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, 256, one, None, one, one, None, one, big, None) == EINVAL
    both = int(lib.sela_hip_index_workspace_bytes(64, 1)) + need
    assert pay(one, 64, 1, 2, 2048, 256, one, None, one, one, one, one, both - 1, None) == ECAPACITY
    sam = lib.sela_hip_envelope_samples_i32_device
    # (d_samples, d_counts, n_frames, channels, stride, bucket, d_env, d_status, d_workspace, bytes, stream)
    assert sam(one, None, 1, 0, 2048, 256, one, one, one, big, None) == EINVAL and b"channels" in err()
    assert sam(one, None, 1, 2, 0, 256, one, one, one, big, None) == EINVAL and b"stride" in err()
    assert sam(one, None, 1 << 30, 2, 1, 256, one, one, one, big, None) == EINVAL and b"2^31" in err()
    assert sam(one, None, 1, 2, 2048, 4096, one, one, one, big, None) == EINVAL and b"bucket" in err()
    assert sam(one, None, 1, 2, 2048, 256, None, one, one, big, None) == EINVAL and b"null device pointer" in err()
    assert sam(one, None, 1, 2, 2048, 256, one, None, one, big, None) == EINVAL and b"null device pointer" in err()
    assert sam(one, None, 1, 2, 2048, 256, one, one, None, big, None) == EINVAL and b"null device pointer" in err()
    assert sam(one, None, 1, 2, 2048, 256, one + 4, one, one, big, None) == EINVAL and b"d_env" in err()
    assert sam(None, None, 1, 2, 2048, 256, one, one, one, big, None) == EINVAL and b"null device pointer" in err()
    assert sam(one + 2, None, 1, 2, 2048, 256, one, one, one, big, None) == EINVAL and b"4-byte aligned" in err()
    assert sam(one, one + 1, 1, 2, 2048, 256, one, one, one, big, None) == EINVAL and b"4-byte aligned" in err()
    token = int(lib.sela_hip_envelope_samples_i32_workspace_bytes(1, 2, 2048))
    assert sam(one, None, 1, 2, 2048, 256, one, one, one, token - 1, None) == ECAPACITY and b"sela_hip_envelope_samples_i32_workspace_bytes" in err()
    # the order there too: shape, bucket, the call's pointers, the record's alignment, the samples, the capacity
    assert sam(None, one + 1, 1, 2, 2048, 48, one + 4, None, one, 0, None) == EINVAL and b"bucket" in err()
    assert sam(None, one + 1, 1, 2, 2048, 64, one + 4, None, one, 0, None) == EINVAL and b"null device pointer" in err()
    assert sam(None, one + 1, 1, 2, 2048, 64, one + 4, one, one, 0, None) == EINVAL and b"d_env" in err()
    assert sam(one, one + 1, 1, 2, 2048, 64, one, one, one, 0, None) == EINVAL and b"4-byte aligned" in err()
    host = lib.sela_hip_envelope_i32
    # (frames, frame_offsets, n_frames, channels, stride, bucket, env)
    assert host(None, None, 1, 2, 2048, 256, None) == EINVAL
    assert host(one, one, 1, 0, 2048, 256, one) == EINVAL and b"channels" in err()
    assert host(one, one, 1, 256, 2048, 256, one) == EINVAL
    assert host(one, one, 1, 2, 0, 256, one) == EINVAL and b"stride" in err()
    assert host(one, one, 1 << 30, 2, 2048, 256, one) == EINVAL and b"2^31" in err()
    assert host(one, one, 1, 2, 2048, 48, one) == EINVAL and b"bucket" in err()
    assert host(one, one, 1, 255, 0xFFFFFFFF, 32, one) == EINVAL and b"fit 32 bits" in err()
    assert host(one, one, 1, 255, 0xFFFFFFFF, 2048, None) == EINVAL and b"null pointer" in err()
    assert host(one, one, 1, 2, 2048, 256, None) == EINVAL
    assert host(None, one, 1, 2, 2048, 256, one) == EINVAL
    assert host(one, None, 0, 2, 2048, 256, one) == EINVAL


def test_the_host_call_without_frames_returns_0():
    offs = np.zeros(1, np.uint64)
    assert capi.lib().sela_hip_envelope_i32(None, offs.ctypes.data, 0, 2, 2048, 256, None) == 0


def test_the_python_layer_has_the_enveloper():
    import inspect

    from sela_amd import codec

    for name in ("measure", "measure_payload", "records", "fallback_frames", "check"):
        assert callable(getattr(codec.Enveloper32, name))
    assert str(inspect.signature(codec.Enveloper32.__init__)) == "(self, max_frames: 'int', channels: 'int', stride: 'int', bucket: 'int', device=None)"
    assert issubclass(codec.Enveloper32, codec._DeviceCall) and codec.Enveloper32.__doc__.startswith("sela_hip_envelope_i32_device")
    assert all(callable(f) for f in (codec.envelope_i32_host, codec.envelope_samples_i32, codec.track_envelope32, codec.fold_envelope32))
    with pytest.raises(ValueError):
        codec.Enveloper32(1, 2, 2048, 48)


def _random_records(rng, shape):
    from sela_amd import codec

    rec = np.zeros(shape, codec.ENVELOPE32_DTYPE)
    a, b = rng.integers(INT32_MIN, INT32_MAX, shape, endpoint=True), rng.integers(INT32_MIN, INT32_MAX, shape, endpoint=True)
    rec["min"], rec["max"] = np.minimum(a, b), np.maximum(a, b)
    rec["sum"] = rng.integers(-(1 << 42), (1 << 42) + 1, shape)
    rec["sum_squares_lo"] = rng.integers(0, (1 << 64) - 1, shape, dtype=np.uint64, endpoint=True)
    rec["sum_squares_hi"] = rng.integers(0, 513, shape, dtype=np.uint64)
    return rec


def _fold_by_hand(rec, factor):
    """big-integer arithmetic, record by record -> nested lists [frames][groups][channels] of 5-tuples"""
    frames, slots, ch = rec.shape
    out = []
    for f in range(frames):
        rows = []
        for g in range(-(-slots // factor)):
            part = rec[f, g * factor:(g + 1) * factor]
            row = []
            for c in range(ch):
                energy = sum(int(lo) + (int(hi) << 64) for lo, hi in zip(part["sum_squares_lo"][:, c], part["sum_squares_hi"][:, c]))
                row.append((min(int(x) for x in part["min"][:, c]), max(int(x) for x in part["max"][:, c]), sum(int(x) for x in part["sum"][:, c]),
                            energy & ((1 << 64) - 1), energy >> 64))
            rows.append(row)
        out.append(rows)
    return out


def test_fold_envelope32_matches_big_integer_arithmetic():
    from sela_amd import codec

    rng = np.random.default_rng(33)
    for bucket in (32, 256, 2048):
        rec = _random_records(rng, (4, 2048 // bucket, 3))
        rec[1, 0, 0] = (INT32_MIN, INT32_MIN, INT32_MIN * bucket, (bucket << 62) & ((1 << 64) - 1), (bucket << 62) >> 64)  # the extremes of a record
        rec[1, 0, 1] = (INT32_MAX, INT32_MAX, INT32_MAX * bucket, (bucket * INT32_MAX * INT32_MAX) & ((1 << 64) - 1), (bucket * INT32_MAX * INT32_MAX) >> 64)
        for factor in {1, 2, 3, 8, 2048 // bucket}:
            got = codec.fold_envelope32(rec, factor)
            assert got.dtype == codec.ENVELOPE32_DTYPE and got.shape == (4, -(-rec.shape[1] // factor), 3)
            assert got.tolist() == [[[tuple(r) for r in row] for row in frame] for frame in _fold_by_hand(rec, factor)], (bucket, factor)
    # a fold that passes 2^64: four full-scale samples a record, two records -- the low words carry into the high one
    full = np.zeros((1, 2, 1), codec.ENVELOPE32_DTYPE)
    full["min"], full["max"], full["sum"], full["sum_squares_lo"], full["sum_squares_hi"] = INT32_MIN, INT32_MIN, 3 * INT32_MIN, 3 << 62, 0
    assert codec.fold_envelope32(full, 2).tolist() == [[[(INT32_MIN, INT32_MIN, 6 * INT32_MIN, (6 << 62) & ((1 << 64) - 1), 1)]]]
    # a full-scale frame at bucket 32 folds to the frame's record: |sum| = 2^42, sum_squares = 2^73
    full = np.zeros((1, 64, 1), codec.ENVELOPE32_DTYPE)
    full["min"], full["max"], full["sum"], full["sum_squares_lo"], full["sum_squares_hi"] = INT32_MIN, INT32_MIN, -(1 << 36), 0, 8
    assert codec.fold_envelope32(full, 64).tolist() == [[[(INT32_MIN, INT32_MIN, -(1 << 42), 0, 512)]]]
    # the track's own records, [buckets, channels], fold the same way
    track = _random_records(rng, (10, 2))
    assert codec.fold_envelope32(track, 4).shape == (3, 2)
    assert codec.fold_envelope32(track, 4).tolist() == [[tuple(r) for r in row] for row in _fold_by_hand(track[None], 4)[0]]
    # a sum that leaves its field's range is an error, not a wrap
    over = np.zeros((1, 2, 1), codec.ENVELOPE32_DTYPE)
    over["sum"] = 1 << 62
    with pytest.raises(OverflowError):
        codec.fold_envelope32(over, 2)


def test_track_envelope32_drops_the_empty_slots_and_refuses_a_ragged_middle_frame():
    from sela_amd import codec

    rng = np.random.default_rng(34)
    for bucket in (32, 512, 2048):
        # a whole-track stream at stride 2825: two frames of 2048 and a last one of 2048 + 777
        so = [0, 2048, 4096, 4096 + 2825]
        slots = -(-2825 // bucket)
        rec = _random_records(rng, (3, slots, 2))
        got = codec.track_envelope32(rec, so, bucket)
        total = 4096 + 2825
        assert got.shape == (-(-total // bucket), 2) and got.dtype == codec.ENVELOPE32_DTYPE
        want = [rec[f, b] for f in range(3) for b in range(-(-(so[f + 1] - so[f]) // bucket))]
        assert got.tolist() == [[tuple(r) for r in row.tolist()] for row in want]
        # with stride 2048 the array is simply [track bucket][channel]
        rec = _random_records(rng, (4, 2048 // bucket, 2))
        assert codec.track_envelope32(rec, np.arange(5, dtype=np.uint64) * 2048, bucket).tolist() == rec.reshape(-1, 2).tolist()
    rec = _random_records(rng, (3, 64, 2))
    with pytest.raises(ValueError):
        codec.track_envelope32(rec, [0, 2048, 2048 + 777, 2048 + 777 + 2048], 32)   # a middle frame of 777 samples
    assert codec.track_envelope32(rec, [0, 2048, 4096, 4096 + 777], 32).shape == (64 + 64 + 25, 2)  # (the last frame may be ragged)
    with pytest.raises(ValueError):
        codec.track_envelope32(rec, [0, 2048, 4096, 4096 + 2049], 32)  # more samples than the frame has slots
    assert codec.track_envelope32(np.zeros((0, 64, 2), codec.ENVELOPE32_DTYPE), [0], 32).shape == (0, 2)
