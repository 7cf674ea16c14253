"""CPU-only: the envelope calls at the boundary -- declared, exported, sized as the level call, and every argument
error found before any device is asked for -- the record's layout, the Python helpers against big-integer arithmetic, and the
header-only host part as a stand-alone program."""
import os

import numpy as np
import pytest

from sela_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
NAMES = ["sela_hip_envelope_slots", "sela_hip_envelope_workspace_bytes", "sela_hip_envelope_device", "sela_hip_envelope_payload_device", "sela_hip_envelope"]
BUCKETS = (32, 64, 128, 256, 512, 1024, 2048)


def test_envelope_report(tmp_path):
    """tests/c/envelope_report.cpp: host/include/sela_host/envelope.hpp alone under -fsanitize=address,undefined, run directly."""
    import subprocess

    from test_pcm_cpu import _compile

    exe = _compile(tmp_path, "envelope_report", [os.path.join(ROOT, "tests", "c", "envelope_report.cpp")], ["-I" + os.path.join(ROOT, "host", "include")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "envelope_report: 0 failures" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    assert "sela_hip_debug_envelope_lds_bytes" in capi.DEBUG_EXPORTS
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES) and hasattr(lib, "sela_hip_debug_envelope_lds_bytes")
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert "struct sela_hip_envelope {" in header
    assert "sela_hip_debug_envelope_lds_bytes(" in open(os.path.join(ROOT, "include", "sela_hip_debug.h")).read()


def test_the_kernels_have_a_translation_unit_of_their_own():
    import __graft_entry__ as entry

    assert "sela_envelope.hip" in entry.HIP_SOURCES
    text = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_envelope.hip")).read()
    assert "k_envelope_frames" in text and "k_envelope_channels" in text and '#include "sela_decode_core.inc"' in text
    assert "kResidencyEnvelope" in text and "kResidencyEnvelope" in open(os.path.join(ROOT, "sela_amd", "csrc", "sela_device.h")).read()


def test_the_record_is_16_bytes():
    from sela_amd import codec

    assert codec.ENVELOPE_DTYPE.itemsize == 16
    assert [(n, codec.ENVELOPE_DTYPE.fields[n][0].str, codec.ENVELOPE_DTYPE.fields[n][1]) for n in codec.ENVELOPE_DTYPE.names] == [
        ("min", "<i2", 0), ("max", "<i2", 2), ("sum", "<i4", 4), ("sum_squares", "<u8", 8)]


def test_slots():
    slots = capi.lib().sela_hip_envelope_slots
    table = {(1, 32): 1, (2047, 32): 64, (2048, 32): 64, (2049, 32): 65, (4095, 32): 128, (65535, 32): 2048,
             (1, 2048): 1, (2047, 2048): 1, (2048, 2048): 1, (2049, 2048): 2, (4095, 2048): 2, (65535, 2048): 32}
    for (stride, bucket), want in table.items():
        assert int(slots(stride, bucket)) == want == -(-stride // bucket), (stride, bucket)
    for bucket in BUCKETS:
        assert int(slots(2048, bucket)) == 2048 // bucket and int(slots(0xFFFFFFFF, bucket)) == -(-0xFFFFFFFF // bucket)
    for bucket in (0, 16, 48, 4096, 1, 33, 2047, 0x80000000, 0xFFFFFFFF):
        assert int(slots(2048, bucket)) == 0, bucket
    # stride 0 has no slots
    assert all(int(slots(0, b)) == 0 for b in BUCKETS)


def test_the_workspace_is_the_level_call_s():
    lib = capi.lib()
    ws, lev = lib.sela_hip_envelope_workspace_bytes, lib.sela_hip_levels_workspace_bytes
    for shape in [(0, 1, 1), (1, 2, 2048), (1, 2, 2049), (3875, 2, 2048), (4097, 3, 777), (5, 8, 4096), (5, 9, 4096), (7, 255, 65535), (1, 1, 1),
                  ((1 << 31) // 255, 255, 1)]:
        assert int(ws(*shape)) == int(lev(*shape)) != SIZE_MAX, shape
    for shape in [(0xFFFFFFFF, 255, 0xFFFFFFFF), (1 << 31, 1, 1), (0x80000000, 2, 0xFFFFFFFF), (0xFFFFFFFF, 255, 0x01010102), ((1 << 31) // 255 + 1, 255, 1),
                  (1 << 30, 1, 1 << 30), (1, 0, 2048), (0, 0, 1)]:
        assert int(lev(*shape)) == SIZE_MAX and int(ws(*shape)) == SIZE_MAX, shape


def test_argument_errors_are_found_before_any_device_is_asked_for():
    lib = capi.lib()
    one = 0x1000  # (never dereferenced: every call below fails on its arguments)
    big = 1 << 40
    dev = lib.sela_hip_envelope_device
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
    need = int(lib.sela_hip_envelope_workspace_bytes(1, 2, 2048))
    assert dev(one, one, 1, 2, 2048, 64, one, None, one, one, need - 1, None) == ECAPACITY and b"sela_hip_envelope_workspace_bytes" in err()
    assert dev(one, one, 1 << 20, 255, 65535, 64, one, None, one, one, big, None) == ECAPACITY  # (more than `big`)
    # no frames: d_env may be null, the other pointers may not
    assert dev(None, one, 0, 2, 2048, 64, None, None, None, one, big, None) == EINVAL and b"null device pointer" in err()
    pay = lib.sela_hip_envelope_payload_device
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
    host = lib.sela_hip_envelope
    # (frames, frame_offsets, n_frames, channels, stride, bucket, env)
    assert host(None, None, 1, 2, 2048, 256, None) == EINVAL
    assert host(one, one, 1, 0, 2048, 256, one) == EINVAL and b"channels" in err()
    assert host(one, one, 1, 256, 2048, 256, one) == EINVAL
    assert host(one, one, 1, 2, 0, 256, one) == EINVAL and b"stride" in err()
    assert host(one, one, 1 << 30, 2, 2048, 256, one) == EINVAL and b"2^31" in err()
    assert host(one, one, 1, 2, 2048, 48, one) == EINVAL and b"bucket" in err()
    # a frame's records are counted in 32 bits: 2^27 slots of 32 samples times 255 channels do not fit, 2^21 slots of 2048 do
    assert host(one, one, 1, 255, 0xFFFFFFFF, 32, one) == EINVAL and b"fit 32 bits" in err()
    assert host(one, one, 1, 32, 0xFFFFFFFF, 32, one) == EINVAL and b"fit 32 bits" in err()
    assert host(one, one, 1, 255, 0xFFFFFFFF, 2048, None) == EINVAL and b"null pointer" in err()
    assert host(one, one, 1, 2, 2048, 256, None) == EINVAL
    assert host(None, one, 1, 2, 2048, 256, one) == EINVAL
    assert host(one, None, 0, 2, 2048, 256, one) == EINVAL


def test_the_host_call_without_frames_returns_0():
    offs = np.zeros(1, np.uint64)
    assert capi.lib().sela_hip_envelope(None, offs.ctypes.data, 0, 2, 2048, 256, None) == 0


def test_the_python_layer_has_the_enveloper():
    import inspect

    from sela_amd import codec

    for name in ("measure", "measure_payload", "records", "route", "check"):
        assert callable(getattr(codec.Enveloper, name))
    assert str(inspect.signature(codec.Enveloper.__init__)) == "(self, max_frames: 'int', channels: 'int', stride: 'int', bucket: 'int', device=None)"
    assert issubclass(codec.Enveloper, codec._DeviceCall) and "self.status = " in inspect.getsource(codec._DeviceCall.__init__)
    assert codec.Enveloper.__doc__.startswith("sela_hip_envelope_device")
    assert all(callable(f) for f in (codec.envelope_host, codec.track_envelope, codec.fold_envelope))
    with pytest.raises(ValueError):
        codec.Enveloper(1, 2, 2048, 48)


def _random_records(rng, shape):
    from sela_amd import codec

    rec = np.zeros(shape, codec.ENVELOPE_DTYPE)
    a, b = rng.integers(-32768, 32768, shape), rng.integers(-32768, 32768, shape)
    rec["min"], rec["max"] = np.minimum(a, b), np.maximum(a, b)
    rec["sum"] = rng.integers(-(1 << 26), (1 << 26) + 1, shape)
    rec["sum_squares"] = rng.integers(0, (1 << 41) + 1, shape, dtype=np.uint64)
    return rec


def _fold_by_hand(rec, factor):
    """big-integer arithmetic, record by record -> nested lists [..., groups, channels] of 4-tuples"""
    frames, slots, ch = rec.shape
    out = []
    for f in range(frames):
        rows = []
        for g in range(-(-slots // factor)):
            part = rec[f, g * factor:(g + 1) * factor]
            rows.append([(min(int(x) for x in part["min"][:, c]), max(int(x) for x in part["max"][:, c]), sum(int(x) for x in part["sum"][:, c]),
                          sum(int(x) for x in part["sum_squares"][:, c])) for c in range(ch)])
        out.append(rows)
    return out


def test_fold_envelope_matches_big_integer_arithmetic():
    from sela_amd import codec

    rng = np.random.default_rng(31)
    for bucket in (32, 256, 2048):
        rec = _random_records(rng, (5, 2048 // bucket, 3))
        rec[1, 0, 0] = (-32768, -32768, -32768 * bucket, bucket << 30)  # the extremes of a record
        rec[1, 0, 1] = (32767, 32767, 32767 * bucket, bucket * 32767 * 32767)
        for factor in {1, 2, 3, 8, 2048 // bucket}:
            got = codec.fold_envelope(rec, factor)
            assert got.dtype == codec.ENVELOPE_DTYPE and got.shape == (5, -(-rec.shape[1] // factor), 3)
            assert got.tolist() == [[[tuple(r) for r in row] for row in frame] for frame in _fold_by_hand(rec, factor)], (bucket, factor)
        # folding by 2048 / bucket gives one record per frame
        assert codec.fold_envelope(rec, 2048 // bucket).shape == (5, 1, 3)
    # a full-scale frame at bucket 32 folds to the frame's record: |sum| = 2^26, sum_squares = 2^41
    full = np.zeros((1, 64, 1), codec.ENVELOPE_DTYPE)
    full["min"], full["max"], full["sum"], full["sum_squares"] = -32768, -32768, -32768 * 32, 32 << 30
    assert codec.fold_envelope(full, 64).tolist() == [[[(-32768, -32768, -(1 << 26), 1 << 41)]]]
    # the track's own records, [buckets, channels], fold the same way
    track = _random_records(rng, (10, 2))
    assert codec.fold_envelope(track, 4).shape == (3, 2)
    assert codec.fold_envelope(track, 4).tolist() == [[tuple(r) for r in row] for row in _fold_by_hand(track[None], 4)[0]]
    # a sum that leaves its field's range is an error, not a wrap
    over = np.zeros((1, 64, 1), codec.ENVELOPE_DTYPE)
    over["sum"] = 1 << 26
    with pytest.raises(OverflowError):
        codec.fold_envelope(over, 64)


def test_track_envelope_drops_the_empty_slots_and_refuses_a_ragged_middle_frame():
    from sela_amd import codec

    rng = np.random.default_rng(32)
    for bucket in (32, 512, 2048):
        # a whole-track stream at stride 4095: two frames of 2048 and a last one of 2048 + 777
        so = [0, 2048, 4096, 4096 + 2825]
        slots = -(-4095 // bucket)
        rec = _random_records(rng, (3, slots, 2))
        got = codec.track_envelope(rec, so, bucket)
        total = 4096 + 2825
        assert got.shape == (-(-total // bucket), 2) and got.dtype == codec.ENVELOPE_DTYPE
        want = [rec[f, b] for f in range(3) for b in range(-(-(so[f + 1] - so[f]) // bucket))]
        assert got.tolist() == [[tuple(r) for r in row.tolist()] for row in want]
        # with stride 2048 the array is simply [track bucket][channel]
        rec = _random_records(rng, (4, 2048 // bucket, 2))
        assert codec.track_envelope(rec, np.arange(5, dtype=np.uint64) * 2048, bucket).tolist() == rec.reshape(-1, 2).tolist()
    rec = _random_records(rng, (3, 64, 2))
    with pytest.raises(ValueError):
        codec.track_envelope(rec, [0, 2048, 2048 + 777, 2048 + 777 + 2048], 32)   # a middle frame of 777 samples
    assert codec.track_envelope(rec, [0, 2048, 4096, 4096 + 777], 32).shape == (64 + 64 + 25, 2)  # (the last frame may be ragged)
    with pytest.raises(ValueError):
        codec.track_envelope(rec, [0, 2048, 4096, 4096 + 2049], 32)  # more samples than the frame has slots
    assert codec.track_envelope(np.zeros((0, 64, 2), codec.ENVELOPE_DTYPE), [0], 32).shape == (0, 2)
