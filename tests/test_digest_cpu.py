"""CPU-only side of the digest calls: sela_hip_crc32_combine against zlib, the generated table of x^(8 * 2^k)
against big-integer arithmetic, the C ABI's declarations and exports, the record, the workspace formula and every argument check
-- none of which needs a GPU."""
import os
import subprocess
import sys
import zlib

import numpy as np

from sela_amd import capi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
NAMES = ["sela_hip_digest_workspace_bytes", "sela_hip_digest_device", "sela_hip_digest_payload_device", "sela_hip_digest", "sela_hip_crc32_combine",
         "sela_hip_crc32_workspace_bytes", "sela_hip_crc32_device"]
P = (1 << 32) | 0x04C11DB7  # the CRC-32 polynomial, x^32 included, as an integer with bit k = x^k


def _reflect(v: int) -> int:
    return int(f"{v:032b}"[::-1], 2)


def _x_power(e: int) -> int:
    """x^e mod P over GF(2) in Python's integers (bit k = x^k), by square-and-multiply."""
    def mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            a <<= 1
            if a >> 32:
                a ^= P
            b >>= 1
        return r
    result, base = 1, 2
    while e:
        if e & 1:
            result = mul(result, base)
        base = mul(base, base)
        e >>= 1
    return result


def test_crc32_combine_against_zlib():
    rng = np.random.default_rng(28)
    a = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    for nb in (0, 1, 3, 4, 8192):
        b = rng.integers(0, 256, nb, dtype=np.uint8).tobytes()
        for first in (b"", a[:1], a):
            assert codec.crc32_combine(zlib.crc32(first), zlib.crc32(b), nb) == zlib.crc32(first + b), (len(first), nb)
    # six parts, one of them empty
    parts = [a[:7], b"", a[7:2055], a[2055:2058], a[2058:], bytes(9000)]
    crc = 0
    for p in parts:
        crc = codec.crc32_combine(crc, zlib.crc32(p), len(p))
    assert crc == zlib.crc32(b"".join(parts))
    # 2^32 + 5 and 2^40 bytes: the identity twice on halves, and the same distance in big integers
    ca, cb = zlib.crc32(a), zlib.crc32(a[:100])
    for n in ((1 << 32) + 5, 1 << 40):
        half = n // 2
        assert codec.crc32_combine(ca, cb, n) == codec.crc32_combine(codec.crc32_combine(ca, 0, half), cb, n - half)
        assert codec.crc32_combine(0x80000000, 0, n) == _reflect(_x_power(8 * n)), n   # (0x80000000 is x^0: the call returns x^(8 n))
    # zeros behind a message: the distance and the CRC of the zeros themselves
    assert codec.crc32_combine(ca, zlib.crc32(bytes(70000)), 70000) == zlib.crc32(a + bytes(70000))


def test_the_generated_table_against_big_integers():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_crc32_tables as gen
    finally:
        sys.path.pop(0)
    want = [_reflect(_x_power(8 << k)) for k in range(48)]
    assert gen.table() == want
    text = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_crc32_tables.h")).read()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_crc32_tables.py")], capture_output=True, text=True, check=True).stdout
    assert out == text, "sela_crc32_tables.h is not what tools/gen_crc32_tables.py writes"
    import re

    assert [int(v, 16) for v in re.findall(r"0x([0-9A-F]{8})u", text)] == want


def test_crc32_combine_stand_alone(tmp_path):
    """tests/c/crc32_combine.cpp: sela_amd/csrc/sela_crc32.h and host/include/sela_host/digest.hpp alone under
    -fsanitize=address,undefined, run directly."""
    from test_pcm_cpu import _compile

    exe = _compile(tmp_path, "crc32_combine", [os.path.join(ROOT, "tests", "c", "crc32_combine.cpp")],
                   ["-I" + os.path.join(ROOT, "sela_amd", "csrc"), "-I" + os.path.join(ROOT, "host", "include")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "crc32_combine: 0 failures" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    assert "sela_hip_debug_digest_lds_bytes" in capi.DEBUG_EXPORTS
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES) and hasattr(lib, "sela_hip_debug_digest_lds_bytes")
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    assert all(n + "(" in header for n in NAMES) and "struct sela_hip_digest {" in header
    assert "sela_hip_debug_digest_lds_bytes(" in open(os.path.join(ROOT, "include", "sela_hip_debug.h")).read()


def test_the_kernels_have_a_translation_unit_of_their_own():
    import __graft_entry__ as entry

    assert "sela_digest.hip" in entry.HIP_SOURCES
    text = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_digest.hip")).read()
    assert all(k in text for k in ("k_digest_frames", "k_digest_pcm", "k_digest_fold")) and '#include "sela_decode_core.inc"' in text


def test_the_record_is_8_bytes():
    d = codec.DIGEST_DTYPE
    assert d.itemsize == 8 and [(n, d.fields[n][0].str, d.fields[n][1]) for n in d.names] == [("crc32", "<u4", 0), ("samples", "<u4", 4)]


def test_the_lds_plan_is_the_levels_kernels():
    lib = capi.lib()
    for ch in range(0, 10):
        assert int(lib.sela_hip_debug_digest_lds_bytes(ch)) == int(lib.sela_hip_debug_levels_lds_bytes(ch)), ch


def test_the_workspace_formula_piece_by_piece():
    lib = capi.lib()
    ws, lev = lib.sela_hip_digest_workspace_bytes, lib.sela_hip_levels_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for frames, ch, stride in [(0, 1, 1), (1, 2, 2048), (1, 2, 2049), (3875, 2, 2048), (4097, 3, 777), (5, 8, 4096), (5, 9, 4096), (7, 255, 65535), (1, 1, 1),
                               (70000, 1, 16384), (65536, 2, 8193)]:
        slices = max((2 * ch * stride + 32767) // 32768, 1)
        # the levels call's two pieces | a word per (frame, slice of 32 KiB) | the fold's word per workgroup
        want = int(lev(frames, ch, stride)) + up(4 * max(frames * slices, 1)) + up(4 * min(max((frames + 255) // 256, 1), 256))
        assert int(ws(frames, ch, stride)) == want, (frames, ch, stride)
    for shape in [(0xFFFFFFFF, 255, 0xFFFFFFFF), (1 << 31, 1, 1), (0x80000000, 2, 0xFFFFFFFF), ((1 << 31) // 255 + 1, 255, 1), (1 << 30, 1, 1 << 30), (1, 0, 2048),
                  (0, 0, 1)]:
        assert int(lev(*shape)) == SIZE_MAX and int(ws(*shape)) == SIZE_MAX, shape
    # sela_hip_crc32_device: a word per slice of max(32 KiB, n / 4096 rounded up to 16), one piece
    cw = lib.sela_hip_crc32_workspace_bytes
    for n, slices in [(0, 1), (1, 1), (32768, 1), (32769, 2), ((1 << 20) + 3, 33), (4096 * 32768, 4096), (4096 * 32768 + 1, 4095), (1 << 40, 4096)]:
        slice_bytes = max(32768, ((n + 4095) // 4096 + 15) // 16 * 16)
        assert max((n + slice_bytes - 1) // slice_bytes, 1) == slices and slices <= 4096, n
        assert int(cw(n)) == up(4 * slices) + 256, n


def test_argument_errors_are_found_before_any_device_is_asked_for():
    lib = capi.lib()
    one = 0x1000  # (never dereferenced: every call below fails on its arguments)
    big = 1 << 40
    dev = lib.sela_hip_digest_device
    err = lib.sela_hip_last_error
    # (d_frames, d_frame_offsets, n_frames, channels, stride, d_digests, d_track, d_sample_offsets, d_status, d_workspace, bytes, stream)
    assert dev(None, None, 1, 0, 2048, None, None, None, None, None, 0, None) == EINVAL and b"channels" in err()
    assert dev(one, one, 1, 256, 2048, one, one, None, one, one, big, None) == EINVAL and b"channels" in err()
    assert dev(one, one, 1, 2, 0, one, one, None, one, one, big, None) == EINVAL and b"stride" in err()
    assert dev(one, one, 1 << 30, 2, 1, one, one, None, one, one, big, None) == EINVAL and b"2^31" in err()
    assert dev(one, one, 1, 2, 2048, None, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_digests
    assert dev(one, one, 1, 2, 2048, one, None, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_track
    assert dev(one, one, 0, 2, 2048, None, None, None, one, one, big, None) == EINVAL and b"null device pointer" in err()  # d_track, no frames
    assert dev(one, one, 1, 2, 2048, one, one, None, None, one, big, None) == EINVAL and b"null device pointer" in err()   # d_status
    assert dev(one, one, 1, 2, 2048, one, one, None, one, None, big, None) == EINVAL and b"null device pointer" in err()   # d_workspace
    assert dev(one, one, 1, 2, 2048, one + 4, one, None, one, one, big, None) == EINVAL and b"8-byte aligned" in err()
    assert dev(one, one, 1, 2, 2048, one, one + 4, None, one, one, big, None) == EINVAL and b"8-byte aligned" in err()
    assert dev(one, None, 1, 2, 2048, one, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_frame_offsets
    assert dev(None, one, 1, 2, 2048, one, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_frames
    assert dev(one + 1, one, 1, 2, 2048, one, one, None, one, one, big, None) == EINVAL and b"d_frames must be 4-byte aligned" in err()
    # the order: the shape, the call's pointers, the alignment of its outputs, the form's pointers, the capacity
    assert dev(one + 1, None, 1, 0, 0, one + 4, None, None, None, one, 0, None) == EINVAL and b"channels" in err()
    assert dev(one + 1, None, 1, 2, 0, one + 4, None, None, None, one, 0, None) == EINVAL and b"stride" in err()
    assert dev(one + 1, None, 1, 2, 2048, one + 4, None, None, None, one, 0, None) == EINVAL and b"null device pointer" in err()
    assert dev(one + 1, None, 1, 2, 2048, one + 4, one, None, one, one, 0, None) == EINVAL and b"d_digests" in err()
    assert dev(one + 1, one, 1, 2, 2048, one, one, None, one, one, 0, None) == EINVAL and b"d_frames" in err()
    need = int(lib.sela_hip_digest_workspace_bytes(1, 2, 2048))
    assert dev(one, one, 1, 2, 2048, one, one, None, one, one, need - 1, None) == ECAPACITY and b"sela_hip_digest_workspace_bytes" in err()
    assert dev(one, one, 1 << 20, 255, 65535, one, one, None, one, one, big, None) == ECAPACITY  # (more than `big`)
    pay = lib.sela_hip_digest_payload_device
    # (d_payload, payload_bytes, max_frames, channels, stride, d_digests, d_track, d_sample_offsets, d_frame_offsets, d_n_frames, d_status, ws, bytes, stream)
    assert pay(None, 0, 1, 2, 2048, None, None, None, None, None, None, None, 0, None) == EINVAL
    assert pay(one, 64, 1, 0, 2048, one, one, None, one, one, one, one, big, None) == EINVAL and b"channels" in err()
    assert pay(one + 2, 64, 1, 2, 2048, one, one, None, one, one, one, one, big, None) == EINVAL and b"d_payload" in err()
    assert pay(one, 64, 1, 2, 0, one, one, None, one, one, one, one, big, None) == EINVAL and b"stride" in err()
    assert pay(one, 64, 1, 2, 2048, None, one, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one, None, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one + 4, one, None, one, one, one, one, big, None) == EINVAL and b"d_digests" in err()
    assert pay(one, 64, 1, 2, 2048, one, one, None, None, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one, one, None, one, None, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one, one, None, one, one, None, one, big, None) == EINVAL
    both = int(lib.sela_hip_index_workspace_bytes(64, 1)) + need
    assert pay(one, 64, 1, 2, 2048, one, one, None, one, one, one, one, both - 1, None) == ECAPACITY
    host = lib.sela_hip_digest
    # (frames, frame_offsets, n_frames, channels, digests, track_crc32, track_bytes)
    assert host(None, None, 1, 2, None, None, None) == EINVAL
    assert host(one, one, 1, 0, None, None, None) == EINVAL and b"channels" in err()
    assert host(one, one, 1, 256, None, None, None) == EINVAL
    assert host(one, one, 1 << 30, 2, None, None, None) == EINVAL and b"2^31" in err()
    assert host(None, one, 1, 2, None, None, None) == EINVAL
    assert host(one, None, 0, 2, None, None, None) == EINVAL
    raw = lib.sela_hip_crc32_device
    # (d_bytes, n_bytes, d_out, d_workspace, bytes, stream)
    assert raw(one, 8, None, one, big, None) == EINVAL and b"null device pointer" in err()
    assert raw(one, 8, one, None, big, None) == EINVAL and b"null device pointer" in err()
    assert raw(None, 8, one, one, big, None) == EINVAL and b"null device pointer" in err()
    assert raw(one, 8, one + 4, one, big, None) == EINVAL and b"d_out" in err()
    assert raw(one, 8, one, one, int(lib.sela_hip_crc32_workspace_bytes(8)) - 1, None) == ECAPACITY and b"sela_hip_crc32_workspace_bytes" in err()


def test_the_host_call_without_frames_returns_0():
    offs = np.zeros(1, np.uint64)
    crc, total = np.full(1, 7, np.uint32), np.full(1, 7, np.uint64)
    assert capi.lib().sela_hip_digest(None, offs.ctypes.data, 0, 2, None, crc.ctypes.data, total.ctypes.data) == 0
    assert int(crc[0]) == 0 and int(total[0]) == 0


def test_the_python_layer_has_the_digester():
    for name in ("digest", "digest_payload", "records", "track_words", "route", "check"):
        assert callable(getattr(codec.Digester, name))
    assert callable(codec.digest_host) and callable(codec.crc32_device) and callable(codec.crc32_combine)
