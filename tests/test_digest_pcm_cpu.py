"""CPU-only side of the digest of 24- and 32-bit streams: the C ABI's declarations and exports, the workspace
formula piece by piece and every argument check of the three calls -- none of which needs a GPU."""
import os

import numpy as np

from sela_amd import capi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
NAMES = ["sela_hip_digest_pcm_workspace_bytes", "sela_hip_digest_pcm_device", "sela_hip_digest_payload_pcm_device", "sela_hip_digest_pcm"]


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    assert "sela_hip_debug_digest_pcm_fallback_frames" in capi.DEBUG_EXPORTS
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES) and hasattr(lib, "sela_hip_debug_digest_pcm_fallback_frames")
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert header.count("struct sela_hip_digest {") == 1, "the record is the 16-bit digest's: no new struct"
    assert "has no digest yet" not in header
    assert "sela_hip_debug_digest_pcm_fallback_frames(" in open(os.path.join(ROOT, "include", "sela_hip_debug.h")).read()


def test_the_kernels_have_a_translation_unit_of_their_own():
    import __graft_entry__ as entry

    assert "sela_digest_pcm.hip" in entry.HIP_SOURCES
    text = open(os.path.join(ROOT, "sela_amd", "csrc", "sela_digest_pcm.hip")).read()
    assert "k_digest32_tiles" in text and '#include "sela_pcm_layout.h"' in text and '#include "sela_verify32_rule.h"' in text


def test_the_python_layer_has_the_digester():
    for name in ("digest", "digest_payload", "records", "track_words", "wide_samples", "check", "fallback_frames"):
        assert callable(getattr(codec.DigesterPcm, name)), name
    assert callable(codec.digest_pcm_host)


def test_the_workspace_formula_piece_by_piece():
    lib = capi.lib()
    ws, dec, ver = lib.sela_hip_digest_pcm_workspace_bytes, lib.sela_hip_decode_i32_workspace_bytes, lib.sela_hip_verify_pcm_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for frames, ch, stride in [(0, 1, 1), (1, 2, 2048), (1, 2, 2049), (3875, 2, 2048), (4097, 3, 777), (5, 8, 4096), (5, 9, 4096), (7, 255, 65535), (1, 1, 1),
                               (70000, 1, 16384), (65536, 2, 8193)]:
        tile = max((4096 // ch) & ~3, 4)
        tiles = (stride + tile - 1) // tile
        want = (int(dec(frames, ch, stride))                       # the subframes as decoded, their records, the index
                + up(frames * ch * stride * 4)                     # the samples by channel, for frames of any other layout
                + up(frames * ch * 4)                              # ... and their counts
                + up(max(frames, 1) * 4)                           # a mark per frame
                + up(max(frames * tiles, 1) * 8)                   # the raw CRC per (frame, tile)
                + 256                                              # the two control words
                + up((frames + 1) * 8)                             # the sample offsets of a caller that passes none
                + up(4 * min(max((frames + 255) // 256, 1), 256)))  # the track fold's word per workgroup
        assert int(ws(frames, ch, stride)) == want, (frames, ch, stride)
        assert int(ws(frames, ch, stride)) == int(ver(frames, ch, stride)) + up(4 * min(max((frames + 255) // 256, 1), 256))
    for shape in [(0xFFFFFFFF, 255, 0xFFFFFFFF), (1 << 31, 1, 1), (0x80000000, 2, 0xFFFFFFFF), ((1 << 31) // 255 + 1, 255, 1), (1 << 30, 1, 1 << 30), (1, 0, 2048),
                  (0, 0, 1)]:
        assert int(ver(*shape)) == SIZE_MAX and int(ws(*shape)) == SIZE_MAX, shape


def test_argument_errors_are_found_before_any_device_is_asked_for():
    lib = capi.lib()
    one = 0x1000  # (never dereferenced: every call below fails on its arguments)
    big = 1 << 40
    dev = lib.sela_hip_digest_pcm_device
    err = lib.sela_hip_last_error
    # (d_frames, d_frame_offsets, n_frames, channels, stride, bytes_per_sample, d_digests, d_track, d_sample_offsets, d_status, d_workspace, bytes, stream)
    assert dev(None, None, 1, 0, 2048, 3, None, None, None, None, None, 0, None) == EINVAL and b"channels" in err()
    assert dev(one, one, 1, 256, 2048, 3, one, one, None, one, one, big, None) == EINVAL and b"channels" in err()
    assert dev(one, one, 1, 2, 0, 3, one, one, None, one, one, big, None) == EINVAL and b"stride" in err()
    assert dev(one, one, 1 << 30, 2, 1, 3, one, one, None, one, one, big, None) == EINVAL and b"2^31" in err()
    assert dev(one, one, 1, 2, 2048, 3, None, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_digests
    assert dev(one, one, 1, 2, 2048, 3, one, None, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_track
    assert dev(one, one, 0, 2, 2048, 3, None, None, None, one, one, big, None) == EINVAL and b"null device pointer" in err()  # d_track, no frames
    assert dev(one, one, 1, 2, 2048, 3, one, one, None, None, one, big, None) == EINVAL and b"null device pointer" in err()   # d_status
    assert dev(one, one, 1, 2, 2048, 3, one, one, None, one, None, big, None) == EINVAL and b"null device pointer" in err()   # d_workspace
    assert dev(one, one, 1, 2, 2048, 3, one + 4, one, None, one, one, big, None) == EINVAL and b"8-byte aligned" in err()
    assert dev(one, one, 1, 2, 2048, 4, one, one + 4, None, one, one, big, None) == EINVAL and b"8-byte aligned" in err()
    for bad in (0, 2, 5):
        assert dev(one, one, 1, 2, 2048, bad, one, one, None, one, one, big, None) == EINVAL and b"bytes_per_sample" in err(), bad
    assert dev(one, one, 1, 2, 2048, 3, one, one, one + 4, one, one, big, None) == EINVAL and b"d_sample_offsets" in err()
    assert dev(one, None, 1, 2, 2048, 3, one, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_frame_offsets
    assert dev(None, one, 1, 2, 2048, 3, one, one, None, one, one, big, None) == EINVAL and b"null device pointer" in err()   # d_frames
    assert dev(one + 1, one, 1, 2, 2048, 3, one, one, None, one, one, big, None) == EINVAL and b"d_frames must be 4-byte aligned" in err()
    # the order: the shape, the call's pointers, the alignment of its outputs, the container, the form's pointers, the capacity
    assert dev(one + 1, None, 1, 0, 0, 2, one + 4, None, None, None, one, 0, None) == EINVAL and b"channels" in err()
    assert dev(one + 1, None, 1, 2, 0, 2, one + 4, None, None, None, one, 0, None) == EINVAL and b"stride" in err()
    assert dev(one + 1, None, 1, 2, 2048, 2, one + 4, None, None, None, one, 0, None) == EINVAL and b"null device pointer" in err()
    assert dev(one + 1, None, 1, 2, 2048, 2, one + 4, one, None, one, one, 0, None) == EINVAL and b"d_digests" in err()
    assert dev(one + 1, None, 1, 2, 2048, 2, one, one, None, one, one, 0, None) == EINVAL and b"bytes_per_sample" in err()
    assert dev(one + 1, one, 1, 2, 2048, 3, one, one, None, one, one, 0, None) == EINVAL and b"d_frames" in err()
    need = int(lib.sela_hip_digest_pcm_workspace_bytes(1, 2, 2048))
    assert dev(one, one, 1, 2, 2048, 3, one, one, None, one, one, need - 1, None) == ECAPACITY and b"sela_hip_digest_pcm_workspace_bytes" in err()
    assert dev(one, one, 1 << 20, 255, 65535, 4, one, one, None, one, one, big, None) == ECAPACITY  # (more than `big`)
    pay = lib.sela_hip_digest_payload_pcm_device
    # (d_payload, payload_bytes, max_frames, channels, stride, bytes_per_sample, d_digests, d_track, d_sample_offsets, d_frame_offsets, d_n_frames, d_status, ws, bytes, stream)
    assert pay(None, 0, 1, 2, 2048, 3, None, None, None, None, None, None, None, 0, None) == EINVAL
    assert pay(one, 64, 1, 0, 2048, 3, one, one, None, one, one, one, one, big, None) == EINVAL and b"channels" in err()
    assert pay(one + 2, 64, 1, 2, 2048, 3, one, one, None, one, one, one, one, big, None) == EINVAL and b"d_payload" in err()
    assert pay(one, 64, 1, 2, 0, 3, one, one, None, one, one, one, one, big, None) == EINVAL and b"stride" in err()
    assert pay(one, 64, 1, 2, 2048, 3, None, one, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, 3, one, None, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, 3, one + 4, one, None, one, one, one, one, big, None) == EINVAL and b"d_digests" in err()
    for bad in (0, 2, 5):
        assert pay(one, 64, 1, 2, 2048, bad, one, one, None, one, one, one, one, big, None) == EINVAL and b"bytes_per_sample" in err(), bad
    assert pay(one, 64, 1, 2, 2048, 3, one, one, None, None, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, 3, one, one, None, one, None, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, 3, one, one, None, one, one, None, one, big, None) == EINVAL
    both = int(lib.sela_hip_index_workspace_bytes(64, 1)) + need
    assert pay(one, 64, 1, 2, 2048, 3, one, one, None, one, one, one, one, both - 1, None) == ECAPACITY
    host = lib.sela_hip_digest_pcm
    # (frames, frame_offsets, n_frames, channels, bytes_per_sample, digests, track_crc32, track_bytes, wide_samples)
    assert host(None, None, 1, 2, 3, None, None, None, None) == EINVAL
    assert host(one, one, 1, 0, 3, None, None, None, None) == EINVAL and b"channels" in err()
    assert host(one, one, 1, 256, 3, None, None, None, None) == EINVAL
    assert host(one, one, 1 << 30, 2, 3, None, None, None, None) == EINVAL and b"2^31" in err()
    assert host(None, one, 1, 2, 3, None, None, None, None) == EINVAL
    assert host(one, None, 0, 2, 3, None, None, None, None) == EINVAL
    for bad in (0, 2, 5):
        assert host(one, one, 1, 2, bad, None, None, None, None) == EINVAL and b"bytes_per_sample" in err(), bad
    assert host(one, one, 1, 0, 2, None, None, None, None) == EINVAL and b"channels" in err()  # the shape comes first


def test_the_host_call_without_frames_returns_0():
    offs = np.zeros(1, np.uint64)
    for bps in (3, 4):
        crc, total, wide = np.full(1, 7, np.uint32), np.full(1, 7, np.uint64), np.full(1, 7, np.uint32)
        assert capi.lib().sela_hip_digest_pcm(None, offs.ctypes.data, 0, 2, bps, None, crc.ctypes.data, total.ctypes.data, wide.ctypes.data) == 0
        assert int(crc[0]) == 0 and int(total[0]) == 0 and int(wide[0]) == 0
        assert capi.lib().sela_hip_digest_pcm(None, offs.ctypes.data, 0, 2, bps, None, None, None, None) == 0
