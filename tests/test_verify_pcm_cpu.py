"""CPU-only side of the verification against packed PCM: tests/c/verify_pcm_layout.cpp, a stand-alone program
built with -fsanitize=address,undefined and run directly, replays the packed side of k_verify_pcm from sela_pcm_layout.h; the C
ABI declares and exports the calls, their sizing follows the formula of include/sela_hip.h piece by piece, and argument errors
need no GPU."""
import os
import subprocess

from sela_amd import capi
from test_pcm_cpu import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = (1 << 64) - 1
NAMES = ["sela_hip_verify_pcm_workspace_bytes", "sela_hip_verify_pcm_device", "sela_hip_verify_payload_pcm_device", "sela_hip_verify_pcm"]
EINVAL, ECAPACITY = -2, -4


def test_verify_pcm_layout(tmp_path):
    exe = _compile(tmp_path, "verify_pcm_layout", [os.path.join(ROOT, "tests", "c", "verify_pcm_layout.cpp")], ["-I" + os.path.join(ROOT, "sela_amd", "csrc")])
    out = subprocess.run([exe], capture_output=True, text=True)
    # 2 containers x 6 channel counts x (12 lengths x 10 tables + 2 of mixed lengths)
    assert out.returncode == 0 and "verify_pcm_layout ok: 1464 launches" in out.stdout, out.stdout + out.stderr


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    assert "sela_hip_debug_verify_pcm_fallback_frames" in capi.DEBUG_EXPORTS
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES + ["sela_hip_debug_verify_pcm_fallback_frames"])
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert "verification against packed PCM" in header
    assert "sela_hip_debug_verify_pcm_fallback_frames(" in open(os.path.join(ROOT, "include", "sela_hip_debug.h")).read()


def test_the_kernel_has_a_translation_unit_of_its_own():
    import __graft_entry__ as entry

    assert "sela_verify_pcm.hip" in entry.HIP_SOURCES


def test_the_workspace_formula_piece_by_piece():
    lib = capi.lib()
    ws, dec, v32 = lib.sela_hip_verify_pcm_workspace_bytes, lib.sela_hip_decode_i32_workspace_bytes, lib.sela_hip_verify_i32_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for frames, ch, stride in [(0, 1, 1), (1, 2, 2048), (1, 2, 2049), (1500, 2, 2048), (3875, 2, 2048), (4097, 3, 777), (2, 255, 65535), (3, 5, 4096), (1, 8, 1),
                               (1, 255, 0xFFFFFFFF)]:  # (the last: stride + tile - 1 does not fit 32 bits)
        tile = max((4096 // ch) & ~3, 4)
        tiles = (stride + tile - 1) // tile
        want = (int(dec(frames, ch, stride))              # the subframes as decoded, their records, the index
                + up(frames * ch * stride * 4)           # the samples by channel, for frames of any other layout
                + up(frames * ch * 4)                    # ... and their counts
                + up(max(frames, 1) * 4)                 # a mark per frame
                + up(max(frames * tiles, 1) * 8)         # two words per (frame, tile)
                + 256                                    # the control words
                + up((frames + 1) * 8))                  # the sample offsets
        assert int(ws(frames, ch, stride)) == want, (frames, ch, stride)
    assert (max((4096 // 2) & ~3, 4), max((4096 // 255) & ~3, 4), max((4096 // 3) & ~3, 4)) == (2048, 16, 1364)
    # SIZE_MAX where the int32 verifier's is ...
    for shape in [(1 << 30, 1, 1 << 30), (1 << 23, 255, 1 << 30), (0xFFFFFFFF, 255, 0xFFFFFFFF), (1 << 31, 1, 1), (0x80000000, 2, 0xFFFFFFFF),
                  (0xFFFFFFFF, 255, 0x01010102), ((1 << 31) // 255 + 1, 255, 1)]:
        assert int(v32(*shape)) == SIZE_MAX and int(ws(*shape)) == SIZE_MAX, shape
    assert int(ws((1 << 31) // 255, 255, 1)) < (1 << 40)
    # ... and without channels (a tile has no size)
    assert int(ws(1, 0, 2048)) == SIZE_MAX


def test_argument_errors_are_found_before_any_device_is_asked_for():
    lib = capi.lib()
    one = 0x1000  # (never dereferenced: every call below fails on its arguments)
    big = 1 << 40
    dev = lib.sela_hip_verify_pcm_device
    # (d_frames, d_frame_offsets, n_frames, channels, stride, d_pcm, bytes, pcm_samples, d_diff_counts, d_first_diff, d_sample_offsets, d_status, d_workspace, bytes, stream)
    assert dev(None, None, 1, 0, 2048, None, 3, 0, None, None, None, None, None, 0, None) == EINVAL
    assert dev(one, one, 1, 256, 2048, one, 3, 2048, one, one, None, one, one, big, None) == EINVAL       # channels
    assert dev(one, one, 1, 2, 0, one, 3, 2048, one, one, None, one, one, big, None) == EINVAL            # stride
    assert dev(one, one, 1 << 30, 2, 1, one, 3, 2048, one, one, None, one, one, big, None) == EINVAL      # frames x channels
    assert dev(one, one, 1, 2, 2048, None, 3, 2048, one, one, None, one, one, big, None) == EINVAL        # d_pcm
    assert dev(one, one, 1, 2, 2048, one, 3, 2048, None, one, None, one, one, big, None) == EINVAL        # d_diff_counts
    assert dev(one, one, 1, 2, 2048, one, 3, 2048, one, None, None, one, one, big, None) == EINVAL        # d_first_diff
    assert dev(one, one, 1, 2, 2048, one, 3, 2048, one, one, None, None, one, big, None) == EINVAL        # d_status
    assert dev(one, one, 1, 2, 2048, one, 3, 2048, one, one, None, one, None, big, None) == EINVAL        # d_workspace
    assert dev(one, one, 1, 2, 2048, one, 3, 2048, one + 2, one, None, one, one, big, None) == EINVAL     # misaligned d_diff_counts
    assert dev(one, one, 1, 2, 2048, one, 3, 2048, one, one + 1, None, one, one, big, None) == EINVAL     # misaligned d_first_diff
    for bytes_per_sample in (0, 1, 2, 5, 8):
        assert dev(one, one, 1, 2, 2048, one, bytes_per_sample, 2048, one, one, None, one, one, big, None) == EINVAL
    for off in (1, 2, 3):
        assert dev(one, one, 1, 2, 2048, one + off, 4, 2048, one, one, None, one, one, big, None) == EINVAL  # misaligned d_pcm
    assert dev(one, one, 1, 2, 2048, one, 3, 2048, one, one, one + 4, one, one, big, None) == EINVAL      # misaligned d_sample_offsets
    assert dev(one + 1, one, 1, 2, 2048, one, 3, 2048, one, one, None, one, one, big, None) == EINVAL     # misaligned d_frames
    assert dev(one, None, 1, 2, 2048, one, 3, 2048, one, one, None, one, one, big, None) == EINVAL        # d_frame_offsets
    # the order: the int32 verifier's errors, then the container, then the original's alignment
    assert dev(one, one, 1, 2, 2048, one + 1, 7, 2048, None, one, None, one, one, big, None) == EINVAL and b"null device pointer" in lib.sela_hip_last_error()
    assert dev(one, one, 1, 2, 2048, one + 1, 7, 2048, one, one, None, one, one, big, None) == EINVAL and b"bytes_per_sample" in lib.sela_hip_last_error()
    assert dev(one, one, 1, 2, 2048, one + 1, 3, 2048, one, one, None, one, one, big, None) == EINVAL and b"d_pcm must be 4-byte aligned" in lib.sela_hip_last_error()
    need = int(lib.sela_hip_verify_pcm_workspace_bytes(1, 2, 2048))
    assert dev(one, one, 1, 2, 2048, one, 3, 2048, one, one, None, one, one, need - 1, None) == ECAPACITY  # a smaller workspace
    pay = lib.sela_hip_verify_payload_pcm_device
    # (d_payload, payload_bytes, max_frames, channels, stride, d_pcm, bytes, pcm_samples, d_diff_counts, d_first_diff, d_sample_offsets, d_frame_offsets, d_n_frames, d_status, ws, bytes, stream)
    assert pay(None, 0, 1, 2, 2048, None, 3, 0, None, None, None, None, None, None, None, 0, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, None, 3, 2048, one, one, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one, 2, 2048, one, one, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one + 2, 3, 2048, one, one, None, one, one, one, one, big, None) == EINVAL
    assert pay(one, 64, 1, 2, 2048, one, 3, 2048, one, one, None, one, one, one, one, need - 1, None) == ECAPACITY
    host = lib.sela_hip_verify_pcm
    # (frames, frame_offsets, n_frames, channels, bytes, pcm, pcm_samples, diff_counts, first_diff, lossy_frames)
    assert host(None, None, 1, 2, 3, None, 0, None, None, None) == EINVAL
    assert host(one, one, 1, 0, 3, one, 1, one, one, None) == EINVAL
    assert host(one, one, 1, 256, 3, one, 1, one, one, None) == EINVAL
    assert host(one, one, 1, 2, 3, None, 1, one, one, None) == EINVAL
    assert host(one, one, 1 << 30, 2, 3, one, 1, one, one, None) == EINVAL
    assert host(one, one, 1, 2, 2, one, 1, one, one, None) == EINVAL
    assert host(None, None, 0, 2, 3, None, 0, None, None, None) == 0  # no frames: nothing to do


def test_the_python_layer_has_the_verifier():
    from sela_amd import codec

    for name in ("verify", "verify_payload", "lossy_frames", "fallback_frames", "check"):
        assert callable(getattr(codec.VerifierPcm, name))
    assert callable(codec.verify_pcm_host)
