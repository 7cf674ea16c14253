"""CPU-only: packed 3- / 4-byte PCM as far as it needs no device -- the names, the sizing functions, every refusal the
entries give for their arguments -- its code and the whole text of sela_hip_last_error() (the pointers are made-up addresses, so
a row that got past its refusal would fault: that nothing is enqueued is not observed here) --, the verdict on the status words in
its order, and the two kernels' resources from the shipped code object."""
import os

import numpy as np
import pytest

from sela_amd import capi, codec

EINVAL, ECAPACITY, EFORMAT, ERANGE, ENODEV = -2, -4, -5, -6, -1
SIZE_MAX = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["sela_hip_pcm_unpack_device", "sela_hip_pcm_pack_device", "sela_hip_encode_pcm_workspace_bytes", "sela_hip_encode_pcm_bound_bytes",
         "sela_hip_encode_pcm_device", "sela_hip_decode_pcm_workspace_bytes", "sela_hip_decode_pcm_device", "sela_hip_decode_pcm_status_error",
         "sela_hip_encode_pcm", "sela_hip_decode_pcm"]


def A(k):
    """a made-up device address, 4096-aligned"""
    return 0x7F0000000000 + 0x100000 * k


def test_exports_and_python_names():
    lib = capi.lib()
    header = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert name + "(" in header, name
    assert "sela_hip_debug_pcm_chunk_frames" in capi.DEBUG_EXPORTS and hasattr(lib, "sela_hip_debug_pcm_chunk_frames")
    assert "sela_hip_debug_pcm_chunk_frames(" in open(os.path.join(ROOT, "include", "sela_hip_debug.h")).read()
    for name in ("EncoderPcm", "DecoderPcm", "encode_pcm_host", "decode_pcm_host", "decode_pcm_status_error", "pcm_unpack", "pcm_pack"):
        assert callable(getattr(codec, name)), name
    for method in ("encode", "check", "to_host", "needed_bytes"):
        assert callable(getattr(codec.EncoderPcm, method))
    for method in ("decode", "check", "wide_samples"):
        assert callable(getattr(codec.DecoderPcm, method))


SHAPES = [(1, 1, 1), (1, 2, 2048), (3, 2, 2048), (3, 3, 1000), (7, 5, 2049), (2, 255, 65535), (3875, 2, 2048)]


def test_workspace_bytes():
    lib = capi.lib()
    for f, c, n in SHAPES:
        assert int(lib.sela_hip_encode_pcm_workspace_bytes(f, c, n)) >= int(lib.sela_hip_encode_i32_workspace_bytes(f, c, n)) + 4 * f * c * n
        # the decode's: the i32 call's, its samples, counts and sample offsets
        assert int(lib.sela_hip_decode_pcm_workspace_bytes(f, c, n)) >= int(lib.sela_hip_decode_i32_workspace_bytes(f, c, n)) + 4 * f * c * n + 4 * f * c + 8 * (f + 1)
    for bad in ((1, 0, 2048), (1, 256, 2048), (1, 2, 0), (1, 2, 65536), (1 << 31, 1, 16)):
        assert int(lib.sela_hip_encode_pcm_workspace_bytes(*bad)) == SIZE_MAX, bad


def test_bound_bytes():
    lib = capi.lib()
    bound = lambda f, c, n, b: int(lib.sela_hip_encode_pcm_bound_bytes(f, c, n, b))  # noqa: E731
    for f, c, n in SHAPES:
        for b in (3, 4):
            here = bound(f, c, n, b)
            assert here >= int(lib.sela_hip_encode_bound_bytes_n(f, c, n))
            assert bound(f + 1, c, n, b) >= here and bound(f, c + 1, n, b) >= here and bound(f, c, n + 1, b) >= here and bound(f, c, n, 4) >= bound(f, c, n, 3)
    # the derivation of include/sela_hip.h, restated: per subframe the header, 32 coefficient words and the residue words of k = 19
    for f, c, n in SHAPES:
        words = min(65535, (n * 4115 + 31) // 32)
        assert bound(f, c, n, 3) >= f * (4 + c * (12 + 4 * (32 + words)))


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------
T_BYTES = "bytes_per_sample must be 3 or 4 (16-bit samples: sela_hip_encode_n_device / sela_hip_decode_n_device and the int16 host calls)"
T_CHANNELS = "channels must be in 1..255"
T_SAMPLES = "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)"
T_STRIDE = "stride must not be 0"
T_SIGNALS = "n_frames * signals per frame must stay below 2^31"
T_OPTIONS = "options: a bit this library does not know (SELA_HIP_ENCODE_LOSSLESS is the only one)"
T_NULL_DEVICE = "null device pointer"
T_NULL = "null pointer"

ENCODE = [("d_pcm", A(1)), ("bytes_per_sample", 3), ("n_frames", 3), ("channels", 2), ("samples_per_channel", 2048), ("options", 0), ("d_frames", A(2)),
          ("frames_cap", 1 << 20), ("d_frame_offsets", A(3)), ("d_status", A(4)), ("d_workspace", A(5)), ("workspace_bytes", None), ("stream", 0)]
DECODE = [("d_frames", A(1)), ("d_frame_offsets", A(2)), ("n_frames", 3), ("channels", 2), ("stride", 2048), ("bytes_per_sample", 3), ("d_pcm_out", A(3)),
          ("d_sample_offsets", A(4)), ("d_status", A(5)), ("d_workspace", A(6)), ("workspace_bytes", None), ("stream", 0)]
UNPACK = [("d_pcm", A(1)), ("bytes_per_sample", 3), ("n_frames", 3), ("channels", 2), ("samples_per_channel", 2048), ("d_samples", A(2)), ("stream", 0)]
PACK = [("d_samples", A(1)), ("d_counts", A(2)), ("d_sample_offsets", A(3)), ("n_frames", 3), ("channels", 2), ("stride", 2048), ("bytes_per_sample", 3),
        ("d_pcm_out", A(4)), ("d_status", A(5)), ("stream", 0)]
HOST_ENCODE = [("pcm", A(1)), ("bytes_per_sample", 3), ("n_frames", 3), ("channels", 2), ("samples_per_channel", 2048), ("options", 0), ("frames_out", A(2)),
               ("frames_cap", 1 << 20), ("frame_offsets_out", A(3))]
HOST_DECODE = [("frames", A(1)), ("frame_offsets", A(2)), ("n_frames", 3), ("channels", 2), ("bytes_per_sample", 3), ("pcm_out", A(3)), ("pcm_cap", 1 << 20),
               ("wide_samples", 0)]
CALLS = {"encode": ("sela_hip_encode_pcm_device", ENCODE, "sela_hip_encode_pcm_workspace_bytes", "samples_per_channel"),
         "decode": ("sela_hip_decode_pcm_device", DECODE, "sela_hip_decode_pcm_workspace_bytes", "stride"),
         "unpack": ("sela_hip_pcm_unpack_device", UNPACK, None, None), "pack": ("sela_hip_pcm_pack_device", PACK, None, None),
         "host_encode": ("sela_hip_encode_pcm", HOST_ENCODE, None, None), "host_decode": ("sela_hip_decode_pcm", HOST_DECODE, None, None)}


def _call(which, **changes):
    name, table, sizing, length = CALLS[which]
    short = changes.pop("short", 0)
    a = dict(table)
    assert not set(changes) - set(a), changes
    a.update(changes)
    lib = capi.lib()
    if a.get("workspace_bytes", 0) is None:
        a["workspace_bytes"] = max(int(getattr(lib, sizing)(a["n_frames"], a["channels"], a[length])) - short, 0) & SIZE_MAX
    rc = getattr(lib, name)(*[a[key] for key, _ in table])
    return rc, lib.sela_hip_last_error().decode()


ROWS = [
    # the container, and the order: it is asked first
    ("encode", EINVAL, T_BYTES, dict(bytes_per_sample=2)), ("encode", EINVAL, T_BYTES, dict(bytes_per_sample=0, channels=0)),
    ("encode", EINVAL, T_BYTES, dict(bytes_per_sample=5)), ("decode", EINVAL, T_BYTES, dict(bytes_per_sample=2)),
    ("decode", EINVAL, T_BYTES, dict(bytes_per_sample=8, stride=0)), ("unpack", EINVAL, T_BYTES, dict(bytes_per_sample=1)),
    ("pack", EINVAL, T_BYTES, dict(bytes_per_sample=2)), ("host_encode", EINVAL, T_BYTES, dict(bytes_per_sample=2)),
    ("host_decode", EINVAL, T_BYTES, dict(bytes_per_sample=6)),
    # channels
    ("encode", EINVAL, T_CHANNELS, dict(channels=0)), ("encode", EINVAL, T_CHANNELS, dict(channels=256, samples_per_channel=0)),
    ("decode", EINVAL, T_CHANNELS, dict(channels=0)), ("decode", EINVAL, T_CHANNELS, dict(channels=256)), ("unpack", EINVAL, T_CHANNELS, dict(channels=256)),
    ("pack", EINVAL, T_CHANNELS, dict(channels=0)), ("host_encode", EINVAL, T_CHANNELS, dict(channels=0)), ("host_decode", EINVAL, T_CHANNELS, dict(channels=256)),
    # the length
    ("encode", EINVAL, T_SAMPLES, dict(samples_per_channel=0)), ("encode", EINVAL, T_SAMPLES, dict(samples_per_channel=65536, bytes_per_sample=4)),
    ("unpack", EINVAL, T_SAMPLES, dict(samples_per_channel=0)), ("unpack", EINVAL, T_SAMPLES, dict(samples_per_channel=65536)),
    ("host_encode", EINVAL, T_SAMPLES, dict(samples_per_channel=65536)),
    ("decode", EINVAL, T_STRIDE, dict(stride=0)), ("pack", EINVAL, T_STRIDE, dict(stride=0)),
    # frames x signals
    ("encode", EINVAL, T_SIGNALS, dict(n_frames=1 << 31, channels=1)), ("encode", EINVAL, T_SIGNALS, dict(n_frames=(1 << 31) // 3 + 1, channels=2)),
    ("decode", EINVAL, T_SIGNALS, dict(n_frames=1 << 31, channels=1)), ("unpack", EINVAL, T_SIGNALS, dict(n_frames=(1 << 31) // 255 + 1, channels=255)),
    ("pack", EINVAL, T_SIGNALS, dict(n_frames=(1 << 31) // 3 + 1, channels=2)), ("host_encode", EINVAL, T_SIGNALS, dict(n_frames=1 << 31, channels=1)),
    # options
    ("encode", EINVAL, T_OPTIONS, dict(options=2)), ("encode", EINVAL, T_OPTIONS, dict(options=capi.ENCODE_LOSSLESS | 0x80000000, d_pcm=0)),
    ("host_encode", EINVAL, T_OPTIONS, dict(options=4)),
    # pointers
    ("encode", EINVAL, T_NULL_DEVICE, dict(d_pcm=0)), ("encode", EINVAL, T_NULL_DEVICE, dict(d_frames=0)), ("encode", EINVAL, T_NULL_DEVICE, dict(d_frame_offsets=0)),
    ("encode", EINVAL, T_NULL_DEVICE, dict(d_frame_offsets=0, n_frames=0)), ("encode", EINVAL, T_NULL_DEVICE, dict(d_status=0)),
    ("encode", EINVAL, T_NULL_DEVICE, dict(d_workspace=0)),
    ("decode", EINVAL, T_NULL_DEVICE, dict(d_frames=0)), ("decode", EINVAL, T_NULL_DEVICE, dict(d_frame_offsets=0)), ("decode", EINVAL, T_NULL_DEVICE, dict(d_pcm_out=0)),
    ("decode", EINVAL, T_NULL_DEVICE, dict(d_status=0)), ("decode", EINVAL, T_NULL_DEVICE, dict(d_workspace=0, d_sample_offsets=0)),
    ("unpack", EINVAL, T_NULL_DEVICE, dict(d_pcm=0)), ("unpack", EINVAL, T_NULL_DEVICE, dict(d_samples=0)),
    ("pack", EINVAL, T_NULL_DEVICE, dict(d_samples=0)), ("pack", EINVAL, T_NULL_DEVICE, dict(d_counts=0)), ("pack", EINVAL, T_NULL_DEVICE, dict(d_sample_offsets=0)),
    ("pack", EINVAL, T_NULL_DEVICE, dict(d_pcm_out=0)), ("pack", EINVAL, T_NULL_DEVICE, dict(d_status=0, n_frames=0)),
    ("host_encode", EINVAL, T_NULL, dict(pcm=0)), ("host_encode", EINVAL, T_NULL, dict(frames_out=0)), ("host_encode", EINVAL, T_NULL, dict(frame_offsets_out=0, n_frames=0)),
    ("host_decode", EINVAL, T_NULL, dict(frames=0)), ("host_decode", EINVAL, T_NULL, dict(frame_offsets=0)), ("host_decode", EINVAL, T_NULL, dict(pcm_out=0)),
    # alignment of the base pointers, before the capacity
    ("encode", EINVAL, "d_pcm and d_frames must be 4-byte aligned", dict(d_pcm=A(1) + 1)),
    ("encode", EINVAL, "d_pcm and d_frames must be 4-byte aligned", dict(d_pcm=A(1) + 3, bytes_per_sample=4)),
    ("encode", EINVAL, "d_pcm and d_frames must be 4-byte aligned", dict(d_frames=A(2) + 2, short=1)),
    ("decode", EINVAL, "d_frames and d_pcm_out must be 4-byte aligned", dict(d_frames=A(1) + 2)),
    ("decode", EINVAL, "d_frames and d_pcm_out must be 4-byte aligned", dict(d_pcm_out=A(3) + 3, short=1)),
    ("unpack", EINVAL, "d_pcm and d_samples must be 4-byte aligned", dict(d_pcm=A(1) + 2)),
    ("unpack", EINVAL, "d_pcm and d_samples must be 4-byte aligned", dict(d_samples=A(2) + 1)),
    ("pack", EINVAL, "d_samples, d_counts, d_pcm_out and d_status must be 4-byte aligned, d_sample_offsets 8-byte aligned", dict(d_pcm_out=A(4) + 1)),
    ("pack", EINVAL, "d_samples, d_counts, d_pcm_out and d_status must be 4-byte aligned, d_sample_offsets 8-byte aligned", dict(d_sample_offsets=A(3) + 4)),
    # the workspace
    ("encode", ECAPACITY, "workspace smaller than sela_hip_encode_pcm_workspace_bytes()", dict(short=1)),
    ("encode", ECAPACITY, "workspace smaller than sela_hip_encode_pcm_workspace_bytes()", dict(short=1, bytes_per_sample=4, options=capi.ENCODE_LOSSLESS)),
    ("encode", ECAPACITY, "workspace smaller than sela_hip_encode_pcm_workspace_bytes()", dict(short=1, n_frames=0, d_pcm=0, d_frames=0)),
    ("encode", ECAPACITY, "workspace smaller than sela_hip_encode_pcm_workspace_bytes()", dict(workspace_bytes=0)),
    ("decode", ECAPACITY, "workspace smaller than sela_hip_decode_pcm_workspace_bytes()", dict(short=1)),
    ("decode", ECAPACITY, "workspace smaller than sela_hip_decode_pcm_workspace_bytes()", dict(short=1, d_sample_offsets=0, bytes_per_sample=4)),
    ("decode", ECAPACITY, "workspace smaller than sela_hip_decode_pcm_workspace_bytes()", dict(short=1, n_frames=0, d_frames=0, d_pcm_out=0)),
]


@pytest.mark.parametrize("which, code, text, changes", ROWS, ids=["%02d-%s" % (i, r[0]) for i, r in enumerate(ROWS)])
def test_refusal(which, code, text, changes):
    assert _call(which, **changes) == (code, text)


# ---- the verdict on the status words ------------------------------------------------------------------------------------------------
def test_status_error_order():
    """sela_hip_decode_status_error's order -- the stride, malformed frames and dry Rice streams, the range errors, the internal
    flag -- on [0..2]; [3] decides nothing."""
    judge = codec.decode_pcm_status_error
    F = capi
    assert judge([0, 0, 2048, 0]) == 0 and judge([0, 0, 2048, 12345]) == 0 and judge([F.FLAG_Q_RANGE, 0, 0, 7]) == codec.decode_status_error([F.FLAG_Q_RANGE, 0, 0, 0])
    ladder = [(F.FLAG_STRIDE, ECAPACITY), (F.FLAG_BAD_FRAME, EFORMAT), (F.FLAG_RICE_OVERRUN, EFORMAT), (F.FLAG_COEF_OVERFLOW, ERANGE), (F.FLAG_SHORT_BLOCK, ERANGE),
              (F.FLAG_INTERNAL, ENODEV)]
    for flag, code in ladder:
        for wide in (0, 9):
            assert judge([flag, 0, 100, wide]) == code == codec.decode_status_error([flag, 0, 100, 0]), flag
    assert judge([0, 3, 100, 0]) == EFORMAT  # malformed frames counted, no flag
    for i, (flag, code) in enumerate(ladder):  # an earlier rung wins over every later one
        later = 0
        for other, _ in ladder[i + 1:]:
            later |= other
        assert judge([flag | later, 0, 100, 1]) == codec.decode_status_error([flag | later, 0, 100, 0])
    assert judge([F.FLAG_STRIDE | F.FLAG_BAD_FRAME, 1, 100, 0]) == ECAPACITY
    lib = capi.lib()
    assert (lib.sela_hip_decode_pcm_status_error(None), lib.sela_hip_last_error().decode()) == (EINVAL, "null pointer")


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
def test_the_kernels_use_no_scratch():
    """From the shipped code object (tools/kernel_resources.py): both kernels in both widths, no spill, no scratch, the image in LDS."""
    import sys
    import tempfile

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    found = {}
    with tempfile.TemporaryDirectory() as d:
        for co in kernel_resources.code_objects(capi.LIB_PATH, d):
            for name, res in kernel_resources.resources(co):
                if "k_pcm_" in name:
                    found[name] = res
    for kernel in ("k_pcm_unpack", "k_pcm_pack"):
        for width in (3, 4):
            names = [n for n in found if kernel + "ILi%dEE" % width in n]
            assert len(names) == 1, (kernel, width, sorted(found))
            r = found[names[0]]
            assert int(r[".private_segment_fixed_size"]) == 0 and int(r[".vgpr_spill_count"]) == 0 and int(r[".sgpr_spill_count"]) == 0, (names[0], r)
            assert 4 * 4096 <= int(r[".group_segment_fixed_size"]) <= 17 * 1024, (names[0], r)  # the image (4100 dwords) and the words of the block-wide reductions
    assert len(found) == 4, sorted(found)


def test_host_layout_matches_numpy():
    """The scalar rule the GPU tests compare against, on the sign-extension traps: 3 little-endian bytes -> int32 and back."""
    raw = np.array([0x80, 0, 0, 0xFF, 0xFF, 0x7F, 0xFF, 0xFF, 0xFF, 0, 0, 0x80], dtype=np.uint8).reshape(-1, 3)
    v = (raw[:, 0].astype(np.int32) | (raw[:, 1].astype(np.int32) << 8) | (raw[:, 2].astype(np.int8).astype(np.int32) << 16))
    assert v.tolist() == [128, 8388607, -1, -8388608]
