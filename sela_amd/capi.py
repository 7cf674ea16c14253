"""ctypes bindings of libsela_hip.so (the C ABI declared in include/sela_hip.h).

Importing this module does not need a GPU; calling into it does.  If the shared library has not
been built, `lib()` raises -- there is no fallback implementation.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsela_hip.so")

OK = 0
ERRORS = {-1: "ENODEV", -2: "EINVAL", -3: "ENOMEM", -4: "ECAPACITY", -5: "EFORMAT", -6: "ERANGE"}
SAMPLES_PER_FRAME = 2048

FLAG_Q_RANGE, FLAG_COEF_OVERFLOW, FLAG_RICE_RANGE, FLAG_RICE_OVERRUN, FLAG_WORDS_CAP, FLAG_BAD_FRAME, FLAG_INTERNAL, FLAG_SHORT_BLOCK = 1, 2, 4, 8, 16, 32, 64, 128
FLAG_STRIDE = 256

# every symbol include/sela_hip.h declares
EXPORTS = [
    "sela_hip_init", "sela_hip_shutdown", "sela_hip_thread_release", "sela_hip_last_error", "sela_hip_device_count",
    "sela_hip_signals_per_frame", "sela_hip_encode_workspace_bytes", "sela_hip_decode_workspace_bytes",
    "sela_hip_encode_bound_bytes", "sela_hip_encode_device", "sela_hip_decode_device",
    "sela_hip_encode", "sela_hip_decode", "sela_hip_index_frames",
    "sela_hip_enable_kernel_timing", "sela_hip_kernel_times",
    "sela_hip_lpc_encode", "sela_hip_lpc_decode", "sela_hip_rice_encode", "sela_hip_rice_decode",
    "sela_hip_host_alloc", "sela_hip_host_free", "sela_hip_decode_max_channels",
    "sela_hip_encode_begin", "sela_hip_encode_feed", "sela_hip_encode_end",
    "sela_hip_decode_begin", "sela_hip_decode_feed", "sela_hip_decode_end",
    "sela_hip_encode_bound_bytes_n", "sela_hip_index_samples", "sela_hip_encode_i32", "sela_hip_decode_i32", "sela_hip_encode_ragged_i32",
    "sela_hip_lpc_encode_n", "sela_hip_lpc_decode_n",
    "sela_hip_index_workspace_bytes", "sela_hip_index_frames_device", "sela_hip_decode_payload_device",
    "sela_hip_decode_i32_workspace_bytes", "sela_hip_decode_i32_device", "sela_hip_decode_payload_i32_device", "sela_hip_decode_status_error",
    "sela_hip_decode_n_workspace_bytes", "sela_hip_decode_n_device", "sela_hip_decode_payload_n_device", "sela_hip_decode_n_status_error",
    "sela_hip_encode_i32_workspace_bytes", "sela_hip_encode_i32_device", "sela_hip_encode_n_device", "sela_hip_encode_status_error",
    "sela_hip_verify_workspace_bytes", "sela_hip_verify_device", "sela_hip_verify_payload_device", "sela_hip_verify",
    "sela_hip_verify_i32_workspace_bytes", "sela_hip_verify_i32_device", "sela_hip_verify_payload_i32_device", "sela_hip_verify_i32",
    "sela_hip_encode_device_opt", "sela_hip_encode_n_device_opt", "sela_hip_encode_i32_device_opt", "sela_hip_encode_opt", "sela_hip_encode_i32_opt",
    "sela_hip_encode_ragged_i32_opt", "sela_hip_encode_begin_opt",
    "sela_hip_decode_windows_workspace_bytes", "sela_hip_decode_windows_device", "sela_hip_decode_windows",
    "sela_hip_decode_windows_whole_workspace_bytes", "sela_hip_decode_windows_whole_device", "sela_hip_decode_windows_whole",
    "sela_hip_decode_windows_i32_workspace_bytes", "sela_hip_decode_windows_i32_device", "sela_hip_decode_windows_i32",
    "sela_hip_decode_windows_i32_whole_workspace_bytes", "sela_hip_decode_windows_i32_whole_device", "sela_hip_decode_windows_i32_whole",
    "sela_hip_encode_whole_pcm_bound_bytes", "sela_hip_encode_whole_pcm_workspace_bytes", "sela_hip_encode_whole_pcm_device", "sela_hip_encode_whole_pcm",
    "sela_hip_paired_signals_per_frame", "sela_hip_encode_paired_workspace_bytes", "sela_hip_encode_paired_i32_device", "sela_hip_encode_paired_n_device",
    "sela_hip_encode_paired_i32", "sela_hip_encode_paired",
    "sela_hip_whole_frames", "sela_hip_whole_frame", "sela_hip_encode_whole_bound_bytes", "sela_hip_encode_whole_workspace_bytes",
    "sela_hip_encode_whole_device", "sela_hip_encode_whole",
    "sela_hip_decode_whole_workspace_bytes", "sela_hip_decode_whole_device", "sela_hip_decode_whole_payload_device", "sela_hip_decode_whole_status_error",
    "sela_hip_decode_whole",
    "sela_hip_pcm_unpack_device", "sela_hip_pcm_pack_device", "sela_hip_encode_pcm_workspace_bytes", "sela_hip_encode_pcm_bound_bytes",
    "sela_hip_encode_pcm_device", "sela_hip_decode_pcm_workspace_bytes", "sela_hip_decode_pcm_device", "sela_hip_decode_pcm_status_error",
    "sela_hip_encode_pcm", "sela_hip_decode_pcm",
    "sela_hip_verify_pcm_workspace_bytes", "sela_hip_verify_pcm_device", "sela_hip_verify_payload_pcm_device", "sela_hip_verify_pcm",
    "sela_hip_levels_workspace_bytes", "sela_hip_levels_device", "sela_hip_levels_payload_device", "sela_hip_levels",
    "sela_hip_levels_i32_workspace_bytes", "sela_hip_levels_i32_device", "sela_hip_levels_payload_i32_device", "sela_hip_levels_samples_i32_workspace_bytes",
    "sela_hip_levels_samples_i32_device", "sela_hip_levels_i32",
    "sela_hip_digest_workspace_bytes", "sela_hip_digest_device", "sela_hip_digest_payload_device", "sela_hip_digest", "sela_hip_crc32_combine",
    "sela_hip_crc32_workspace_bytes", "sela_hip_crc32_device",
    "sela_hip_digest_pcm_workspace_bytes", "sela_hip_digest_pcm_device", "sela_hip_digest_payload_pcm_device", "sela_hip_digest_pcm",
    "sela_hip_salvage_frames", "sela_hip_salvage_workspace_bytes", "sela_hip_salvage_frames_device", "sela_hip_salvage_payload_device",
    "sela_hip_salvage_frames_unaligned", "sela_hip_salvage_unaligned_workspace_bytes", "sela_hip_salvage_frames_unaligned_device",
    "sela_hip_salvage_payload_unaligned_device",
    "sela_hip_envelope_slots", "sela_hip_envelope_workspace_bytes", "sela_hip_envelope_device", "sela_hip_envelope_payload_device", "sela_hip_envelope",
    "sela_hip_envelope_i32_workspace_bytes", "sela_hip_envelope_i32_device", "sela_hip_envelope_payload_i32_device",
    "sela_hip_envelope_samples_i32_workspace_bytes", "sela_hip_envelope_samples_i32_device", "sela_hip_envelope_i32",
]
WINDOW_I16_INTERLEAVED, WINDOW_F32_PLANAR = 0, 1  # SELA_HIP_WINDOW_*
WINDOW_I32_PLANAR, WINDOW_PCM24_INTERLEAVED, WINDOW_PCM32_INTERLEAVED = 2, 3, 4  # (sela_hip_decode_windows_i32*: these and F32_PLANAR)
ENCODE_LOSSLESS = 1  # SELA_HIP_ENCODE_LOSSLESS



# the test hooks include/sela_hip_debug.h declares (not part of the boundary)
DEBUG_EXPORTS = [
    "sela_hip_debug_phase_buffer", "sela_hip_debug_force_plain_fir", "sela_hip_debug_mean_workers", "sela_hip_debug_encode_teams", "sela_hip_debug_encode_kernel", "sela_hip_debug_encode_fused", "sela_hip_debug_priorities", "sela_hip_debug_priorities_adaptive", "sela_hip_debug_launches_alone", "sela_hip_debug_block_forms", "sela_hip_debug_encode_hashes", "sela_hip_debug_standard_first", "sela_hip_debug_standard_chunks", "sela_hip_debug_segment_subframes", "sela_hip_debug_generic_wrap_taps", "sela_hip_debug_encode_split", "sela_hip_debug_launches_split", "sela_hip_debug_keep_both_candidates", "sela_hip_debug_stage_wait",
    "sela_hip_debug_reissued_feeds", "sela_hip_debug_contexts_created", "sela_hip_debug_decode_recurrence", "sela_hip_debug_coalesced", "sela_hip_debug_verify_lds_bytes",
    "sela_hip_debug_verify_i32_fallback_frames", "sela_hip_debug_window_lds_bytes", "sela_hip_debug_windows_staged_bytes",
    "sela_hip_debug_workspace_pieces", "sela_hip_debug_pcm_chunk_frames", "sela_hip_debug_verify_pcm_fallback_frames",
    "sela_hip_debug_levels_lds_bytes", "sela_hip_debug_levels_i32_fallback_frames", "sela_hip_debug_digest_lds_bytes",
    "sela_hip_debug_digest_pcm_fallback_frames", "sela_hip_debug_envelope_lds_bytes", "sela_hip_debug_envelope_i32_fallback_frames",
]
# `call` of sela_hip_debug_workspace_pieces, in the order of the enum in include/sela_hip_debug.h
WORKSPACE_CALLS = ("encode", "decode", "index", "decode_i32", "decode_n", "verify", "verify_i32", "encode_i32", "encode_paired", "windows", "windows_whole",
                   "encode_whole", "encode_split", "decode_whole", "windows_i32", "windows_i32_whole", "encode_whole_pcm", "salvage")


class Trace(C.Structure):
    """sela_hip_trace"""
    _fields_ = [
        ("mean", C.c_double), ("ac", C.c_double * 101), ("k", C.c_double * 100), ("a", C.c_int64 * 101),
        ("q", C.c_int32 * 100), ("order", C.c_int32), ("coef_k", C.c_uint32), ("coef_words", C.c_uint32),
        ("res_k", C.c_uint32), ("res_words", C.c_uint32), ("flags", C.c_uint32),
    ]


class SelaHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libsela_hip: {ERRORS.get(code, code)}: {message}")
        self.code = code


_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  The SELA MI355X path has no CPU fallback.")
    # PyTorch ships its own libamdhip64 (same SONAME as /opt/rocm's).  Whichever is loaded first serves both
    # users; loaded second, torch would bring up a second HIP runtime in the process and this library's calls
    # would land in one that sees no device.  So: torch first, when there is a torch.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, u64p, sz = C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t
    L.sela_hip_init.argtypes = [C.c_int]
    L.sela_hip_init.restype = C.c_int
    L.sela_hip_shutdown.argtypes = []
    L.sela_hip_shutdown.restype = None
    L.sela_hip_thread_release.argtypes = []
    L.sela_hip_thread_release.restype = None
    L.sela_hip_last_error.argtypes = []
    L.sela_hip_last_error.restype = C.c_char_p
    L.sela_hip_device_count.argtypes = []
    L.sela_hip_device_count.restype = C.c_int
    L.sela_hip_signals_per_frame.argtypes = [u32]
    L.sela_hip_signals_per_frame.restype = u32
    for name in ("sela_hip_encode_workspace_bytes", "sela_hip_decode_workspace_bytes", "sela_hip_encode_bound_bytes"):
        getattr(L, name).argtypes = [u32, u32]
        getattr(L, name).restype = sz
    L.sela_hip_encode_device.argtypes = [vp, u32, u32, vp, sz, u64p, vp, vp, sz, vp, vp]
    L.sela_hip_encode_device.restype = C.c_int
    L.sela_hip_decode_device.argtypes = [vp, u64p, u32, u32, vp, vp, vp, sz, vp]
    L.sela_hip_decode_device.restype = C.c_int
    L.sela_hip_encode.argtypes = [vp, u32, u32, u32, vp, sz, vp]
    L.sela_hip_encode.restype = C.c_int
    L.sela_hip_decode.argtypes = [vp, vp, u32, u32, vp]
    L.sela_hip_decode.restype = C.c_int
    L.sela_hip_index_frames.argtypes = [vp, sz, u32, u32, vp]
    L.sela_hip_index_frames.restype = u32
    L.sela_hip_index_workspace_bytes.argtypes = [sz, u32]
    L.sela_hip_index_workspace_bytes.restype = sz
    L.sela_hip_index_frames_device.argtypes = [vp, sz, u32, u32, vp, vp, vp, sz, vp]
    L.sela_hip_index_frames_device.restype = C.c_int
    L.sela_hip_salvage_frames.argtypes = [vp, sz, u32, u32, vp, vp]
    L.sela_hip_salvage_frames.restype = u32
    L.sela_hip_salvage_workspace_bytes.argtypes = [sz, u32]
    L.sela_hip_salvage_workspace_bytes.restype = sz
    L.sela_hip_salvage_frames_device.argtypes = [vp, sz, u32, u32, vp, vp, vp, sz, vp]
    L.sela_hip_salvage_frames_device.restype = C.c_int
    L.sela_hip_salvage_payload_device.argtypes = [vp, sz, u32, u32, vp, sz, vp, vp, vp, vp, sz, vp]
    L.sela_hip_salvage_payload_device.restype = C.c_int
    L.sela_hip_salvage_frames_unaligned.argtypes = [vp, sz, u32, u32, vp, vp]
    L.sela_hip_salvage_frames_unaligned.restype = u32
    L.sela_hip_salvage_unaligned_workspace_bytes.argtypes = [sz, u32]
    L.sela_hip_salvage_unaligned_workspace_bytes.restype = sz
    L.sela_hip_salvage_frames_unaligned_device.argtypes = [vp, sz, u32, u32, vp, vp, vp, sz, vp]
    L.sela_hip_salvage_frames_unaligned_device.restype = C.c_int
    L.sela_hip_salvage_payload_unaligned_device.argtypes = [vp, sz, u32, u32, vp, sz, vp, vp, vp, vp, sz, vp]
    L.sela_hip_salvage_payload_unaligned_device.restype = C.c_int
    L.sela_hip_decode_payload_device.argtypes = [vp, sz, u32, u32, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_payload_device.restype = C.c_int
    L.sela_hip_decode_i32_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_decode_i32_workspace_bytes.restype = sz
    L.sela_hip_decode_i32_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_i32_device.restype = C.c_int
    L.sela_hip_decode_payload_i32_device.argtypes = [vp, sz, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_payload_i32_device.restype = C.c_int
    L.sela_hip_decode_status_error.argtypes = [vp]
    L.sela_hip_decode_status_error.restype = C.c_int
    L.sela_hip_decode_n_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_decode_n_workspace_bytes.restype = sz
    L.sela_hip_decode_n_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_n_device.restype = C.c_int
    L.sela_hip_decode_payload_n_device.argtypes = [vp, sz, u32, u32, u32, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_payload_n_device.restype = C.c_int
    L.sela_hip_decode_n_status_error.argtypes = [vp]
    L.sela_hip_decode_n_status_error.restype = C.c_int
    L.sela_hip_verify_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_verify_workspace_bytes.restype = sz
    L.sela_hip_verify_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_verify_device.restype = C.c_int
    L.sela_hip_verify_payload_device.argtypes = [vp, sz, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_verify_payload_device.restype = C.c_int
    L.sela_hip_verify.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    L.sela_hip_verify.restype = C.c_int
    L.sela_hip_verify_i32_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_verify_i32_workspace_bytes.restype = sz
    L.sela_hip_verify_i32_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_verify_i32_device.restype = C.c_int
    L.sela_hip_verify_payload_i32_device.argtypes = [vp, sz, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_verify_payload_i32_device.restype = C.c_int
    L.sela_hip_verify_i32.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp]
    L.sela_hip_verify_i32.restype = C.c_int
    L.sela_hip_decode_windows_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_decode_windows_workspace_bytes.restype = sz
    L.sela_hip_decode_windows_device.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_windows_device.restype = C.c_int
    L.sela_hip_decode_windows.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, vp, vp]
    L.sela_hip_decode_windows.restype = C.c_int
    L.sela_hip_decode_windows_whole_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_decode_windows_whole_workspace_bytes.restype = sz
    L.sela_hip_decode_windows_whole_device.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_windows_whole_device.restype = C.c_int
    L.sela_hip_decode_windows_whole.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, vp, vp]
    L.sela_hip_decode_windows_whole.restype = C.c_int
    L.sela_hip_decode_windows_i32_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_decode_windows_i32_workspace_bytes.restype = sz
    L.sela_hip_decode_windows_i32_device.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_windows_i32_device.restype = C.c_int
    L.sela_hip_decode_windows_i32.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, u32, vp, vp]
    L.sela_hip_decode_windows_i32.restype = C.c_int
    L.sela_hip_decode_windows_i32_whole_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_decode_windows_i32_whole_workspace_bytes.restype = sz
    L.sela_hip_decode_windows_i32_whole_device.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_windows_i32_whole_device.restype = C.c_int
    L.sela_hip_decode_windows_i32_whole.argtypes = [vp, vp, u32, u32, vp, u32, u32, u32, u32, vp, vp]
    L.sela_hip_decode_windows_i32_whole.restype = C.c_int
    L.sela_hip_encode_i32_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_encode_i32_workspace_bytes.restype = sz
    L.sela_hip_encode_i32_device.argtypes = [vp, u32, u32, u32, vp, sz, vp, vp, vp, sz, vp]
    L.sela_hip_encode_i32_device.restype = C.c_int
    L.sela_hip_encode_n_device.argtypes = [vp, u32, u32, u32, vp, sz, vp, vp, vp, sz, vp]
    L.sela_hip_encode_n_device.restype = C.c_int
    # the *_opt calls: their namesakes' arguments and a trailing options word (SELA_HIP_ENCODE_LOSSLESS)
    L.sela_hip_encode_device_opt.argtypes = L.sela_hip_encode_device.argtypes + [u32]
    L.sela_hip_encode_i32_device_opt.argtypes = L.sela_hip_encode_i32_device.argtypes + [u32]
    L.sela_hip_encode_n_device_opt.argtypes = L.sela_hip_encode_n_device.argtypes + [u32]
    L.sela_hip_encode_opt.argtypes = L.sela_hip_encode.argtypes + [u32]
    L.sela_hip_encode_i32_opt.argtypes = [vp, u32, u32, u32, vp, sz, vp, u32]
    L.sela_hip_encode_ragged_i32_opt.argtypes = [vp, vp, u32, vp, sz, vp, u32]
    L.sela_hip_encode_begin_opt.argtypes = [C.POINTER(C.c_void_p), u32, u32, vp, sz, vp, u32]
    for name in ("sela_hip_encode_device_opt", "sela_hip_encode_i32_device_opt", "sela_hip_encode_n_device_opt", "sela_hip_encode_opt", "sela_hip_encode_i32_opt",
                 "sela_hip_encode_ragged_i32_opt", "sela_hip_encode_begin_opt"):
        getattr(L, name).restype = C.c_int
    # the paired calls: the plain calls' arguments and their own options word
    L.sela_hip_paired_signals_per_frame.argtypes = [u32]
    L.sela_hip_paired_signals_per_frame.restype = u32
    L.sela_hip_encode_paired_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_encode_paired_workspace_bytes.restype = sz
    L.sela_hip_encode_paired_i32_device.argtypes = L.sela_hip_encode_i32_device.argtypes + [u32]
    L.sela_hip_encode_paired_n_device.argtypes = L.sela_hip_encode_n_device.argtypes + [u32]
    L.sela_hip_encode_paired_i32.argtypes = [vp, u32, u32, u32, vp, sz, vp, u32]
    L.sela_hip_encode_paired.argtypes = [vp, u32, u32, u32, vp, sz, vp, u32]
    for name in ("sela_hip_encode_paired_i32_device", "sela_hip_encode_paired_n_device", "sela_hip_encode_paired_i32", "sela_hip_encode_paired"):
        getattr(L, name).restype = C.c_int
    # a whole track with its tail: the sample count is a uint64
    u64 = C.c_uint64
    L.sela_hip_whole_frames.argtypes = [u64]
    L.sela_hip_whole_frames.restype = u64
    L.sela_hip_whole_frame.argtypes = [u64, u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.sela_hip_whole_frame.restype = C.c_int
    for name in ("sela_hip_encode_whole_bound_bytes", "sela_hip_encode_whole_workspace_bytes"):
        getattr(L, name).argtypes = [u64, u32]
        getattr(L, name).restype = sz
    L.sela_hip_encode_whole_device.argtypes = [vp, u64, u32, vp, sz, vp, vp, vp, sz, vp, u32]
    L.sela_hip_encode_whole_device.restype = C.c_int
    L.sela_hip_encode_whole.argtypes = [vp, u64, u32, vp, sz, vp, u32]
    L.sela_hip_encode_whole.restype = C.c_int
    L.sela_hip_encode_whole_pcm_bound_bytes.argtypes = [u64, u32, u32]
    L.sela_hip_encode_whole_pcm_bound_bytes.restype = sz
    L.sela_hip_encode_whole_pcm_workspace_bytes.argtypes = [u64, u32]
    L.sela_hip_encode_whole_pcm_workspace_bytes.restype = sz
    L.sela_hip_encode_whole_pcm_device.argtypes = [vp, u32, u64, u32, u32, vp, sz, vp, vp, vp, sz, vp]
    L.sela_hip_encode_whole_pcm_device.restype = C.c_int
    L.sela_hip_encode_whole_pcm.argtypes = [vp, u32, u64, u32, u32, vp, sz, vp]
    L.sela_hip_encode_whole_pcm.restype = C.c_int
    L.sela_hip_decode_whole_workspace_bytes.argtypes = [u32, u32]
    L.sela_hip_decode_whole_workspace_bytes.restype = sz
    L.sela_hip_decode_whole_device.argtypes = [vp, vp, u32, u32, vp, u64, vp, vp, vp, sz, vp]
    L.sela_hip_decode_whole_device.restype = C.c_int
    L.sela_hip_decode_whole_payload_device.argtypes = [vp, sz, u32, u32, vp, u64, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_whole_payload_device.restype = C.c_int
    L.sela_hip_decode_whole_status_error.argtypes = [vp]
    L.sela_hip_decode_whole_status_error.restype = C.c_int
    L.sela_hip_decode_whole.argtypes = [vp, vp, u32, u32, vp, u64, vp]
    L.sela_hip_decode_whole.restype = C.c_int
    # packed 3- / 4-byte PCM
    L.sela_hip_encode_pcm_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_encode_pcm_bound_bytes.argtypes = [u32, u32, u32, u32]
    L.sela_hip_decode_pcm_workspace_bytes.argtypes = [u32, u32, u32]
    for name in ("sela_hip_encode_pcm_workspace_bytes", "sela_hip_encode_pcm_bound_bytes", "sela_hip_decode_pcm_workspace_bytes"):
        getattr(L, name).restype = sz
    L.sela_hip_pcm_unpack_device.argtypes = [vp, u32, u32, u32, u32, vp, vp]
    L.sela_hip_pcm_pack_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.sela_hip_encode_pcm_device.argtypes = [vp, u32, u32, u32, u32, u32, vp, sz, vp, vp, vp, sz, vp]
    L.sela_hip_decode_pcm_device.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_decode_pcm_status_error.argtypes = [vp]
    L.sela_hip_encode_pcm.argtypes = [vp, u32, u32, u32, u32, u32, vp, sz, vp]
    L.sela_hip_decode_pcm.argtypes = [vp, vp, u32, u32, u32, vp, sz, vp]
    for name in ("sela_hip_pcm_unpack_device", "sela_hip_pcm_pack_device", "sela_hip_encode_pcm_device", "sela_hip_decode_pcm_device",
                 "sela_hip_decode_pcm_status_error", "sela_hip_encode_pcm", "sela_hip_decode_pcm"):
        getattr(L, name).restype = C.c_int
    # verification against packed PCM
    L.sela_hip_verify_pcm_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_verify_pcm_workspace_bytes.restype = sz
    L.sela_hip_verify_pcm_device.argtypes = [vp, vp, u32, u32, u32, vp, u32, u64, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_verify_payload_pcm_device.argtypes = [vp, sz, u32, u32, u32, vp, u32, u64, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_verify_pcm.argtypes = [vp, vp, u32, u32, u32, vp, u64, vp, vp, vp]
    for name in ("sela_hip_verify_pcm_device", "sela_hip_verify_payload_pcm_device", "sela_hip_verify_pcm"):
        getattr(L, name).restype = C.c_int
    # level scan
    L.sela_hip_levels_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_levels_workspace_bytes.restype = sz
    L.sela_hip_levels_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_levels_payload_device.argtypes = [vp, sz, u32, u32, u32, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_levels.argtypes = [vp, vp, u32, u32, vp]
    for name in ("sela_hip_levels_device", "sela_hip_levels_payload_device", "sela_hip_levels"):
        getattr(L, name).restype = C.c_int
    L.sela_hip_levels_i32_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_levels_i32_workspace_bytes.restype = sz
    L.sela_hip_levels_samples_i32_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_levels_samples_i32_workspace_bytes.restype = sz
    L.sela_hip_levels_i32_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_levels_payload_i32_device.argtypes = [vp, sz, u32, u32, u32, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_levels_samples_i32_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, sz, vp]
    L.sela_hip_levels_i32.argtypes = [vp, vp, u32, u32, vp]
    for name in ("sela_hip_levels_i32_device", "sela_hip_levels_payload_i32_device", "sela_hip_levels_samples_i32_device", "sela_hip_levels_i32"):
        getattr(L, name).restype = C.c_int
    L.sela_hip_debug_levels_i32_fallback_frames.argtypes = [vp, u32, u32, u32]
    L.sela_hip_debug_levels_i32_fallback_frames.restype = C.c_longlong
    L.sela_hip_debug_levels_lds_bytes.argtypes = [u32]
    L.sela_hip_debug_levels_lds_bytes.restype = sz
    # envelope
    L.sela_hip_envelope_slots.argtypes = [u32, u32]
    L.sela_hip_envelope_slots.restype = u32
    L.sela_hip_envelope_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_envelope_workspace_bytes.restype = sz
    L.sela_hip_envelope_device.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_envelope_payload_device.argtypes = [vp, sz, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_envelope.argtypes = [vp, vp, u32, u32, u32, u32, vp]
    for name in ("sela_hip_envelope_device", "sela_hip_envelope_payload_device", "sela_hip_envelope"):
        getattr(L, name).restype = C.c_int
    L.sela_hip_debug_envelope_lds_bytes.argtypes = [u32]
    L.sela_hip_debug_envelope_lds_bytes.restype = sz
    # envelope of 24- and 32-bit streams
    L.sela_hip_envelope_i32_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_envelope_i32_workspace_bytes.restype = sz
    L.sela_hip_envelope_samples_i32_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_envelope_samples_i32_workspace_bytes.restype = sz
    L.sela_hip_envelope_i32_device.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    L.sela_hip_envelope_payload_i32_device.argtypes = [vp, sz, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_envelope_samples_i32_device.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, sz, vp]
    L.sela_hip_envelope_i32.argtypes = [vp, vp, u32, u32, u32, u32, vp]
    for name in ("sela_hip_envelope_i32_device", "sela_hip_envelope_payload_i32_device", "sela_hip_envelope_samples_i32_device", "sela_hip_envelope_i32"):
        getattr(L, name).restype = C.c_int
    L.sela_hip_debug_envelope_i32_fallback_frames.argtypes = [vp, u32, u32, u32]
    L.sela_hip_debug_envelope_i32_fallback_frames.restype = C.c_longlong
    # digest
    L.sela_hip_digest_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_digest_workspace_bytes.restype = sz
    L.sela_hip_digest_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_digest_payload_device.argtypes = [vp, sz, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_digest.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.sela_hip_crc32_device.argtypes = [vp, C.c_uint64, vp, vp, sz, vp]
    for name in ("sela_hip_digest_device", "sela_hip_digest_payload_device", "sela_hip_digest", "sela_hip_crc32_device"):
        getattr(L, name).restype = C.c_int
    L.sela_hip_crc32_combine.argtypes = [u32, u32, C.c_uint64]
    L.sela_hip_crc32_combine.restype = u32
    L.sela_hip_crc32_workspace_bytes.argtypes = [C.c_uint64]
    L.sela_hip_crc32_workspace_bytes.restype = sz
    L.sela_hip_debug_digest_lds_bytes.argtypes = [u32]
    L.sela_hip_debug_digest_lds_bytes.restype = sz
    # digest of 24- and 32-bit streams: the digest calls' arguments with bytes_per_sample behind the stride / the channels
    L.sela_hip_digest_pcm_workspace_bytes.argtypes = [u32, u32, u32]
    L.sela_hip_digest_pcm_workspace_bytes.restype = sz
    L.sela_hip_digest_pcm_device.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_digest_payload_pcm_device.argtypes = [vp, sz, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sela_hip_digest_pcm.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp]
    for name in ("sela_hip_digest_pcm_device", "sela_hip_digest_payload_pcm_device", "sela_hip_digest_pcm"):
        getattr(L, name).restype = C.c_int
    L.sela_hip_debug_digest_pcm_fallback_frames.argtypes = [vp, u32, u32, u32]
    L.sela_hip_debug_digest_pcm_fallback_frames.restype = C.c_longlong
    L.sela_hip_debug_pcm_chunk_frames.argtypes = [u32]
    L.sela_hip_debug_pcm_chunk_frames.restype = None
    L.sela_hip_encode_status_error.argtypes = [vp]
    L.sela_hip_encode_status_error.restype = C.c_int
    L.sela_hip_enable_kernel_timing.argtypes = [C.c_int]
    L.sela_hip_enable_kernel_timing.restype = None
    L.sela_hip_kernel_times.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.sela_hip_kernel_times.restype = C.c_int
    L.sela_hip_lpc_encode.argtypes = [vp, u32, vp, vp, vp]
    L.sela_hip_lpc_decode.argtypes = [vp, vp, vp, u32, vp, vp]
    L.sela_hip_rice_encode.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.sela_hip_rice_decode.argtypes = [vp, vp, vp, vp, u32, vp]
    for name in ("sela_hip_lpc_encode", "sela_hip_lpc_decode", "sela_hip_rice_encode", "sela_hip_rice_decode"):
        getattr(L, name).restype = C.c_int
    L.sela_hip_encode_bound_bytes_n.argtypes = [u32, u32, u32]
    L.sela_hip_encode_bound_bytes_n.restype = sz
    L.sela_hip_index_samples.argtypes = [vp, vp, u32, u32, vp]
    L.sela_hip_index_samples.restype = u32
    L.sela_hip_encode_i32.argtypes = [vp, u32, u32, u32, vp, sz, vp]
    L.sela_hip_decode_i32.argtypes = [vp, vp, u32, u32, vp, u32, vp]
    L.sela_hip_encode_ragged_i32.argtypes = [vp, vp, u32, vp, sz, vp]
    L.sela_hip_lpc_encode_n.argtypes = [vp, u32, u32, vp, vp, vp]
    L.sela_hip_lpc_decode_n.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    for name in ("sela_hip_encode_i32", "sela_hip_decode_i32", "sela_hip_encode_ragged_i32", "sela_hip_lpc_encode_n", "sela_hip_lpc_decode_n"):
        getattr(L, name).restype = C.c_int
    L.sela_hip_debug_phase_buffer.argtypes = [C.c_void_p]
    L.sela_hip_debug_phase_buffer.restype = None
    L.sela_hip_debug_force_plain_fir.argtypes = [C.c_int]
    L.sela_hip_debug_force_plain_fir.restype = None
    L.sela_hip_debug_mean_workers.argtypes = [C.c_int]
    L.sela_hip_debug_mean_workers.restype = None
    L.sela_hip_debug_encode_teams.argtypes = [C.c_int]
    L.sela_hip_debug_encode_teams.restype = None
    L.sela_hip_debug_encode_fused.argtypes = [C.c_int]
    L.sela_hip_debug_encode_fused.restype = None
    L.sela_hip_debug_priorities.argtypes = [C.c_uint32]
    L.sela_hip_debug_priorities.restype = None
    L.sela_hip_debug_priorities_adaptive.argtypes = []
    L.sela_hip_debug_priorities_adaptive.restype = None
    L.sela_hip_debug_launches_alone.argtypes = []
    L.sela_hip_debug_launches_alone.restype = C.c_int
    L.sela_hip_debug_encode_hashes.argtypes = [C.c_int]
    L.sela_hip_debug_encode_hashes.restype = None
    L.sela_hip_debug_standard_first.argtypes = [C.c_int]
    L.sela_hip_debug_standard_first.restype = None
    L.sela_hip_debug_standard_chunks.argtypes = []
    L.sela_hip_debug_standard_chunks.restype = C.c_int
    L.sela_hip_debug_segment_subframes.argtypes = []
    L.sela_hip_debug_segment_subframes.restype = C.c_longlong
    L.sela_hip_debug_generic_wrap_taps.argtypes = [C.c_int]
    L.sela_hip_debug_generic_wrap_taps.restype = None
    L.sela_hip_debug_encode_split.argtypes = [C.c_int]
    L.sela_hip_debug_encode_split.restype = None
    L.sela_hip_debug_launches_split.argtypes = []
    L.sela_hip_debug_launches_split.restype = C.c_int
    L.sela_hip_debug_block_forms.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.sela_hip_debug_block_forms.restype = C.c_int
    L.sela_hip_debug_keep_both_candidates.argtypes = [C.c_int]
    L.sela_hip_debug_keep_both_candidates.restype = None
    L.sela_hip_debug_encode_kernel.argtypes = [C.c_uint32, C.c_uint32]
    L.sela_hip_debug_encode_kernel.restype = C.c_int
    L.sela_hip_debug_stage_wait.argtypes = [C.c_int]
    L.sela_hip_debug_stage_wait.restype = None
    L.sela_hip_debug_reissued_feeds.argtypes = []
    L.sela_hip_debug_reissued_feeds.restype = C.c_int
    L.sela_hip_debug_decode_recurrence.argtypes = [C.c_int]
    L.sela_hip_debug_decode_recurrence.restype = None
    L.sela_hip_debug_contexts_created.argtypes = []
    L.sela_hip_debug_contexts_created.restype = C.c_int
    L.sela_hip_debug_coalesced.argtypes = [C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.sela_hip_debug_coalesced.restype = None
    L.sela_hip_debug_verify_lds_bytes.argtypes = [u32]
    L.sela_hip_debug_verify_lds_bytes.restype = sz
    L.sela_hip_debug_verify_i32_fallback_frames.argtypes = [vp, u32, u32, u32]
    L.sela_hip_debug_verify_pcm_fallback_frames.argtypes = [vp, u32, u32, u32]
    L.sela_hip_debug_verify_pcm_fallback_frames.restype = C.c_longlong
    L.sela_hip_debug_verify_i32_fallback_frames.restype = C.c_longlong
    L.sela_hip_debug_window_lds_bytes.argtypes = [u32]
    L.sela_hip_debug_window_lds_bytes.restype = sz
    L.sela_hip_debug_windows_staged_bytes.argtypes = []
    L.sela_hip_debug_windows_staged_bytes.restype = C.c_uint64
    L.sela_hip_debug_workspace_pieces.argtypes = [C.c_int, u64, u32, u32, u64p, C.c_int]
    L.sela_hip_debug_workspace_pieces.restype = C.c_int
    L.sela_hip_host_alloc.argtypes = [sz]
    L.sela_hip_host_alloc.restype = C.c_void_p
    L.sela_hip_host_free.argtypes = [C.c_void_p]
    L.sela_hip_host_free.restype = None
    L.sela_hip_decode_max_channels.argtypes = []
    L.sela_hip_decode_max_channels.restype = u32
    L.sela_hip_encode_begin.argtypes = [C.POINTER(C.c_void_p), u32, u32, vp, sz, vp]
    L.sela_hip_encode_feed.argtypes = [vp, vp, u32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.sela_hip_encode_end.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.sela_hip_decode_begin.argtypes = [C.POINTER(C.c_void_p), u32, u32, vp]
    L.sela_hip_decode_feed.argtypes = [vp, vp, vp, u32, C.POINTER(C.c_uint32)]
    L.sela_hip_decode_end.argtypes = [vp, C.POINTER(C.c_uint32)]
    for name in ("sela_hip_encode_begin", "sela_hip_encode_feed", "sela_hip_encode_end", "sela_hip_decode_begin",
                 "sela_hip_decode_feed", "sela_hip_decode_end"):
        getattr(L, name).restype = C.c_int
    _LIB = L
    return L


def kernel_times(capacity: int = 4):
    """Durations (ms) of the kernels of the calling thread's last *_device call (timing must be enabled)."""
    buf = (C.c_float * capacity)()
    n = lib().sela_hip_kernel_times(buf, capacity)
    return [float(buf[i]) for i in range(n)]


def workspace_pieces(call: str, a: int, b: int = 0, c: int = 0):
    """The (offset, bytes) of every piece the named call (WORKSPACE_CALLS) cuts its workspace into, or None where its sizing
    function refuses the shape.  No device (sela_hip_debug_workspace_pieces)."""
    which = WORKSPACE_CALLS.index(call)
    n = lib().sela_hip_debug_workspace_pieces(which, a, b, c, None, 0)
    if n < 0:
        return None
    buf = (C.c_uint64 * (2 * n))()
    assert lib().sela_hip_debug_workspace_pieces(which, a, b, c, C.addressof(buf), n) == n
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n)]


def check(rc: int) -> None:
    if rc != OK:
        raise SelaHipError(rc, lib().sela_hip_last_error().decode("utf-8", "replace"))
