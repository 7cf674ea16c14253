"""Torch/numpy wrappers over the C ABI.  PyTorch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi

BLOCK = capi.SAMPLES_PER_FRAME


@dataclass
class EncodedFrames:
    """Device-resident result of an encode: the .sela frame byte stream + per-frame offsets."""
    frames: "torch.Tensor"       # uint8 [capacity]; the first offsets[-1] bytes are valid
    offsets: "torch.Tensor"      # int64 [n_frames + 1] (bit pattern of the library's uint64)
    status: "torch.Tensor"       # int32 [4]
    n_frames: int
    channels: int

    def total_bytes(self) -> int:
        return int(self.offsets[-1].item())

    def check(self) -> None:
        st = self.status.cpu().numpy().view(np.uint32)
        bad = int(st[0]) & (capi.FLAG_WORDS_CAP | capi.FLAG_RICE_RANGE | capi.FLAG_COEF_OVERFLOW)
        if bad:
            raise capi.SelaHipError(-6, f"a block left the range the .sela format can carry (flags 0x{int(st[0]):x})")
        if int(st[1]):
            raise capi.SelaHipError(-4, "frame buffer too small")

    def to_host(self):
        self.check()
        n = self.total_bytes()
        return self.frames[:n].cpu().numpy(), self.offsets.cpu().numpy().view(np.uint64)


class Encoder:
    """Reusable device buffers for encoding batches of up to `max_frames` frames on the current device.
    lossless: SELA_HIP_ENCODE_LOSSLESS -- residues against the decoder's rounding, so that every frame decodes back exactly
    (not together with with_trace: the trace is the reference's arithmetic)."""

    def __init__(self, max_frames: int, channels: int, device=None, with_trace: bool = False, lossless: bool = False):
        import torch

        if lossless and with_trace:
            raise ValueError("lossless and with_trace exclude each other")
        self.options = capi.ENCODE_LOSSLESS if lossless else 0

        self.torch = torch
        self.lib = capi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_frames, self.channels = max_frames, channels
        self.n_sig = int(self.lib.sela_hip_signals_per_frame(channels))
        ws = int(self.lib.sela_hip_encode_workspace_bytes(max_frames, channels))
        # the algorithmic output never exceeds the input for audio; keep the certain bound small by
        # default (2x PCM) and let callers who want certainty pass frames_capacity explicitly
        self.capacity = max(2 * max_frames * BLOCK * channels * 2, 4096)
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
            self.frames = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
            self.offsets = torch.empty(max_frames + 1, dtype=torch.int64, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
            self.trace = (torch.zeros(max_frames * self.n_sig * C.sizeof(capi.Trace), dtype=torch.uint8, device=self.device)
                          if with_trace else None)

    def encode(self, pcm, status=None) -> EncodedFrames:
        """pcm: int16 cuda tensor [n_frames, 2048, channels] (contiguous).  Asynchronous on the current stream.
        status: where this call leaves its four status words (int32 cuda tensor [4]); default: the encoder's own."""
        torch = self.torch
        status = self.status if status is None else status
        assert status.dtype == torch.int32 and status.numel() == 4 and status.is_cuda and status.is_contiguous()
        assert pcm.dtype == torch.int16 and pcm.is_cuda and pcm.is_contiguous()
        n_frames = pcm.shape[0]
        assert pcm.shape[1] == BLOCK and pcm.shape[2] == self.channels and n_frames <= self.max_frames
        stream = torch.cuda.current_stream(self.device).cuda_stream
        args = (pcm.data_ptr(), n_frames, self.channels, self.frames.data_ptr(), self.capacity, self.offsets.data_ptr(),
                status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
                self.trace.data_ptr() if self.trace is not None else None, stream)
        if self.options:
            capi.check(self.lib.sela_hip_encode_device_opt(*args, self.options))
        else:
            capi.check(self.lib.sela_hip_encode_device(*args))
        return EncodedFrames(self.frames, self.offsets[: n_frames + 1], status, n_frames, self.channels)

    def traces(self, n_frames: int):
        raw = self.trace[: n_frames * self.n_sig * C.sizeof(capi.Trace)].cpu().numpy().tobytes()
        return (capi.Trace * (n_frames * self.n_sig)).from_buffer_copy(raw)


class Decoder:
    def __init__(self, max_frames: int, channels: int, device=None):
        import torch

        self.torch = torch
        self.lib = capi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_frames, self.channels = max_frames, channels
        with torch.cuda.device(self.device):
            self.pcm = torch.empty((max_frames, BLOCK, channels), dtype=torch.int16, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
            ws = int(self.lib.sela_hip_decode_workspace_bytes(max_frames, channels))
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)

    def decode(self, frames, offsets, n_frames: int, status=None):
        """frames: uint8 cuda tensor, offsets: int64 cuda tensor [n_frames+1].  Asynchronous.
        status: where this call leaves its status words (int32 cuda tensor [4]); default: the decoder's own."""
        torch = self.torch
        status = self.status if status is None else status
        assert status.dtype == torch.int32 and status.numel() == 4 and status.is_cuda and status.is_contiguous()
        assert frames.is_cuda and offsets.is_cuda and offsets.dtype == torch.int64 and n_frames <= self.max_frames
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.sela_hip_decode_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.pcm.data_ptr(), status.data_ptr(),
            self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.pcm[:n_frames]

    def decode_payload(self, payload, max_frames=None, status=None):
        """Index and decode a .sela payload (the bytes after the file header: uint8 cuda tensor, 4-byte aligned) in one
        asynchronous call: the frame count never leaves the device, so the call can be captured into a graph.
        -> (pcm int16 [max_frames, 2048, channels], offsets int64 [max_frames + 1], count int32 [1]); frames from count[0] on
        are not decoded.  All three are the decoder's own buffers, overwritten by the next call; so is its workspace, which
        grows to the largest payload seen (make one call before capturing)."""
        torch = self.torch
        max_frames = self.max_frames if max_frames is None else max_frames
        status = self.status if status is None else status
        assert status.dtype == torch.int32 and status.numel() == 4 and status.is_cuda and status.is_contiguous()
        assert payload.dtype == torch.uint8 and payload.is_cuda and payload.is_contiguous() and max_frames <= self.max_frames
        need = int(self.lib.sela_hip_index_workspace_bytes(payload.numel(), max_frames)) + int(
            self.lib.sela_hip_decode_workspace_bytes(max_frames, self.channels))
        with torch.cuda.device(self.device):
            if getattr(self, "payload_workspace", None) is None or self.payload_workspace.numel() < need:
                self.payload_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            if getattr(self, "payload_offsets", None) is None:
                self.payload_offsets = torch.empty(self.max_frames + 1, dtype=torch.int64, device=self.device)
                self.payload_count = torch.zeros(1, dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.sela_hip_decode_payload_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.pcm.data_ptr(), self.payload_offsets.data_ptr(),
            self.payload_count.data_ptr(), status.data_ptr(), self.payload_workspace.data_ptr(), self.payload_workspace.numel(), stream))
        return self.pcm[:max_frames], self.payload_offsets[: max_frames + 1], self.payload_count

    def check(self) -> None:
        st = self.status.cpu().numpy().view(np.uint32)
        if int(st[0]) & capi.FLAG_BAD_FRAME:
            raise capi.SelaHipError(-5, f"malformed frame stream ({int(st[1])} bad frames)")
        if int(st[0]) & capi.FLAG_RICE_OVERRUN:
            raise capi.SelaHipError(-5, "a Rice stream ended before all its values were read")


def decode_status_error(status) -> int:
    """sela_hip_decode_status_error on a host copy of four status words (any integer array of 4) -> the host call's code."""
    st = np.ascontiguousarray(np.asarray(status).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    assert st.shape == (4,)
    return int(capi.lib().sela_hip_decode_status_error(st.ctypes.data))


def decode_n_status_error(status) -> int:
    """sela_hip_decode_n_status_error on a host copy of four status words (any integer array of 4) -> the host call's code."""
    st = np.ascontiguousarray(np.asarray(status).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    assert st.shape == (4,)
    return int(capi.lib().sela_hip_decode_n_status_error(st.ctypes.data))


class _DeviceCall:
    """What the classes over sela_hip_<_call>_device and its payload form share: the device, the offsets, the frame count and the
    status words, the workspace of sela_hip_<_call>_workspace_bytes, the payload form's grow-only workspace, the argument asserts
    and check().  A class names its call and its status judge, allocates its outputs in _allocate(), and lists the status
    accessors it has (route = _DeviceCall._route, ...)."""

    _call = None          # "verify_i32": sela_hip_verify_i32_workspace_bytes, sela_hip_debug_verify_i32_fallback_frames
    _judge = None         # decode_status_error or decode_n_status_error
    _own_count = True     # status[2] holds the call's own count of frames (lossy, loud), not the largest frame: zeroed for the judge

    def __init__(self, max_frames: int, channels: int, stride: int, device=None):
        import torch

        self.torch = torch
        self.lib = capi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_frames, self.channels, self.stride = max_frames, channels, stride
        self.payload_workspace = None
        with torch.cuda.device(self.device):
            self._allocate(torch)
            self.sample_offsets = torch.zeros(max_frames + 1, dtype=torch.int64, device=self.device)
            self.frame_offsets = torch.zeros(max_frames + 1, dtype=torch.int64, device=self.device)
            self.count = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
            self.workspace = torch.empty(self._workspace_bytes(max_frames), dtype=torch.uint8, device=self.device)

    def _workspace_bytes(self, max_frames: int) -> int:
        return int(getattr(self.lib, f"sela_hip_{self._call}_workspace_bytes")(max_frames, self.channels, self.stride))

    def _allocate_diffs(self, torch) -> None:
        self.diff_counts = torch.zeros(self.max_frames, dtype=torch.int32, device=self.device)
        self.first_diff = torch.zeros(self.max_frames, dtype=torch.int32, device=self.device)

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _frames_ok(self, frames, offsets, n_frames: int) -> None:
        torch = self.torch
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()
        assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous() and n_frames <= self.max_frames

    def _payload_ok(self, payload, max_frames) -> int:
        """The payload form's opening: max_frames (None: the class's own), the payload's asserts, and payload_workspace grown to
        what the index and the call need for it."""
        torch = self.torch
        max_frames = self.max_frames if max_frames is None else max_frames
        assert payload.dtype == torch.uint8 and payload.is_cuda and payload.is_contiguous() and max_frames <= self.max_frames
        need = int(self.lib.sela_hip_index_workspace_bytes(payload.numel(), max_frames)) + self._workspace_bytes(max_frames)
        with torch.cuda.device(self.device):
            if self.payload_workspace is None or self.payload_workspace.numel() < need:
                self.payload_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return max_frames

    def _route(self) -> int:
        """Waits for the last call -> the route it took: 0 nothing decoded, 1 the 2048-sample decoder, 2 the any-length kernels."""
        return int(self.status[3].item())

    def _lossy_frames(self) -> int:
        """Waits for the last call -> the number of frames with a difference (status[2])."""
        return int(self.status[2].item())

    def _loud_frames(self) -> int:
        """Waits for the last call -> the number of frames in which some channel is not digital silence (status[2])."""
        return int(self.status[2].item())

    def _fallback_frames(self, n_frames=None) -> int:
        """Waits for the last call on frames and offsets (not the payload form) -> the frames whose layout was not direct
        (sela_hip_debug_<call>_fallback_frames, a test hook)."""
        return int(getattr(self.lib, f"sela_hip_debug_{self._call}_fallback_frames")(
            self.workspace.data_ptr(), self.max_frames if n_frames is None else n_frames, self.channels, self.stride))

    def check(self) -> None:
        """Waits for the last call and raises SelaHipError with the code the host call of the class's judge (sela_hip_decode for
        decode_n_status_error, sela_hip_decode_i32 for decode_status_error) gives for the same stream."""
        st = self.status.cpu().numpy().copy()
        if self._own_count:
            st[2] = 0
        capi.check(type(self)._judge(st))


class Decoder32(_DeviceCall):
    """sela_hip_decode_i32 on the device: streams of any samplesPerChannel (0 .. 65535), 32-bit samples, channels of
    different lengths -- what frame::FrameDecoder returns, nothing narrowed.  Owns its outputs and its workspace on the current
    device (or `device`); every call is asynchronous on the current stream and overwrites them."""

    _call, _judge, _own_count = "decode_i32", staticmethod(decode_status_error), False

    def _allocate(self, torch) -> None:
        self.samples = torch.empty((self.max_frames, self.channels, self.stride), dtype=torch.int32, device=self.device)
        self.counts = torch.zeros((self.max_frames, self.channels), dtype=torch.int32, device=self.device)

    def decode(self, frames, offsets, n_frames: int):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1]
        -> (samples int32 [n, channels, stride], counts int32 [n, channels], sample_offsets int64 [n + 1]), views of the
        decoder's own buffers (counts and offsets hold the library's uint32 / uint64 bit patterns)."""
        self._frames_ok(frames, offsets, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_decode_i32_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.samples.data_ptr(), self.counts.data_ptr(),
            self.sample_offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.samples[:n_frames], self.counts[:n_frames], self.sample_offsets[: n_frames + 1]

    def decode_payload(self, payload, max_frames=None):
        """Index and decode a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device, so the call can be captured into a graph.  -> (samples [max_frames, channels, stride],
        counts [max_frames, channels], sample_offsets [max_frames + 1], frame_offsets int64 [max_frames + 1], count int32 [1]):
        entries up to count[0] (samples and counts: below it) are the stream's, the rest are not written.  The workspace grows
        to the largest payload seen (make one call before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_decode_payload_i32_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, self.samples.data_ptr(), self.counts.data_ptr(),
            self.sample_offsets.data_ptr(), self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(),
            self.payload_workspace.data_ptr(), self.payload_workspace.numel(), stream))
        return (self.samples[:max_frames], self.counts[:max_frames], self.sample_offsets[: max_frames + 1],
                self.frame_offsets[: max_frames + 1], self.count)


class DecoderN(_DeviceCall):
    """sela_hip_decode on the device: int16 interleaved PCM of streams of any samplesPerChannel (0 .. 65535), samples wider
    than 16 bits narrowed as the host call narrows them, the route (2048-sample decoder or any-length kernels) chosen on the
    device.  Owns its outputs and its workspace on the current device (or `device`); every call is asynchronous on the current
    stream and overwrites them."""

    _call, _judge, _own_count = "decode_n", staticmethod(decode_n_status_error), False

    def _allocate(self, torch) -> None:
        self.pcm = torch.empty((self.max_frames * self.stride, self.channels), dtype=torch.int16, device=self.device)

    route = _DeviceCall._route

    def decode(self, frames, offsets, n_frames: int):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1]
        -> (pcm int16 [max_frames * stride, channels], sample_offsets int64 [n + 1]), views of the decoder's own buffers: frame f
        at pcm[sample_offsets[f]], sample_offsets[n] samples in all (the library's uint64 bit patterns)."""
        self._frames_ok(frames, offsets, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_decode_n_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.pcm.data_ptr(), self.sample_offsets.data_ptr(),
            self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.pcm, self.sample_offsets[: n_frames + 1]

    def decode_payload(self, payload, max_frames=None):
        """Index and decode a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device, so the call can be captured into a graph.  -> (pcm int16 [max_frames * stride, channels],
        sample_offsets [max_frames + 1], frame_offsets int64 [max_frames + 1], count int32 [1]): offsets up to count[0] are the
        stream's, pcm up to sample_offsets[count[0]].  The workspace grows to the largest payload seen (make one call before
        capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_decode_payload_n_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, self.pcm.data_ptr(), self.sample_offsets.data_ptr(),
            self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(), self.payload_workspace.data_ptr(),
            self.payload_workspace.numel(), stream))
        return self.pcm[: max_frames * self.stride], self.sample_offsets[: max_frames + 1], self.frame_offsets[: max_frames + 1], self.count


class Verifier(_DeviceCall):
    """sela_hip_verify_device: a stream held against the PCM it was made from, frame by frame, on the device -- which frames the
    decoder returns differently (the reference's rounding ties), how many values, and the first of them.  Owns its
    outputs and its workspace on the current device (or `device`); every call is asynchronous on the current stream and
    overwrites them.  No PCM is written: on the 2048-sample route of up to eight channels not even into the workspace."""

    _call, _judge = "verify", staticmethod(decode_n_status_error)
    _allocate = _DeviceCall._allocate_diffs
    lossy_frames = _DeviceCall._lossy_frames
    route = _DeviceCall._route

    def _pcm_ok(self, pcm) -> bool:
        return pcm.dtype == self.torch.int16 and pcm.is_cuda and pcm.is_contiguous()

    def verify(self, frames, offsets, n_frames: int, pcm):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1], pcm: int16 cuda tensor in the
        layout DecoderN.decode returns (frame f at sample_offsets[f]; [n_frames, 2048, channels] for a 2048 stream)
        -> (diff_counts int32 [n_frames], first_diff int32 [n_frames]; -1: nothing differs), views of the verifier's own buffers."""
        self._frames_ok(frames, offsets, n_frames)
        assert self._pcm_ok(pcm)
        stream = self._stream()
        capi.check(self.lib.sela_hip_verify_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, pcm.data_ptr(), self.diff_counts.data_ptr(),
            self.first_diff.data_ptr(), self.sample_offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
            stream))
        return self.diff_counts[:n_frames], self.first_diff[:n_frames]

    def verify_payload(self, payload, pcm, max_frames=None):
        """Index and verify a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device, so the call can be captured into a graph.  -> (diff_counts [max_frames], first_diff [max_frames],
        count int32 [1]): entries up to count[0] are the stream's.  The workspace grows to the largest payload seen (make one call
        before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        assert self._pcm_ok(pcm)
        stream = self._stream()
        capi.check(self.lib.sela_hip_verify_payload_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, pcm.data_ptr(), self.diff_counts.data_ptr(),
            self.first_diff.data_ptr(), self.sample_offsets.data_ptr(), self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(),
            self.payload_workspace.data_ptr(), self.payload_workspace.numel(), stream))
        return self.diff_counts[:max_frames], self.first_diff[:max_frames], self.count


# sela_hip_level (include/sela_hip.h): 24 bytes per (frame, channel)
LEVEL_DTYPE = np.dtype([("peak", "<u4"), ("samples", "<u4"), ("sum", "<i8"), ("sum_squares", "<u8")])
TRACK_LEVEL_DTYPE = np.dtype([("peak", "<u4"), ("samples", "<u8"), ("sum", "<i8"), ("sum_squares", "<u8")])


class Leveler(_DeviceCall):
    """sela_hip_levels_device: how loud a stream is, frame by frame and channel by channel, on the device -- the peak |v|, the sum
    and the sum of squares of the int16 samples DecoderN.decode would write.  All integers, so exact.  Owns its
    records and its workspace on the current device (or `device`); every call is asynchronous on the current stream and overwrites
    them.  No PCM is written: on the 2048-sample route of up to eight channels not even into the workspace."""

    _call, _judge = "levels", staticmethod(decode_n_status_error)

    def _allocate(self, torch) -> None:
        # the records as int64 [max_frames, channels, 3]: word 0 peak | samples << 32, word 1 sum, word 2 sum_squares
        self.levels = torch.zeros((self.max_frames, self.channels, 3), dtype=torch.int64, device=self.device)

    loud_frames = _DeviceCall._loud_frames
    route = _DeviceCall._route

    def measure(self, frames, offsets, n_frames: int):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1] -> the records of the first
        n_frames frames, int64 cuda tensor [n_frames, channels, 3], a view of the leveler's own buffer (records(): as LEVEL_DTYPE)."""
        self._frames_ok(frames, offsets, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_levels_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.levels.data_ptr(), self.sample_offsets.data_ptr(),
            self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.levels[:n_frames]

    def measure_payload(self, payload, max_frames=None):
        """Index and measure a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device, so the call can be captured into a graph.  -> (records [max_frames, channels, 3], count int32 [1]):
        records up to count[0] are the stream's.  The workspace grows to the largest payload seen (make one call before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_levels_payload_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, self.levels.data_ptr(), self.sample_offsets.data_ptr(),
            self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(), self.payload_workspace.data_ptr(),
            self.payload_workspace.numel(), stream))
        return self.levels[:max_frames], self.count

    @staticmethod
    def records(levels) -> np.ndarray:
        """Waits for the last call -> a host copy of records as LEVEL_DTYPE [n_frames, channels]."""
        host = np.ascontiguousarray(levels.cpu().numpy())
        return host.view(LEVEL_DTYPE).reshape(host.shape[:-1])


def levels_host(frames: np.ndarray, offsets: np.ndarray, channels: int) -> np.ndarray:
    """sela_hip_levels on numpy arrays -> the records, LEVEL_DTYPE [n_frames, channels]."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    out = np.zeros((n_frames, channels), LEVEL_DTYPE)
    capi.check(lib.sela_hip_levels(fr.ctypes.data, offs.ctypes.data, n_frames, channels, out.ctypes.data))
    return out


def track_levels(levels: np.ndarray) -> np.ndarray:
    """Folds records (LEVEL_DTYPE [n_frames, channels]) into one row per channel (TRACK_LEVEL_DTYPE [channels]): the largest peak
    and the sums of samples, sum and sum_squares, in Python's integers -- a sum that leaves its field's range raises OverflowError."""
    rec = np.asarray(levels, dtype=LEVEL_DTYPE)
    assert rec.ndim == 2
    out = np.zeros(rec.shape[1], TRACK_LEVEL_DTYPE)
    for c in range(rec.shape[1]):
        col = rec[:, c]
        out[c] = (max((int(p) for p in col["peak"]), default=0), sum(int(s) for s in col["samples"]), sum(int(s) for s in col["sum"]),
                  sum(int(s) for s in col["sum_squares"]))
    return out


# struct sela_hip_envelope (include/sela_hip.h): 16 bytes per (frame, bucket, channel)
ENVELOPE_DTYPE = np.dtype([("min", "<i2"), ("max", "<i2"), ("sum", "<i4"), ("sum_squares", "<u8")])
ENVELOPE_BUCKETS = (32, 64, 128, 256, 512, 1024, 2048)


class Enveloper(_DeviceCall):
    """sela_hip_envelope_device: the envelope of a stream on the device -- per frame, bucket of `bucket` samples (a power of two,
    32 .. 2048) and channel the smallest and the largest value, the sum and the sum of squares of the int16 samples DecoderN.decode
    would write.  All integers, so exact.  Owns its records and its workspace on the current device (or `device`);
    every call is asynchronous on the current stream and overwrites them.  No PCM is written: on the 2048-sample route of up to
    eight channels not even into the workspace."""

    _call, _judge = "envelope", staticmethod(decode_n_status_error)

    def __init__(self, max_frames: int, channels: int, stride: int, bucket: int, device=None):
        self.bucket = bucket
        self.slots = int(capi.lib().sela_hip_envelope_slots(stride, bucket))
        if self.slots == 0:
            raise ValueError(f"bucket must be one of {ENVELOPE_BUCKETS} and stride positive")
        super().__init__(max_frames, channels, stride, device)

    def _allocate(self, torch) -> None:
        # the records as int64 [max_frames, slots, channels, 2]: word 0 min | max << 16 | sum << 32, word 1 sum_squares
        self.envelope = torch.zeros((self.max_frames, self.slots, self.channels, 2), dtype=torch.int64, device=self.device)

    route = _DeviceCall._route

    def measure(self, frames, offsets, n_frames: int):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1] -> the records of the first
        n_frames frames, int64 cuda tensor [n_frames, slots, channels, 2], a view of the enveloper's own buffer (records(): as
        ENVELOPE_DTYPE)."""
        self._frames_ok(frames, offsets, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_envelope_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.bucket, self.envelope.data_ptr(),
            self.sample_offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.envelope[:n_frames]

    def measure_payload(self, payload, max_frames=None):
        """Index and measure a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device, so the call can be captured into a graph.  -> (records [max_frames, slots, channels, 2], count int32 [1]):
        records up to count[0] are the stream's.  The workspace grows to the largest payload seen (make one call before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_envelope_payload_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, self.bucket, self.envelope.data_ptr(),
            self.sample_offsets.data_ptr(), self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(),
            self.payload_workspace.data_ptr(), self.payload_workspace.numel(), stream))
        return self.envelope[:max_frames], self.count

    @staticmethod
    def records(envelope) -> np.ndarray:
        """Waits for the last call -> a host copy of records as ENVELOPE_DTYPE [n_frames, slots, channels]."""
        host = np.ascontiguousarray(envelope.cpu().numpy())
        return host.view(ENVELOPE_DTYPE).reshape(host.shape[:-1])


def envelope_host(frames: np.ndarray, offsets: np.ndarray, channels: int, bucket: int, stride=None) -> np.ndarray:
    """sela_hip_envelope on numpy arrays -> the records, ENVELOPE_DTYPE [n_frames, slots, channels].  stride None: the stream's
    largest samplesPerChannel (index_samples)."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    if stride is None:
        stride = max(index_samples(fr, offs, channels)[1], 1)
    slots = int(lib.sela_hip_envelope_slots(stride, bucket))
    out = np.zeros((n_frames, slots, channels), ENVELOPE_DTYPE)
    capi.check(lib.sela_hip_envelope(fr.ctypes.data, offs.ctypes.data, n_frames, channels, stride, bucket, out.ctypes.data))
    return out


def track_envelope(records: np.ndarray, sample_offsets, bucket: int) -> np.ndarray:
    """Records (ENVELOPE_DTYPE [n_frames, slots, channels]) on the track's grid: [ceil(total / bucket), channels], the empty slots
    behind each frame's end dropped.  Every frame but the last must hold a multiple of `bucket` samples (ValueError): frames of
    2048 samples and a whole-track stream's long last frame do."""
    rec = np.asarray(records, dtype=ENVELOPE_DTYPE)
    so = [int(s) for s in sample_offsets]
    assert rec.ndim == 3 and len(so) == rec.shape[0] + 1
    parts = []
    for f in range(rec.shape[0]):
        n = so[f + 1] - so[f]
        if f + 1 < rec.shape[0] and n % bucket:
            raise ValueError(f"frame {f} holds {n} samples, not a multiple of the bucket ({bucket}): its buckets are not the track's")
        used = -(-n // bucket)
        if used > rec.shape[1]:
            raise ValueError(f"frame {f} holds {n} samples, more than its {rec.shape[1]} slots of {bucket}")
        parts.append(rec[f, :used])
    return np.concatenate(parts) if parts else np.zeros((0, rec.shape[2]), ENVELOPE_DTYPE)


def fold_envelope(records: np.ndarray, factor: int) -> np.ndarray:
    """Merges `factor` adjacent buckets along the slot axis (the last but one: [..., slots, channels] -> [..., ceil(slots / factor),
    channels]): min of mins, max of maxes, the sums added in Python's integers -- a coarser zoom level of a waveform display
    without another device call.  The records are taken as they are: an all-zero record of an empty slot counts as a 0 seen."""
    rec = np.asarray(records, dtype=ENVELOPE_DTYPE)
    assert rec.ndim >= 2 and factor >= 1
    slots = rec.shape[-2]
    groups = -(-slots // factor)
    out = np.zeros(rec.shape[:-2] + (groups, rec.shape[-1]), ENVELOPE_DTYPE)
    for g in range(groups):
        part = rec[..., g * factor:(g + 1) * factor, :]
        out["min"][..., g, :] = part["min"].min(axis=-2)
        out["max"][..., g, :] = part["max"].max(axis=-2)
        # (Python's integers: a sum that leaves its field's range raises OverflowError, as in track_levels)
        out["sum"][..., g, :] = np.asarray(part["sum"].astype(object).sum(axis=-2), dtype=object)
        out["sum_squares"][..., g, :] = np.asarray(part["sum_squares"].astype(object).sum(axis=-2), dtype=object)
    return out


# struct sela_hip_digest (include/sela_hip.h): 8 bytes per frame
DIGEST_DTYPE = np.dtype([("crc32", "<u4"), ("samples", "<u4")])


class Digester(_DeviceCall):
    """sela_hip_digest_device: the CRC-32 (zlib.crc32) of the int16 PCM DecoderN.decode would write, per frame and for the whole
    track, on the device.  Owns its records, its two track words and its workspace on the current device (or
    `device`); every call is asynchronous on the current stream, one serial chain, and overwrites them -- so it can be captured
    into a graph.  No PCM is written: on the 2048-sample route of up to eight channels not even into the workspace."""

    _call, _judge = "digest", staticmethod(decode_n_status_error)

    def _allocate(self, torch) -> None:
        # the records as int64 [max_frames]: crc32 | samples << 32; the track: [crc32, bytes]
        self.digests = torch.zeros(self.max_frames, dtype=torch.int64, device=self.device)
        self.track = torch.zeros(2, dtype=torch.int64, device=self.device)

    route = _DeviceCall._route

    def digest(self, frames, offsets, n_frames: int):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1] -> (records int64 [n_frames],
        track int64 [2]: the CRC-32 of all frames' bytes and their number), views of the digester's own buffers (records(): as
        DIGEST_DTYPE)."""
        self._frames_ok(frames, offsets, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_digest_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.digests.data_ptr(), self.track.data_ptr(),
            self.sample_offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.digests[:n_frames], self.track

    def digest_payload(self, payload, max_frames=None):
        """Index and digest a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device.  -> (records [max_frames], track [2], count int32 [1]): records up to count[0] are the stream's, the
        track covers those.  The workspace grows to the largest payload seen (make one call before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_digest_payload_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, self.digests.data_ptr(), self.track.data_ptr(),
            self.sample_offsets.data_ptr(), self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(),
            self.payload_workspace.data_ptr(), self.payload_workspace.numel(), stream))
        return self.digests[:max_frames], self.track, self.count

    @staticmethod
    def records(digests) -> np.ndarray:
        """Waits for the last call -> a host copy of records as DIGEST_DTYPE [n_frames]."""
        host = np.ascontiguousarray(digests.cpu().numpy())
        return host.view(DIGEST_DTYPE).reshape(host.shape)

    def track_words(self):
        """Waits for the last call -> (the track's CRC-32, its bytes)."""
        t = self.track.cpu().numpy()
        return int(t[0]) & 0xFFFFFFFF, int(t[1])


def digest_host(frames: np.ndarray, offsets: np.ndarray, channels: int):
    """sela_hip_digest on numpy arrays -> (records DIGEST_DTYPE [n_frames], the track's CRC-32, its bytes)."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    out = np.zeros(n_frames, DIGEST_DTYPE)
    crc, total = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    capi.check(lib.sela_hip_digest(fr.ctypes.data, offs.ctypes.data, n_frames, channels, out.ctypes.data, crc.ctypes.data, total.ctypes.data))
    return out, int(crc[0]), int(total[0])


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """sela_hip_crc32_combine: crc32(A + B) from crc32(A), crc32(B) and len(B) -- pure host arithmetic."""
    return int(capi.lib().sela_hip_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, len_b))


def crc32_device(data, n_bytes=None, offset: int = 0, workspace=None, out=None):
    """sela_hip_crc32_device: the CRC-32 of n_bytes bytes of a contiguous cuda tensor from byte `offset` on (default: all of it)
    -> int64 cuda tensor [2] (`out`, or a new one): the CRC-32 and the byte count; asynchronous on the current stream."""
    import torch

    assert data.is_cuda and data.is_contiguous()
    total = data.numel() * data.element_size()
    n_bytes = total - offset if n_bytes is None else n_bytes
    assert 0 <= offset and offset + n_bytes <= total
    lib = capi.lib()
    need = int(lib.sela_hip_crc32_workspace_bytes(n_bytes))
    with torch.cuda.device(data.device):
        if out is None:
            out = torch.zeros(2, dtype=torch.int64, device=data.device)
        assert out.dtype == torch.int64 and out.is_cuda and out.numel() >= 2
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=data.device)
        capi.check(lib.sela_hip_crc32_device(
            data.data_ptr() + offset if n_bytes else None, n_bytes, out.data_ptr(), workspace.data_ptr(), workspace.numel(),
            torch.cuda.current_stream(data.device).cuda_stream))
    return out


# sela_hip_level32 (include/sela_hip.h): 32 bytes per (frame, channel); the energy is sum_squares_lo + (sum_squares_hi << 64)
LEVEL32_DTYPE = np.dtype([("peak", "<u4"), ("samples", "<u4"), ("sum", "<i8"), ("sum_squares_lo", "<u8"), ("sum_squares_hi", "<u8")])


class Leveler32(_DeviceCall):
    """sela_hip_levels_i32_device: Leveler on the whole domain of sela_hip_decode_i32_device -- samples of up to 32 bits, channels
    of different lengths, every subframe layout.  Record [f][c] is taken over the samples that call writes for
    channel c of frame f, with a 128-bit sum of squares.  Owns its records and its workspace on the current device (or `device`);
    every call is asynchronous on the current stream and overwrites them.  No decoded sample is stored for the layouts this
    project's encoders write."""

    _call, _judge = "levels_i32", staticmethod(decode_status_error)

    def _allocate(self, torch) -> None:
        # the records as int64 [max_frames, channels, 4]: word 0 peak | samples << 32, word 1 sum, words 2 and 3 the energy
        self.levels = torch.zeros((self.max_frames, self.channels, 4), dtype=torch.int64, device=self.device)

    loud_frames = _DeviceCall._loud_frames
    fallback_frames = _DeviceCall._fallback_frames

    def measure(self, frames, offsets, n_frames: int):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1] -> the records of the first
        n_frames frames, int64 cuda tensor [n_frames, channels, 4], a view of the leveler's own buffer (records(): as LEVEL32_DTYPE)."""
        self._frames_ok(frames, offsets, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_levels_i32_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.levels.data_ptr(), self.sample_offsets.data_ptr(),
            self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.levels[:n_frames]

    def measure_payload(self, payload, max_frames=None):
        """Index and measure a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device, so the call can be captured into a graph.  -> (records [max_frames, channels, 4], count int32 [1]):
        records up to count[0] are the stream's.  The workspace grows to the largest payload seen (make one call before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_levels_payload_i32_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, self.levels.data_ptr(), self.sample_offsets.data_ptr(),
            self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(), self.payload_workspace.data_ptr(),
            self.payload_workspace.numel(), stream))
        return self.levels[:max_frames], self.count

    @staticmethod
    def records(levels) -> np.ndarray:
        """Waits for the last call -> a host copy of records as LEVEL32_DTYPE [n_frames, channels]."""
        host = np.ascontiguousarray(levels.cpu().numpy())
        return host.view(LEVEL32_DTYPE).reshape(host.shape[:-1])


def levels_i32_host(frames: np.ndarray, offsets: np.ndarray, channels: int) -> np.ndarray:
    """sela_hip_levels_i32 on numpy arrays -> the records, LEVEL32_DTYPE [n_frames, channels]."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    out = np.zeros((n_frames, channels), LEVEL32_DTYPE)
    capi.check(lib.sela_hip_levels_i32(fr.ctypes.data, offs.ctypes.data, n_frames, channels, out.ctypes.data))
    return out


def levels_samples_i32(samples, counts=None):
    """sela_hip_levels_samples_i32_device: samples int32 cuda tensor [n_frames, channels, stride] (contiguous), counts int32 cuda
    tensor [n_frames * channels] or None (stride samples each) -> (records int64 cuda tensor [n_frames, channels, 4], status int32
    cuda tensor [4]); asynchronous on the current stream.  Leveler32.records() turns the records into LEVEL32_DTYPE."""
    import torch

    assert samples.dtype == torch.int32 and samples.is_cuda and samples.is_contiguous() and samples.dim() == 3
    n_frames, channels, stride = samples.shape
    assert counts is None or (counts.dtype == torch.int32 and counts.is_cuda and counts.is_contiguous() and counts.numel() == n_frames * channels)
    lib = capi.lib()
    levels = torch.zeros((n_frames, channels, 4), dtype=torch.int64, device=samples.device)
    status = torch.zeros(4, dtype=torch.int32, device=samples.device)
    workspace = torch.empty(int(lib.sela_hip_levels_samples_i32_workspace_bytes(n_frames, channels, stride)), dtype=torch.uint8, device=samples.device)
    capi.check(lib.sela_hip_levels_samples_i32_device(
        samples.data_ptr(), None if counts is None else counts.data_ptr(), n_frames, channels, stride, levels.data_ptr(), status.data_ptr(),
        workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream(samples.device).cuda_stream))
    return levels, status


def track_levels32(levels: np.ndarray) -> list:
    """Folds records (LEVEL32_DTYPE [n_frames, channels]) into one dict per channel -- peak, samples, sum, sum_squares -- in
    Python's integers: a track's sum of squares passes 2^64 within a few frames at full scale."""
    rec = np.asarray(levels, dtype=LEVEL32_DTYPE)
    assert rec.ndim == 2
    out = []
    for c in range(rec.shape[1]):
        col = rec[:, c]
        out.append({
            "peak": max((int(p) for p in col["peak"]), default=0), "samples": sum(int(s) for s in col["samples"]), "sum": sum(int(s) for s in col["sum"]),
            "sum_squares": sum(int(lo) + (int(hi) << 64) for lo, hi in zip(col["sum_squares_lo"], col["sum_squares_hi"])),
        })
    return out


# struct sela_hip_envelope32 (include/sela_hip.h): 32 bytes per (frame, bucket, channel); the energy is sum_squares_lo +
# (sum_squares_hi << 64)
ENVELOPE32_DTYPE = np.dtype([("min", "<i4"), ("max", "<i4"), ("sum", "<i8"), ("sum_squares_lo", "<u8"), ("sum_squares_hi", "<u8")])


class Enveloper32(_DeviceCall):
    """sela_hip_envelope_i32_device: Enveloper on the whole domain of sela_hip_decode_i32_device -- samples of up to 32 bits as
    they are, channels of different lengths, every subframe layout.  Record [f][b][c] is taken over the samples
    that call writes for channel c of frame f in bucket b, with a 128-bit sum of squares.  All integers, so exact.  Owns its
    records and its workspace on the current device (or `device`); every call is asynchronous on the current stream and overwrites
    them.  No decoded sample is stored for the layouts this project's encoders write."""

    _call, _judge = "envelope_i32", staticmethod(decode_status_error)

    def __init__(self, max_frames: int, channels: int, stride: int, bucket: int, device=None):
        self.bucket = bucket
        self.slots = int(capi.lib().sela_hip_envelope_slots(stride, bucket))
        if self.slots == 0:
            raise ValueError(f"bucket must be one of {ENVELOPE_BUCKETS} and stride positive")
        super().__init__(max_frames, channels, stride, device)

    def _allocate(self, torch) -> None:
        # the records as int64 [max_frames, slots, channels, 4]: word 0 min | max << 32, word 1 sum, words 2 and 3 the energy
        self.envelope = torch.zeros((self.max_frames, self.slots, self.channels, 4), dtype=torch.int64, device=self.device)

    fallback_frames = _DeviceCall._fallback_frames

    def measure(self, frames, offsets, n_frames: int):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1] -> the records of the first
        n_frames frames, int64 cuda tensor [n_frames, slots, channels, 4], a view of the enveloper's own buffer (records(): as
        ENVELOPE32_DTYPE)."""
        self._frames_ok(frames, offsets, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_envelope_i32_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.bucket, self.envelope.data_ptr(),
            self.sample_offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.envelope[:n_frames]

    def measure_payload(self, payload, max_frames=None):
        """Index and measure a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device, so the call can be captured into a graph.  -> (records [max_frames, slots, channels, 4], count int32 [1]):
        records up to count[0] are the stream's.  The workspace grows to the largest payload seen (make one call before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_envelope_payload_i32_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, self.bucket, self.envelope.data_ptr(),
            self.sample_offsets.data_ptr(), self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(),
            self.payload_workspace.data_ptr(), self.payload_workspace.numel(), stream))
        return self.envelope[:max_frames], self.count

    @staticmethod
    def records(envelope) -> np.ndarray:
        """Waits for the last call -> a host copy of records as ENVELOPE32_DTYPE [n_frames, slots, channels]."""
        host = np.ascontiguousarray(envelope.cpu().numpy())
        return host.view(ENVELOPE32_DTYPE).reshape(host.shape[:-1])


def envelope_i32_host(frames: np.ndarray, offsets: np.ndarray, channels: int, bucket: int, stride=None) -> np.ndarray:
    """sela_hip_envelope_i32 on numpy arrays -> the records, ENVELOPE32_DTYPE [n_frames, slots, channels].  stride None: the
    stream's largest samplesPerChannel (index_samples)."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    if stride is None:
        stride = max(index_samples(fr, offs, channels)[1], 1)
    slots = int(lib.sela_hip_envelope_slots(stride, bucket))
    out = np.zeros((n_frames, slots, channels), ENVELOPE32_DTYPE)
    capi.check(lib.sela_hip_envelope_i32(fr.ctypes.data, offs.ctypes.data, n_frames, channels, stride, bucket, out.ctypes.data))
    return out


def envelope_samples_i32(samples, bucket: int, counts=None):
    """sela_hip_envelope_samples_i32_device: samples int32 cuda tensor [n_frames, channels, stride] (contiguous), counts int32 cuda
    tensor [n_frames * channels] or None (stride samples each) -> (records int64 cuda tensor [n_frames, slots, channels, 4], status
    int32 cuda tensor [4]); asynchronous on the current stream.  Enveloper32.records() turns the records into ENVELOPE32_DTYPE."""
    import torch

    assert samples.dtype == torch.int32 and samples.is_cuda and samples.is_contiguous() and samples.dim() == 3
    n_frames, channels, stride = samples.shape
    assert counts is None or (counts.dtype == torch.int32 and counts.is_cuda and counts.is_contiguous() and counts.numel() == n_frames * channels)
    lib = capi.lib()
    slots = int(lib.sela_hip_envelope_slots(stride, bucket))
    if slots == 0:
        raise ValueError(f"bucket must be one of {ENVELOPE_BUCKETS} and stride positive")
    envelope = torch.zeros((n_frames, slots, channels, 4), dtype=torch.int64, device=samples.device)
    status = torch.zeros(4, dtype=torch.int32, device=samples.device)
    workspace = torch.empty(int(lib.sela_hip_envelope_samples_i32_workspace_bytes(n_frames, channels, stride)), dtype=torch.uint8, device=samples.device)
    capi.check(lib.sela_hip_envelope_samples_i32_device(
        samples.data_ptr(), None if counts is None else counts.data_ptr(), n_frames, channels, stride, bucket, envelope.data_ptr(), status.data_ptr(),
        workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream(samples.device).cuda_stream))
    return envelope, status


def track_envelope32(records: np.ndarray, sample_offsets, bucket: int) -> np.ndarray:
    """track_envelope for ENVELOPE32_DTYPE [n_frames, slots, channels]: the records on the track's grid, [ceil(total / bucket),
    channels], the empty slots behind each frame's end dropped.  Every frame but the last must hold a multiple of `bucket` samples
    (ValueError): frames of 2048 samples and a whole-track stream's long last frame do."""
    rec = np.asarray(records, dtype=ENVELOPE32_DTYPE)
    so = [int(s) for s in sample_offsets]
    assert rec.ndim == 3 and len(so) == rec.shape[0] + 1
    parts = []
    for f in range(rec.shape[0]):
        n = so[f + 1] - so[f]
        if f + 1 < rec.shape[0] and n % bucket:
            raise ValueError(f"frame {f} holds {n} samples, not a multiple of the bucket ({bucket}): its buckets are not the track's")
        used = -(-n // bucket)
        if used > rec.shape[1]:
            raise ValueError(f"frame {f} holds {n} samples, more than its {rec.shape[1]} slots of {bucket}")
        parts.append(rec[f, :used])
    return np.concatenate(parts) if parts else np.zeros((0, rec.shape[2]), ENVELOPE32_DTYPE)


def fold_envelope32(records: np.ndarray, factor: int) -> np.ndarray:
    """fold_envelope for ENVELOPE32_DTYPE: merges `factor` adjacent buckets along the slot axis (the last but one), min of mins,
    max of maxes, the sums and the 128-bit energies added in Python's integers.  The records are taken as they are: an all-zero
    record of an empty slot counts as a 0 seen.  A sum that leaves its field's range raises OverflowError."""
    rec = np.asarray(records, dtype=ENVELOPE32_DTYPE)
    assert rec.ndim >= 2 and factor >= 1
    slots = rec.shape[-2]
    groups = -(-slots // factor)
    out = np.zeros(rec.shape[:-2] + (groups, rec.shape[-1]), ENVELOPE32_DTYPE)
    for g in range(groups):
        part = rec[..., g * factor:(g + 1) * factor, :]
        out["min"][..., g, :] = part["min"].min(axis=-2)
        out["max"][..., g, :] = part["max"].max(axis=-2)
        out["sum"][..., g, :] = np.asarray(part["sum"].astype(object).sum(axis=-2), dtype=object)
        energy = np.asarray((part["sum_squares_lo"].astype(object) + part["sum_squares_hi"].astype(object) * (1 << 64)).sum(axis=-2), dtype=object)
        out["sum_squares_lo"][..., g, :] = energy % (1 << 64)
        out["sum_squares_hi"][..., g, :] = energy // (1 << 64)
    return out


class _WindowCall:
    """What WindowDecoder and WindowDecoder32 share: the buffers they own -- output, flags, status, and the workspace of
    sela_hip_<_entry>[_whole]_workspace_bytes -- the asserted decode(), flags, pack() and check().  A class names its entry, gives
    _allocate() its format and its output's shape and dtype, and lists in _extra what its call takes between the format and the
    output."""

    _entry = None  # "decode_windows": sela_hip_decode_windows_device, or with whole sela_hip_decode_windows_whole_device
    _extra = ()

    def _allocate(self, max_windows: int, window_samples: int, channels: int, format: int, shape, dtype: str, device, whole: bool) -> None:
        import torch

        self.torch = torch
        self.lib = capi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_windows, self.window_samples, self.channels, self.format = max_windows, window_samples, channels, format
        entry = f"sela_hip_{self._entry}_whole" if whole else f"sela_hip_{self._entry}"
        self.call = getattr(self.lib, entry + "_device")
        with torch.cuda.device(self.device):
            self.out = torch.empty(shape, dtype=getattr(torch, dtype), device=self.device)
            self.window_flags = torch.zeros(max(max_windows, 1), dtype=torch.int32, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
            ws = int(getattr(self.lib, entry + "_workspace_bytes")(max_windows, window_samples, channels))
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self.n_windows = 0

    @staticmethod
    def pack(starts, first_frames, n_frames) -> np.ndarray:
        """The descriptors of sela_hip_window as int64 [n, 2] on the host (send it to the device with torch.from_numpy(...).cuda()):
        word 0 the start (any uint64, as its bit pattern), word 1 first_frame | n_frames << 32.  Scalars are broadcast."""
        starts = np.atleast_1d(np.asarray(starts, dtype=np.uint64))
        first = np.broadcast_to(np.asarray(first_frames, dtype=np.uint64), starts.shape)
        count = np.broadcast_to(np.asarray(n_frames, dtype=np.uint64), starts.shape)
        assert (first < 2 ** 32).all() and (count < 2 ** 32).all()
        packed = np.empty((len(starts), 2), np.uint64)
        packed[:, 0] = starts
        packed[:, 1] = first | (count << np.uint64(32))
        return packed.view(np.int64)

    def decode(self, frames, offsets, n_frames_total: int, windows):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames_total + 1], windows: int64 cuda tensor
        [n, 2] (pack()) -> the first n windows of the decoder's own output buffer."""
        torch = self.torch
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()
        assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous() and offsets.numel() >= n_frames_total + 1
        assert windows.dtype == torch.int64 and windows.is_cuda and windows.is_contiguous() and windows.dim() == 2 and windows.shape[1] == 2
        n = int(windows.shape[0])
        assert n <= self.max_windows
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.call(
            frames.data_ptr(), offsets.data_ptr(), n_frames_total, self.channels, windows.data_ptr(), n, self.window_samples, self.format, *self._extra,
            self.out.data_ptr(), self.window_flags.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        self.n_windows = n
        return self.out[:n]

    @property
    def flags(self):
        """int32 cuda tensor [n]: the OR of the flag bits of the frames each window of the last call touched."""
        return self.window_flags[: self.n_windows]

    def check(self) -> None:
        """Waits for the last call and raises SelaHipError with the code the class's host call (sela_hip_decode_windows,
        sela_hip_decode_windows_i32) returns for the same batch."""
        st = self.status.cpu().numpy().copy()
        # sela_hip_decode_n_status_error judges [0] flag bits and [1] bad frames by the route named in [3]; 1 is the 2048-sample
        # decoder's, the mapping the host call uses (a malformed frame or a dry Rice stream: EFORMAT; a coefficient outside the
        # tables or beyond int64: ERANGE).  This call's [2] counts flagged windows, which that function does not read, and the
        # 32-bit call's [3] is its wide count.
        st[2], st[3] = 0, 1
        capi.check(decode_n_status_error(st))


def _windows_host(call, frames: np.ndarray, offsets: np.ndarray, channels: int, windows: np.ndarray, window_samples: int, format: int, extra, shape_of):
    """The body of decode_windows_host and decode_windows_i32_host: `call` on contiguous copies, `extra` between the format and
    the output, which is shape_of(n)'s (shape, dtype); any code but 0, EFORMAT and ERANGE raises."""
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    win = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(*shape_of(len(win)))
    flags = np.zeros(len(win), np.uint32)
    rc = call(fr.ctypes.data, offs.ctypes.data, len(offs) - 1, channels, win.ctypes.data, len(win), window_samples, format, *extra, out.ctypes.data, flags.ctypes.data)
    if rc not in (capi.OK, -5, -6):
        capi.check(rc)
    return out, flags, rc


class WindowDecoder(_WindowCall):
    """sela_hip_decode_windows_device: windows of `window_samples` samples cut from streams of 2048-sample frames that lie in
    device memory -- only the frames a window touches are decoded.  Owns its output, flags, status and workspace
    on the current device (or `device`); every call is asynchronous on the current stream and overwrites them.  planar_float:
    float32 [n, channels, window_samples] holding value / 32768 instead of int16 [n, window_samples, channels].  whole:
    sela_hip_decode_windows_whole_device -- the streams are whole-track streams, whose last frame of 1 .. 4095
    samples is decoded too."""

    _entry = "decode_windows"

    def __init__(self, max_windows: int, window_samples: int, channels: int, planar_float: bool = False, device=None, whole: bool = False):
        if planar_float:
            self._allocate(max_windows, window_samples, channels, capi.WINDOW_F32_PLANAR, (max_windows, channels, window_samples), "float32", device, whole)
        else:
            self._allocate(max_windows, window_samples, channels, capi.WINDOW_I16_INTERLEAVED, (max_windows, window_samples, channels), "int16", device, whole)


def decode_windows_host(frames: np.ndarray, offsets: np.ndarray, channels: int, windows: np.ndarray, window_samples: int, planar_float: bool = False,
                        whole: bool = False):
    """sela_hip_decode_windows (whole: sela_hip_decode_windows_whole) on numpy arrays; windows: int64 [n, 2] (WindowDecoder.pack).  Returns three values: the windows
    (int16 [n, window_samples, channels], or float32 [n, channels, window_samples]), the per-window flags (uint32 [n]) and the
    call's return code -- 0, or EFORMAT / ERANGE (capi.ERRORS) for a batch with a bad frame, whose other windows are good all
    the same; any other code raises."""
    lib = capi.lib()
    call = lib.sela_hip_decode_windows_whole if whole else lib.sela_hip_decode_windows
    if planar_float:
        return _windows_host(call, frames, offsets, channels, windows, window_samples, capi.WINDOW_F32_PLANAR, (), lambda n: ((n, channels, window_samples), np.float32))
    return _windows_host(call, frames, offsets, channels, windows, window_samples, capi.WINDOW_I16_INTERLEAVED, (), lambda n: ((n, window_samples, channels), np.int16))


def _window32_shape(n: int, window_samples: int, channels: int, format: int):
    """(shape, numpy dtype name) of n windows in one of sela_hip_decode_windows_i32's formats."""
    if format == capi.WINDOW_I32_PLANAR:
        return (n, channels, window_samples), "int32"
    if format == capi.WINDOW_F32_PLANAR:
        return (n, channels, window_samples), "float32"
    if format == capi.WINDOW_PCM32_INTERLEAVED:
        return (n, window_samples, channels), "int32"
    if format == capi.WINDOW_PCM24_INTERLEAVED:
        return (n, window_samples, channels, 3), "uint8"
    raise ValueError("format must be capi.WINDOW_F32_PLANAR, WINDOW_I32_PLANAR, WINDOW_PCM24_INTERLEAVED or WINDOW_PCM32_INTERLEAVED")


class WindowDecoder32(_WindowCall):
    """sela_hip_decode_windows_i32_device: windows of `window_samples` samples of up to 32 bits cut from streams of 2048-sample
    frames that lie in device memory.  Owns its output, flags, status and workspace on the current device (or
    `device`); every call is asynchronous on the current stream and overwrites them.  format (capi.WINDOW_*): I32_PLANAR int32
    [n, channels, window_samples]; F32_PLANAR float32 of that shape holding value * 2^-(sample_bits - 1); PCM32_INTERLEAVED int32
    [n, window_samples, channels]; PCM24_INTERLEAVED uint8 [n, window_samples, channels, 3], each sample's low three bytes."""

    _entry = "decode_windows_i32"

    def __init__(self, max_windows: int, window_samples: int, channels: int, format: int, sample_bits: int = 24, device=None, whole: bool = False):
        # whole: sela_hip_decode_windows_i32_whole_device -- a stream's long last frame is decoded too
        self.sample_bits = sample_bits
        self._extra = (sample_bits,)
        self._allocate(max_windows, window_samples, channels, format, *_window32_shape(max_windows, window_samples, channels, format), device, whole)

    def wide_samples(self) -> int:
        """Waits for the last call: PCM24's count of samples outside [-2^23, 2^23) (their low bytes were written); else 0."""
        return int(self.status.cpu().numpy().view(np.uint32)[3])


def decode_windows_i32_host(frames: np.ndarray, offsets: np.ndarray, channels: int, windows: np.ndarray, window_samples: int, format: int, sample_bits: int = 24,
                            whole: bool = False):
    """sela_hip_decode_windows_i32 (whole: sela_hip_decode_windows_i32_whole) on numpy arrays; windows: int64 [n, 2] (WindowDecoder.pack).  Returns three values: the windows
    in `format` (WindowDecoder32's shapes), the per-window flags (uint32 [n]) and the call's return code -- 0, or EFORMAT / ERANGE
    (capi.ERRORS) for a batch with a bad frame, whose other windows are good all the same; any other code raises."""
    lib = capi.lib()
    call = lib.sela_hip_decode_windows_i32_whole if whole else lib.sela_hip_decode_windows_i32
    return _windows_host(call, frames, offsets, channels, windows, window_samples, format, (sample_bits,), lambda n: _window32_shape(n, window_samples, channels, format))


def verify_host(frames: np.ndarray, offsets: np.ndarray, channels: int, pcm: np.ndarray):
    """sela_hip_verify on numpy arrays; pcm: int16 in the layout decode_host returns.  Returns three values:
    diff_counts (uint32 [n_frames]), first_diff (uint32 [n_frames]; 0xFFFFFFFF where nothing differs) and the number of
    frames with a difference (int)."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    p = np.ascontiguousarray(pcm, dtype=np.int16)
    n_frames = len(offs) - 1
    counts = np.zeros(n_frames, np.uint32)
    first = np.zeros(n_frames, np.uint32)
    lossy = C.c_uint32(0)
    capi.check(lib.sela_hip_verify(fr.ctypes.data, offs.ctypes.data, n_frames, channels, p.ctypes.data, counts.ctypes.data, first.ctypes.data, C.byref(lossy)))
    return counts, first, int(lossy.value)


class Verifier32(_DeviceCall):
    """sela_hip_verify_i32_device: a stream held against the int32 samples it was made from, frame by frame, on the device --
    the whole domain of Decoder32 (samples of up to 32 bits, planar frames, channels of different lengths).  Owns its outputs and
    its workspace on the current device (or `device`); every call is asynchronous on the current stream and overwrites them.  For
    the layouts the encoders write no decoded sample is stored anywhere beyond the subframes as decoded."""

    _call, _judge = "verify_i32", staticmethod(decode_status_error)
    _allocate = _DeviceCall._allocate_diffs
    lossy_frames = _DeviceCall._lossy_frames
    fallback_frames = _DeviceCall._fallback_frames

    def _inputs_ok(self, samples, lengths, n_frames: int) -> bool:
        torch = self.torch
        ok = samples.dtype == torch.int32 and samples.is_cuda and samples.is_contiguous() and samples.numel() >= n_frames * self.channels * self.stride
        if lengths is not None:
            ok = ok and lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n_frames * self.channels
        return ok

    def verify(self, frames, offsets, n_frames: int, samples, lengths=None):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1], samples: int32 cuda tensor
        [n_frames, channels, stride] (the layout Decoder32.decode returns), lengths: int32 cuda tensor [n_frames, channels] (the
        original's length of every channel) or None: every channel is stride long
        -> (diff_counts int32 [n_frames], first_diff int32 [n_frames]; -1: nothing differs), views of the verifier's own buffers."""
        self._frames_ok(frames, offsets, n_frames)
        assert self._inputs_ok(samples, lengths, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_verify_i32_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, samples.data_ptr(),
            None if lengths is None else lengths.data_ptr(), self.diff_counts.data_ptr(), self.first_diff.data_ptr(), self.sample_offsets.data_ptr(),
            self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.diff_counts[:n_frames], self.first_diff[:n_frames]

    def verify_payload(self, payload, samples, lengths=None, max_frames=None):
        """Index and verify a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device, so the call can be captured into a graph.  -> (diff_counts [max_frames], first_diff [max_frames],
        count int32 [1]): entries up to count[0] are the stream's.  The workspace grows to the largest payload seen (make one call
        before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        assert self._inputs_ok(samples, lengths, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_verify_payload_i32_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, samples.data_ptr(),
            None if lengths is None else lengths.data_ptr(), self.diff_counts.data_ptr(), self.first_diff.data_ptr(), self.sample_offsets.data_ptr(),
            self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(), self.payload_workspace.data_ptr(),
            self.payload_workspace.numel(), stream))
        return self.diff_counts[:max_frames], self.first_diff[:max_frames], self.count


def verify_i32(frames: np.ndarray, offsets: np.ndarray, channels: int, samples: np.ndarray, lengths=None):
    """sela_hip_verify_i32 on numpy arrays; samples: int32 [n_frames, channels, stride] (the layout decode_i32 fills), lengths:
    [n_frames, channels] or None (every channel is stride long).  Returns three values: diff_counts (uint32 [n_frames]),
    first_diff (uint32 [n_frames]; 0xFFFFFFFF where nothing differs) and the number of frames with a difference (int)."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    smp = np.ascontiguousarray(samples, dtype=np.int32)
    assert smp.ndim == 3 and smp.shape[:2] == (n_frames, channels)
    stride = smp.shape[2]
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint32)
    assert ln is None or ln.size == n_frames * channels
    counts = np.zeros(n_frames, np.uint32)
    first = np.zeros(n_frames, np.uint32)
    lossy = C.c_uint32(0)
    capi.check(lib.sela_hip_verify_i32(fr.ctypes.data, offs.ctypes.data, n_frames, channels, stride, smp.ctypes.data, None if ln is None else ln.ctypes.data,
                                       counts.ctypes.data, first.ctypes.data, C.byref(lossy)))
    return counts, first, int(lossy.value)


class VerifierPcm(_DeviceCall):
    """sela_hip_verify_pcm_device: a stream held against the packed interleaved PCM it was made from -- 3 or 4
    bytes a sample, little-endian, frame f at sample_offsets[f] (the layout DecoderPcm writes and a WAV's data chunk has), frames
    of any lengths -- frame by frame, on the device, without an unpacked copy of the original.  Owns its outputs and its
    workspace on the current device (or `device`); every call is asynchronous on the current stream and overwrites them."""

    _call, _judge = "verify_pcm", staticmethod(decode_status_error)
    _allocate = _DeviceCall._allocate_diffs
    lossy_frames = _DeviceCall._lossy_frames
    fallback_frames = _DeviceCall._fallback_frames

    def __init__(self, max_frames: int, channels: int, stride: int, bytes_per_sample: int, device=None):
        self.bytes_per_sample = bytes_per_sample
        super().__init__(max_frames, channels, stride, device)

    def _samples(self, pcm, pcm_samples) -> int:
        torch = self.torch
        assert pcm.dtype == torch.uint8 and pcm.is_cuda and pcm.is_contiguous()
        per = self.channels * self.bytes_per_sample
        if pcm_samples is None:
            pcm_samples = pcm.numel() // per
        assert pcm_samples * per <= pcm.numel()
        return pcm_samples

    def verify(self, frames, offsets, n_frames: int, pcm, pcm_samples=None):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1], pcm: uint8 cuda tensor (4-byte
        aligned) of pcm_samples samples per channel (None: all it holds)
        -> (diff_counts int32 [n_frames], first_diff int32 [n_frames]: sample * channels + channel in the frame; -1: nothing
        differs), views of the verifier's own buffers."""
        self._frames_ok(frames, offsets, n_frames)
        pcm_samples = self._samples(pcm, pcm_samples)
        stream = self._stream()
        capi.check(self.lib.sela_hip_verify_pcm_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, pcm.data_ptr(), self.bytes_per_sample, pcm_samples,
            self.diff_counts.data_ptr(), self.first_diff.data_ptr(), self.sample_offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(),
            self.workspace.numel(), stream))
        return self.diff_counts[:n_frames], self.first_diff[:n_frames]

    def verify_payload(self, payload, pcm, pcm_samples=None, max_frames=None):
        """Index and verify a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device.  -> (diff_counts [max_frames], first_diff [max_frames], count int32 [1]): entries up to count[0] are the
        stream's.  The workspace grows to the largest payload seen (make one call before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        pcm_samples = self._samples(pcm, pcm_samples)
        stream = self._stream()
        capi.check(self.lib.sela_hip_verify_payload_pcm_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, pcm.data_ptr(), self.bytes_per_sample, pcm_samples,
            self.diff_counts.data_ptr(), self.first_diff.data_ptr(), self.sample_offsets.data_ptr(), self.frame_offsets.data_ptr(), self.count.data_ptr(),
            self.status.data_ptr(), self.payload_workspace.data_ptr(), self.payload_workspace.numel(), stream))
        return self.diff_counts[:max_frames], self.first_diff[:max_frames], self.count


def verify_pcm_host(frames: np.ndarray, offsets: np.ndarray, channels: int, bytes_per_sample: int, pcm, pcm_samples=None):
    """sela_hip_verify_pcm on numpy arrays; pcm: the packed interleaved bytes (uint8, or anything with a buffer), pcm_samples: the
    samples per channel it holds (None: all of it).  Returns three values: diff_counts (uint32 [n_frames]), first_diff (uint32
    [n_frames]: sample * channels + channel in the frame; 0xFFFFFFFF where nothing differs) and the number of frames with a difference."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    p = np.ascontiguousarray(np.frombuffer(pcm, dtype=np.uint8) if not isinstance(pcm, np.ndarray) else pcm.view(np.uint8).reshape(-1))
    if pcm_samples is None:
        pcm_samples = p.size // (channels * bytes_per_sample) if channels and bytes_per_sample else 0
    assert pcm_samples * channels * bytes_per_sample <= p.size
    counts = np.zeros(n_frames, np.uint32)
    first = np.zeros(n_frames, np.uint32)
    lossy = C.c_uint32(0)
    capi.check(lib.sela_hip_verify_pcm(fr.ctypes.data, offs.ctypes.data, n_frames, channels, bytes_per_sample, p.ctypes.data, pcm_samples, counts.ctypes.data,
                                       first.ctypes.data, C.byref(lossy)))
    return counts, first, int(lossy.value)


class Encoder32:
    """sela_hip_encode_i32 -- and sela_hip_encode of any length -- on the device: frames of any samples_per_channel (1 .. 65535),
    32-bit samples.  Owns its workspace, frames, offsets and status on the current device (or `device`); every call is
    asynchronous on the current stream and overwrites them.  `capacity` (bytes of frames) defaults to the host route's
    estimate -- 4.5 bytes per sample, which holds noise of up to 20 bits -- not the certain bound; a call that did not fit says
    so in check(), and needed_bytes() is what it needs.  lossless: SELA_HIP_ENCODE_LOSSLESS, as Encoder.
    paired: the sela_hip_encode_paired_*_device calls -- every odd channel may be stored as the difference
    against the even channel before it, in a stream every decoder of the format reads."""

    def __init__(self, max_frames: int, channels: int, samples_per_channel: int, capacity=None, device=None, lossless: bool = False, paired: bool = False):
        import torch

        self.options = capi.ENCODE_LOSSLESS if lossless else 0
        self.paired = bool(paired)

        self.torch = torch
        self.lib = capi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_frames, self.channels, self.n = max_frames, channels, samples_per_channel
        if capacity is None:
            capacity = max_frames * ((samples_per_channel * channels * 9) // 2 + channels * 192 + 64)
        self.capacity = max(int(capacity), 4)
        ws = int((self.lib.sela_hip_encode_paired_workspace_bytes if paired else self.lib.sela_hip_encode_i32_workspace_bytes)(max_frames, channels, samples_per_channel))
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
            self.frames = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
            self.offsets = torch.zeros(max_frames + 1, dtype=torch.int64, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.n_frames = 0

    def encode(self, samples):
        """samples: int32 cuda tensor [n_frames, channels, n] (planar) or int16 [n_frames, n, channels] (interleaved), contiguous
        -> (frames uint8 [capacity], offsets int64 [n_frames + 1], status int32 [4]): the encoder's own buffers, the first
        offsets[n_frames] bytes of frames the stream's when check() passes."""
        torch = self.torch
        assert samples.is_cuda and samples.is_contiguous() and samples.dim() == 3
        n_frames = samples.shape[0]
        if samples.dtype == torch.int32:
            assert tuple(samples.shape[1:]) == (self.channels, self.n)
            kind = "i32"
        else:
            assert samples.dtype == torch.int16 and tuple(samples.shape[1:]) == (self.n, self.channels)
            kind = "n"
        assert n_frames <= self.max_frames
        stream = torch.cuda.current_stream(self.device).cuda_stream
        args = [samples.data_ptr(), n_frames, self.channels, self.n, self.frames.data_ptr(), self.capacity, self.offsets.data_ptr(),
                self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream]
        if self.paired:  # (its own options word, always)
            call = getattr(self.lib, "sela_hip_encode_paired_%s_device" % kind)
            args.append(self.options)
        elif self.options:
            call = getattr(self.lib, "sela_hip_encode_%s_device_opt" % kind)
            args.append(self.options)
        else:
            call = getattr(self.lib, "sela_hip_encode_%s_device" % kind)
        capi.check(call(*args))
        self.n_frames = n_frames
        return self.frames, self.offsets[: n_frames + 1], self.status

    def needed_bytes(self) -> int:
        """Waits for the last call: the bytes its frames take (offsets[n_frames])."""
        return int(self.offsets[self.n_frames].item())

    def check(self) -> None:
        """Waits for the last call and raises SelaHipError with the code the host call gives for the same input."""
        capi.check(encode_status_error(self.status.cpu().numpy()))

    def to_host(self):
        """check(), then -> (frames uint8 [...], offsets uint64 [n_frames + 1]) on the host."""
        self.check()
        offs = self.offsets[: self.n_frames + 1].cpu().numpy().view(np.uint64)
        return self.frames[: int(offs[-1])].cpu().numpy(), offs


def whole_frames(n_samples: int):
    """The layout of a whole track of n_samples samples per channel (no GPU): a list of (first_sample, length),
    one per frame -- 2048-sample frames, the tail folded into the last one; one frame for a track below 2048 samples."""
    lib = capi.lib()
    first, length = C.c_uint64(), C.c_uint32()
    out = []
    for f in range(int(lib.sela_hip_whole_frames(n_samples))):
        capi.check(lib.sela_hip_whole_frame(n_samples, f, C.byref(first), C.byref(length)))
        out.append((int(first.value), int(length.value)))
    return out


class _WholeEncode:
    """What WholeEncoder and WholeEncoderPcm share: the track's bounds, the buffers they own, the end of encode(), check() and
    to_host().  A class opens with _bounds(), which its default capacity may ask, then allocates."""

    def _bounds(self, max_samples: int, channels: int, lossless: bool, device) -> None:
        import torch

        self.torch = torch
        self.lib = capi.lib()
        self.options = capi.ENCODE_LOSSLESS if lossless else 0
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_samples, self.channels = int(max_samples), int(channels)
        self.max_frames = int(self.lib.sela_hip_whole_frames(self.max_samples))

    def _allocate(self, capacity: int, workspace_bytes: int) -> None:
        torch = self.torch
        self.capacity = max(int(capacity), 4)
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(int(workspace_bytes), dtype=torch.uint8, device=self.device)
            self.frames = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
            self.offsets = torch.zeros(self.max_frames + 1, dtype=torch.int64, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.n_frames = 0

    def _encoded(self, n_samples: int):
        self.n_frames = int(self.lib.sela_hip_whole_frames(n_samples))
        return self.frames, self.offsets[: self.n_frames + 1], self.status

    def check(self) -> None:
        """Waits for the last call and raises SelaHipError with the code the host call gives for the same input."""
        capi.check(encode_status_error(self.status.cpu().numpy()))

    def to_host(self):
        """check(), then -> (frames uint8 [...], offsets uint64 [frames + 1]) on the host."""
        self.check()
        offs = self.offsets[: self.n_frames + 1].cpu().numpy().view(np.uint64)
        return self.frames[: int(offs[-1])].cpu().numpy(), offs


class WholeEncoder(_WholeEncode):
    """sela_hip_encode_whole_device: a whole track of up to max_samples samples per channel, its tail kept in a long last frame
    (DESIGN.md 5.19).  Owns its workspace, frames, offsets and status on the current device (or `device`); every call is
    asynchronous on the current stream and overwrites them.  `capacity` (bytes of frames) defaults to the certain bound.
    lossless: SELA_HIP_ENCODE_LOSSLESS, as Encoder."""

    def __init__(self, max_samples: int, channels: int, lossless: bool = False, device=None, capacity=None):
        self._bounds(max_samples, channels, lossless, device)
        if capacity is None:
            capacity = int(self.lib.sela_hip_encode_whole_bound_bytes(self.max_samples, channels))
        self._allocate(capacity, self.lib.sela_hip_encode_whole_workspace_bytes(self.max_samples, channels))

    def encode(self, pcm):
        """pcm: int16 cuda tensor [n_samples, channels], contiguous -> (frames uint8 [capacity], offsets int64 [frames + 1],
        status int32 [4]): the encoder's own buffers, the first offsets[-1] bytes of frames the stream's when check() passes."""
        torch = self.torch
        assert pcm.is_cuda and pcm.is_contiguous() and pcm.dtype == torch.int16 and pcm.dim() == 2 and pcm.shape[1] == self.channels
        n_samples = pcm.shape[0]
        assert n_samples <= self.max_samples
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.sela_hip_encode_whole_device(pcm.data_ptr(), n_samples, self.channels, self.frames.data_ptr(), self.capacity, self.offsets.data_ptr(),
                                                         self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream, self.options))
        return self._encoded(n_samples)


def encode_status_error(status) -> int:
    """sela_hip_encode_status_error on a host copy of four status words (any integer array of 4) -> the host call's code."""
    st = np.ascontiguousarray(np.asarray(status).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    assert st.shape == (4,)
    return int(capi.lib().sela_hip_encode_status_error(st.ctypes.data))


# ---- host-pointer API on numpy arrays (what the C++ host calls) --------------------------------------
def encode_host(pcm: np.ndarray, lossless: bool = False, paired: bool = False):
    """pcm: int16 [n_frames, n, channels] (n = 2048: the fast kernels; anything else in 1..65535: the any-length route)
    -> (frames uint8[...], offsets uint64[n_frames+1]).  lossless: SELA_HIP_ENCODE_LOSSLESS (sela_hip_encode_opt).
    paired: sela_hip_encode_paired (the any-length route for every n)."""
    lib = capi.lib()
    p = np.ascontiguousarray(pcm, dtype=np.int16)
    n_frames, n, ch = p.shape
    cap = max(2 * p.nbytes, 4096) if n == BLOCK else int(lib.sela_hip_encode_bound_bytes_n(n_frames, ch, n))
    frames = np.empty(cap, np.uint8)
    offs = np.zeros(n_frames + 1, np.uint64)
    if paired:
        capi.check(lib.sela_hip_encode_paired(p.ctypes.data, n_frames, ch, n, frames.ctypes.data, cap, offs.ctypes.data, capi.ENCODE_LOSSLESS if lossless else 0))
    elif lossless:
        capi.check(lib.sela_hip_encode_opt(p.ctypes.data, n_frames, ch, n, frames.ctypes.data, cap, offs.ctypes.data, capi.ENCODE_LOSSLESS))
    else:
        capi.check(lib.sela_hip_encode(p.ctypes.data, n_frames, ch, n, frames.ctypes.data, cap, offs.ctypes.data))
    return frames[: int(offs[n_frames])].copy(), offs


def encode_whole_host(pcm: np.ndarray, lossless: bool = False):
    """sela_hip_encode_whole: pcm int16 [n_samples, channels] -- a whole track, its tail kept in a long last frame
    -> (frames uint8[...], offsets uint64[frames + 1])."""
    lib = capi.lib()
    p = np.ascontiguousarray(pcm, dtype=np.int16)
    n_samples, ch = p.shape
    n_frames = int(lib.sela_hip_whole_frames(n_samples))
    cap = max(int(lib.sela_hip_encode_whole_bound_bytes(n_samples, ch)), 4)
    frames = np.empty(cap, np.uint8)
    offs = np.zeros(n_frames + 1, np.uint64)
    capi.check(lib.sela_hip_encode_whole(p.ctypes.data, n_samples, ch, frames.ctypes.data, cap, offs.ctypes.data, capi.ENCODE_LOSSLESS if lossless else 0))
    return frames[: int(offs[n_frames])].copy(), offs


class WholeDecoder:
    """sela_hip_decode_whole_device: a full decode of a whole-track stream of up to max_frames frames -- frames of
    2048 samples on the 2048-sample decoder and the long last frame (1 .. 4095 samples) beside them, behind them in the PCM.  Owns
    its outputs and its workspace on the current device (or `device`); every call is asynchronous on the current stream,
    overwrites them, and can be captured into a graph.  `capacity` (samples per channel) defaults to the most such a stream holds."""

    def __init__(self, max_frames: int, channels: int, device=None, capacity=None):
        import torch

        self.torch = torch
        self.lib = capi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_frames, self.channels = max_frames, channels
        self.capacity = max_frames * BLOCK + (BLOCK - 1 if max_frames else 0) if capacity is None else capacity
        with torch.cuda.device(self.device):
            self.pcm = torch.empty((max(self.capacity, 1), channels), dtype=torch.int16, device=self.device)
            self.n_samples = torch.zeros(1, dtype=torch.int64, device=self.device)
            self.frame_offsets = torch.zeros(max_frames + 1, dtype=torch.int64, device=self.device)
            self.count = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
            ws = int(self.lib.sela_hip_decode_whole_workspace_bytes(max_frames, channels))
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)

    def decode(self, frames, offsets, n_frames: int, capacity=None):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1] -> (pcm int16 [capacity, channels],
        n_samples int64 [1]), the decoder's own buffers: the stream's samples are pcm[: n_samples[0]]."""
        torch = self.torch
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()
        assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous() and n_frames <= self.max_frames
        capacity = self.capacity if capacity is None else capacity
        assert capacity <= self.capacity
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.sela_hip_decode_whole_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.pcm.data_ptr(), capacity, self.n_samples.data_ptr(),
            self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.pcm, self.n_samples

    def decode_payload(self, payload, max_frames=None, capacity=None):
        """Index and decode a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count stays on
        the device.  -> (pcm, n_samples int64 [1], frame_offsets int64 [max_frames + 1], count int32 [1]).  The workspace grows to
        the largest payload seen (make one call before capturing)."""
        torch = self.torch
        max_frames = self.max_frames if max_frames is None else max_frames
        capacity = self.capacity if capacity is None else capacity
        assert payload.dtype == torch.uint8 and payload.is_cuda and payload.is_contiguous() and max_frames <= self.max_frames and capacity <= self.capacity
        need = int(self.lib.sela_hip_index_workspace_bytes(payload.numel(), max_frames)) + int(
            self.lib.sela_hip_decode_whole_workspace_bytes(max_frames, self.channels))
        with torch.cuda.device(self.device):
            if getattr(self, "payload_workspace", None) is None or self.payload_workspace.numel() < need:
                self.payload_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.sela_hip_decode_whole_payload_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.pcm.data_ptr(), capacity, self.n_samples.data_ptr(),
            self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(), self.payload_workspace.data_ptr(),
            self.payload_workspace.numel(), stream))
        return self.pcm, self.n_samples, self.frame_offsets[: max_frames + 1], self.count

    def route(self) -> int:
        """Waits for the last call -> 0 nothing decoded, 1 the 2048-sample decoder alone, 3 with the long last frame beside it."""
        return int(self.status[3].item())

    def check(self) -> None:
        """Waits for the last call and raises SelaHipError with sela_hip_decode_whole_status_error's code."""
        capi.check(decode_whole_status_error(self.status.cpu().numpy()))


def decode_whole_status_error(status) -> int:
    """sela_hip_decode_whole_status_error on a host copy of four status words (any integer array of 4) -> the host call's code."""
    st = np.ascontiguousarray(np.asarray(status).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    assert st.shape == (4,)
    return int(capi.lib().sela_hip_decode_whole_status_error(st.ctypes.data))


def decode_whole_host(frames: np.ndarray, offsets: np.ndarray, channels: int, capacity=None, check: bool = True):
    """sela_hip_decode_whole on numpy arrays -> (pcm int16 [capacity, channels], n_samples, the call's code): the stream's samples
    are pcm[:n_samples].  capacity (samples per channel) defaults to what a stream of that many frames can hold; check: raise
    SelaHipError on a code other than 0."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    capacity = n_frames * BLOCK + (BLOCK - 1 if n_frames else 0) if capacity is None else capacity
    pcm = np.zeros((max(capacity, 1), channels), np.int16)
    n_samples = np.zeros(1, np.uint64)
    rc = int(lib.sela_hip_decode_whole(fr.ctypes.data, offs.ctypes.data, n_frames, channels, pcm.ctypes.data, capacity, n_samples.ctypes.data))
    if check:
        capi.check(rc)
    return pcm, int(n_samples[0]), rc


def decode_host(frames: np.ndarray, offsets: np.ndarray, channels: int) -> np.ndarray:
    """-> int16 [n_frames, 2048, channels] for a stream of 2048-sample frames; for any other stream int16 [total samples,
    channels], frame f's samples from index_samples()[0][f] on."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    sample_offsets, largest = index_samples(fr, offs, channels)
    standard = largest == BLOCK and all(int(sample_offsets[f]) == f * BLOCK for f in range(n_frames + 1))
    total = n_frames * BLOCK if standard or largest == 0 else int(sample_offsets[n_frames])
    pcm = np.empty((max(total, n_frames * BLOCK, 1), channels), np.int16)  # (the fast kernels are tried first: sela_hip.h)
    capi.check(lib.sela_hip_decode(fr.ctypes.data, offs.ctypes.data, n_frames, channels, pcm.ctypes.data))
    return pcm[:total].reshape(n_frames, BLOCK, channels) if standard or largest == 0 else pcm[:total]


def index_samples(frames: np.ndarray, offsets: np.ndarray, channels: int):
    """-> (sample_offsets uint64[n_frames+1], largest samplesPerChannel of the stream)."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    so = np.zeros(n_frames + 1, np.uint64)
    largest = lib.sela_hip_index_samples(fr.ctypes.data, offs.ctypes.data, n_frames, channels, so.ctypes.data)
    return so, int(largest)


def encode_i32(samples: np.ndarray, lossless: bool = False, paired: bool = False):
    """frame::FrameEncoder on data::WavFrame values: samples int32 [n_frames, channels, n] -> (frames uint8[...], offsets).
    lossless: SELA_HIP_ENCODE_LOSSLESS (sela_hip_encode_i32_opt).  paired: sela_hip_encode_paired_i32."""
    lib = capi.lib()
    p = np.ascontiguousarray(samples, dtype=np.int32)
    n_frames, ch, n = p.shape
    cap = int(lib.sela_hip_encode_bound_bytes_n(n_frames, ch, n))
    frames = np.empty(max(cap, 16), np.uint8)
    offs = np.zeros(n_frames + 1, np.uint64)
    if paired:
        capi.check(lib.sela_hip_encode_paired_i32(p.ctypes.data, n_frames, ch, n, frames.ctypes.data, cap, offs.ctypes.data, capi.ENCODE_LOSSLESS if lossless else 0))
    elif lossless:
        capi.check(lib.sela_hip_encode_i32_opt(p.ctypes.data, n_frames, ch, n, frames.ctypes.data, cap, offs.ctypes.data, capi.ENCODE_LOSSLESS))
    else:
        capi.check(lib.sela_hip_encode_i32(p.ctypes.data, n_frames, ch, n, frames.ctypes.data, cap, offs.ctypes.data))
    return frames[: int(offs[n_frames])].copy(), offs


def encode_ragged(channels, lossless: bool = False) -> bytes:
    """frame::FrameEncoder on a data::WavFrame whose channels differ in length: list of int32 arrays -> the frame's bytes.
    lossless: SELA_HIP_ENCODE_LOSSLESS (sela_hip_encode_ragged_i32_opt)."""
    lib = capi.lib()
    chans = [np.ascontiguousarray(c, dtype=np.int32).ravel() for c in channels]
    flat = np.concatenate(chans)
    lengths = np.array([len(c) for c in chans], np.uint32)
    cap = 4 + sum(int(lib.sela_hip_encode_bound_bytes_n(1, 1, len(c))) for c in chans)
    out = np.empty(cap, np.uint8)
    used = C.c_size_t(0)
    if lossless:
        capi.check(lib.sela_hip_encode_ragged_i32_opt(flat.ctypes.data, lengths.ctypes.data, len(chans), out.ctypes.data, cap, C.byref(used), capi.ENCODE_LOSSLESS))
    else:
        capi.check(lib.sela_hip_encode_ragged_i32(flat.ctypes.data, lengths.ctypes.data, len(chans), out.ctypes.data, cap, C.byref(used)))
    return out[: used.value].tobytes()


def decode_i32(frames: np.ndarray, offsets: np.ndarray, channels: int, stride=None):
    """frame::FrameDecoder as it returns: -> list (per frame) of lists (per channel) of int32 arrays."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    if stride is None:
        stride = max(index_samples(fr, offs, channels)[1], 1)
    out = np.zeros((n_frames, channels, stride), np.int32)
    counts = np.zeros((n_frames, channels), np.uint32)
    capi.check(lib.sela_hip_decode_i32(fr.ctypes.data, offs.ctypes.data, n_frames, channels, out.ctypes.data, stride, counts.ctypes.data))
    return [[out[f, c, : int(counts[f, c])].copy() for c in range(channels)] for f in range(n_frames)]


def index_frames(frames: np.ndarray, n_frames: int, channels: int) -> np.ndarray:
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.zeros(n_frames + 1, np.uint64)
    found = lib.sela_hip_index_frames(fr.ctypes.data, fr.nbytes, n_frames, channels, offs.ctypes.data)
    return offs[: found + 1]


def index_frames_device(payload, max_frames: int, channels: int, workspace=None):
    """sela_hip_index_frames_device: the frames of a payload (uint8 cuda tensor, 4-byte aligned) found on the device,
    asynchronously on the current stream -> (offsets int64 [max_frames + 1], count int32 [1]), both on the device; entries
    [0 .. count] are what index_frames() returns for the same bytes.  workspace: uint8 cuda tensor of at least
    index_workspace_bytes() bytes (default: a new one)."""
    import torch

    assert payload.dtype == torch.uint8 and payload.is_cuda and payload.is_contiguous()
    lib = capi.lib()
    device = payload.device
    if workspace is None:
        workspace = torch.empty(int(lib.sela_hip_index_workspace_bytes(payload.numel(), max_frames)), dtype=torch.uint8, device=device)
    offsets = torch.empty(max_frames + 1, dtype=torch.int64, device=device)
    count = torch.empty(1, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    capi.check(lib.sela_hip_index_frames_device(payload.data_ptr(), payload.numel(), max_frames, channels, offsets.data_ptr(),
                                                count.data_ptr(), workspace.data_ptr(), workspace.numel(), stream))
    return offsets, count


def index_workspace_bytes(payload_bytes: int, max_frames: int) -> int:
    return int(capi.lib().sela_hip_index_workspace_bytes(payload_bytes, max_frames))


# struct sela_hip_salvaged (include/sela_hip.h): 24 bytes per taken frame
SALVAGED_DTYPE = np.dtype([("offset", "<u8"), ("skipped_before", "<u8"), ("bytes", "<u4"), ("reserved", "<u4")])


def salvage_frames(payload: np.ndarray, channels: int, max_frames=None, unaligned: bool = False):
    """sela_hip_salvage_frames on a numpy array: the frames of a damaged payload, walked on the host (no device needed;
    DESIGN.md 5.30) -> (records SALVAGED_DTYPE [frames taken], totals uint64 [4]: frames taken, records with a gap in front,
    the sum of their bytes, the end of the last one).  max_frames: the cap (default: as many as the bytes could hold).
    unaligned: sela_hip_salvage_frames_unaligned, frames at any byte offset."""
    lib = capi.lib()
    body = np.ascontiguousarray(payload, dtype=np.uint8)
    if max_frames is None:
        max_frames = body.nbytes // (4 + 12 * max(channels, 1))
    records = np.zeros(max_frames, SALVAGED_DTYPE)
    totals = np.zeros(4, np.uint64)
    walk = lib.sela_hip_salvage_frames_unaligned if unaligned else lib.sela_hip_salvage_frames
    found = walk(body.ctypes.data, body.nbytes, max_frames, channels, records.ctypes.data, totals.ctypes.data)
    return records[:found], totals


def salvage_workspace_bytes(payload_bytes: int, max_frames: int, unaligned: bool = False) -> int:
    lib = capi.lib()
    sized = lib.sela_hip_salvage_unaligned_workspace_bytes if unaligned else lib.sela_hip_salvage_workspace_bytes
    return int(sized(payload_bytes, max_frames))


class Salvager:
    """sela_hip_salvage_frames_device / sela_hip_salvage_payload_device: the frames of a damaged .sela payload found on the
    device, past positions where the index stops, and copied back to back.  Owns its records, totals, frame
    offsets, compacted payload and workspace on the current device (or `device`), sized once for payloads of up to
    max_payload_bytes; every call is asynchronous on the current stream and overwrites them -- so it can be captured into a
    graph.  unaligned: the *_unaligned_device calls, frames at any byte offset."""

    def __init__(self, max_payload_bytes: int, max_frames: int, channels: int, device=None, unaligned: bool = False):
        import torch

        self.lib = capi.lib()
        self.unaligned = bool(unaligned)
        self._frames_call = self.lib.sela_hip_salvage_frames_unaligned_device if unaligned else self.lib.sela_hip_salvage_frames_device
        self._payload_call = self.lib.sela_hip_salvage_payload_unaligned_device if unaligned else self.lib.sela_hip_salvage_payload_device
        self.max_payload_bytes, self.max_frames, self.channels = int(max_payload_bytes), int(max_frames), int(channels)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        # the records as int64 [max_frames, 3]: offset, skipped_before, bytes | reserved << 32; the totals as int64 [4]
        self.salvaged = torch.zeros((self.max_frames, 3), dtype=torch.int64, device=self.device)
        self.totals = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.frame_offsets = torch.zeros(self.max_frames + 1, dtype=torch.int64, device=self.device)
        self.out = torch.zeros(self.max_payload_bytes // 4 * 4, dtype=torch.uint8, device=self.device)
        self.workspace = torch.empty(salvage_workspace_bytes(self.max_payload_bytes, self.max_frames, self.unaligned), dtype=torch.uint8, device=self.device)

    def _payload_ok(self, payload) -> None:
        import torch

        assert payload.dtype == torch.uint8 and payload.is_cuda and payload.is_contiguous() and payload.device == self.device
        assert payload.numel() <= self.max_payload_bytes, "payload larger than the salvager was sized for"

    def frames(self, payload):
        """payload: uint8 cuda tensor (4-byte aligned) -> (records int64 [max_frames, 3], totals int64 [4]), views of the
        salvager's own buffers: records up to totals[0] are the walk's (records(): as SALVAGED_DTYPE)."""
        import torch

        self._payload_ok(payload)
        capi.check(self._frames_call(
            payload.data_ptr(), payload.numel(), self.max_frames, self.channels, self.salvaged.data_ptr(), self.totals.data_ptr(),
            self.workspace.data_ptr(), self.workspace.numel(), torch.cuda.current_stream(self.device).cuda_stream))
        return self.salvaged, self.totals

    def payload(self, payload, out=None):
        """The walk, then the taken frames copied back to back into `out` (uint8 cuda tensor, 4-byte aligned, apart from the
        payload; default: the salvager's own, which holds any payload it was sized for) -> (out, frame offsets int64
        [max_frames + 1], records, totals): out[: totals[2]] and offsets[: totals[0] + 1] are ready for every call that takes
        frames with their offsets.  A frame that ends beyond out's size is counted but neither it nor any behind it is written."""
        import torch

        self._payload_ok(payload)
        if out is None:
            out = self.out
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
        capi.check(self._payload_call(
            payload.data_ptr(), payload.numel(), self.max_frames, self.channels, out.data_ptr(), out.numel(), self.frame_offsets.data_ptr(),
            self.salvaged.data_ptr(), self.totals.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
            torch.cuda.current_stream(self.device).cuda_stream))
        return out, self.frame_offsets, self.salvaged, self.totals

    def records(self) -> np.ndarray:
        """Waits for the last call -> a host copy of the records it took, as SALVAGED_DTYPE [totals[0]]."""
        found = int(self.totals.cpu()[0])
        host = np.ascontiguousarray(self.salvaged[:found].cpu().numpy())
        return host.view(SALVAGED_DTYPE).reshape(found)


@dataclass
class SelaPayload:
    """A .sela file's payload on the device, and what its 15-byte header says."""
    payload: "torch.Tensor"  # uint8 [payload bytes], 4-byte aligned
    channels: int
    max_frames: int          # numFrames of the header
    sample_rate: int
    bits_per_sample: int


def read_sela_payload(path, device) -> SelaPayload:
    """Parse the 15-byte .sela header on the host ('SeLa', u32 rate, u16 bits, u8 channels, u32 frames: src/file/sela_file.cpp:
    28-47) and upload the bytes after it into a new device tensor (device allocations are aligned far beyond 4 bytes)."""
    import struct

    import torch

    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 15 or data[:4] != b"SeLa":
        raise ValueError(f"{path}: not a .sela file")
    rate, bits, channels, frames = struct.unpack_from("<IHBI", data, 4)
    body = np.frombuffer(data, np.uint8, offset=15)
    payload = torch.from_numpy(body.copy()).to(device)
    return SelaPayload(payload, channels, frames, rate, bits)


# ---- the stages on their own (sela_hip_lpc_* / sela_hip_rice_*: the reference's L1 classes, batched) -----------------------
def lpc_encode(samples: np.ndarray):
    """samples: int32 [n_blocks, len] -> (order int32[n], q int32[n, 100] (first order[i] entries valid), residues int32[n, len]).
    len = 2048 is sela_hip_lpc_encode (the frame kernels' analysis), any other length sela_hip_lpc_encode_n."""
    lib = capi.lib()
    s = np.ascontiguousarray(samples, dtype=np.int32)
    n = s.shape[0]
    assert s.ndim == 2
    length = s.shape[1]
    order, q, res = np.zeros(n, np.int32), np.full((n, 100), 0x5A5A5A5A, np.int32), np.zeros((n, length), np.int32)
    if length == BLOCK:
        capi.check(lib.sela_hip_lpc_encode(C.c_void_p(s.ctypes.data), n, C.c_void_p(order.ctypes.data), C.c_void_p(q.ctypes.data), C.c_void_p(res.ctypes.data)))
    else:
        capi.check(lib.sela_hip_lpc_encode_n(C.c_void_p(s.ctypes.data), n, length, C.c_void_p(order.ctypes.data), C.c_void_p(q.ctypes.data), C.c_void_p(res.ctypes.data)))
    return order, q, res


def lpc_encode_n(samples: np.ndarray):
    """Always the any-length kernels (also for 2048)."""
    lib = capi.lib()
    s = np.ascontiguousarray(samples, dtype=np.int32)
    n, length = s.shape
    order, q, res = np.zeros(n, np.int32), np.full((n, 100), 0x5A5A5A5A, np.int32), np.zeros((n, length), np.int32)
    capi.check(lib.sela_hip_lpc_encode_n(C.c_void_p(s.ctypes.data), n, length, C.c_void_p(order.ctypes.data), C.c_void_p(q.ctypes.data), C.c_void_p(res.ctypes.data)))
    return order, q, res


def lpc_decode_n(order: np.ndarray, q: np.ndarray, residues: np.ndarray, want_coefficients: bool = False):
    """sela_hip_lpc_decode_n: residues int32 [n_blocks, len] of any length."""
    lib = capi.lib()
    o = np.ascontiguousarray(order, dtype=np.int32)
    n = o.shape[0]
    qq = np.ascontiguousarray(q, dtype=np.int32).reshape(n, 100)
    r = np.ascontiguousarray(residues, dtype=np.int32).reshape(n, -1)
    out = np.zeros_like(r)
    coefs = np.zeros((n, 101), np.int64) if want_coefficients else None
    capi.check(lib.sela_hip_lpc_decode_n(C.c_void_p(o.ctypes.data), C.c_void_p(qq.ctypes.data), C.c_void_p(r.ctypes.data), n, r.shape[1],
                                         C.c_void_p(out.ctypes.data), C.c_void_p(coefs.ctypes.data) if coefs is not None else None))
    return (out, coefs) if want_coefficients else out


def lpc_decode(order: np.ndarray, q: np.ndarray, residues: np.ndarray, want_coefficients: bool = False):
    """The inverse: -> samples int32 [n_blocks, 2048] (and, if asked, the Q35 predictors int64 [n_blocks, 101])."""
    lib = capi.lib()
    o = np.ascontiguousarray(order, dtype=np.int32)
    n = o.shape[0]
    qq = np.ascontiguousarray(q, dtype=np.int32).reshape(n, 100)
    r = np.ascontiguousarray(residues, dtype=np.int32).reshape(n, BLOCK)
    out = np.zeros((n, BLOCK), np.int32)
    coefs = np.zeros((n, 101), np.int64) if want_coefficients else None
    capi.check(lib.sela_hip_lpc_decode(C.c_void_p(o.ctypes.data), C.c_void_p(qq.ctypes.data), C.c_void_p(r.ctypes.data), n, C.c_void_p(out.ctypes.data),
                                       C.c_void_p(coefs.ctypes.data) if coefs is not None else None))
    return (out, coefs) if want_coefficients else out


def rice_encode(streams):
    """streams: list of int32 arrays -> list of (k, words uint32[...]) as rice::RiceEncoder gives them."""
    lib = capi.lib()
    n = len(streams)
    vals = [np.ascontiguousarray(v, dtype=np.int32).ravel() for v in streams]
    voff = np.zeros(n + 1, np.uint64)
    voff[1:] = np.cumsum([len(v) for v in vals])
    flat = np.concatenate(vals) if n and voff[n] else np.zeros(0, np.int32)
    # room: a codeword is at most 1 + 19 + (|value| << 1 >> 19) bits... sized by a first call that only asks for the counts
    woff = np.zeros(n + 1, np.uint64)
    k, counts = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rc = lib.sela_hip_rice_encode(C.c_void_p(flat.ctypes.data), C.c_void_p(voff.ctypes.data), n, C.c_void_p(k.ctypes.data), C.c_void_p(counts.ctypes.data),
                                  None, C.c_void_p(woff.ctypes.data))
    if rc not in (capi.OK, -4):
        capi.check(rc)
    woff[1:] = np.cumsum(counts.astype(np.uint64))
    words = np.zeros(int(woff[n]), np.uint32)
    capi.check(lib.sela_hip_rice_encode(C.c_void_p(flat.ctypes.data), C.c_void_p(voff.ctypes.data), n, C.c_void_p(k.ctypes.data), C.c_void_p(counts.ctypes.data),
                                        C.c_void_p(words.ctypes.data), C.c_void_p(woff.ctypes.data)))
    return [(int(k[i]), words[int(woff[i]): int(woff[i + 1])].copy()) for i in range(n)]


def rice_decode(streams):
    """streams: list of (k, words uint32 array, count) -> list of int32 arrays (rice::RiceDecoder)."""
    lib = capi.lib()
    n = len(streams)
    ws = [np.ascontiguousarray(w, dtype=np.uint32).ravel() for _, w, _ in streams]
    woff, voff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    woff[1:] = np.cumsum([len(w) for w in ws])
    voff[1:] = np.cumsum([c for _, _, c in streams])
    flat = np.concatenate(ws) if n and woff[n] else np.zeros(0, np.uint32)
    k = np.array([kk for kk, _, _ in streams], np.uint32)
    out = np.zeros(int(voff[n]), np.int32)
    capi.check(lib.sela_hip_rice_decode(C.c_void_p(flat.ctypes.data), C.c_void_p(woff.ctypes.data), C.c_void_p(k.ctypes.data), C.c_void_p(voff.ctypes.data), n,
                                        C.c_void_p(out.ctypes.data)))
    return [out[int(voff[i]): int(voff[i + 1])].copy() for i in range(n)]


# ---- packed 3- / 4-byte PCM: what a 24- or 32-bit WAV's data chunk holds ------------------------------------------
def _pcm_args_ok(torch, t) -> bool:
    return t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous()


def pcm_unpack(pcm, n_frames: int, channels: int, samples_per_channel: int, bytes_per_sample: int, out=None):
    """sela_hip_pcm_unpack_device on the current stream: pcm uint8 cuda tensor, little-endian interleaved
    [n_frames][samples_per_channel][channels] of bytes_per_sample (3 or 4) bytes -> int32 [n_frames, channels, samples_per_channel]
    (`out`, or a new tensor), sign-extended: what Encoder32 and Verifier32 take."""
    import torch

    assert _pcm_args_ok(torch, pcm)
    if out is None:
        out = torch.empty((n_frames, channels, samples_per_channel), dtype=torch.int32, device=pcm.device)
    assert out.dtype == torch.int32 and out.is_cuda and out.is_contiguous()
    capi.check(capi.lib().sela_hip_pcm_unpack_device(pcm.data_ptr(), bytes_per_sample, n_frames, channels, samples_per_channel, out.data_ptr(),
                                                     torch.cuda.current_stream(pcm.device).cuda_stream))
    return out


def pcm_pack(samples, counts, sample_offsets, bytes_per_sample: int, out, status):
    """sela_hip_pcm_pack_device on the current stream: Decoder32's outputs (samples int32 [n_frames, channels, stride], counts int32
    [n_frames, channels], sample_offsets int64 [n_frames + 1]) -> frame f interleaved at byte sample_offsets[f] * channels *
    bytes_per_sample of `out` (uint8 cuda tensor).  status (int32 [4] cuda tensor; zeroed, or a decode's) takes the frames not
    written ([0], [1]) and the samples beyond a 3-byte container ([3])."""
    import torch

    n_frames, channels, stride = samples.shape
    assert samples.dtype == torch.int32 and samples.is_cuda and samples.is_contiguous() and _pcm_args_ok(torch, out)
    assert counts.is_cuda and counts.is_contiguous() and counts.numel() == n_frames * channels and sample_offsets.numel() == n_frames + 1
    capi.check(capi.lib().sela_hip_pcm_pack_device(samples.data_ptr(), counts.data_ptr(), sample_offsets.data_ptr(), n_frames, channels, stride, bytes_per_sample,
                                                   out.data_ptr(), status.data_ptr(), torch.cuda.current_stream(samples.device).cuda_stream))
    return out


class EncoderPcm:
    """sela_hip_encode_pcm_device: frames of packed 3- or 4-byte interleaved PCM (any samples_per_channel in 1 .. 65535) to .sela
    frames on the device -- the unpack kernel, then Encoder32's launches.  Owns its workspace, frames, offsets and status, as
    Encoder32 does (`capacity` as there: an estimate, check() and needed_bytes() say when it was too small)."""

    def __init__(self, max_frames: int, channels: int, samples_per_channel: int, bytes_per_sample: int, capacity=None, lossless: bool = False, device=None):
        import torch

        self.options = capi.ENCODE_LOSSLESS if lossless else 0
        self.torch = torch
        self.lib = capi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_frames, self.channels, self.n, self.bytes_per_sample = max_frames, channels, samples_per_channel, bytes_per_sample
        if capacity is None:
            capacity = max_frames * ((samples_per_channel * channels * 9) // 2 + channels * 192 + 64)
        self.capacity = max(int(capacity), 4)
        ws = int(self.lib.sela_hip_encode_pcm_workspace_bytes(max_frames, channels, samples_per_channel))
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
            self.frames = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
            self.offsets = torch.zeros(max_frames + 1, dtype=torch.int64, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.n_frames = 0

    def encode(self, pcm, n_frames=None):
        """pcm: uint8 cuda tensor of n_frames * samples_per_channel * channels * bytes_per_sample bytes (n_frames: from its size)
        -> (frames uint8 [capacity], offsets int64 [n_frames + 1], status int32 [4]), the encoder's own buffers."""
        torch = self.torch
        assert _pcm_args_ok(torch, pcm)
        frame_bytes = self.n * self.channels * self.bytes_per_sample
        if n_frames is None:
            assert pcm.numel() % frame_bytes == 0
            n_frames = pcm.numel() // frame_bytes
        assert n_frames <= self.max_frames and pcm.numel() >= n_frames * frame_bytes
        capi.check(self.lib.sela_hip_encode_pcm_device(
            pcm.data_ptr(), self.bytes_per_sample, n_frames, self.channels, self.n, self.options, self.frames.data_ptr(), self.capacity,
            self.offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
            torch.cuda.current_stream(self.device).cuda_stream))
        self.n_frames = n_frames
        return self.frames, self.offsets[: n_frames + 1], self.status

    needed_bytes = Encoder32.needed_bytes
    check = Encoder32.check
    to_host = Encoder32.to_host


class DecoderPcm:
    """sela_hip_decode_pcm_device: a stream of any samplesPerChannel to packed 3- or 4-byte interleaved PCM on the device --
    Decoder32's launches, then the pack kernel.  Owns its output (max_frames * stride * channels * bytes_per_sample bytes), its
    sample offsets, status and workspace; every call is asynchronous on the current stream and overwrites them."""

    def __init__(self, max_frames: int, channels: int, stride: int, bytes_per_sample: int, device=None):
        import torch

        self.torch = torch
        self.lib = capi.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_frames, self.channels, self.stride, self.bytes_per_sample = max_frames, channels, stride, bytes_per_sample
        with torch.cuda.device(self.device):
            self.pcm = torch.empty(max_frames * stride * channels * bytes_per_sample, dtype=torch.uint8, device=self.device)
            self.sample_offsets = torch.zeros(max_frames + 1, dtype=torch.int64, device=self.device)
            self.status = torch.zeros(4, dtype=torch.int32, device=self.device)
            ws = int(self.lib.sela_hip_decode_pcm_workspace_bytes(max_frames, channels, stride))
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)

    def decode(self, frames, offsets, n_frames: int, out=None):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1] -> (pcm uint8, sample_offsets int64
        [n_frames + 1]): frame f at byte sample_offsets[f] * channels * bytes_per_sample of pcm (the decoder's own buffer, or `out`
        with room for n_frames * stride * channels * bytes_per_sample bytes)."""
        torch = self.torch
        assert _pcm_args_ok(torch, frames)
        assert offsets.dtype == torch.int64 and offsets.is_cuda and offsets.is_contiguous() and n_frames <= self.max_frames
        pcm = self.pcm if out is None else out
        assert _pcm_args_ok(torch, pcm) and pcm.numel() >= n_frames * self.stride * self.channels * self.bytes_per_sample
        capi.check(self.lib.sela_hip_decode_pcm_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.bytes_per_sample, pcm.data_ptr(),
            self.sample_offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
            torch.cuda.current_stream(self.device).cuda_stream))
        return pcm, self.sample_offsets[: n_frames + 1]

    def wide_samples(self) -> int:
        """Waits for the last call -> how many samples did not fit a 3-byte container (their low bytes were written)."""
        return int(self.status[3].item()) & 0xFFFFFFFF

    def check(self) -> None:
        """Waits for the last call and raises SelaHipError with the code sela_hip_decode_pcm gives for the same input."""
        capi.check(decode_pcm_status_error(self.status.cpu().numpy()))


def decode_pcm_status_error(status) -> int:
    """sela_hip_decode_pcm_status_error on a host copy of four status words -> the host call's code ([3] is informational)."""
    st = np.ascontiguousarray(np.asarray(status).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    assert st.shape == (4,)
    return int(capi.lib().sela_hip_decode_pcm_status_error(st.ctypes.data))


def encode_pcm_host(pcm: np.ndarray, channels: int, samples_per_channel: int, bytes_per_sample: int, lossless: bool = False):
    """sela_hip_encode_pcm: packed bytes (uint8, whole frames of samples_per_channel * channels * bytes_per_sample) on the host
    -> (frames uint8, offsets uint64 [n_frames + 1])."""
    pcm = np.ascontiguousarray(pcm, dtype=np.uint8).reshape(-1)
    frame_bytes = samples_per_channel * channels * bytes_per_sample
    assert frame_bytes and pcm.size % frame_bytes == 0
    n_frames = pcm.size // frame_bytes
    lib = capi.lib()
    cap = n_frames * ((samples_per_channel * channels * 9) // 2 + channels * 192 + 64)
    for capacity in (cap, int(lib.sela_hip_encode_pcm_bound_bytes(n_frames, channels, samples_per_channel, bytes_per_sample))):
        frames = np.empty(max(capacity, 4), dtype=np.uint8)
        offsets = np.zeros(n_frames + 1, dtype=np.uint64)
        rc = lib.sela_hip_encode_pcm(pcm.ctypes.data, bytes_per_sample, n_frames, channels, samples_per_channel, capi.ENCODE_LOSSLESS if lossless else 0,
                                     frames.ctypes.data, frames.size, offsets.ctypes.data)
        if rc != -4:
            break
    capi.check(rc)
    return frames[: int(offsets[-1])].copy(), offsets


class WholeEncoderPcm(_WholeEncode):
    """sela_hip_encode_whole_pcm_device: a whole track of up to max_samples samples per channel from packed 3- or 4-byte interleaved
    PCM, its tail kept in a long last frame.  Owns its workspace, frames, offsets and status, as WholeEncoder
    does; `capacity` (bytes of frames) defaults to EncoderPcm's estimate -- check() and needed_bytes() say when it was too small."""

    def __init__(self, max_samples: int, channels: int, bytes_per_sample: int, lossless: bool = False, capacity=None, device=None):
        self._bounds(max_samples, channels, lossless, device)
        self.bytes_per_sample = int(bytes_per_sample)
        if capacity is None:
            capacity = (self.max_samples * channels * 9) // 2 + self.max_frames * (channels * 192 + 64)
        self._allocate(capacity, self.lib.sela_hip_encode_whole_pcm_workspace_bytes(self.max_samples, channels))

    def encode(self, pcm, n_samples=None):
        """pcm: uint8 cuda tensor of n_samples * channels * bytes_per_sample bytes (n_samples: from its size) -> (frames uint8
        [capacity], offsets int64 [frames + 1], status int32 [4]), the encoder's own buffers."""
        torch = self.torch
        assert _pcm_args_ok(torch, pcm)
        value_bytes = self.channels * self.bytes_per_sample
        if n_samples is None:
            assert pcm.numel() % value_bytes == 0
            n_samples = pcm.numel() // value_bytes
        assert n_samples <= self.max_samples and pcm.numel() >= n_samples * value_bytes
        capi.check(self.lib.sela_hip_encode_whole_pcm_device(
            pcm.data_ptr(), self.bytes_per_sample, n_samples, self.channels, self.options, self.frames.data_ptr(), self.capacity, self.offsets.data_ptr(),
            self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), torch.cuda.current_stream(self.device).cuda_stream))
        return self._encoded(n_samples)

    needed_bytes = Encoder32.needed_bytes


def encode_whole_pcm_host(pcm: np.ndarray, channels: int, bytes_per_sample: int, lossless: bool = False):
    """sela_hip_encode_whole_pcm: a whole track's packed bytes (uint8, n_samples * channels * bytes_per_sample of them) on the host
    -> (frames uint8, offsets uint64 [frames + 1]); the tail is kept in a long last frame."""
    pcm = np.ascontiguousarray(pcm, dtype=np.uint8).reshape(-1)
    value_bytes = channels * bytes_per_sample
    assert value_bytes and pcm.size % value_bytes == 0
    n_samples = pcm.size // value_bytes
    lib = capi.lib()
    n_frames = int(lib.sela_hip_whole_frames(n_samples))
    estimate = (n_samples * channels * 9) // 2 + n_frames * (channels * 192 + 64)
    for capacity in (estimate, int(lib.sela_hip_encode_whole_pcm_bound_bytes(n_samples, channels, bytes_per_sample))):
        frames = np.empty(max(capacity, 4), dtype=np.uint8)
        offsets = np.zeros(n_frames + 1, dtype=np.uint64)
        rc = lib.sela_hip_encode_whole_pcm(pcm.ctypes.data, bytes_per_sample, n_samples, channels, capi.ENCODE_LOSSLESS if lossless else 0, frames.ctypes.data,
                                           frames.size, offsets.ctypes.data)
        if rc != -4:
            break
    capi.check(rc)
    return frames[: int(offsets[-1])].copy(), offsets


def decode_pcm_host(frames: np.ndarray, offsets: np.ndarray, channels: int, bytes_per_sample: int):
    """sela_hip_decode_pcm -> (pcm uint8: the stream's samples interleaved, bytes_per_sample bytes each; wide: the samples that
    did not fit a 3-byte container)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = offsets.size - 1
    total = int(index_samples(frames, offsets, channels)[0][-1]) if n_frames else 0
    pcm = np.empty(max(total * channels * bytes_per_sample, 1), dtype=np.uint8)
    wide = C.c_uint32(0)
    capi.check(capi.lib().sela_hip_decode_pcm(frames.ctypes.data, offsets.ctypes.data, n_frames, channels, bytes_per_sample, pcm.ctypes.data,
                                              total * channels * bytes_per_sample, C.addressof(wide)))
    return pcm[: total * channels * bytes_per_sample], int(wide.value)


class DigesterPcm(_DeviceCall):
    """sela_hip_digest_pcm_device: the CRC-32 (zlib.crc32) of the packed 3- or 4-byte PCM DecoderPcm.decode would write, per frame
    and for the whole track, on the device -- Digester for the 24- and 32-bit family.  Owns its records, its two
    track words and its workspace on the current device (or `device`); every call is asynchronous on the current stream, one serial
    chain, and overwrites them -- so it can be captured into a graph.  No PCM is written; the status words are DecoderPcm's."""

    _call, _judge = "digest_pcm", staticmethod(decode_pcm_status_error)
    _own_count = False  # status[2] stays the largest samplesPerChannel, as DecoderPcm leaves it
    fallback_frames = _DeviceCall._fallback_frames

    def __init__(self, max_frames: int, channels: int, stride: int, bytes_per_sample: int, device=None):
        self.bytes_per_sample = bytes_per_sample
        super().__init__(max_frames, channels, stride, device)

    def _allocate(self, torch) -> None:
        # the records as int64 [max_frames]: crc32 | samples << 32; the track: [crc32, bytes]
        self.digests = torch.zeros(self.max_frames, dtype=torch.int64, device=self.device)
        self.track = torch.zeros(2, dtype=torch.int64, device=self.device)

    def digest(self, frames, offsets, n_frames: int):
        """frames: uint8 cuda tensor (4-byte aligned), offsets: int64 cuda tensor [n_frames + 1] -> (records int64 [n_frames],
        track int64 [2]: the CRC-32 of all frames' bytes and their number), views of the digester's own buffers (records(): as
        DIGEST_DTYPE)."""
        self._frames_ok(frames, offsets, n_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_digest_pcm_device(
            frames.data_ptr(), offsets.data_ptr(), n_frames, self.channels, self.stride, self.bytes_per_sample, self.digests.data_ptr(),
            self.track.data_ptr(), self.sample_offsets.data_ptr(), self.status.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), stream))
        return self.digests[:n_frames], self.track

    def digest_payload(self, payload, max_frames=None):
        """Index and digest a .sela payload (uint8 cuda tensor, 4-byte aligned) in one asynchronous call; the frame count never
        leaves the device.  -> (records [max_frames], track [2], count int32 [1]): records up to count[0] are the stream's, the
        track covers those.  The workspace grows to the largest payload seen (make one call before capturing)."""
        max_frames = self._payload_ok(payload, max_frames)
        stream = self._stream()
        capi.check(self.lib.sela_hip_digest_payload_pcm_device(
            payload.data_ptr(), payload.numel(), max_frames, self.channels, self.stride, self.bytes_per_sample, self.digests.data_ptr(),
            self.track.data_ptr(), self.sample_offsets.data_ptr(), self.frame_offsets.data_ptr(), self.count.data_ptr(), self.status.data_ptr(),
            self.payload_workspace.data_ptr(), self.payload_workspace.numel(), stream))
        return self.digests[:max_frames], self.track, self.count

    records = staticmethod(Digester.records)
    track_words = Digester.track_words

    def wide_samples(self) -> int:
        """Waits for the last call -> how many samples of digested frames did not fit a 3-byte container (their low bytes were digested)."""
        return int(self.status[3].item()) & 0xFFFFFFFF


def digest_pcm_host(frames: np.ndarray, offsets: np.ndarray, channels: int, bytes_per_sample: int):
    """sela_hip_digest_pcm on numpy arrays -> (records DIGEST_DTYPE [n_frames], the track's CRC-32, its bytes, the samples beyond a
    3-byte container)."""
    lib = capi.lib()
    fr = np.ascontiguousarray(frames, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_frames = len(offs) - 1
    out = np.zeros(n_frames, DIGEST_DTYPE)
    crc, total, wide = np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    capi.check(lib.sela_hip_digest_pcm(fr.ctypes.data, offs.ctypes.data, n_frames, channels, bytes_per_sample, out.ctypes.data, crc.ctypes.data,
                                       total.ctypes.data, wide.ctypes.data))
    return out, int(crc[0]), int(total[0]), int(wide[0])
