"""The consumers of tail_store_list (sela_tail_store.h) -- k_whole_store and k_tailwin_store for the 16-bit long last frame,
k_tail32_store for the 32-bit one, k_window32_store for the 32-bit windows of 2048-sample frames -- on subframe layouts no
encoder writes: subframes out of channel order, a difference in front of its parent, a parent with the higher channel number,
two differences under one parent, parent - difference beyond int16, and a chain in stream order (a difference under a
difference that stands in front of it), which the list resolves as the reference does.

Streams come from topology_cases.py (tailed_stream: two 2048-sample frames and a last frame of 2049, 2825 or 4095 samples;
accepted_stream for the 32-bit windows).  Every expectation is the CPU oracle's decode, pinned to the reference by
test_oracle_topologies.py: its int16 PCM for the 16-bit calls, its int32 samples for the 32-bit ones, where
parent - difference beyond int16 is kept and not wrapped.  Never another GPU call; only the flag words of a chain frame are
compared with sela_hip_decode_n_device's on that frame alone.  All comparisons are exact."""
import functools

import numpy as np
import pytest

import test_gpu_decode_whole as twh
import test_gpu_decode_windows_i32 as t32
import test_gpu_decode_windows_i32_whole as t32w
import test_gpu_decode_windows_whole as tww
import topology_cases as tc
import wide_cases as wc
from gpu_common import gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from test_gpu_decode_windows import as_format as as_format16
from test_gpu_decode_windows import same_bits
from test_gpu_verify_device import _decode_n

pytestmark = pytest.mark.gpu

B = tc.N
I16, F32 = capi.WINDOW_I16_INTERLEAVED, capi.WINDOW_F32_PLANAR
I32, PCM32, PCM24 = t32.I32, t32.PCM32, t32.PCM24
SCALES = (tc.ORDINARY, tc.WRAPPING)
TAILS = [(ch, n_last) for ch in tc.TAIL_CHANNELS for n_last in tc.TAIL_LENGTHS]
CHAINS = [ch for ch in tc.TAIL_CHANNELS if ch >= 3]
CHAIN_LENGTH = 2825


class _Table:
    """What the sibling modules' raw device calls ask of a table: the stream on the device, inside 0xA5 guards."""

    def __init__(self, torch, stream, offs, ch):
        self.torch, self.ch, self.n = torch, ch, len(offs) - 1
        self.stream, self.offs = np.array(stream), np.array(offs)
        self.big_frames, self.d_frames = t32.guarded(torch, self.stream)
        self.big_offs, d_offs = t32.guarded(torch, self.offs)
        self.d_offs = d_offs.view(torch.int64)


def _cut(flat, starts, ws):
    """flat: [samples of the stream, ch] -> [windows, ws, ch], zeros behind the stream's end"""
    out = np.zeros((len(starts), ws, flat.shape[1]), flat.dtype)
    for w, start in enumerate(starts):
        seg = flat[start: start + ws]
        out[w, : len(seg)] = seg
    return out


def _tail_batches(s):
    """(starts, length) for a stream of s = 4096 + n_last samples: inside the last frame -- at its first sample, one behind it,
    ending at its last sample, running past it into zeros -- across the seam, in front of it; and one window over everything"""
    ws = 777
    return [([2 * B, 2 * B + 1, s - ws, s - 300, 2 * B - 1, 2 * B - 400, B - 5], ws), ([0], s + 9)]


# ---- the 16-bit long last frame -------------------------------------------------------------------------------------------------------
def _whole(torch, ch, n_last, scale, chain=False):
    stream, offs, want = tc.tailed_stream(ch, n_last, scale, chain)
    s = 2 * B + n_last
    out, n_samples, status = twh.device_call(torch, np.array(stream), np.array(offs), ch, s + 5)
    bad = np.argwhere(out[:s] != want)
    assert n_samples == s and status.tolist() == [0, 0, 0, 3], (scale, n_samples, status)
    assert len(bad) == 0, (scale, len(bad), bad[:6].tolist())
    assert twh.sentinel(out[s:]), "written behind the PCM"


@pytest.mark.parametrize("ch,n_last", TAILS)
def test_the_whole_decode_of_a_stream_with_a_long_last_frame(gpu, ch, n_last):  # noqa: F811
    """sela_hip_decode_whole_device (k_whole_store): all 4096 + n_last samples, a clean status, nothing behind the PCM."""
    for scale in SCALES:
        _whole(gpu, ch, n_last, scale)


@pytest.mark.parametrize("ch", tc.TAIL_CHANNELS)
def test_the_whole_decode_through_the_host_pointer_call(gpu, ch):  # noqa: F811
    stream, offs, want = tc.tailed_stream(ch, 2825, tc.WRAPPING)
    out, n_samples, rc = codec.decode_whole_host(np.array(stream), np.array(offs), ch)
    assert rc == 0 and n_samples == len(want) and np.array_equal(out[:n_samples], want)


def _windows_whole(torch, ch, n_last, scale, chain=False, flags_want=0):
    stream, offs, want = tc.tailed_stream(ch, n_last, scale, chain)
    t = _Table(torch, stream, offs, ch)
    for starts, ws in _tail_batches(len(want)):
        windows = [(s, 0, 3) for s in starts]
        for fmt in (I16, F32):
            out, flags, status = tww.device_call(t, windows, ws, fmt)
            expect = as_format16(_cut(want, starts, ws), fmt)
            assert same_bits(out, expect), (scale, ws, fmt, np.argwhere(out != expect)[:6].tolist())
            assert (flags == flags_want).all() and status.tolist() == [0, 0, 0, 0], (scale, ws, fmt, flags, status)


@pytest.mark.parametrize("ch,n_last", TAILS)
def test_16_bit_windows_into_a_long_last_frame(gpu, ch, n_last):  # noqa: F811
    """sela_hip_decode_windows_whole_device (k_tailwin_store), both formats: slices of the oracle's PCM, zeros beyond S, flags 0."""
    for scale in SCALES:
        _windows_whole(gpu, ch, n_last, scale)


# ---- the 32-bit long last frame -------------------------------------------------------------------------------------------------------
def _windows_i32_whole(torch, ch, n_last, scale, chain=False):
    stream, offs, pcm16 = tc.tailed_stream(ch, n_last, scale, chain)
    want = tc.tailed_stream_i32(ch, n_last, scale, chain)
    assert np.array_equal(want.astype(np.uint32).astype(np.uint16).view(np.int16), pcm16)  # (the int16 PCM is these mod 2^16)
    assert int(np.abs(want.astype(np.int64)).max()) < 1 << 23
    t = _Table(torch, stream, offs, ch)
    for starts, ws in _tail_batches(len(want)):
        windows = [(s, 0, 3) for s in starts]
        for fmt in (I32, PCM24):
            out, flags, status = t32w.device_call(t, windows, ws, fmt, 16)
            expect = t32.as_format(_cut(want, starts, ws), fmt, 16)
            assert same_bits(out, expect), (scale, ws, fmt, np.argwhere(out != expect)[:6].tolist())
            assert not flags.any() and status.tolist() == [0, 0, 0, 0], (scale, ws, fmt, flags, status)


@pytest.mark.parametrize("ch,n_last", TAILS)
def test_32_bit_windows_into_a_long_last_frame(gpu, ch, n_last):  # noqa: F811
    """sela_hip_decode_windows_i32_whole_device (k_tail32_store) on the same streams, sample_bits = 16, planar int32 and packed
    3-byte: the same slices widened -- of the oracle's int32 samples, which at +-300 are the int16 PCM and at +-12000 keep
    parent - difference where the 16-bit calls wrap it."""
    for scale in SCALES:
        _windows_i32_whole(gpu, ch, n_last, scale)


# ---- a chain in stream order as the last frame ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", CHAINS)
def test_a_chain_in_stream_order_as_the_last_frame(gpu, ch):  # noqa: F811
    """Channel 2 under channel 1, itself a difference under channel 0 and in front of it in the stream.  tail_store_list writes
    dependent subframes in subframe order, so channel 1 is final when channel 2 subtracts from it, as in the reference: the
    oracle's PCM, and the flag words sela_hip_decode_n_device reports for the frame decoded alone (none)."""
    for scale in SCALES:
        stream, offs, _ = tc.tailed_stream(ch, CHAIN_LENGTH, scale, chain=True)
        last = np.array(stream[int(offs[2]):])
        _, so, st = _decode_n(gpu, last, np.array([0, len(last)], np.uint64), ch, 4095)
        assert int(so[1]) == CHAIN_LENGTH and int(st[0]) == 0 and int(st[1]) == 0 and int(st[3]) == 2, (scale, st)  # (the any-length combine accepts it)
        _whole(gpu, ch, CHAIN_LENGTH, scale, chain=True)
        _windows_whole(gpu, ch, CHAIN_LENGTH, scale, chain=True, flags_want=int(st[0]))
        _windows_i32_whole(gpu, ch, CHAIN_LENGTH, scale, chain=True)


# ---- 32-bit windows of 2048-sample frames ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames32(key):
    """key: a channel count of topology_cases.accepted_stream, or "chain" (CHAIN_IN_STREAM_ORDER at three channels, +-300 and
    +-12000, the frames test_oracle_topologies.py pins) -> (labels, stream, offsets, channels, oracle int32 [frames * 2048, ch])"""
    o = oracle()
    if key == "chain":
        ch, labels = 3, [f"chain +-{scale}" for scale in SCALES]
        blobs = [wc.frame_bytes(o, tc.subframes(tc.CHAIN_IN_STREAM_ORDER, scale, 20261017 + scale)) for scale in SCALES]
    else:
        ch = key
        cs, stream, offs, _ = tc.accepted_stream(ch)
        labels = [c[0] for c in cs]
        blobs = [stream[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(len(cs))]
    parts = []
    for blob in blobs:
        dec, used = o.frame_decode_i32(blob, ch)
        assert used == len(blob) and all(len(d) == B for d in dec)
        parts.append(np.stack(dec, axis=1))
    want = np.concatenate(parts)
    stream = np.frombuffer(b"".join(blobs), np.uint8).copy()
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    for a in (stream, offs, want):
        a.setflags(write=False)
    return labels, stream, offs, ch, want


def _window32_batches(n):
    """as test_gpu_fused_topologies: one window per frame, three samples across every seam, the whole stream"""
    return [([f * B for f in range(n)], B), ([f * B + B - 1 for f in range(n - 1)], 3), ([0], n * B)]


@pytest.mark.parametrize("segments", [False, True], ids=["plan", "by segments"])
@pytest.mark.parametrize("key", [2, 3, 5, 8, "chain"])
def test_32_bit_windows_of_2048_sample_frames(gpu, key, segments):  # noqa: F811
    """sela_hip_decode_windows_i32_device (k_window32_decode / k_window32_store): the oracle's frame_decode_i32 per frame, in planar
    and interleaved int32 and packed 3-byte -- on the bytes of test_gpu_fused_topologies.py, with the opposite expectation where
    parent - difference leaves int16.  segments: sela_hip_debug_standard_first(2), every subframe parsed by segments."""
    labels, stream, offs, ch, want = _frames32(key)
    n = len(labels)
    wrapping = [f for f in range(n) if f"+-{tc.WRAPPING}" in labels[f]]
    assert any(int(np.abs(want[f * B: (f + 1) * B].astype(np.int64)).max()) > 32768 for f in wrapping) and int(np.abs(want.astype(np.int64)).max()) < 1 << 23
    t = _Table(gpu, stream, offs, ch)
    lib = capi.lib()
    if segments:
        lib.sela_hip_debug_standard_first(2)
    try:
        for starts, ws in _window32_batches(n):
            windows = [(s, 0, n) for s in starts]
            for fmt in (I32, PCM32, PCM24):
                out, flags, status = t32.device_call(t, windows, ws, fmt, 24)
                expect = t32.as_format(_cut(want, starts, ws), fmt, 24)
                bad = np.argwhere(out != expect)
                assert same_bits(out, expect), (ws, fmt, len(bad), bad[:6].tolist(), [labels[k] for k in sorted({int(b[0]) for b in bad[:50]})] if ws == B else "")
                assert not flags.any() and status.tolist() == [0, 0, 0, 0], (ws, fmt, flags, status)
    finally:
        if segments:
            lib.sela_hip_debug_standard_first(-1)
