"""The chunk loop of the host-pointer calls (frame_chunks, sela_capi_generic.hip) run more than once: sela_hip_verify,
sela_hip_verify_i32, sela_hip_levels and sela_hip_levels_i32 with sela_hip_debug_pcm_chunk_frames at 1, 2 and 5 frames a chunk.
Without the hook these calls reach a second chunk only with some 768 MB of scratch.

The stream is a whole-track stereo stream (codec.encode_whole_host, lossless) of five frames of 2048 samples and a last frame of
2825: 6 * 2048 + 777 samples, so the sample offsets are no multiple of anything and the stride (2825) is not 2048.  Every forced
chunk size must give exactly what the call gives with the hook at 0 and what its device call gives on the same stream."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import gpu  # noqa: F401
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

CH, FRAMES, LAST = 2, 6, 2048 + 777
N_SAMPLES = 5 * 2048 + LAST
CHUNKS = (1, 2, 5)
UNTOUCHED = 0x5E1A5E1A


def _forced(chunk, call):
    lib = capi.lib()
    lib.sela_hip_debug_pcm_chunk_frames(chunk)
    try:
        return call()
    finally:
        lib.sela_hip_debug_pcm_chunk_frames(0)


def _planar(pcm, so, stride):
    """[total, ch] -> int32 [frames, ch, stride] and the lengths uint32 [frames, ch], as decode_i32 fills them"""
    n = len(so) - 1
    out, lengths = np.zeros((n, pcm.shape[1], stride), np.int32), np.zeros((n, pcm.shape[1]), np.uint32)
    for f in range(n):
        part = pcm[int(so[f]): int(so[f + 1])]
        out[f, :, : len(part)] = part.T
        lengths[f] = len(part)
    return out, lengths


class _Stream:
    """The stream, its originals with one sample flipped in frame 0 and one in the last frame, and what the device calls and the
    host calls at chunk size 0 return for it: computed once, never changed."""

    def __init__(self, torch, widen):
        pcm = synth_frames(FRAMES + 1, CH, 77).reshape(-1, CH)[:N_SAMPLES]
        self.frames, self.offs = codec.encode_whole_host(pcm, lossless=True)
        assert len(self.offs) - 1 == FRAMES
        self.so = np.array([0] + [first + length for first, length in codec.whole_frames(N_SAMPLES)], np.uint64)
        assert np.diff(self.so).tolist() == [2048] * 5 + [LAST]
        back = codec.decode_i32(self.frames, self.offs, CH)
        assert all(np.array_equal(np.stack(back[f]).T, pcm[int(self.so[f]): int(self.so[f + 1])]) for f in range(FRAMES))
        values = pcm.astype(np.int32)
        if widen:  # the same track in a 24-bit container: << 8, plus a low byte
            values = (values << 8) + (np.arange(values.size, dtype=np.int32).reshape(values.shape) * 37 & 0xFF)
            planar, _ = _planar(values, self.so, LAST)
            self.frames, self.offs = _encode_ragged_frames(planar, self.so)
            back = codec.decode_i32(self.frames, self.offs, CH)
            assert all(np.array_equal(np.stack(back[f]).T, values[int(self.so[f]): int(self.so[f + 1])]) for f in range(FRAMES))
        self.values = values
        # one sample flipped in frame 0 (sample 5, channel 1) and one in the last frame (its sample 2800, channel 0)
        changed = values.copy()
        changed[5, 1] ^= 1
        changed[int(self.so[FRAMES - 1]) + 2800, 0] ^= 1
        self.samples, self.lengths = _planar(changed, self.so, LAST)
        self.pcm16 = None if widen else changed.astype(np.int16)
        self.want_counts = [1, 0, 0, 0, 0, 1]
        self.want_first16 = [5 * CH + 1] + [0xFFFFFFFF] * 4 + [2800 * CH]
        self.want_first32 = [LAST + 5] + [0xFFFFFFFF] * 4 + [2800]
        # the device calls
        d_frames = torch.zeros((len(self.frames) + 3) // 4 * 4, dtype=torch.uint8, device="cuda")
        d_frames[: len(self.frames)].copy_(torch.from_numpy(self.frames))
        d_offs = torch.from_numpy(self.offs.view(np.int64).copy()).cuda()
        v32 = codec.Verifier32(FRAMES, CH, LAST)
        c, f = v32.verify(d_frames, d_offs, FRAMES, torch.from_numpy(self.samples).cuda(), torch.from_numpy(self.lengths.view(np.int32)).cuda())
        v32.check()
        self.dev_verify32 = (c.cpu().numpy().view(np.uint32).copy(), f.cpu().numpy().view(np.uint32).copy(), v32.lossy_frames())
        l32 = codec.Leveler32(FRAMES, CH, LAST)
        self.dev_levels32 = codec.Leveler32.records(l32.measure(d_frames, d_offs, FRAMES))
        l32.check()
        if not widen:
            v16 = codec.Verifier(FRAMES, CH, LAST)
            c, f = v16.verify(d_frames, d_offs, FRAMES, torch.from_numpy(self.pcm16).cuda())
            v16.check()
            self.dev_verify16 = (c.cpu().numpy().view(np.uint32).copy(), f.cpu().numpy().view(np.uint32).copy(), v16.lossy_frames())
            l16 = codec.Leveler(FRAMES, CH, LAST)
            self.dev_levels16 = codec.Leveler.records(l16.measure(d_frames, d_offs, FRAMES))
            l16.check()

    def verify16(self):
        return codec.verify_host(self.frames, self.offs, CH, self.pcm16)

    def verify32(self):
        return codec.verify_i32(self.frames, self.offs, CH, self.samples, self.lengths)

    def levels16(self):
        return codec.levels_host(self.frames, self.offs, CH)

    def levels32(self):
        return codec.levels_i32_host(self.frames, self.offs, CH)


def _encode_ragged_frames(planar, so):
    """int32 [frames, ch, stride], frame f so[f + 1] - so[f] samples long -> (frames, offsets): each frame coded on its own"""
    blobs = [codec.encode_ragged([planar[f, c, : int(so[f + 1] - so[f])] for c in range(planar.shape[1])], lossless=True) for f in range(len(so) - 1)]
    offs = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), offs


@pytest.fixture(scope="module")
def track(gpu):  # noqa: F811
    return _Stream(gpu, widen=False)


@pytest.fixture(scope="module")
def track24(gpu):  # noqa: F811
    return _Stream(gpu, widen=True)


def _same_verify(got, want, label):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (label, got, want)


def _same_records(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape
    for name in got.dtype.names:
        assert np.array_equal(got[name], want[name]), (label, name)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_verify_in_chunks(track, chunk):
    whole = track.verify16()
    got = _forced(chunk, track.verify16)
    _same_verify(got, whole, "the hook at 0")
    _same_verify(got, track.dev_verify16, "the device call")
    assert got[0].tolist() == track.want_counts and got[1].tolist() == track.want_first16 and got[2] == 2


@pytest.mark.parametrize("chunk", CHUNKS)
def test_verify_i32_in_chunks(track, chunk):
    whole = track.verify32()
    got = _forced(chunk, track.verify32)
    _same_verify(got, whole, "the hook at 0")
    _same_verify(got, track.dev_verify32, "the device call")
    assert got[0].tolist() == track.want_counts and got[1].tolist() == track.want_first32 and got[2] == 2


@pytest.mark.parametrize("chunk", CHUNKS)
def test_levels_in_chunks(track, chunk):
    whole = track.levels16()
    got = _forced(chunk, track.levels16)
    _same_records(got, whole, "the hook at 0")
    _same_records(got, track.dev_levels16, "the device call")
    assert got["samples"].tolist() == [[2048] * CH] * 5 + [[LAST] * CH] and (got["peak"] > 0).all()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_levels_i32_in_chunks(track, chunk):
    whole = track.levels32()
    got = _forced(chunk, track.levels32)
    _same_records(got, whole, "the hook at 0")
    _same_records(got, track.dev_levels32, "the device call")
    assert got["samples"].tolist() == [[2048] * CH] * 5 + [[LAST] * CH] and (got["peak"] > 0).all()


def test_a_24_bit_track_in_chunks(track24):
    whole_v, whole_l = track24.verify32(), track24.levels32()
    got_v, got_l = _forced(2, lambda: (track24.verify32(), track24.levels32()))
    _same_verify(got_v, whole_v, "the hook at 0")
    _same_verify(got_v, track24.dev_verify32, "the device call")
    assert got_v[0].tolist() == track24.want_counts and got_v[1].tolist() == track24.want_first32 and got_v[2] == 2
    _same_records(got_l, whole_l, "the hook at 0")
    _same_records(got_l, track24.dev_levels32, "the device call")
    assert int(got_l["peak"].max()) > 1 << 16 and got_l["samples"].tolist() == [[2048] * CH] * 5 + [[LAST] * CH]


def test_a_malformed_frame_ends_the_call_at_its_chunk(track):
    """A bad byte at the head of frame 3, two frames a chunk: every call fails with sela_hip_decode_i32's code, -5, and nothing is
    written for the chunk behind it (frames 4 and 5)."""
    lib = capi.lib()
    bad = track.frames.copy()
    bad[int(track.offs[3])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as d:
        codec.decode_i32(bad, track.offs, CH, LAST)
    assert d.value.code == -5
    fr, offs = bad.ctypes.data, track.offs.ctypes.data
    counts, first = np.full(FRAMES, UNTOUCHED, np.uint32), np.full(FRAMES, UNTOUCHED, np.uint32)
    lev16, lev32 = np.full((FRAMES, CH, 3), UNTOUCHED, np.uint64), np.full((FRAMES, CH, 4), UNTOUCHED, np.uint64)
    lossy = C.c_uint32(0)

    def calls():
        out = [lib.sela_hip_verify(fr, offs, FRAMES, CH, track.pcm16.ctypes.data, counts.ctypes.data, first.ctypes.data, C.byref(lossy))]
        assert (counts[4:] == UNTOUCHED).all() and (first[4:] == UNTOUCHED).all()
        counts[:], first[:] = UNTOUCHED, UNTOUCHED
        out.append(lib.sela_hip_verify_i32(fr, offs, FRAMES, CH, LAST, track.samples.ctypes.data, track.lengths.ctypes.data, counts.ctypes.data,
                                           first.ctypes.data, C.byref(lossy)))
        out.append(lib.sela_hip_levels(fr, offs, FRAMES, CH, lev16.ctypes.data))
        out.append(lib.sela_hip_levels_i32(fr, offs, FRAMES, CH, lev32.ctypes.data))
        return out

    assert _forced(2, calls) == [-5, -5, -5, -5]
    assert (counts[4:] == UNTOUCHED).all() and (first[4:] == UNTOUCHED).all()
    assert (lev16[4:] == UNTOUCHED).all() and (lev32[4:] == UNTOUCHED).all()
