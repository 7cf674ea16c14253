"""Packed 3- / 4-byte PCM on the device: k_pcm_unpack / k_pcm_pack alone against numpy, with guard bytes round
every input and output; sela_hip_encode_pcm_device against sela_hip_encode_i32 on the unpacked samples and, per frame, the
reference; sela_hip_decode_pcm_device against the numpy pack of sela_hip_decode_i32's output and the reference's decoder; one
graph capture of both; the host-pointer pair against the device calls.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import _signal, gpu  # noqa: F401
from oracle_lib import oracle, reference
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes of 0xA5 in front of and behind every view (a multiple of 4: the views stay 4-byte aligned)
LENGTHS = [1, 2, 3, 5, 7, 64, 2047, 2048, 2049]
TRAPS = bytes([0x80, 0, 0, 0xFF, 0xFF, 0x7F, 0xFF, 0xFF, 0xFF, 0, 0, 0x80])


def _ref():
    return reference() or oracle()


# ---- the layouts in numpy ---------------------------------------------------------------------------------------------------------
def np_unpack(raw, n_frames, n, channels, b):
    """packed bytes -> int32 [n_frames, channels, n]"""
    v = raw.reshape(n_frames, n, channels, b).astype(np.uint32)
    x = sum(v[..., k] << np.uint32(8 * k) for k in range(b)).astype(np.uint32)
    if b == 3:
        x = (x ^ np.uint32(0x800000)) - np.uint32(0x800000)
    return np.ascontiguousarray(x.astype(np.uint32).view(np.int32).transpose(0, 2, 1))


def np_pack(planar, b):
    """planar int32 [channels, n] -> the frame's packed bytes"""
    u = np.ascontiguousarray(np.asarray(planar, np.int32).T).view(np.uint32)
    return np.stack([(u >> np.uint32(8 * k)).astype(np.uint8) for k in range(b)], axis=-1).reshape(-1)


def pack_interleaved(x, b):
    """int32 [..., n, channels] (interleaved, frames in front) -> packed bytes"""
    u = np.ascontiguousarray(x, np.int32).view(np.uint32)
    return np.stack([(u >> np.uint32(8 * k)).astype(np.uint8) for k in range(b)], axis=-1).reshape(-1)


class Guarded:
    """an exact-size view inside a larger tensor filled with 0xA5"""

    def __init__(self, torch, nbytes, fill=None):
        self.torch, self.nbytes = torch, nbytes
        self.big = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.big[GUARD: GUARD + nbytes]
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)))

    def i32(self, *shape):
        return self.view.view(self.torch.int32).view(*shape) if self.nbytes else self.torch.empty(shape, dtype=self.torch.int32, device="cuda")

    def intact(self):
        g = self.big.cpu().numpy()
        return bool((g[:GUARD] == 0xA5).all() and (g[GUARD + self.nbytes:] == 0xA5).all())

    def numpy(self):
        return self.view.cpu().numpy()


def _random_packed(rng, nbytes):
    raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
    k = min(len(TRAPS), nbytes)
    raw[:k] = np.frombuffer(TRAPS, np.uint8)[:k]
    if nbytes >= 2 * len(TRAPS):
        raw[-len(TRAPS):] = np.frombuffer(TRAPS, np.uint8)
    return raw


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8])
def test_unpack_and_pack_alone(gpu, channels, b):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(100 * channels + b)
    for n in LENGTHS:
        for n_frames in (1, 3):
            raw = _random_packed(rng, n_frames * n * channels * b)
            want = np_unpack(raw, n_frames, n, channels, b)
            src = Guarded(torch, raw.size, raw)
            dst = Guarded(torch, want.size * 4)
            out = codec.pcm_unpack(src.view, n_frames, channels, n, b, out=dst.i32(n_frames, channels, n))
            torch.cuda.synchronize()
            assert src.intact() and dst.intact(), (n, n_frames)
            assert np.array_equal(out.cpu().numpy(), want), (n, n_frames)
            assert np.array_equal(src.numpy(), raw)
            # ... and back: the same samples under a stride of their own
            stride = n + (3 if n % 2 else 0)
            padded = np.full((n_frames, channels, stride), 0x5A5A5A5A, np.int32)
            padded[:, :, :n] = want
            samples = Guarded(torch, padded.size * 4, padded)
            counts = torch.full((n_frames, channels), n, dtype=torch.int32, device="cuda")
            so = torch.arange(n_frames + 1, dtype=torch.int64, device="cuda") * n
            status = torch.zeros(4, dtype=torch.int32, device="cuda")
            back = Guarded(torch, raw.size)
            codec.pcm_pack(samples.i32(n_frames, channels, stride), counts, so, b, back.view, status)
            torch.cuda.synchronize()
            assert samples.intact() and back.intact(), (n, n_frames)
            assert np.array_equal(back.numpy(), raw), (n, n_frames)
            assert status.cpu().tolist() == [0, 0, 0, 0]


def _pack_call(torch, frames, stride, b):
    """frames: list of lists of int32 arrays (a channel each) -> (output bytes, status, guards intact)"""
    n_frames, channels = len(frames), len(frames[0])
    samples = np.full((n_frames, channels, stride), 0x5A5A5A5A, np.int32)
    counts = np.zeros((n_frames, channels), np.int32)
    so = np.zeros(n_frames + 1, np.int64)
    for f, chans in enumerate(frames):
        for c, x in enumerate(chans):
            samples[f, c, : len(x)] = x
            counts[f, c] = len(x)
        so[f + 1] = so[f] + len(chans[0])
    g_samples = Guarded(torch, samples.size * 4, samples)
    out = Guarded(torch, n_frames * stride * channels * b)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    codec.pcm_pack(g_samples.i32(n_frames, channels, stride), torch.from_numpy(counts).cuda(), torch.from_numpy(so).cuda(), b, out.view, status)
    torch.cuda.synchronize()
    return out.numpy(), [int(v) & 0xFFFFFFFF for v in status.cpu().tolist()], out.intact() and g_samples.intact(), so


@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_pack_a_stream_of_mixed_lengths(gpu, channels, b):  # noqa: F811
    rng = np.random.default_rng(7 * channels + b)
    amp = 23 if b == 3 else 31
    frames = [[rng.integers(-(1 << amp), 1 << amp, n).astype(np.int32) for _ in range(channels)] for n in (128, 1000, 2048, 128)]
    got, status, intact, so = _pack_call(gpu, frames, 2048, b)
    want = np.concatenate([np_pack(np.stack(chans), b) for chans in frames])
    assert intact and status == [0, 0, 0, 0]
    assert np.array_equal(got[: want.size], want)
    assert (got[want.size:] == 0xA5).all()  # nothing at or past sample_offsets[n_frames] * channels * bytes


@pytest.mark.parametrize("b", [3, 4])
def test_pack_leaves_a_ragged_frame_alone_and_flags_it(gpu, b):  # noqa: F811
    rng = np.random.default_rng(11 + b)
    mk = lambda n: rng.integers(-(1 << 20), 1 << 20, n).astype(np.int32)  # noqa: E731
    frames = [[mk(301), mk(301), mk(301)], [mk(300), mk(200), mk(300)], [mk(77), mk(77), mk(77)]]
    got, status, intact, so = _pack_call(gpu, frames, 301, b)
    v = 3 * b
    assert intact and status == [capi.FLAG_BAD_FRAME, 1, 0, 0]
    assert codec.decode_pcm_status_error(status) == -5
    assert np.array_equal(got[: 301 * v], np_pack(np.stack(frames[0]), b))
    assert (got[301 * v: 601 * v] == 0xA5).all()  # the ragged frame's place
    assert np.array_equal(got[601 * v: 678 * v], np_pack(np.stack(frames[2]), b))
    assert (got[678 * v:] == 0xA5).all()


def test_pack_counts_what_does_not_fit_three_bytes(gpu):  # noqa: F811
    rng = np.random.default_rng(5)
    frames = [[rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32) for _ in range(2)] for n in (2049, 513)]
    frames[0][0][:4] = [(1 << 23) - 1, 1 << 23, -(1 << 23), -(1 << 23) - 1]  # the edges: in, out, in, out
    wide = sum(int(((x < -(1 << 23)) | (x >= (1 << 23))).sum()) for chans in frames for x in chans)
    got, status, intact, so = _pack_call(gpu, frames, 2049, 3)
    want = np.concatenate([np_pack(np.stack(chans), 3) for chans in frames])
    assert intact and status == [0, 0, 0, wide] and wide > 4000
    assert np.array_equal(got[: want.size], want)  # the low bytes
    got4, status4, intact4, _ = _pack_call(gpu, frames, 2049, 4)
    assert intact4 and status4 == [0, 0, 0, 0]
    assert np.array_equal(got4[: want.size // 3 * 4], np.concatenate([np_pack(np.stack(chans), 4) for chans in frames]))


# ---- 2. / 3. the composed calls ---------------------------------------------------------------------------------------------------
def _music24(n_frames, channels, seed):
    """the synthetic music widened to 24 bits: shifted left 8, the low byte filled with noise -> int32 [n_frames, 2048, channels]"""
    rng = np.random.default_rng(seed)
    pcm = synth_frames(n_frames, channels, seed).astype(np.int32)
    return (pcm << 8) | rng.integers(0, 256, pcm.shape).astype(np.int32)


def _cases():
    rng = np.random.default_rng(2024)
    mono = np.stack([_signal(rng, "tone", 300, 22) for _ in range(2)])[:, :, None]
    three = np.stack([np.stack([_signal(rng, k, 1000, 21) for k in ("tone", "noise", "sparse")], axis=1) for _ in range(2)])
    wide = np.stack([np.stack([_signal(rng, "tone", 700, 27), _signal(rng, "tone", 700, 27)], axis=1) for _ in range(2)])
    return {"music24": (_music24(3, 2, 3), 3), "mono300": (mono, 3), "three1000": (three, 3), "wide28": (wide, 4)}


CASES = _cases()  # name -> (int32 [n_frames, n, channels] interleaved, bytes per sample)
_SHARED = {}


def _expected(name, lossless):
    """codec.encode_i32 on the unpacked samples, once per case"""
    key = (name, lossless)
    if key not in _SHARED:
        x, b = CASES[name]
        planar = np.ascontiguousarray(x.transpose(0, 2, 1))
        _SHARED[key] = (planar,) + tuple(codec.encode_i32(planar, lossless=lossless))
    return _SHARED[key]


def _encode_device(torch, name, lossless, capacity=None):
    x, b = CASES[name]
    n_frames, n, channels = x.shape
    raw = pack_interleaved(x, b)
    enc = codec.EncoderPcm(n_frames, channels, n, b, capacity=capacity, lossless=lossless)
    src = Guarded(torch, raw.size, raw)
    enc.encode(src.view)
    torch.cuda.synchronize()
    assert src.intact()
    return enc, raw


@pytest.mark.parametrize("lossless", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_encode_pcm_device(gpu, name, lossless):  # noqa: F811
    torch = gpu
    planar, want_frames, want_offs = _expected(name, lossless)
    enc, raw = _encode_device(torch, name, lossless)
    frames, offs = enc.to_host()
    assert np.array_equal(offs, want_offs) and np.array_equal(frames, want_frames)
    x, b = CASES[name]
    n_frames, n, channels = x.shape
    if not lossless:
        for f in range(n_frames):
            assert frames[int(offs[f]): int(offs[f + 1])].tobytes() == _ref().frame_encode_i32(planar[f]), f
    else:  # the decode returns the input bytes
        dec = codec.DecoderPcm(n_frames, channels, n, b)
        out = Guarded(torch, n_frames * n * channels * b)
        dec.decode(enc.frames, enc.offsets, n_frames, out=out.view)
        torch.cuda.synchronize()
        dec.check()
        assert out.intact() and np.array_equal(out.numpy(), raw) and dec.wide_samples() == 0
        assert dec.sample_offsets.cpu().tolist() == [f * n for f in range(n_frames + 1)]


def test_encode_pcm_device_with_too_small_a_capacity(gpu):  # noqa: F811
    torch = gpu
    planar, want_frames, want_offs = _expected("music24", False)
    cap = int(want_offs[2]) + 10  # two frames fit, the third does not
    x, b = CASES["music24"]
    raw = pack_interleaved(x, b)
    lib = capi.lib()
    frames = Guarded(torch, cap)
    offsets = torch.zeros(4, dtype=torch.int64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sela_hip_encode_pcm_workspace_bytes(3, 2, 2048)), dtype=torch.uint8, device="cuda")
    capi.check(lib.sela_hip_encode_pcm_device(torch.from_numpy(raw).cuda().data_ptr(), 3, 3, 2, 2048, 0, frames.view.data_ptr(), cap, offsets.data_ptr(),
                                              status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert frames.intact() and st[1] == 1 and codec.encode_status_error(st) == -4
    assert np.array_equal(offsets.cpu().numpy().view(np.uint64), want_offs)  # the offsets in full
    assert np.array_equal(frames.numpy()[: int(want_offs[2])], want_frames[: int(want_offs[2])])


def test_full_scale_noise_fits_the_bound(gpu):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(9)
    n_frames, channels, n = 2, 2, 2048
    raw = rng.integers(0, 256, n_frames * n * channels * 3, dtype=np.uint8)
    bound = int(capi.lib().sela_hip_encode_pcm_bound_bytes(n_frames, channels, n, 3))
    enc = codec.EncoderPcm(n_frames, channels, n, 3, capacity=bound)
    enc.encode(torch.from_numpy(raw).cuda())
    frames, offs = enc.to_host()  # (check() inside: no capacity error)
    assert int(offs[-1]) <= bound and int(offs[-1]) > raw.size // 2
    plain = codec.Encoder32(n_frames, channels, n, capacity=bound)  # (codec.encode_i32 sizes its buffer for 17 bits)
    plain.encode(torch.from_numpy(np_unpack(raw, n_frames, n, channels, 3)).cuda())
    want_frames, want_offs = plain.to_host()
    assert np.array_equal(offs, want_offs) and np.array_equal(frames, want_frames)


def _stream_of(blobs):
    return np.frombuffer(b"".join(bytes(b) for b in blobs), np.uint8).copy(), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)


def _decode_streams(generic_kats):
    out = {}
    for name in CASES:
        _, frames, offs = _expected(name, False)
        out[name] = (frames, offs, CASES[name][0].shape[2], CASES[name][1])
    blobs = [generic_kats[f"n{n}_stereo_diff_i17/bytes"] for n in (128, 1000, 2047, 2049, 128)]
    for b in (3, 4):
        out["mixed%d" % b] = _stream_of(blobs) + (2, b)
    return out


def _decode_device(torch, frames, offs, channels, stride, b):
    n_frames = len(offs) - 1
    dec = codec.DecoderPcm(n_frames, channels, stride, b)
    out = Guarded(torch, n_frames * stride * channels * b)
    src = Guarded(torch, (len(frames) + 3) & ~3, np.concatenate([frames, np.zeros(-len(frames) % 4, np.uint8)]))
    dec.decode(src.view, torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda(), n_frames, out=out.view)
    torch.cuda.synchronize()
    assert src.intact() and out.intact()
    return dec, out


@pytest.mark.parametrize("name", list(CASES) + ["mixed3", "mixed4"])
def test_decode_pcm_device(gpu, generic_kats, name):  # noqa: F811
    torch = gpu
    frames, offs, channels, b = _decode_streams(generic_kats)[name]
    n_frames = len(offs) - 1
    so, stride = codec.index_samples(frames, offs, channels)
    decoded = codec.decode_i32(frames, offs, channels)
    want = np.concatenate([np_pack(np.stack(decoded[f]), b) for f in range(n_frames)])
    dec, out = _decode_device(torch, frames, offs, channels, stride, b)
    dec.check()
    got = out.numpy()
    assert np.array_equal(got[: want.size], want) and want.size == int(so[-1]) * channels * b
    assert (got[want.size:] == 0xA5).all()
    assert np.array_equal(dec.sample_offsets.cpu().numpy().view(np.uint64), so)
    for f in range(n_frames):  # per frame: the reference's decoder
        ref_channels, _ = _ref().frame_decode_i32(frames[int(offs[f]): int(offs[f + 1])].tobytes(), channels)
        at = int(so[f]) * channels * b
        assert np.array_equal(got[at: at + len(ref_channels[0]) * channels * b], np_pack(np.stack(ref_channels), b)), f
    assert int(dec.status[1].item()) == 0 and int(dec.status[2].item()) == stride and dec.wide_samples() == 0
    # a stride one short: refused as sela_hip_decode_i32_device refuses it, nothing written
    short, out2 = _decode_device(torch, frames, offs, channels, stride - 1, b) if stride > 1 else (None, None)
    if short is not None:
        st = short.status.cpu().tolist()
        assert st[0] & capi.FLAG_STRIDE and st[2] == stride and (out2.numpy() == 0xA5).all()
        assert codec.decode_pcm_status_error(st) == -4
        ref32 = codec.Decoder32(n_frames, channels, stride - 1)
        ref32.decode(torch.from_numpy(np.concatenate([frames, np.zeros(-len(frames) % 4, np.uint8)])).cuda(),
                     torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda(), n_frames)
        assert ref32.status.cpu().tolist()[0] & capi.FLAG_STRIDE


def test_decode_pcm_device_flags_a_ragged_frame(gpu, generic_kats):  # noqa: F811
    torch = gpu
    blob = generic_kats["crafted/mixed_lengths/bytes"]
    frames, offs = _stream_of([generic_kats["n128_three_i17/bytes"], blob, generic_kats["n128_three_i17/bytes"]])
    dec, out = _decode_device(torch, frames, offs, 3, 300, 3)
    st = dec.status.cpu().tolist()
    assert st[0] & capi.FLAG_BAD_FRAME and st[1] == 1 and codec.decode_pcm_status_error(st) == -5
    decoded = codec.decode_i32(frames[: int(offs[1])], offs[:2], 3)
    first = np_pack(np.stack(decoded[0]), 3)
    got = out.numpy()
    assert np.array_equal(got[: first.size], first)
    assert (got[128 * 9: 428 * 9] == 0xA5).all()  # the ragged frame's 300 samples
    assert np.array_equal(got[428 * 9: 556 * 9], first) and (got[556 * 9:] == 0xA5).all()


# ---- 4. one graph of both ---------------------------------------------------------------------------------------------------------
def test_one_graph_of_encode_and_decode(gpu):  # noqa: F811
    torch = gpu
    n_frames, channels, n, b = 3, 2, 2048, 3
    inputs = [pack_interleaved(_music24(n_frames, channels, seed), b) for seed in (11, 12)]
    eager = []
    for raw in inputs:
        enc = codec.EncoderPcm(n_frames, channels, n, b, lossless=True)
        enc.encode(torch.from_numpy(raw).cuda())
        eager.append(enc.to_host())
    enc = codec.EncoderPcm(n_frames, channels, n, b, lossless=True)
    dec = codec.DecoderPcm(n_frames, channels, n, b)
    src = torch.from_numpy(inputs[0]).cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):  # (one call before the capture: lazy initialisation is not capturable)
        enc.encode(src)
        dec.decode(enc.frames, enc.offsets, n_frames)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        enc.encode(src)
        dec.decode(enc.frames, enc.offsets, n_frames)
    for raw, (want_frames, want_offs) in zip(inputs, eager):
        src.copy_(torch.from_numpy(raw).cuda())
        dec.pcm.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        frames, offs = enc.to_host()
        dec.check()
        assert np.array_equal(offs, want_offs) and np.array_equal(frames, want_frames)
        assert np.array_equal(dec.pcm.cpu().numpy(), raw)


# ---- 5. host pointers -------------------------------------------------------------------------------------------------------------
def test_host_pointer_pair(gpu):  # noqa: F811
    lib = capi.lib()
    n_frames, channels, n, b = 5, 2, 2048, 3
    x = _music24(n_frames, channels, 21)
    raw = pack_interleaved(x, b)
    planar = np.ascontiguousarray(x.transpose(0, 2, 1))
    for lossless in (False, True):
        want_frames, want_offs = codec.encode_i32(planar, lossless=lossless)
        want_pcm = np.concatenate([np_pack(np.stack(chans), b) for chans in codec.decode_i32(want_frames, want_offs, channels)])
        for chunk in (0, 2):
            lib.sela_hip_debug_pcm_chunk_frames(chunk)
            try:
                frames, offs = codec.encode_pcm_host(raw, channels, n, b, lossless=lossless)
                pcm, wide = codec.decode_pcm_host(frames, offs, channels, b)
            finally:
                lib.sela_hip_debug_pcm_chunk_frames(0)
            assert np.array_equal(offs, want_offs) and np.array_equal(frames, want_frames), (lossless, chunk)
            assert np.array_equal(pcm, want_pcm) and wide == 0, (lossless, chunk)
            if lossless:
                assert np.array_equal(pcm, raw)
    # the device calls give the same bytes
    enc = codec.EncoderPcm(n_frames, channels, n, b, lossless=True)
    enc.encode(gpu.from_numpy(raw).cuda())
    dev_frames, dev_offs = enc.to_host()
    assert np.array_equal(dev_frames, want_frames) and np.array_equal(dev_offs, want_offs)


def test_host_pointer_pair_leaves_an_open_job_alone(gpu):  # noqa: F811
    lib = capi.lib()
    pcm16 = synth_frames(12, 2, 5)
    frames16, offs16 = codec.encode_host(pcm16)
    back = np.zeros(pcm16.size, np.int16)
    job, ff = C.c_void_p(), C.c_uint32(0)
    capi.check(lib.sela_hip_decode_begin(C.byref(job), 2, 12, back.ctypes.data))
    o = np.ascontiguousarray(offs16[:6])
    capi.check(lib.sela_hip_decode_feed(job, frames16.ctypes.data, o.ctypes.data, 5, C.byref(ff)))
    x = _music24(2, 2, 31)
    raw = pack_interleaved(x, 3)
    frames, offs = codec.encode_pcm_host(raw, 2, 2048, 3, lossless=True)
    pcm, wide = codec.decode_pcm_host(frames, offs, 2, 3)
    assert np.array_equal(pcm, raw) and wide == 0
    o = np.ascontiguousarray(offs16[5:] - offs16[5])
    capi.check(lib.sela_hip_decode_feed(job, frames16[int(offs16[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12 and np.array_equal(back, pcm16.reshape(-1))
