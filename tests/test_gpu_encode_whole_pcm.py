"""GPU: a whole track from packed 3- or 4-byte PCM, its tail kept in a long last frame --
sela_hip_encode_whole_pcm_device and sela_hip_encode_whole_pcm.  The rule is sela_hip_whole_frames': frames 0 .. F - 2 of 2048
samples and a last frame of 2048 + t, each byte for byte frame::FrameEncoder's for a frame of that length.  Expected bytes are the
reference's (tests/whole_pcm_cases.py: frame_encode_i32 per frame; lossless: tests/lossless_model.py).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import whole_pcm_cases as W
from gpu_common import gpu  # noqa: F401
from sela_amd import capi, codec

pytestmark = pytest.mark.gpu

N = W.N
POISON = 0xA5
GUARD = 256
CHANNELS = (1, 2, 3)
SAMPLES = [2 * N + t for t in (1, 77, 101, 2047)] + [N + 5, 3 * N, 300]


def _guarded(torch, nbytes, fill=None):
    """an exact-size view inside a larger tensor filled with 0xA5 -> (the whole tensor, the view)"""
    big = torch.full((nbytes + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    view = big[GUARD: GUARD + nbytes]
    if fill is not None and nbytes:
        view.copy_(torch.from_numpy(fill))
    return big, view


def _intact(big, nbytes):
    g = big.cpu().numpy()
    return bool((g[:GUARD] == POISON).all() and (g[GUARD + nbytes:] == POISON).all())


def _device(torch, x, b, lossless=False, capacity=None):
    """one call on a fresh encoder with poisoned frames inside guards, the source an exact-size view inside guards ->
    (frames uint8 [capacity], offsets uint64, status int64 [4])"""
    n, ch = x.shape
    raw = W.packed(x, b)
    enc = codec.WholeEncoderPcm(n, ch, b, lossless=lossless, capacity=capacity)
    big_out, enc.frames = _guarded(torch, enc.capacity)
    enc.offsets.fill_(-1)
    enc.status.fill_(-1)
    big_in, src = _guarded(torch, raw.size, raw)
    enc.encode(src, n)
    torch.cuda.synchronize()
    assert _intact(big_in, raw.size) and np.array_equal(src.cpu().numpy(), raw), "the source must stay intact"
    assert _intact(big_out, enc.capacity), "nothing outside the frames' room may be written"
    return enc.frames.cpu().numpy(), enc.offsets[: enc.n_frames + 1].cpu().numpy().view(np.uint64), enc.status.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


# ---- 1. bytes, offsets and status against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("n", SAMPLES)
def test_bytes_equal_the_references(gpu, n, ch, b):  # noqa: F811
    k = SAMPLES.index(n)
    x = W.track(n, ch, b, k)
    want, want_offs = W.expected(n, ch, b, k)
    layout = codec.whole_frames(n)
    assert len(layout) == len(want_offs) - 1 == (n // N if n >= N else 1)
    assert [(a, l) for a, l in layout] == [(f * N, N) for f in range(len(layout) - 1)] + [((len(layout) - 1) * N, n - (len(layout) - 1) * N)]
    frames, offs, st = _device(gpu, x, b, capacity=len(want) + 64)
    assert np.array_equal(offs, want_offs) and st.tolist() == [0, 0, 0, 0], (offs, want_offs, st)
    assert frames[: len(want)].tobytes() == want
    assert (frames[len(want):] == POISON).all()  # nothing behind the stream
    h_frames, h_offs = codec.encode_whole_pcm_host(W.packed(x, b), ch, b)
    assert h_frames.tobytes() == want and np.array_equal(h_offs, want_offs)
    if n % N == 0:  # whole frames only: the plain call's stream
        p_frames, p_offs = codec.encode_pcm_host(W.packed(x, b), ch, N, b)
        assert p_frames.tobytes() == want and np.array_equal(p_offs, want_offs)


def test_both_stereo_decisions_occur_in_the_long_last_frames():
    for b in (3, 4):
        types = set()
        for n in SAMPLES:
            if n > N and n % N:
                want, offs = W.expected(n, 2, b, SAMPLES.index(n))
                types.add(W.second_subframe_type(want[int(offs[-2]):]))
        assert types == {0, 1}, b


def test_frames_of_three_byte_samples_on_three_channels_sit_at_odd_byte_counts():
    """(the last frame's packed bytes still start at a multiple of 4: 2048 * 9 bytes a frame)"""
    assert (N + 5) * 9 % 2 == 1 and (2 * N + 77) * 9 % 4 != 0 and N * 9 % 4 == 0


# ---- 2. lossless -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("n", [2 * N + 77, 2 * N + 2047, N + 5, 300])
def test_lossless_streams_give_every_sample_back(gpu, n, ch, b):  # noqa: F811
    torch = gpu
    k = SAMPLES.index(n)
    x = W.track(n, ch, b, k)
    raw = W.packed(x, b)
    want, want_offs = W.expected(n, ch, b, k, True)
    enc = codec.WholeEncoderPcm(n, ch, b, lossless=True)
    d_raw = torch.from_numpy(raw).cuda()
    frames, offs, _ = enc.encode(d_raw)
    got, got_offs = enc.to_host()
    assert np.array_equal(got_offs, want_offs) and got.tobytes() == want
    h_frames, h_offs = codec.encode_whole_pcm_host(raw, ch, b, lossless=True)
    assert h_frames.tobytes() == want and np.array_equal(h_offs, want_offs)
    n_last = codec.whole_frames(n)[-1][1]
    dec = codec.DecoderPcm(enc.n_frames, ch, n_last, b)
    pcm, sample_offs = dec.decode(frames, offs.contiguous(), enc.n_frames)
    torch.cuda.synchronize()
    dec.check()
    assert sample_offs.cpu().numpy().tolist() == [f * N for f in range(enc.n_frames)] + [n]
    assert np.array_equal(pcm[: raw.size].cpu().numpy(), raw)  # all N samples, the input's bytes
    ver = codec.VerifierPcm(enc.n_frames, ch, n_last, b)
    ver.verify(frames, offs.contiguous(), enc.n_frames, d_raw, n)
    ver.check()
    assert ver.lossy_frames() == 0
    # without lossless: the decode is the reference's frame_decode_i32 of the same stream
    plain = codec.WholeEncoderPcm(n, ch, b)
    p_frames, p_offs, _ = plain.encode(d_raw)
    p_host, p_host_offs = plain.to_host()
    pcm, _ = dec.decode(p_frames, p_offs.contiguous(), plain.n_frames)
    torch.cuda.synchronize()
    dec.check()
    assert np.array_equal(pcm[: raw.size].cpu().numpy(), W.packed(W.decoded(p_host.tobytes(), p_host_offs, ch), b))


# ---- 3. capacity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b, ch", [(3, 3), (4, 2)])
def test_capacity(gpu, b, ch):  # noqa: F811
    n = 3 * N + 777
    x = W.track(n, ch, b, 2)
    want, want_offs = W.expected(n, ch, b, 2)
    # room for all but the last frame; a capacity that cuts the second 2048-sample frame
    for cap, fits, lost in ((int(want_offs[2]), 2, 1), (int(want_offs[1]) + 8, 1, 2)):
        frames, offs, st = _device(gpu, x, b, capacity=cap)
        assert np.array_equal(offs, want_offs), cap  # (complete)
        assert st.tolist() == [0, lost, 0, 0] and codec.encode_status_error(st) == -4, (cap, st)
        assert frames[: int(want_offs[fits])].tobytes() == want[: int(want_offs[fits])], cap
        assert (frames[int(want_offs[fits]):] == POISON).all(), cap  # (not a byte of a frame that does not fit)
    frames, offs, st = _device(gpu, x, b, capacity=len(want))
    assert st.tolist() == [0, 0, 0, 0] and frames.tobytes() == want


# ---- 4. further cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [3, 4])
def test_no_samples(gpu, b):  # noqa: F811
    frames, offs, st = _device(gpu, np.zeros((0, 2), np.int32), b, capacity=64)
    assert offs.tolist() == [0] and st.tolist() == [0, 0, 0, 0] and (frames == POISON).all()
    h_frames, h_offs = codec.encode_whole_pcm_host(np.zeros(0, np.uint8), 2, b)
    assert len(h_frames) == 0 and h_offs.tolist() == [0]


def test_a_short_noise_track_is_refused_as_the_plain_call_refuses_it(gpu):  # noqa: F811
    lib = capi.lib()
    x = np.random.default_rng(2).integers(-(1 << 22), 1 << 22, (20, 1)).astype(np.int32)
    raw = W.packed(x, 3)
    out = np.zeros(1 << 16, np.uint8)
    offs = np.zeros(2, np.uint64)
    plain = lib.sela_hip_encode_pcm(raw.ctypes.data, 3, 1, 1, 20, 0, out.ctypes.data, out.nbytes, offs.ctypes.data)
    assert plain == -6  # SELA_HIP_ERANGE: the block is no longer than the order its analysis picks
    assert lib.sela_hip_encode_whole_pcm(raw.ctypes.data, 3, 20, 1, 0, out.ctypes.data, out.nbytes, offs.ctypes.data) == plain
    _, _, st = _device(gpu, x, 3, capacity=4096)
    assert int(st[0]) & capi.FLAG_SHORT_BLOCK and codec.encode_status_error(st) == plain


def test_graph_replay_on_new_samples(gpu):  # noqa: F811
    torch = gpu
    n, ch, b = 3 * N + 77, 2, 3
    a, x1, x2 = (W.track(n, ch, b, k) for k in (4, 7, 10))
    enc = codec.WholeEncoderPcm(n, ch, b)
    d_x = torch.from_numpy(W.packed(a, b)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.encode(d_x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert enc.to_host()[0].tobytes() == W.expected(n, ch, b, 4)[0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enc.encode(d_x)
    for x, k in ((x1, 7), (x2, 10)):
        d_x.copy_(torch.from_numpy(W.packed(x, b)))
        enc.frames.fill_(POISON)
        enc.offsets.fill_(-1)
        enc.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert enc.status.cpu().numpy().tolist() == [0, 0, 0, 0]
        frames, offs = enc.to_host()
        want, want_offs = W.expected(n, ch, b, k)
        assert frames.tobytes() == want and np.array_equal(offs, want_offs)


def test_a_thread_with_an_open_streaming_job_is_left_alone(gpu):  # noqa: F811
    from sela_amd.synth import synth_frames

    lib = capi.lib()
    job_pcm = synth_frames(12, 2, 5)
    want_frames, want_offs = codec.encode_host(job_pcm)
    out = np.zeros(int(lib.sela_hip_encode_bound_bytes(12, 2)), np.uint8)
    offs = np.zeros(13, np.uint64)
    job = C.c_void_p()
    capi.check(lib.sela_hip_encode_begin(C.byref(job), 2, 12, out.ctypes.data, out.nbytes, offs.ctypes.data))
    capi.check(lib.sela_hip_encode_feed(job, job_pcm.ctypes.data, 5, None, None))
    n = 2 * N + 101
    for lossless in (False, True):
        h_frames, h_offs = codec.encode_whole_pcm_host(W.packed(W.track(n, 2, 3, 3), 3), 2, 3, lossless=lossless)
        want, w_offs = W.expected(n, 2, 3, 3, lossless)
        assert h_frames.tobytes() == want and np.array_equal(h_offs, w_offs)
    capi.check(lib.sela_hip_encode_feed(job, job_pcm[5:].ctypes.data, 7, None, None))
    total = C.c_uint64(0)
    capi.check(lib.sela_hip_encode_end(job, None, C.byref(total)))
    assert np.array_equal(offs, want_offs) and out[: total.value].tobytes() == want_frames.tobytes()
