"""sela_hip_levels_device, sela_hip_levels_payload_device and sela_hip_levels: per frame and channel the peak,
the sample count, the sum and the sum of squares of the int16 samples sela_hip_decode_n_device writes.  The expectation is always
numpy on int16 PCM -- the CPU oracle's decode, for encoder-made streams and for hand-built frames alike -- and every
comparison is exact equality of all four fields.  status[0], [1] and [3] are the decode call's; status[2] counts the frames that
are not digital silence."""
import ctypes as C

import numpy as np
import pytest

from gpu_common import _build_frame, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from sela_amd.synth import synth_frames
from test_gpu_verify_device import _bytes, _channels_pcm, _decode_n, _status_cases, _stream

pytestmark = pytest.mark.gpu

NONE, FAST, ANY = 0, 1, 2
GUARD = 16              # records behind d_levels that no call may write
SENTINEL = 0x5E1A5E1A5E1A5E1A


def _expect(pcm, so):
    """pcm: int16 [total samples, ch]; so: sample offsets [n + 1] -> the records, LEVEL_DTYPE [n, ch], in numpy's int64."""
    p = np.asarray(pcm, np.int16)
    n, ch = len(so) - 1, p.shape[1]
    out = np.zeros((n, ch), codec.LEVEL_DTYPE)
    for f in range(n):
        v = p[int(so[f]): int(so[f + 1])].astype(np.int64)
        out["samples"][f] = len(v)
        if len(v):
            out["peak"][f] = np.abs(v).max(0)
            out["sum"][f] = v.sum(0)
            out["sum_squares"][f] = (v * v).sum(0)
    return out


def _same(got, want, label=""):
    for name in codec.LEVEL_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (label, name, np.argwhere(got[name] != want[name])[:6].tolist())


class _Device:
    """Buffers of one sela_hip_levels_device call, the raw C ABI: guard records behind d_levels, d_frames kept for a look afterwards."""

    def __init__(self, torch, n, ch, stride):
        self.torch, self.n, self.ch, self.stride = torch, n, ch, stride
        self.levels = torch.full(((n * ch + GUARD) * 3,), SENTINEL, dtype=torch.int64, device="cuda")
        self.sample_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_levels_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")

    def measure(self, blob, offs, with_offsets=True):
        torch = self.torch
        data = _bytes(blob)
        frames = torch.zeros(max(len(data), 4), dtype=torch.uint8, device="cuda")
        if len(data):
            frames[: len(data)].copy_(torch.from_numpy(data))
        o = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).cuda()
        before = frames.clone()
        assert self.levels.data_ptr() % 8 == 0
        capi.check(capi.lib().sela_hip_levels_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, self.levels.data_ptr(),
            self.sample_offsets.data_ptr() if with_offsets else None, self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(frames, before), "d_frames was written"
        return self.results()

    def results(self):
        words = self.levels.cpu().numpy()
        k = self.n * self.ch * 3
        assert (words[k:] == np.int64(SENTINEL)).all(), "written past d_levels"
        return words[:k].copy().view(codec.LEVEL_DTYPE).reshape(self.n, self.ch), self.status.cpu().numpy().view(np.uint32).copy()


def _check(torch, blob, offs, ch, stride, pcm, route, label=""):
    """The records of (stream) == numpy on pcm ([total, ch] int16), status as the decode call leaves it -> (records, status)."""
    n = len(offs) - 1
    _, so, dst = _decode_n(torch, blob, offs, ch, stride)
    assert codec.decode_n_status_error(dst) == 0, (label, dst)
    p = np.ascontiguousarray(pcm, np.int16).reshape(-1, ch)
    assert len(p) == int(so[n]), (label, len(p), int(so[n]))
    want = _expect(p, so)
    dev = _Device(torch, n, ch, stride)
    got, st = dev.measure(blob, offs)
    assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (label, st, dst)
    assert int(st[3]) == route, (label, st)
    _same(got, want, label)
    assert int(st[2]) == int((want["peak"] != 0).any(1).sum()), (label, st)
    assert np.array_equal(dev.sample_offsets.cpu().numpy().view(np.uint64), so), label
    return got, st


# ---- 1. the fused route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_2048_sample_frames_on_the_fused_route(gpu, ch):  # noqa: F811
    pcm = _channels_pcm(9, ch, 30 + ch)
    frames, offs = codec.encode_i32(np.ascontiguousarray(pcm.transpose(0, 2, 1)).astype(np.int32))
    back, _ = oracle().decode_frames(frames, offs, ch, threads=4)
    got, _ = _check(gpu, frames, offs, ch, 2048, back.reshape(-1, ch), FAST, f"{ch} channels")
    assert (got["samples"] == 2048).all() and (got["peak"] > 0).all()
    wider, _ = _check(gpu, frames, offs, ch, 3000, back.reshape(-1, ch), FAST, f"{ch} channels, a larger stride")
    _same(wider, got, "a larger stride gives the same records")


def test_the_golden_stereo_frames(gpu, kats):  # noqa: F811
    names = ["stereo_same_sine", "stereo_synth_diff", "stereo_silence", "stereo_synth_diff", "stereo_silence"]
    stream, offs = _stream([kats[f"frame/{n}/bytes"].tobytes() for n in names])
    back, _ = oracle().decode_frames(stream, offs, 2)
    got, st = _check(gpu, stream, offs, 2, 2048, back.reshape(-1, 2), FAST, "golden frames")
    for f in (2, 4):  # digital silence: all-zero records but for the sample count
        assert got[f].tolist() == [(0, 2048, 0, 0), (0, 2048, 0, 0)]
    assert int(st[2]) == 3, "status[2] counts only the frames that are not silent"
    assert (got["peak"][[0, 1, 3]] > 0).any(1).all()


def test_full_scale_constants(gpu):  # noqa: F811
    pcm = np.empty((2048, 2), np.int16)
    pcm[:, 0], pcm[:, 1] = -32768, 32767
    blob = oracle().frame_encode(pcm)
    back, used = oracle().frame_decode(blob, 2)
    assert used == len(blob) and np.array_equal(back, pcm), "the oracle does not give this frame back"
    stream, offs = _stream([blob, blob])
    got, st = _check(gpu, stream, offs, 2, 2048, np.concatenate([back, back]), FAST, "full scale")
    assert got[0].tolist() == [(32768, 2048, -(1 << 26), 1 << 41), (32767, 2048, 2048 * 32767, 2048 * 32767 * 32767)]
    assert got[1].tolist() == got[0].tolist() and int(st[2]) == 2


def _oracle_pcm(blobs, ch):
    """the CPU oracle's decode of hand-built 2048-sample frames -> int16 [frames * 2048, ch]"""
    out = []
    for blob in blobs:
        pcm, used = oracle().frame_decode(blob, ch)
        assert used == len(blob)
        out.append(pcm)
    return np.concatenate(out)


def test_a_frame_on_the_serial_parse_fallback(gpu, kats):  # noqa: F811
    """A Rice stream beyond the parser's plan (kStreamCap words): the serial parse into the workspace, then the same reduction."""
    rng = np.random.default_rng(77)
    q_sine = kats["blk/sine_deg/q"]
    big = _build_frame([(0, 0, 0, q_sine, rng.integers(-120000, 120000, 2048))])
    small = _build_frame([(0, 0, 0, q_sine, rng.integers(-200, 200, 2048))])
    assert (len(big) - 16) // 4 + 2 > 1072 + 50, "the subframe's words (coefficients + 2 + residues) are meant to exceed kStreamCap"
    stream, offs = _stream([small, big, small])
    _, so, st = _decode_n(gpu, stream, offs, 1, 2048)
    assert codec.decode_n_status_error(st) == 0 and int(st[3]) == FAST and int(so[-1]) == 3 * 2048
    _check(gpu, stream, offs, 1, 2048, _oracle_pcm([small, big, small], 1), FAST, "serial parse")
    # ... and as one channel of a stereo frame beside a subframe that fits the plan (the whole frame takes the fallback)
    two = _build_frame([(0, 0, 0, q_sine, rng.integers(-120000, 120000, 2048)), (1, 0, 1, q_sine, rng.integers(-50, 50, 2048))])
    stream, offs = _stream([two, two])
    _, so, st = _decode_n(gpu, stream, offs, 2, 2048)
    assert codec.decode_n_status_error(st) == 0 and int(st[3]) == FAST and int(so[-1]) == 2 * 2048
    _check(gpu, stream, offs, 2, 2048, _oracle_pcm([two, two], 2), FAST, "serial parse, stereo")


# ---- 2. the cold route -------------------------------------------------------------------------------------------------------------
def test_twelve_channels_of_2048(gpu):  # noqa: F811
    """k_decode_frames_wide into the workspace, then k_level_channels"""
    pcm = _channels_pcm(5, 12, 50)
    frames, offs = codec.encode_i32(np.ascontiguousarray(pcm.transpose(0, 2, 1)).astype(np.int32))
    back, _ = oracle().decode_frames(frames, offs, 12, threads=4)
    got, _ = _check(gpu, frames, offs, 12, 2048, back.reshape(-1, 12), FAST, "12 channels")
    wider, _ = _check(gpu, frames, offs, 12, 2100, back.reshape(-1, 12), FAST, "12 channels, a larger stride")
    _same(wider, got)


@pytest.mark.parametrize("n", [1000, 5000])
def test_frames_of_other_lengths_from_the_device_encoder(gpu, n):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(n)
    pcm = np.stack([np.stack([_signal(rng, "tone", n, 15), _signal(rng, "noise", n, 12)], axis=1) for _ in range(5)]).astype(np.int16)
    enc = codec.Encoder32(5, 2, n)
    enc.encode(torch.from_numpy(np.ascontiguousarray(pcm)).cuda())  # (sela_hip_encode_n_device)
    frames, offs = enc.to_host()
    back, _ = oracle().decode_frames(frames, offs, 2, n=n, threads=4)
    got, _ = _check(torch, frames, offs, 2, n, back.reshape(-1, 2), ANY, f"length {n}")
    assert (got["samples"] == n).all()
    _same(_check(torch, frames, offs, 2, n + 123, back.reshape(-1, 2), ANY, f"length {n}, a larger stride")[0], got)
    for mode in (0, 2):
        capi.lib().sela_hip_debug_standard_first(mode)
        try:
            _same(_check(torch, frames, offs, 2, n, back.reshape(-1, 2), ANY, (n, "mode", mode))[0], got, ("mode", mode))
        finally:
            capi.lib().sela_hip_debug_standard_first(-1)


def _odd_frame(n, seeds=(1, 2)):
    pcm = np.stack([_signal(np.random.default_rng(seeds[0]), "tone", n, 15), _signal(np.random.default_rng(seeds[1]), "noise", n, 12)], axis=1).astype(np.int16)
    blob = oracle().frame_encode(pcm)
    back, used = oracle().frame_decode(blob, 2, n=n)
    assert used == len(blob)
    return blob, back


def test_a_stream_that_mixes_2048_with_another_length(gpu):  # noqa: F811
    pcm = synth_frames(6, 2, 3)
    frames, offs, _ = oracle().encode_frames(pcm)
    back, _ = oracle().decode_frames(frames, offs, 2)
    blobs = [frames[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(6)]
    odd, odd_back = _odd_frame(777)
    stream, so = _stream(blobs[:4] + [odd] + blobs[4:])
    flat = np.concatenate([back[:4].reshape(-1, 2), odd_back, back[4:].reshape(-1, 2)])
    got, _ = _check(gpu, stream, so, 2, 2048, flat, ANY, "mixed lengths")
    assert got["samples"][:, 0].tolist() == [2048] * 4 + [777] + [2048] * 2


def test_a_stream_with_a_long_last_frame(gpu):  # noqa: F811
    """the shape of a --keep-tail stream: 3 frames of 2048 and one of 2048 + 777"""
    pcm = synth_frames(3, 2, 9)
    frames, offs, _ = oracle().encode_frames(pcm)
    back, _ = oracle().decode_frames(frames, offs, 2)
    last, last_back = _odd_frame(2048 + 777, seeds=(5, 6))
    stream, so = _stream([frames.tobytes(), last])
    so = np.concatenate([offs[:3], so[1:]]).astype(np.uint64)
    got, _ = _check(gpu, stream, so, 2, 2048 + 777, np.concatenate([back.reshape(-1, 2), last_back]), ANY, "a long last frame")
    assert got["samples"][:, 1].tolist() == [2048, 2048, 2048, 2825]


# ---- 3. status, guards, arguments ----------------------------------------------------------------------------------------------------
def test_status_words_are_the_decode_calls(gpu, kats):  # noqa: F811
    seen = set()
    for label, blob, offs, ch, stride, _pcm in _status_cases(kats):
        n = len(offs) - 1
        _, _, dst = _decode_n(gpu, blob, offs, ch, stride)
        _, st = _Device(gpu, n, ch, stride).measure(blob, offs)
        assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (label, st, dst)
        code = codec.decode_n_status_error(st)
        assert code == codec.decode_n_status_error(dst), (label, st, dst)
        seen.add(code)
        if label == "clean":
            assert code == 0 and int(st[2]) == n
    assert {0, -4, -5, -6} <= seen, seen


def test_no_frames(gpu):  # noqa: F811
    dev = _Device(gpu, 0, 2, 2048)
    got, st = dev.measure(b"", np.zeros(1, np.uint64))
    assert (st == 0).all() and got.shape == (0, 2)
    assert int(dev.sample_offsets[0].item()) == 0


def test_nothing_else_is_written_without_sample_offsets(gpu):  # noqa: F811
    pcm = synth_frames(4, 2, 4)
    frames, offs, _ = oracle().encode_frames(pcm)
    back, _ = oracle().decode_frames(frames, offs, 2)
    for stride in (2048, 2500):
        dev = _Device(gpu, 4, 2, stride)
        got, st = dev.measure(frames, offs, with_offsets=False)
        assert (dev.sample_offsets.cpu().numpy() == -1).all()
        _same(got, _expect(back.reshape(-1, 2), np.arange(5) * 2048), stride)
        assert int(st[2]) == 4 and int(st[3]) == FAST


def test_argument_errors_enqueue_nothing(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    pcm = synth_frames(2, 2, 1)
    blob, o, _ = oracle().encode_frames(pcm)
    n = len(blob)
    buf = torch.from_numpy(np.concatenate([blob, np.zeros(4, np.uint8)])).cuda()
    offs = torch.from_numpy(o.view(np.int64).copy()).cuda()
    ws_bytes = int(lib.sela_hip_levels_workspace_bytes(2, 2, 2048))
    ix_bytes = int(lib.sela_hip_index_workspace_bytes(n, 2))
    ws = torch.empty(ws_bytes + ix_bytes, dtype=torch.uint8, device="cuda")
    levels = torch.full((2 * 2 * 3,), -1, dtype=torch.int64, device="cuda")
    so = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    fo = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    nf = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def dev(frames=buf.data_ptr(), fo_=offs.data_ptr(), nfr=2, channels=2, stride=2048, lv=levels.data_ptr(), st=status.data_ptr(), w=ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_levels_device(frames, fo_, nfr, channels, stride, lv, so.data_ptr(), st, w, wb, stream)

    def pay(payload=buf.data_ptr(), channels=2, stride=2048, lv=levels.data_ptr(), st=status.data_ptr(), o_=fo.data_ptr(), k=nf.data_ptr(), w=ws.data_ptr(),
            wb=ws_bytes + ix_bytes):
        return lib.sela_hip_levels_payload_device(payload, n, 2, channels, stride, lv, so.data_ptr(), o_, k, st, w, wb, stream)

    for call, code in [(lambda: dev(frames=buf.data_ptr() + 1), -2), (lambda: dev(channels=0), -2), (lambda: dev(channels=256), -2),
                       (lambda: dev(stride=0), -2), (lambda: dev(lv=None), -2), (lambda: dev(lv=levels.data_ptr() + 4), -2),
                       (lambda: dev(st=None), -2), (lambda: dev(w=None), -2), (lambda: dev(fo_=None), -2), (lambda: dev(frames=None), -2),
                       (lambda: dev(wb=ws_bytes - 1), -4), (lambda: dev(nfr=0x40000000), -2),
                       (lambda: pay(payload=buf.data_ptr() + 2), -2), (lambda: pay(channels=0), -2), (lambda: pay(stride=0), -2),
                       (lambda: pay(lv=None), -2), (lambda: pay(lv=levels.data_ptr() + 4), -2), (lambda: pay(st=None), -2),
                       (lambda: pay(o_=None), -2), (lambda: pay(k=None), -2), (lambda: pay(w=None), -2),
                       (lambda: pay(wb=ws_bytes + ix_bytes - 1), -4)]:
        assert call() == code
    torch.cuda.synchronize()  # nothing was enqueued: every output is as it was
    for t in (levels, so, fo, nf, status):
        assert (t.cpu().numpy() == -1).all()
    # a workspace of the size asked for is enough, and no initialisation is needed
    ws.fill_(0xFF)
    back, _ = oracle().decode_frames(blob, o, 2)
    want = _expect(back.reshape(-1, 2), np.arange(3) * 2048)
    assert dev() == 0
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert codec.decode_n_status_error(st) == 0 and int(st[2]) == 2 and int(st[3]) == FAST
    _same(levels.cpu().numpy().view(codec.LEVEL_DTYPE).reshape(2, 2), want)
    levels.fill_(-1)
    assert pay() == 0
    torch.cuda.synchronize()
    assert int(nf.item()) == 2 and int(status[2].item()) == 2
    _same(levels.cpu().numpy().view(codec.LEVEL_DTYPE).reshape(2, 2), want)


# ---- 4. the payload form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["2048", "long last frame"])
def test_a_payload_with_trailing_garbage(gpu, shape):  # noqa: F811
    torch = gpu
    pcm = synth_frames(7, 2, 8)
    frames, offs, _ = oracle().encode_frames(pcm)
    back = oracle().decode_frames(frames, offs, 2)[0].reshape(-1, 2)
    so = np.arange(8) * 2048
    stride = 2048
    blob = frames.tobytes()
    if shape != "2048":
        last, last_back = _odd_frame(2048 + 777, seeds=(7, 8))
        blob, back, so, stride = blob + last, np.concatenate([back, last_back]), np.append(so, so[-1] + 2825), 2825
        offs = np.append(offs, offs[-1] + len(last)).astype(np.uint64)
    n = len(offs) - 1
    payload = np.frombuffer(blob + b"\x11" * 40, np.uint8).copy()  # (no sync word in the garbage: the walk ends at it)
    max_frames = n + 5
    lev = codec.Leveler(max_frames, 2, stride)
    lev.levels.fill_(SENTINEL)
    records, count = lev.measure_payload(torch.from_numpy(payload).cuda())
    lev.check()
    assert int(count.item()) == n and lev.route() == (FAST if shape == "2048" else ANY) and lev.loud_frames() == n
    got = lev.records(records)
    assert got.shape == (max_frames, 2)
    _same(got[:n], _expect(back, so), shape)
    assert (records[n:].cpu().numpy() == np.int64(SENTINEL)).all(), "frames from *d_n_frames on are left alone"
    assert np.array_equal(lev.frame_offsets[: n + 1].cpu().numpy().view(np.uint64), offs)
    track = codec.track_levels(got[:n])
    v = back.astype(np.int64)
    assert track["peak"].tolist() == np.abs(v).max(0).tolist() and track["sum"].tolist() == v.sum(0).tolist()
    assert track["sum_squares"].tolist() == (v * v).sum(0).tolist() and track["samples"].tolist() == [len(v)] * 2


# ---- 5. capture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["measure", "measure_payload"])
def test_in_a_graph(gpu, form):  # noqa: F811
    torch = gpu
    n = 40
    inputs = []
    for seed in (2, 5):
        frames, offs, _ = oracle().encode_frames(synth_frames(n, 2, seed), threads=4)
        back, _ = oracle().decode_frames(frames, offs, 2, threads=4)
        inputs.append((frames, offs, _expect(back.reshape(-1, 2), np.arange(n + 1) * 2048)))
    assert not np.array_equal(inputs[0][2]["sum_squares"], inputs[1][2]["sum_squares"])
    room = max(len(i[0]) for i in inputs)
    d_frames = torch.zeros(room, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

    def load(k):
        frames, offs, _ = inputs[k]
        d_frames.zero_()
        d_frames[: len(frames)].copy_(torch.from_numpy(frames))
        d_offs.copy_(torch.from_numpy(offs.view(np.int64).copy()))

    lev = codec.Leveler(n, 2, 2048)
    call = (lambda: lev.measure(d_frames, d_offs, n)) if form == "measure" else (lambda: lev.measure_payload(d_frames))
    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # (the workspace is allocated here, not under capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    records = out if form == "measure" else out[0]
    for k in (0, 1):
        load(k)
        lev.levels.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        _same(lev.records(records), inputs[k][2], (form, k))
        assert lev.status.cpu().numpy().tolist() == [0, 0, n, FAST], (form, k)
        if form == "measure_payload":
            assert int(out[1].item()) == n


# ---- 6. the host-pointer call ----------------------------------------------------------------------------------------------------------
def test_the_host_pointer_call_equals_the_device_call(gpu):  # noqa: F811
    frames, offs, _ = oracle().encode_frames(synth_frames(40, 2, 2), threads=4)
    want, st = _Device(gpu, 40, 2, 2048).measure(frames, offs)
    assert int(st[3]) == FAST and codec.decode_n_status_error(st) == 0
    _same(codec.levels_host(frames, offs, 2), want, "host call")
    # another length
    blobs = [_odd_frame(1500, seeds=(s, s + 10))[0] for s in (1, 2, 3)]
    stream, o = _stream(blobs)
    want, st = _Device(gpu, 3, 2, 1500).measure(stream, o)
    assert int(st[3]) == ANY
    _same(codec.levels_host(stream, o, 2), want, "host call, another length")
    # a malformed stream: the decode call's code
    bad = frames.copy()
    bad[int(offs[3])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as e:
        codec.levels_host(bad, offs, 2)
    assert e.value.code == -5
    assert codec.levels_host(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2).shape == (0, 2)


def test_the_host_pointer_call_leaves_an_open_job_alone(gpu):  # noqa: F811
    lib = capi.lib()
    pcm = synth_frames(12, 2, 5)
    frames, offs = codec.encode_host(pcm)
    back = np.zeros(pcm.size, np.int16)
    job = C.c_void_p()
    ff = C.c_uint32(0)
    capi.check(lib.sela_hip_decode_begin(C.byref(job), 2, 12, back.ctypes.data))
    o = np.ascontiguousarray(offs[:6])
    capi.check(lib.sela_hip_decode_feed(job, frames.ctypes.data, o.ctypes.data, 5, C.byref(ff)))
    got = codec.levels_host(frames, offs, 2)
    o = np.ascontiguousarray(offs[5:] - offs[5])
    capi.check(lib.sela_hip_decode_feed(job, frames[int(offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12
    _same(got, _expect(back.reshape(-1, 2), np.arange(13) * 2048), "beside an open job")
