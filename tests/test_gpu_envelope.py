"""sela_hip_envelope_device, sela_hip_envelope_payload_device and sela_hip_envelope: per frame, bucket of samples
and channel the smallest and the largest value, the sum and the sum of squares of the int16 samples sela_hip_decode_n_device
writes.  The expectation is always numpy on int16 PCM, bucketed by _expect below -- for encoder-made streams the CPU oracle's
decode, for hand-built frames the oracle's decode of them too -- and every comparison is exact equality of all four fields.  status[0],
[1] and [3] are the decode call's; status[2] stays 0."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpu_common import _build_frame, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from sela_amd.synth import synth_frames
from test_gpu_verify_device import _bytes, _channels_pcm, _decode_n, _status_cases, _stream

pytestmark = pytest.mark.gpu

NONE, FAST, ANY = 0, 1, 2
GUARD = 16              # records behind d_env that no call may write
SENTINEL = 0x5E1A5E1A5E1A5E1A
ZERO = (0, 0, 0, 0)


def _slots(stride, bucket):
    return -(-stride // bucket)


def _expect(pcm, so, stride, bucket):
    """pcm: int16 [total samples, ch]; so: sample offsets [n + 1] -> the records, ENVELOPE_DTYPE [n, slots, ch], in numpy's int64."""
    p = np.asarray(pcm, np.int16)
    n, ch, slots = len(so) - 1, p.shape[1], _slots(stride, bucket)
    out = np.zeros((n, slots, ch), codec.ENVELOPE_DTYPE)
    for f in range(n):
        frame = p[int(so[f]): int(so[f + 1])].astype(np.int64)
        for b in range(slots):
            v = frame[b * bucket: (b + 1) * bucket]
            if len(v):
                out["min"][f, b], out["max"][f, b] = v.min(0), v.max(0)
                out["sum"][f, b], out["sum_squares"][f, b] = v.sum(0), (v * v).sum(0)
    return out


def _same(got, want, label=""):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    for name in codec.ENVELOPE_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (label, name, np.argwhere(got[name] != want[name])[:6].tolist())


class _Device:
    """Buffers of one sela_hip_envelope_device call, the raw C ABI: guard records behind d_env, d_frames kept for a look afterwards."""

    def __init__(self, torch, n, ch, stride, bucket):
        self.torch, self.n, self.ch, self.stride, self.bucket = torch, n, ch, stride, bucket
        self.slots = int(capi.lib().sela_hip_envelope_slots(stride, bucket))
        assert self.slots == _slots(stride, bucket)
        self.env = torch.full(((n * self.slots * ch + GUARD) * 2,), SENTINEL, dtype=torch.int64, device="cuda")
        self.sample_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_envelope_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")

    def measure(self, blob, offs, with_offsets=True):
        torch = self.torch
        data = _bytes(blob)
        frames = torch.zeros(max(len(data), 4), dtype=torch.uint8, device="cuda")
        if len(data):
            frames[: len(data)].copy_(torch.from_numpy(data))
        o = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).cuda()
        before = frames.clone()
        assert self.env.data_ptr() % 8 == 0
        capi.check(capi.lib().sela_hip_envelope_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, self.bucket, self.env.data_ptr(),
            self.sample_offsets.data_ptr() if with_offsets else None, self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(frames, before), "d_frames was written"
        return self.results()

    def results(self):
        words = self.env.cpu().numpy()
        k = self.n * self.slots * self.ch * 2
        assert (words[k:] == np.int64(SENTINEL)).all(), "written past d_env"
        return words[:k].copy().view(codec.ENVELOPE_DTYPE).reshape(self.n, self.slots, self.ch), self.status.cpu().numpy().view(np.uint32).copy()


def _check(torch, blob, offs, ch, stride, bucket, pcm, route, label="", dst=None, so=None):
    """The records of (stream) == numpy on pcm ([total, ch] int16), status as the decode call leaves it -> (records, status)."""
    n = len(offs) - 1
    if dst is None:
        _, so, dst = _decode_n(torch, blob, offs, ch, stride)
    assert codec.decode_n_status_error(dst) == 0, (label, dst)
    p = np.ascontiguousarray(pcm, np.int16).reshape(-1, ch)
    assert len(p) == int(so[n]), (label, len(p), int(so[n]))
    dev = _Device(torch, n, ch, stride, bucket)
    dev.env[: n * dev.slots * ch * 2] = SENTINEL + 1  # (nothing is pre-cleared: every record of a frame that ran is written)
    got, st = dev.measure(blob, offs)
    assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (label, st, dst)
    assert int(st[3]) == route and int(st[2]) == 0, (label, st)
    _same(got, _expect(p, so, stride, bucket), label)
    assert np.array_equal(dev.sample_offsets.cpu().numpy().view(np.uint64), so), label
    return got, st


@functools.lru_cache(maxsize=None)
def _channel_stream(n, ch, seed):
    """an encoder-made stream of n 2048-sample frames and the oracle's decode of it, made once"""
    pcm = _channels_pcm(n, ch, seed)
    frames, offs = codec.encode_i32(np.ascontiguousarray(pcm.transpose(0, 2, 1)).astype(np.int32))
    back, _ = oracle().decode_frames(frames, offs, ch, threads=4)
    return frames, offs, back.reshape(-1, ch)


# ---- 1. the fused route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bucket", [32, 64, 256, 512, 2048])
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_2048_sample_frames_on_the_fused_route(gpu, ch, bucket):  # noqa: F811
    frames, offs, back = _channel_stream(9, ch, 30 + ch)
    got, _ = _check(gpu, frames, offs, ch, 2048, bucket, back, FAST, f"{ch} channels, bucket {bucket}")
    assert got.shape == (9, 2048 // bucket, ch) and (got["max"] > got["min"]).any()
    wider, _ = _check(gpu, frames, offs, ch, 3000, bucket, back, FAST, f"{ch} channels, bucket {bucket}, a larger stride")
    filled = 2048 // bucket
    assert wider.shape[1] == _slots(3000, bucket) > filled
    _same(wider[:, :filled], got, "a larger stride gives the same records")
    assert all(r == ZERO for r in wider[:, filled:].reshape(-1).tolist()), "the slots behind the frame's end are zero records"


@pytest.mark.parametrize("bucket", [32, 256, 2048])
def test_the_golden_stereo_frames(gpu, kats, bucket):  # noqa: F811
    names = ["stereo_same_sine", "stereo_synth_diff", "stereo_silence", "stereo_synth_diff", "stereo_silence"]
    stream, offs = _stream([kats[f"frame/{n}/bytes"].tobytes() for n in names])
    back, _ = oracle().decode_frames(stream, offs, 2)
    got, st = _check(gpu, stream, offs, 2, 2048, bucket, back.reshape(-1, 2), FAST, "golden frames")
    for f in (2, 4):  # digital silence: all-zero records
        assert all(r == ZERO for r in got[f].reshape(-1).tolist())
    assert (got["sum_squares"][[0, 1, 3]] > 0).any(axis=(1, 2)).all()


@pytest.mark.parametrize("bucket", [32, 64, 128, 256, 512, 1024, 2048])
def test_full_scale_constants(gpu, bucket):  # noqa: F811
    pcm = np.empty((2048, 2), np.int16)
    pcm[:, 0], pcm[:, 1] = -32768, 32767
    blob = oracle().frame_encode(pcm)
    back, used = oracle().frame_decode(blob, 2)
    assert used == len(blob) and np.array_equal(back, pcm), "the oracle does not give this frame back"
    stream, offs = _stream([blob, blob])
    got, _ = _check(gpu, stream, offs, 2, 2048, bucket, np.concatenate([back, back]), FAST, "full scale")
    want = [(-32768, -32768, -32768 * bucket, bucket << 30), (32767, 32767, 32767 * bucket, bucket * 32767 * 32767)]
    for f in range(2):
        for b in range(2048 // bucket):
            assert got[f, b].tolist() == want, (f, b)
    if bucket == 2048:
        assert got[0, 0, 0].tolist() == (-32768, -32768, -(1 << 26), 1 << 41)


def _planted(amplitude, p):
    pcm = np.zeros((2048, 2), np.int16)
    pcm[p, 0] = amplitude
    pcm[(p + 1) % 2048, 1] = -amplitude if amplitude != -32768 else 32767
    return pcm


def _ramp():
    i = np.arange(2048)
    noise = np.random.default_rng(13).integers(-3, 4, (2048, 2))
    return (np.stack([13 * i, -7 * i], axis=1) + noise).astype(np.int16)


@pytest.mark.parametrize("bucket", [32, 256, 2048])
def test_bucket_edges(gpu, bucket):  # noqa: F811
    """One sample planted in silence on either channel, at the first and the last position of a bucket, across a bucket's and the
    frame's edge: exactly the buckets that hold the planted samples are not zero, and their extremes are the planted values."""
    cases = [(a, p) for a in (1000, -32768, 32767) for p in (0, bucket - 1, bucket % 2048, 1000, 2047)]
    pcms = [_planted(a, p) for a, p in cases] + [_ramp()]
    blobs = []
    for pcm in pcms:
        blob = oracle().frame_encode(pcm)
        back, used = oracle().frame_decode(blob, 2)
        assert used == len(blob) and np.array_equal(back, pcm), "the oracle does not give this frame back: the spike is not where the test says"
        blobs.append(blob)
    stream, offs = _stream(blobs)
    got, _ = _check(gpu, stream, offs, 2, 2048, bucket, np.concatenate(pcms), FAST, f"edges, bucket {bucket}")
    for f, (a, p) in enumerate(cases):
        other = -a if a != -32768 else 32767
        for c, (value, at) in enumerate(((a, p), (other, (p + 1) % 2048))):
            loud = np.flatnonzero([r != ZERO for r in got[f, :, c].tolist()]).tolist()
            assert loud == [at // bucket], (a, p, c, loud)
            r = got[f, at // bucket, c]
            assert (int(r["min"]), int(r["max"]), int(r["sum"]), int(r["sum_squares"])) == (min(value, 0), max(value, 0), value, value * value), (a, p, c, r)


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
    for bucket in (32, 512):
        _check(gpu, stream, offs, 1, 2048, bucket, _oracle_pcm([small, big, small], 1), FAST, "serial parse", st, so)
    # ... and as one channel of a stereo frame beside a subframe that fits the plan (the whole frame takes the fallback)
    two = _build_frame([(0, 0, 0, q_sine, rng.integers(-120000, 120000, 2048)), (1, 0, 1, q_sine, rng.integers(-50, 50, 2048))])
    stream, offs = _stream([two, two])
    _, so, st = _decode_n(gpu, stream, offs, 2, 2048)
    assert codec.decode_n_status_error(st) == 0 and int(st[3]) == FAST and int(so[-1]) == 2 * 2048
    for bucket in (64, 2048):
        _check(gpu, stream, offs, 2, 2048, bucket, _oracle_pcm([two, two], 2), FAST, "serial parse, stereo", st, so)


# ---- 2. the cold route -------------------------------------------------------------------------------------------------------------
def test_twelve_channels_of_2048(gpu):  # noqa: F811
    """k_decode_frames_wide into the workspace, then k_envelope_channels"""
    frames, offs, back = _channel_stream(5, 12, 50)
    for bucket in (32, 256, 2048):
        got, _ = _check(gpu, frames, offs, 12, 2048, bucket, back, FAST, f"12 channels, bucket {bucket}")
        wider, _ = _check(gpu, frames, offs, 12, 2100, bucket, back, FAST, f"12 channels, bucket {bucket}, a larger stride")
        _same(wider[:, : 2048 // bucket], got)
        assert all(r == ZERO for r in wider[:, 2048 // bucket:].reshape(-1).tolist())


@pytest.mark.parametrize("n", [1000, 5000])
def test_frames_of_other_lengths_from_the_device_encoder(gpu, n):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(n)
    pcm = np.stack([np.stack([_signal(rng, "tone", n, 15), _signal(rng, "noise", n, 12)], axis=1) for _ in range(5)]).astype(np.int16)
    enc = codec.Encoder32(5, 2, n)
    enc.encode(torch.from_numpy(np.ascontiguousarray(pcm)).cuda())  # (sela_hip_encode_n_device)
    frames, offs = enc.to_host()
    back, _ = oracle().decode_frames(frames, offs, 2, n=n, threads=4)
    flat = back.reshape(-1, 2)
    for bucket in (32, 256, 2048):
        got, _ = _check(torch, frames, offs, 2, n, bucket, flat, ANY, f"length {n}, bucket {bucket}")
        assert got.shape[1] == _slots(n, bucket)  # (5000: partial last buckets of 8, 136 and 904 samples)
        wider, _ = _check(torch, frames, offs, 2, n + 123, bucket, flat, ANY, f"length {n}, bucket {bucket}, a larger stride")
        _same(wider[:, : got.shape[1]], got)
        for mode in (0, 2):
            capi.lib().sela_hip_debug_standard_first(mode)
            try:
                _same(_check(torch, frames, offs, 2, n, bucket, flat, ANY, (n, bucket, "mode", mode))[0], got, ("mode", mode))
            finally:
                capi.lib().sela_hip_debug_standard_first(-1)
    if n == 5000:
        assert 5000 % 256 == 136 and 5000 % 2048 == 904


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
    for bucket in (32, 512):
        got, _ = _check(gpu, stream, so, 2, 2048, bucket, flat, ANY, "mixed lengths")
        assert all(r == ZERO for r in got[4, _slots(777, bucket):].reshape(-1).tolist()), "zero records behind the short frame's end"
        with pytest.raises(ValueError):
            codec.track_envelope(got, np.cumsum([0] + [2048] * 4 + [777] + [2048] * 2), bucket)


def test_a_whole_track_stream_on_the_absolute_grid(gpu):  # noqa: F811
    """a --keep-tail stream: 3 * 2048 + 777 samples as two frames of 2048 and a long last one, at the largest stride of such a stream"""
    rng = np.random.default_rng(21)
    total = 3 * 2048 + 777
    pcm = np.stack([_signal(rng, "tone", total, 15), _signal(rng, "noise", total, 12)], axis=1).astype(np.int16)
    frames, offs = codec.encode_whole_host(pcm, lossless=True)
    back, n_samples, _ = codec.decode_whole_host(frames, offs, 2)
    assert n_samples == total and np.array_equal(back[:total], pcm)
    n = len(offs) - 1
    for bucket in (32, 256, 2048):
        got, _ = _check(gpu, frames, offs, 2, 4095, bucket, pcm, ANY, f"whole track, bucket {bucket}")
        so = codec.index_samples(frames, offs, 2)[0]
        track = codec.track_envelope(got, so, bucket)
        want = _expect(pcm, np.array([0, total]), total, bucket)[0]
        _same(track, want, f"the track's grid, bucket {bucket}")
        assert track.shape == (_slots(total, bucket), 2) and n == 3


# ---- 3. consistency between calls ----------------------------------------------------------------------------------------------------
def test_folded_records_are_the_coarser_call_and_the_level_call(gpu):  # noqa: F811
    torch = gpu
    frames, offs, back = _channel_stream(9, 2, 32)
    fine, _ = _Device(torch, 9, 2, 2048, 32).measure(frames, offs)
    coarse, _ = _Device(torch, 9, 2, 2048, 256).measure(frames, offs)
    _same(codec.fold_envelope(fine, 8), coarse, "bucket 32 folded by 8 is bucket 256")
    whole = codec.fold_envelope(fine, 64)
    assert whole.shape == (9, 1, 2)
    lev = codec.Leveler(9, 2, 2048)
    d = torch.from_numpy(_bytes(frames)).cuda()
    o = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    levels = lev.records(lev.measure(d, o, 9))
    lev.check()
    assert np.array_equal(np.maximum(-whole["min"][:, 0].astype(np.int64), whole["max"][:, 0].astype(np.int64)), levels["peak"].astype(np.int64))
    assert np.array_equal(whole["sum"][:, 0].astype(np.int64), levels["sum"]) and np.array_equal(whole["sum_squares"][:, 0], levels["sum_squares"])


# ---- 4. status, guards, arguments ----------------------------------------------------------------------------------------------------
def test_status_words_are_the_decode_calls(gpu, kats):  # noqa: F811
    seen = set()
    for label, blob, offs, ch, stride, _pcm in _status_cases(kats):
        n = len(offs) - 1
        _, _, dst = _decode_n(gpu, blob, offs, ch, stride)
        for bucket in (32, 2048):
            _, st = _Device(gpu, n, ch, stride, bucket).measure(blob, offs)
            assert (int(st[0]), int(st[1]), int(st[2]), int(st[3])) == (int(dst[0]), int(dst[1]), 0, int(dst[3])), (label, st, dst)
            code = codec.decode_n_status_error(st)
            assert code == codec.decode_n_status_error(dst), (label, st, dst)
            seen.add(code)
    assert {0, -4, -5, -6} <= seen, seen


def test_no_frames(gpu):  # noqa: F811
    dev = _Device(gpu, 0, 2, 2048, 256)
    got, st = dev.measure(b"", np.zeros(1, np.uint64))
    assert (st == 0).all() and got.shape == (0, 8, 2)
    assert int(dev.sample_offsets[0].item()) == 0


def test_nothing_else_is_written_without_sample_offsets(gpu):  # noqa: F811
    pcm = synth_frames(4, 2, 4)
    frames, offs, _ = oracle().encode_frames(pcm)
    back, _ = oracle().decode_frames(frames, offs, 2)
    for stride in (2048, 2500):
        dev = _Device(gpu, 4, 2, stride, 128)
        got, st = dev.measure(frames, offs, with_offsets=False)
        assert (dev.sample_offsets.cpu().numpy() == -1).all()
        _same(got, _expect(back.reshape(-1, 2), np.arange(5) * 2048, stride, 128), stride)
        assert int(st[2]) == 0 and int(st[3]) == FAST


def test_argument_errors_enqueue_nothing(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    pcm = synth_frames(2, 2, 1)
    blob, o, _ = oracle().encode_frames(pcm)
    n = len(blob)
    buf = torch.from_numpy(np.concatenate([blob, np.zeros(4, np.uint8)])).cuda()
    offs = torch.from_numpy(o.view(np.int64).copy()).cuda()
    ws_bytes = int(lib.sela_hip_envelope_workspace_bytes(2, 2, 2048))
    ix_bytes = int(lib.sela_hip_index_workspace_bytes(n, 2))
    ws = torch.empty(ws_bytes + ix_bytes, dtype=torch.uint8, device="cuda")
    env = torch.full((2 * 8 * 2 * 2,), -1, dtype=torch.int64, device="cuda")
    so = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    fo = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    nf = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def dev(frames=buf.data_ptr(), fo_=offs.data_ptr(), nfr=2, channels=2, stride=2048, bucket=256, e=env.data_ptr(), st=status.data_ptr(), w=ws.data_ptr(),
            wb=ws_bytes):
        return lib.sela_hip_envelope_device(frames, fo_, nfr, channels, stride, bucket, e, so.data_ptr(), st, w, wb, stream)

    def pay(payload=buf.data_ptr(), channels=2, stride=2048, bucket=256, e=env.data_ptr(), st=status.data_ptr(), o_=fo.data_ptr(), k=nf.data_ptr(), w=ws.data_ptr(),
            wb=ws_bytes + ix_bytes):
        return lib.sela_hip_envelope_payload_device(payload, n, 2, channels, stride, bucket, e, so.data_ptr(), o_, k, st, w, wb, stream)

    for call, code in [(lambda: dev(frames=buf.data_ptr() + 1), -2), (lambda: dev(channels=0), -2), (lambda: dev(channels=256), -2),
                       (lambda: dev(stride=0), -2), (lambda: dev(e=None), -2), (lambda: dev(e=env.data_ptr() + 4), -2),
                       (lambda: dev(st=None), -2), (lambda: dev(w=None), -2), (lambda: dev(fo_=None), -2), (lambda: dev(frames=None), -2),
                       (lambda: dev(wb=ws_bytes - 1), -4), (lambda: dev(nfr=0x40000000), -2),
                       (lambda: dev(bucket=0), -2), (lambda: dev(bucket=16), -2), (lambda: dev(bucket=48), -2), (lambda: dev(bucket=4096), -2),
                       (lambda: pay(payload=buf.data_ptr() + 2), -2), (lambda: pay(channels=0), -2), (lambda: pay(stride=0), -2),
                       (lambda: pay(e=None), -2), (lambda: pay(e=env.data_ptr() + 4), -2), (lambda: pay(st=None), -2),
                       (lambda: pay(o_=None), -2), (lambda: pay(k=None), -2), (lambda: pay(w=None), -2), (lambda: pay(bucket=48), -2),
                       (lambda: pay(wb=ws_bytes + ix_bytes - 1), -4)]:
        assert call() == code
    torch.cuda.synchronize()  # nothing was enqueued: every output is as it was
    for t in (env, so, fo, nf, status):
        assert (t.cpu().numpy() == -1).all()
    # a workspace of the size asked for is enough, and no initialisation is needed
    ws.fill_(0xFF)
    back, _ = oracle().decode_frames(blob, o, 2)
    want = _expect(back.reshape(-1, 2), np.arange(3) * 2048, 2048, 256)
    assert dev() == 0
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert codec.decode_n_status_error(st) == 0 and int(st[2]) == 0 and int(st[3]) == FAST
    _same(env.cpu().numpy().view(codec.ENVELOPE_DTYPE).reshape(2, 8, 2), want)
    env.fill_(-1)
    assert pay() == 0
    torch.cuda.synchronize()
    assert int(nf.item()) == 2 and int(status[2].item()) == 0
    _same(env.cpu().numpy().view(codec.ENVELOPE_DTYPE).reshape(2, 8, 2), want)


# ---- 5. the payload form ---------------------------------------------------------------------------------------------------------------
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
    bucket = 64
    env = codec.Enveloper(max_frames, 2, stride, bucket)
    env.envelope.fill_(SENTINEL)
    records, count = env.measure_payload(torch.from_numpy(payload).cuda())
    env.check()
    assert int(count.item()) == n and env.route() == (FAST if shape == "2048" else ANY) and int(env.status[2].item()) == 0
    got = env.records(records)
    assert got.shape == (max_frames, _slots(stride, bucket), 2)
    _same(got[:n], _expect(back, so, stride, bucket), shape)
    assert (records[n:].cpu().numpy() == np.int64(SENTINEL)).all(), "frames from *d_n_frames on are left alone"
    assert np.array_equal(env.frame_offsets[: n + 1].cpu().numpy().view(np.uint64), offs)
    # ... and the device call on the index the payload call found gives the same records
    dev, _ = _Device(torch, n, 2, stride, bucket).measure(np.frombuffer(blob, np.uint8), offs)
    _same(got[:n], dev, "the payload call equals the device call on the index")
    track = codec.track_envelope(got[:n], so, bucket)
    _same(track, _expect(back, np.array([0, len(back)]), len(back), bucket)[0], "the track's grid")


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["measure", "measure_payload"])
def test_in_a_graph(gpu, form):  # noqa: F811
    torch = gpu
    n, bucket = 40, 128
    inputs = []
    for seed in (2, 5):
        frames, offs, _ = oracle().encode_frames(synth_frames(n, 2, seed), threads=4)
        back, _ = oracle().decode_frames(frames, offs, 2, threads=4)
        inputs.append((frames, offs, _expect(back.reshape(-1, 2), np.arange(n + 1) * 2048, 2048, bucket)))
    assert not np.array_equal(inputs[0][2]["sum_squares"], inputs[1][2]["sum_squares"])
    room = max(len(i[0]) for i in inputs)
    d_frames = torch.zeros(room, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

    def load(k):
        frames, offs, _ = inputs[k]
        d_frames.zero_()
        d_frames[: len(frames)].copy_(torch.from_numpy(frames))
        d_offs.copy_(torch.from_numpy(offs.view(np.int64).copy()))

    env = codec.Enveloper(n, 2, 2048, bucket)
    call = (lambda: env.measure(d_frames, d_offs, n)) if form == "measure" else (lambda: env.measure_payload(d_frames))
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
        env.envelope.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        _same(env.records(records), inputs[k][2], (form, k))
        assert env.status.cpu().numpy().tolist() == [0, 0, 0, FAST], (form, k)
        if form == "measure_payload":
            assert int(out[1].item()) == n


# ---- 7. the host-pointer call ----------------------------------------------------------------------------------------------------------
def test_the_host_pointer_call_equals_the_device_call(gpu):  # noqa: F811
    frames, offs, _ = oracle().encode_frames(synth_frames(40, 2, 2), threads=4)
    want, st = _Device(gpu, 40, 2, 2048, 256).measure(frames, offs)
    assert int(st[3]) == FAST and codec.decode_n_status_error(st) == 0
    _same(codec.envelope_host(frames, offs, 2, 256), want, "host call")
    wider, _ = _Device(gpu, 40, 2, 3000, 32).measure(frames, offs)
    _same(codec.envelope_host(frames, offs, 2, 32, stride=3000), wider, "host call, a stride of the caller's")
    capi.lib().sela_hip_debug_pcm_chunk_frames(7)  # (chunks that do not divide the stream)
    try:
        _same(codec.envelope_host(frames, offs, 2, 256), want, "host call in chunks of 7 frames")
    finally:
        capi.lib().sela_hip_debug_pcm_chunk_frames(0)
    # another length
    blobs = [_odd_frame(1500, seeds=(s, s + 10))[0] for s in (1, 2, 3)]
    stream, o = _stream(blobs)
    want, st = _Device(gpu, 3, 2, 1500, 512).measure(stream, o)
    assert int(st[3]) == ANY
    _same(codec.envelope_host(stream, o, 2, 512), want, "host call, another length")
    # a malformed stream, and a stride below the stream's frames: the decode call's codes
    bad = frames.copy()
    bad[int(offs[3])] ^= 0xFF
    for call, code in ((lambda: codec.envelope_host(bad, offs, 2, 256), -5), (lambda: codec.envelope_host(frames, offs, 2, 256, stride=2047), -4)):
        with pytest.raises(capi.SelaHipError) as e:
            call()
        assert e.value.code == code
    assert codec.envelope_host(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2, 256, stride=2048).shape == (0, 8, 2)


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
    got = codec.envelope_host(frames, offs, 2, 256)
    o = np.ascontiguousarray(offs[5:] - offs[5])
    capi.check(lib.sela_hip_decode_feed(job, frames[int(offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12
    _same(got, _expect(back.reshape(-1, 2), np.arange(13) * 2048, 2048, 256), "beside an open job")
