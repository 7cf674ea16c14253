"""sela_hip_digest_device, sela_hip_digest_payload_device, sela_hip_digest and sela_hip_crc32_device: per frame
the CRC-32 of the int16 bytes sela_hip_decode_n_device writes, and the track's from those.  The expectation is always zlib.crc32
on bytes -- for encoder-made streams the CPU oracle's decode, for hand-built ones the decode call's own output -- and every
comparison is exact equality.  status[0], [1] and [3] are the decode call's; status[2] is 0."""
import zlib

import numpy as np
import pytest

from gpu_common import _build_frame, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from sela_amd.synth import synth_frames
from test_gpu_verify_device import _bytes, _channels_pcm, _decode_n, _status_cases, _stream

pytestmark = pytest.mark.gpu

NONE, FAST, ANY = 0, 1, 2
GUARD = 16              # records behind d_digests that no call may write
SENTINEL = 0x5E1A5E1A5E1A5E1A


def _expect(pcm, so):
    """pcm: int16 [total samples, ch]; so: sample offsets [n + 1] -> (the records DIGEST_DTYPE [n], the track's CRC-32, its bytes)."""
    p = np.ascontiguousarray(pcm, "<i2")
    n = len(so) - 1
    out = np.zeros(n, codec.DIGEST_DTYPE)
    for f in range(n):
        part = p[int(so[f]): int(so[f + 1])]
        out[f] = (zlib.crc32(part.tobytes()), len(part))
    whole = p[int(so[0]): int(so[n])].tobytes()
    return out, zlib.crc32(whole), len(whole)


def _same(got, want, label=""):
    for name in codec.DIGEST_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (label, name, np.argwhere(got[name] != want[name])[:6].tolist())


class _Device:
    """Buffers of one sela_hip_digest_device call, the raw C ABI: guard records behind d_digests, d_frames kept for a look afterwards."""

    def __init__(self, torch, n, ch, stride):
        self.torch, self.n, self.ch, self.stride = torch, n, ch, stride
        self.digests = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
        self.track = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        self.sample_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_digest_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")

    def digest(self, blob, offs, with_offsets=True):
        torch = self.torch
        data = _bytes(blob)
        frames = torch.zeros(max(len(data), 4), dtype=torch.uint8, device="cuda")
        if len(data):
            frames[: len(data)].copy_(torch.from_numpy(data))
        o = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).cuda()
        before = frames.clone()
        capi.check(capi.lib().sela_hip_digest_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, self.digests.data_ptr(), self.track.data_ptr(),
            self.sample_offsets.data_ptr() if with_offsets else None, self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(frames, before), "d_frames was written"
        return self.results()

    def results(self):
        """-> (records, (track crc, track bytes), status)"""
        words = self.digests.cpu().numpy()
        assert (words[self.n:] == np.int64(SENTINEL)).all(), "written past d_digests"
        track = self.track.cpu().numpy().view(np.uint64)
        return words[: self.n].copy().view(codec.DIGEST_DTYPE).reshape(self.n), (int(track[0]), int(track[1])), self.status.cpu().numpy().view(np.uint32).copy()


def _check(torch, blob, offs, ch, stride, pcm, route, label=""):
    """The records and the track words of (stream) == zlib on pcm ([total, ch] int16), status as the decode call leaves it
    -> (records, track, status)."""
    n = len(offs) - 1
    decoded, so, dst = _decode_n(torch, blob, offs, ch, stride)
    assert codec.decode_n_status_error(dst) == 0, (label, dst)
    p = np.ascontiguousarray(pcm, np.int16).reshape(-1, ch)
    assert len(p) == int(so[n]), (label, len(p), int(so[n]))
    assert np.array_equal(decoded[: len(p)].cpu().numpy(), p), (label, "the decode call writes other bytes than the expectation's")
    want, want_crc, want_bytes = _expect(p, so)
    dev = _Device(torch, n, ch, stride)
    got, track, st = dev.digest(blob, offs)
    assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (label, st, dst)
    assert int(st[3]) == route and int(st[2]) == 0, (label, st)
    _same(got, want, label)
    assert track == (want_crc, want_bytes), (label, [hex(track[0]), track[1]], [hex(want_crc), want_bytes])
    assert np.array_equal(dev.sample_offsets.cpu().numpy().view(np.uint64), so), label
    return got, track, st


def _recurrence(form):
    capi.lib().sela_hip_debug_decode_recurrence(form)


# ---- 1. the fused route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_2048_sample_frames_on_the_fused_route(gpu, ch):  # noqa: F811
    pcm = _channels_pcm(9, ch, 30 + ch)
    frames, offs = codec.encode_i32(np.ascontiguousarray(pcm.transpose(0, 2, 1)).astype(np.int32))
    back, _ = oracle().decode_frames(frames, offs, ch, threads=4)
    got, track, _ = _check(gpu, frames, offs, ch, 2048, back.reshape(-1, ch), FAST, f"{ch} channels")
    assert (got["samples"] == 2048).all() and len(set(got["crc32"].tolist())) == 9
    wider, wide_track, _ = _check(gpu, frames, offs, ch, 3000, back.reshape(-1, ch), FAST, f"{ch} channels, a larger stride")
    _same(wider, got, "a larger stride gives the same records")
    assert wide_track == track
    for form in (0, 1):  # both forms of the synthesis recurrence
        _recurrence(form)
        try:
            again, again_track, _ = _check(gpu, frames, offs, ch, 2048, back.reshape(-1, ch), FAST, (ch, "recurrence form", form))
        finally:
            _recurrence(-1)
        _same(again, got, ("recurrence form", form))
        assert again_track == track


def test_the_golden_stereo_frames(gpu, kats):  # noqa: F811
    names = ["stereo_same_sine", "stereo_synth_diff", "stereo_silence", "stereo_synth_diff", "stereo_silence"]
    stream, offs = _stream([kats[f"frame/{n}/bytes"].tobytes() for n in names])
    back, _ = oracle().decode_frames(stream, offs, 2)
    got, _, _ = _check(gpu, stream, offs, 2, 2048, back.reshape(-1, 2), FAST, "golden frames")
    for f in (2, 4):  # digital silence
        assert int(got["crc32"][f]) == zlib.crc32(bytes(8192))
    assert int(got["crc32"][1]) == int(got["crc32"][3]) != int(got["crc32"][0])


def test_full_scale_constants(gpu):  # noqa: F811
    pcm = np.empty((2048, 2), np.int16)
    pcm[:, 0], pcm[:, 1] = -32768, 32767
    blob = oracle().frame_encode(pcm)
    back, used = oracle().frame_decode(blob, 2)
    assert used == len(blob) and np.array_equal(back, pcm), "the oracle does not give this frame back"
    stream, offs = _stream([blob, blob])
    got, _, _ = _check(gpu, stream, offs, 2, 2048, np.concatenate([back, back]), FAST, "full scale")
    assert int(got["crc32"][0]) == zlib.crc32(b"\x00\x80\xff\x7f" * 2048) == int(got["crc32"][1])


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_a_byte_wise_asymmetric_ramp(gpu, ch):  # noqa: F811
    """Every sample of the frame is another value, and no two channels agree anywhere: lanes, waves or channels that changed
    places would leave every sum as it is and change the CRC."""
    i = np.arange(2048, dtype=np.int32)
    pcm = np.stack([((i * (3 + 2 * c) + 257 * c + 11) % 60000 - 30000) for c in range(ch)], axis=1).astype(np.int16)
    assert len({pcm[:, c].tobytes() for c in range(ch)}) == ch and all(len(set(pcm[:, c].tolist())) == 2048 for c in range(ch))
    blob = oracle().frame_encode(pcm)
    back, used = oracle().frame_decode(blob, ch)
    assert used == len(blob)
    got, _, _ = _check(gpu, *_stream([blob]), ch, 2048, back, FAST, f"ramp, {ch} channels")
    flat = np.ascontiguousarray(back, "<i2")
    swapped = flat.copy()
    swapped[[64, 65]] = swapped[[65, 64]]           # two neighbouring lanes' samples
    assert int(got["crc32"][0]) != zlib.crc32(swapped.tobytes())
    if ch > 1:
        assert int(got["crc32"][0]) != zlib.crc32(np.ascontiguousarray(flat[:, ::-1]).tobytes())   # the channels


# ---- 2. the cold routes ------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 63, 64, 65, 2047, 2049, 4095, 65535]


def _odd_frame(n, ch, seed):
    """One frame of n samples and the PCM it decodes to.  Up to 100 samples the frame is hand-built from subframes of order 0 (the
    residues are the samples): an encoder's frame that short is routinely no longer than its own predictor's order, which the
    decode call refuses (SELA_HIP_FLAG_SHORT_BLOCK)."""
    rng = np.random.default_rng(seed)
    pcm = np.stack([_signal(rng, "tone" if c % 2 == 0 else "noise", n, 15 - 3 * (c % 2)) for c in range(ch)], axis=1).astype(np.int16)
    if n <= 100:
        return _build_frame([(c, 0, c, [], pcm[:, c].astype(np.int32)) for c in range(ch)]), pcm
    blob = oracle().frame_encode(pcm)
    back, used = oracle().frame_decode(blob, ch, n=n)
    assert used == len(blob) and back.shape == (n, ch)
    return blob, back


@pytest.mark.parametrize("ch", [1, 2])
def test_frames_of_other_lengths(gpu, ch):  # noqa: F811
    """odd byte counts, dword and line edges, frames of more than one slice: one frame a stream, and all of them in one stream"""
    made = [_odd_frame(n, ch, 100 * ch + k) for k, n in enumerate(LENGTHS)]
    for n, (blob, back) in zip(LENGTHS, made):
        got, track, _ = _check(gpu, *_stream([blob]), ch, n, back, ANY, f"length {n}, {ch} channels")
        assert got["samples"].tolist() == [n] and track[1] == n * ch * 2
    stream, offs = _stream([blob for blob, _ in made])
    got, _, _ = _check(gpu, stream, offs, ch, 65535, np.concatenate([back for _, back in made]), ANY, f"all lengths, {ch} channels")
    assert got["samples"].tolist() == LENGTHS


def test_nine_channels_of_2048(gpu):  # noqa: F811
    """k_decode_frames_wide into the workspace, then k_digest_pcm"""
    pcm = _channels_pcm(5, 9, 50)
    frames, offs = codec.encode_i32(np.ascontiguousarray(pcm.transpose(0, 2, 1)).astype(np.int32))
    back, _ = oracle().decode_frames(frames, offs, 9, threads=4)
    got, track, _ = _check(gpu, frames, offs, 9, 2048, back.reshape(-1, 9), FAST, "9 channels")
    wider, wide_track, _ = _check(gpu, frames, offs, 9, 2100, back.reshape(-1, 9), FAST, "9 channels, a larger stride")
    _same(wider, got)
    assert wide_track == track


@pytest.mark.parametrize("tail", [1, 777, 2047])
def test_a_whole_track_stream(gpu, tail):  # noqa: F811
    """codec.encode_whole_host, lossless: frames of 2048 and a last frame of 2048 + tail; the track word is zlib's of the original"""
    n_samples = 4 * 2048 + tail
    pcm = synth_frames(5, 2, 40 + tail).reshape(-1, 2)[:n_samples]
    frames, offs = codec.encode_whole_host(pcm, lossless=True)
    assert len(offs) - 1 == 4
    got, track, _ = _check(gpu, frames, offs, 2, 2048 + tail, pcm, ANY, f"whole track, tail {tail}")
    assert got["samples"].tolist() == [2048] * 3 + [2048 + tail]
    assert track == (zlib.crc32(np.ascontiguousarray(pcm, "<i2").tobytes()), n_samples * 4)


def test_a_frame_of_no_samples_between_two_others(gpu):  # noqa: F811
    """The decode call itself refuses a frame of no samples (SELA_HIP_FLAG_SHORT_BLOCK: the reference writes samples[0] whatever the
    length), so the status words say so and the records are formally not defined; the call still leaves the empty frame's record
    at (0, 0), and its neighbours' at the CRC of what the decode call writes for them."""
    rng = np.random.default_rng(3)
    a = _build_frame([(0, 0, 0, [], rng.integers(-900, 900, 300)), (1, 0, 1, [], rng.integers(-900, 900, 300))])
    z = _build_frame([(0, 0, 0, [], np.zeros(0, np.int32)), (1, 0, 1, [], np.zeros(0, np.int32))])
    b = _build_frame([(0, 0, 0, [], rng.integers(-900, 900, 300)), (1, 0, 1, [], rng.integers(-900, 900, 300))])
    stream, offs = _stream([a, z, b])
    back, so, dst = _decode_n(gpu, stream, offs, 2, 300)
    assert so.tolist() == [0, 300, 300, 600] and int(dst[3]) == ANY
    assert int(dst[0]) == capi.FLAG_SHORT_BLOCK and codec.decode_n_status_error(dst) == -6
    dev = _Device(gpu, 3, 2, 300)
    got, track, st = dev.digest(stream, offs)
    assert (int(st[0]), int(st[1]), int(st[2]), int(st[3])) == (int(dst[0]), int(dst[1]), 0, int(dst[3]))
    want, want_crc, want_bytes = _expect(back[:600].cpu().numpy(), so)
    _same(got, want, "an empty frame")
    assert got[1].tolist() == (0, 0) and track == (want_crc, want_bytes) and want_bytes == 2400


# ---- 3. the track fold -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(gpu):  # noqa: F811
    """300 stereo frames as blobs, and the oracle's decode of each: computed once, never changed."""
    pcm = synth_frames(300, 2, 12)
    frames, offs, _ = oracle().encode_frames(pcm, threads=4)
    back, _ = oracle().decode_frames(frames, offs, 2, threads=4)
    return [frames[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(300)], back.reshape(300, 2048, 2)


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_the_track_word_over_many_frames(gpu, many, n):  # noqa: F811
    blobs, back = many
    _, track, _ = _check(gpu, *_stream(blobs[:n]), 2, 2048, back[:n].reshape(-1, 2), FAST, f"{n} frames")
    if n > 1:
        order = np.random.default_rng(n).permutation(n) if n > 2 else np.array([1, 0])
        assert order.tolist() != list(range(n))
        _, shuffled, _ = _check(gpu, *_stream([blobs[k] for k in order]), 2, 2048, back[order].reshape(-1, 2), FAST, f"{n} frames, shuffled")
        assert shuffled[0] != track[0] and shuffled[1] == track[1]


# ---- 4. the payload form -----------------------------------------------------------------------------------------------------------
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
        last, last_back = _odd_frame(2048 + 777, 2, 7)
        blob, back, so, stride = blob + last, np.concatenate([back, last_back]), np.append(so, so[-1] + 2825), 2825
        offs = np.append(offs, offs[-1] + len(last)).astype(np.uint64)
    n = len(offs) - 1
    payload = np.frombuffer(blob + b"\x11" * 40, np.uint8).copy()  # (no sync word in the garbage: the walk ends at it)
    max_frames = n + 5
    dig = codec.Digester(max_frames, 2, stride)
    dig.digests = torch.full((max_frames + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")  # (guard records behind the call's)
    d_payload = torch.from_numpy(payload).cuda()
    before = d_payload.clone()
    records, track, count = dig.digest_payload(d_payload)
    dig.check()
    assert int(count.item()) == n and dig.route() == (FAST if shape == "2048" else ANY) and int(dig.status[2].item()) == 0
    want, want_crc, want_bytes = _expect(back, so)
    _same(dig.records(records)[:n], want, shape)
    assert dig.track_words() == (want_crc, want_bytes)
    assert (dig.digests[n:].cpu().numpy() == np.int64(SENTINEL)).all(), "frames from *d_n_frames on, and the guard behind d_digests, are left alone"
    assert np.array_equal(dig.frame_offsets[: n + 1].cpu().numpy().view(np.uint64), offs)
    assert torch.equal(d_payload, before), "the payload was written"


# ---- 5. bytes in device memory -----------------------------------------------------------------------------------------------------
def test_crc32_of_bytes_in_device_memory(gpu):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(32)
    host = rng.integers(0, 256, (1 << 20) + 3 + 3 + 16, dtype=np.uint8)
    data = torch.from_numpy(host).cuda()
    assert data.data_ptr() % 16 == 0
    outs = []
    for n in (0, 1, 2, 3, 4, 5, 255, 256, 257, (1 << 20) + 3):
        for offset in (0, 1, 2, 3):
            outs.append((n, offset, codec.crc32_device(data, n, offset)))
    torch.cuda.synchronize()
    for n, offset, out in outs:
        got = out.cpu().numpy().view(np.uint64)
        assert (int(got[0]), int(got[1])) == (zlib.crc32(host[offset: offset + n].tobytes()), n), (n, offset, hex(int(got[0])))
    # a decode's output against the digest of its stream: two figures, 16 bytes moved
    pcm = synth_frames(6, 2, 2)
    frames, offs, _ = oracle().encode_frames(pcm)
    back, so, st = _decode_n(torch, frames, offs, 2, 2048)
    _, track, _ = _Device(torch, 6, 2, 2048).digest(frames, offs)
    out = codec.crc32_device(back, 6 * 2048 * 4).cpu().numpy().view(np.uint64)
    assert (int(out[0]), int(out[1])) == track


# ---- 6. status, no frames, arguments -------------------------------------------------------------------------------------------------
def test_status_words_are_the_decode_calls(gpu, kats):  # noqa: F811
    seen = set()
    for label, blob, offs, ch, stride, _pcm in _status_cases(kats):
        n = len(offs) - 1
        _, _, dst = _decode_n(gpu, blob, offs, ch, stride)
        _, _, st = _Device(gpu, n, ch, stride).digest(blob, offs)
        assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (label, st, dst)
        assert int(st[2]) == 0, (label, st)
        code = codec.decode_n_status_error(st)
        assert code == codec.decode_n_status_error(dst), (label, st, dst)
        seen.add(code)
    assert {0, -4, -5, -6} <= seen, seen


def test_no_frames(gpu):  # noqa: F811
    dev = _Device(gpu, 0, 2, 2048)
    got, track, st = dev.digest(b"", np.zeros(1, np.uint64))
    assert (st == 0).all() and got.shape == (0,) and track == (0, 0)
    assert int(dev.sample_offsets[0].item()) == 0


def test_nothing_else_is_written_without_sample_offsets(gpu):  # noqa: F811
    pcm = synth_frames(4, 2, 4)
    frames, offs, _ = oracle().encode_frames(pcm)
    back, _ = oracle().decode_frames(frames, offs, 2)
    want, want_crc, want_bytes = _expect(back.reshape(-1, 2), np.arange(5) * 2048)
    for stride in (2048, 2500):
        dev = _Device(gpu, 4, 2, stride)
        dev.ws.fill_(0xFF)  # (no initialisation is needed)
        got, track, st = dev.digest(frames, offs, with_offsets=False)
        assert (dev.sample_offsets.cpu().numpy() == -1).all()
        _same(got, want, stride)
        assert track == (want_crc, want_bytes) and int(st[3]) == FAST


# ---- 7. capture --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["digest", "digest_payload"])
def test_in_a_graph(gpu, form):  # noqa: F811
    torch = gpu
    n = 40
    inputs = []
    for seed in (2, 5):
        frames, offs, _ = oracle().encode_frames(synth_frames(n, 2, seed), threads=4)
        back, _ = oracle().decode_frames(frames, offs, 2, threads=4)
        inputs.append((frames, offs, _expect(back.reshape(-1, 2), np.arange(n + 1) * 2048)))
    assert inputs[0][2][1] != inputs[1][2][1]
    room = max(len(i[0]) for i in inputs)
    d_frames = torch.zeros(room, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

    def load(k):
        frames, offs, _ = inputs[k]
        d_frames.zero_()
        d_frames[: len(frames)].copy_(torch.from_numpy(frames))
        d_offs.copy_(torch.from_numpy(offs.view(np.int64).copy()))

    dig = codec.Digester(n, 2, 2048)
    call = (lambda: dig.digest(d_frames, d_offs, n)) if form == "digest" else (lambda: dig.digest_payload(d_frames))
    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # (the workspace is allocated here, not under capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for k in (0, 1):
        load(k)
        dig.digests.fill_(-7)
        dig.track.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        want, want_crc, want_bytes = inputs[k][2]
        _same(dig.records(out[0]), want, (form, k))
        assert dig.track_words() == (want_crc, want_bytes), (form, k)
        assert dig.status.cpu().numpy().tolist() == [0, 0, 0, FAST], (form, k)
        if form == "digest_payload":
            assert int(out[2].item()) == n


# ---- 8. the host-pointer call ------------------------------------------------------------------------------------------------------
def test_the_host_pointer_call_equals_the_device_call(gpu):  # noqa: F811
    frames, offs, _ = oracle().encode_frames(synth_frames(40, 2, 2), threads=4)
    want, track, st = _Device(gpu, 40, 2, 2048).digest(frames, offs)
    assert int(st[3]) == FAST and codec.decode_n_status_error(st) == 0
    got, crc, total = codec.digest_host(frames, offs, 2)
    _same(got, want, "host call")
    assert (crc, total) == track
    # a whole-track stream, several chunks: the chunks' track words folded on the host
    pcm = synth_frames(7, 2, 77).reshape(-1, 2)[: 6 * 2048 + 777]
    stream, o = codec.encode_whole_host(pcm, lossless=True)
    want, track, st = _Device(gpu, 6, 2, 2825).digest(stream, o)
    assert int(st[3]) == ANY and track == (zlib.crc32(np.ascontiguousarray(pcm, "<i2").tobytes()), pcm.size * 2)
    for chunk in (0, 1, 2, 5):
        capi.lib().sela_hip_debug_pcm_chunk_frames(chunk)
        try:
            got, crc, total = codec.digest_host(stream, o, 2)
        finally:
            capi.lib().sela_hip_debug_pcm_chunk_frames(0)
        _same(got, want, ("chunk", chunk))
        assert (crc, total) == track, ("chunk", chunk)
    # a malformed stream: the decode call's code
    bad = frames.copy()
    bad[int(offs[3])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as e:
        codec.digest_host(bad, offs, 2)
    assert e.value.code == -5
    assert codec.digest_host(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2)[1:] == (0, 0)


def test_the_host_pointer_call_leaves_an_open_job_alone(gpu):  # noqa: F811
    import ctypes as C

    lib = capi.lib()
    pcm = synth_frames(12, 2, 5)
    frames, offs = codec.encode_host(pcm)
    back = np.zeros(pcm.size, np.int16)
    job = C.c_void_p()
    ff = C.c_uint32(0)
    capi.check(lib.sela_hip_decode_begin(C.byref(job), 2, 12, back.ctypes.data))
    o = np.ascontiguousarray(offs[:6])
    capi.check(lib.sela_hip_decode_feed(job, frames.ctypes.data, o.ctypes.data, 5, C.byref(ff)))
    got, crc, total = codec.digest_host(frames, offs, 2)
    o = np.ascontiguousarray(offs[5:] - offs[5])
    capi.check(lib.sela_hip_decode_feed(job, frames[int(offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12
    want, want_crc, want_bytes = _expect(back.reshape(-1, 2), np.arange(13) * 2048)
    _same(got, want, "beside an open job")
    assert (crc, total) == (want_crc, want_bytes)
