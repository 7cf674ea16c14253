"""sela_hip_digest_pcm_device, sela_hip_digest_payload_pcm_device and sela_hip_digest_pcm: per frame the CRC-32 of
the packed 3- or 4-byte PCM sela_hip_decode_pcm_device writes, and the track's from those.  Two yardsticks that share no code:
zlib.crc32 of the ORIGINAL packed bytes for lossless streams (no decoder of this project stands between), and zlib.crc32 of what
DecoderPcm.decode writes for everything else (that call is held against the reference elsewhere).  Every comparison is exact
equality; the four status words are DecoderPcm's; every output sits between guard words."""
import zlib

import numpy as np
import pytest

import topology_cases as tc
from gpu_common import _build_frame, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from test_gpu_pcm import pack_interleaved
from test_gpu_verify_i32_device import _fallback_layouts, _layout_blob, _on_device, _status_cases, _stream

pytestmark = pytest.mark.gpu

GUARD = 16                       # 8-byte words in front of and behind each output that no call may write
SENTINEL = 0x5E1A5E1A5E1A5E1A
WIDTHS = [3, 4]


def _tile(ch):
    return max((4096 // ch) & ~3, 4)


def _expect(raw, so, ch, b):
    """raw: the packed bytes of the whole stream; so: sample offsets [n + 1] -> (records DIGEST_DTYPE [n], the track's CRC-32, its bytes)."""
    raw = np.ascontiguousarray(raw, np.uint8)
    n = len(so) - 1
    out = np.zeros(n, codec.DIGEST_DTYPE)
    for f in range(n):
        part = raw[int(so[f]) * ch * b: int(so[f + 1]) * ch * b]
        out[f] = (zlib.crc32(part.tobytes()) if len(part) else 0, int(so[f + 1]) - int(so[f]))
    whole = raw[: int(so[n]) * ch * b].tobytes()
    return out, zlib.crc32(whole), len(whole)


def _same(got, want, label=""):
    for name in codec.DIGEST_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (label, name, np.argwhere(got[name] != want[name])[:6].tolist())


class _Guarded:
    """an exact-size int64 view inside a larger tensor of SENTINEL words"""

    def __init__(self, torch, words, fill):
        self.words = words
        self.big = torch.full((words + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
        self.view = self.big[GUARD: GUARD + words]
        self.view.fill_(fill)

    def intact(self):
        g = self.big.cpu().numpy()
        return bool((g[:GUARD] == np.int64(SENTINEL)).all() and (g[GUARD + self.words:] == np.int64(SENTINEL)).all())


class _Device:
    """Buffers of one sela_hip_digest_pcm_device call, the raw C ABI, each output between guard words; d_frames looked at afterwards."""

    def __init__(self, torch, n, ch, stride, b):
        self.torch, self.n, self.ch, self.stride, self.b = torch, n, ch, stride, b
        self.digests = _Guarded(torch, n, -7)
        self.track = _Guarded(torch, 2, -1)
        self.sample_offsets = _Guarded(torch, n + 1, -1)
        self.status = _Guarded(torch, 2, -1)  # (four 32-bit words)
        self.ws = torch.empty(int(capi.lib().sela_hip_digest_pcm_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")

    def digest(self, blob, offs, with_offsets=True):
        torch = self.torch
        frames, o = _on_device(torch, blob, offs)
        before = frames.clone()
        capi.check(capi.lib().sela_hip_digest_pcm_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, self.b, self.digests.view.data_ptr(), self.track.view.data_ptr(),
            self.sample_offsets.view.data_ptr() if with_offsets else None, self.status.view.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(frames, before), "d_frames was written"
        return self.results()

    def fallback(self):
        return int(capi.lib().sela_hip_debug_digest_pcm_fallback_frames(self.ws.data_ptr(), self.n, self.ch, self.stride))

    def results(self):
        """-> (records, (track crc, track bytes), status uint32 [4])"""
        for name in ("digests", "track", "sample_offsets", "status"):
            assert getattr(self, name).intact(), f"written outside {name}"
        words = self.digests.view.cpu().numpy()
        track = self.track.view.cpu().numpy().view(np.uint64)
        return (words.copy().view(codec.DIGEST_DTYPE).reshape(self.n), (int(track[0]), int(track[1])),
                self.status.view.cpu().numpy().view(np.uint32).copy())


def _decode_pcm(torch, blob, offs, ch, stride, b):
    """DecoderPcm.decode -> (its bytes uint8, sample offsets uint64 [n + 1], status uint32 [4])"""
    n = len(offs) - 1
    dec = codec.DecoderPcm(max(n, 1), ch, stride, b)
    dec.pcm.fill_(0xA5)
    frames, o = _on_device(torch, blob, offs)
    pcm, so = dec.decode(frames, o, n)
    torch.cuda.synchronize()
    return pcm.cpu().numpy().copy(), so.cpu().numpy().view(np.uint64).copy(), dec.status.cpu().numpy().view(np.uint32).copy()


def _check(torch, blob, offs, ch, stride, b, original=None, fallback=0, label=""):
    """The records and the track words of the stream == zlib on what DecoderPcm writes (and on `original`, the packed bytes the
    stream was made from, where given); the four status words are DecoderPcm's -> (records, track, status)."""
    n = len(offs) - 1
    decoded, so, dst = _decode_pcm(torch, blob, offs, ch, stride, b)
    assert codec.decode_pcm_status_error(dst) == 0, (label, dst)
    total = int(so[n]) * ch * b
    want, want_crc, want_bytes = _expect(decoded[:total], so, ch, b)
    dev = _Device(torch, n, ch, stride, b)
    got, track, st = dev.digest(blob, offs)
    assert st.tolist() == dst.tolist(), (label, st, dst)
    _same(got, want, label)
    assert track == (want_crc, want_bytes), (label, [hex(track[0]), track[1]], [hex(want_crc), want_bytes])
    assert np.array_equal(dev.sample_offsets.view.cpu().numpy().view(np.uint64), so), label
    assert dev.fallback() == fallback, (label, dev.fallback())
    if original is not None:
        original = np.ascontiguousarray(original, np.uint8).reshape(-1)
        assert original.size == total, (label, original.size, total)
        first, first_crc, _ = _expect(original, so, ch, b)
        _same(got, first, (label, "against the original bytes"))
        assert track[0] == first_crc, label
    return got, track, st


def _music(rng, n, ch, bits):
    """int32 [n, ch] interleaved: a tone or noise per channel"""
    return np.stack([_signal(rng, "tone" if c % 2 == 0 else "noise", n, bits - 2 - 3 * (c % 2)) for c in range(ch)], axis=1).astype(np.int32)


def _frame(n, ch, b, seed, bits=None):
    """One lossless frame of n samples and the packed bytes it was made from.  Up to 100 samples the frame is hand-built from
    subframes of order 0 (the residues are the samples): an encoder's frame that short is routinely no longer than its own
    predictor's order, which the decode call refuses (SELA_HIP_FLAG_SHORT_BLOCK)."""
    x = _music(np.random.default_rng(seed), n, ch, bits or (24 if b == 3 else 28))
    raw = pack_interleaved(x, b)
    if n <= 100:
        return _build_frame([(c, 0, c, [], x[:, c]) for c in range(ch)]), raw
    frames, offs = codec.encode_pcm_host(raw, ch, n, b, lossless=True)
    assert len(offs) == 2
    return frames.tobytes(), raw


def _strides(largest):
    up = (largest + 3) & ~3
    return [up, up + 1]


# ---- 1. channels and tile edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("ch", [1, 2, 3, 5, 8, 9])
def test_channels_and_tile_edges(gpu, ch, b):  # noqa: F811
    tile = _tile(ch)
    assert {1: 4096, 2: 2048, 3: 1364}.get(ch, tile) == tile
    lengths = [1, 2, 3, 4, 5, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1]
    made = [_frame(n, ch, b, 1000 * ch + 10 * b + k) for k, n in enumerate(lengths)]
    stream, offs = _stream([blob for blob, _ in made])
    original = np.concatenate([raw for _, raw in made])
    for stride in _strides(max(lengths)):
        got, track, _ = _check(gpu, stream, offs, ch, stride, b, original, 0, f"{ch} channels, {b} bytes, stride {stride}")
        assert got["samples"].tolist() == lengths and track[1] == sum(lengths) * ch * b
    # ... and the longest frame alone, at its own length for a stride
    blob, raw = made[-1]
    _check(gpu, *_stream([blob]), ch, lengths[-1], b, raw, 0, f"{ch} channels, {b} bytes, one frame")


@pytest.mark.parametrize("b", WIDTHS)
def test_255_channels(gpu, b):  # noqa: F811
    assert _tile(255) == 16
    lengths = [15, 16, 17, 33]
    made = [_frame(n, 255, b, 255 + k, bits=20) for k, n in enumerate(lengths)]
    stream, offs = _stream([blob for blob, _ in made])
    for stride in _strides(33):
        got, _, _ = _check(gpu, stream, offs, 255, stride, b, np.concatenate([raw for _, raw in made]), 0, f"255 channels, stride {stride}")
        assert got["samples"].tolist() == lengths


@pytest.mark.parametrize("b", WIDTHS)
def test_a_mono_frame_of_65535(gpu, b):  # noqa: F811
    blob, raw = _frame(65535, 1, b, 65)
    for stride in (65535, 65536):
        got, track, _ = _check(gpu, *_stream([blob]), 1, stride, b, raw, 0, f"65535 samples, stride {stride}")
        assert got["samples"].tolist() == [65535] and track == (zlib.crc32(raw.tobytes()), 65535 * b)


# ---- 2. orders -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_a_byte_wise_asymmetric_ramp(gpu, ch, b):  # noqa: F811
    """Every sample of a channel is another value, every byte of a sample differs from its other bytes, and no two channels agree
    anywhere: bytes, channels, lanes or tiles that changed places would change the CRC.  Two tiles and a bit."""
    n = 2 * _tile(ch) + 5
    i = np.arange(n, dtype=np.int64)
    top = 1 << (8 * b - 5)  # (a wrap of the ramp stays far inside what a residue can carry)
    x = np.stack([((i * (65537 + 2 * c) + 0x010203 * (c + 1)) % (2 * top) - top) for c in range(ch)], axis=1).astype(np.int32)
    assert all(len(set(x[:, c].tolist())) == n for c in range(ch)) and len({x[:, c].tobytes() for c in range(ch)}) == ch
    raw = pack_interleaved(x, b)
    frames, offs = codec.encode_pcm_host(raw, ch, n, b, lossless=True)
    for stride in _strides(n):
        got, _, _ = _check(gpu, frames, offs, ch, stride, b, raw, 0, f"ramp, {ch} channels, {b} bytes")
    crc = int(got["crc32"][0])
    assert crc != zlib.crc32(pack_interleaved(x.astype(">i4").view(np.int32), b).tobytes())      # the bytes of a sample
    swapped = x.copy()
    swapped[[64, 65]] = swapped[[65, 64]]                                                        # two neighbouring lanes' samples
    assert crc != zlib.crc32(pack_interleaved(swapped, b).tobytes())
    tiles = x.copy()
    t = _tile(ch)
    tiles[:t], tiles[t: 2 * t] = x[t: 2 * t], x[:t]                                              # two tiles
    assert crc != zlib.crc32(pack_interleaved(tiles, b).tobytes())
    if ch > 1:
        assert crc != zlib.crc32(pack_interleaved(np.ascontiguousarray(x[:, ::-1]), b).tobytes())  # the channels


def test_samples_beyond_24_bits_in_a_3_byte_container(gpu):  # noqa: F811
    """A 32-bit stream digested as 3-byte PCM: status[3] counts the planted samples, the CRC is that of their low three bytes."""
    rng = np.random.default_rng(24)
    n, ch = 2048 + 300, 2
    x = _music(rng, 2 * n, ch, 23).reshape(2, n, ch)
    assert x.min() >= -(1 << 23) and x.max() < (1 << 23)
    planted = [(0, 0, 0), (0, 1, 5), (0, 0, n - 1), (1, 1, 2047), (1, 0, 2048), (1, 1, n - 1), (1, 0, 77)]
    for k, (f, c, i) in enumerate(planted):
        x[f, i, c] = [1 << 23, -(1 << 23) - 1, (1 << 27) - 1, -(1 << 27), (1 << 24) + 3][k % 5]  # (a lossless residue stays below 2^30)
    frames, offs = codec.encode_pcm_host(pack_interleaved(x, 4), ch, n, 4, lossless=True)
    low = pack_interleaved(x, 3)
    for stride in _strides(n):
        got, track, st = _check(gpu, frames, offs, ch, stride, 3, low, 0, f"wide samples, stride {stride}")
        assert int(st[3]) == len(planted)
    dig = codec.DigesterPcm(2, ch, n, 3)
    dig.digest(*_on_device(gpu, frames, offs), 2)
    dig.check()
    assert dig.wide_samples() == len(planted)
    _, _, st4 = _check(gpu, frames, offs, ch, n, 4, pack_interleaved(x, 4), 0, "wide samples, 4 bytes")
    assert int(st4[3]) == 0


# ---- 3. layouts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("ch", [2, 3, 5])
def test_every_fallback_layout(gpu, ch, b):  # noqa: F811
    """Layouts the direct kernel leaves alone go through the combine: the control word counts them, the status words stay
    DecoderPcm's, and where DecoderPcm accepts the frame the record is that of its bytes -- and of a direct frame of the same audio."""
    o = oracle()
    layouts = _fallback_layouts(ch)
    if ch == 5:
        layouts.append(("a chain in stream order", dict(tc.refused_layouts(5))["a chain in stream order"]))
    good = [_layout_blob(o, layout, 7 * ch + k) for k, (_, layout) in enumerate(tc.ACCEPTED_LAYOUTS[ch][:2])]
    complete = []
    for k, (name, layout) in enumerate(layouts):
        blob = _layout_blob(o, layout, 900 + 10 * ch + k)
        offs = np.array([0, len(blob)], np.uint64)
        decoded, so, dst = _decode_pcm(gpu, blob, offs, ch, tc.N, b)
        dev = _Device(gpu, 1, ch, tc.N, b)
        got, track, st = dev.digest(blob, offs)
        assert st.tolist() == dst.tolist() and dev.fallback() == 1, (name, st, dst, dev.fallback())
        if codec.decode_pcm_status_error(dst) != 0:
            assert "chain" not in name
            continue
        _check(gpu, blob, offs, ch, tc.N + 2, b, None, 1, (name, "an odd stride"))
        # the same audio in a layout of the encoder's: the direct kernel's record
        raw = decoded[: tc.N * ch * b]
        again, again_offs = codec.encode_pcm_host(raw, ch, tc.N, b, lossless=True)
        direct, direct_track, _ = _check(gpu, again, again_offs, ch, tc.N, b, raw, 0, (name, "re-encoded"))
        _same(got, direct, name)
        assert track == direct_track
        complete.append(blob)
    assert len(complete) == (0 if ch == 2 else 1)
    # direct and fallback frames in one stream
    blobs = [good[0]] + complete + [good[1]] + complete + [good[0]]
    got, _, _ = _check(gpu, *_stream(blobs), ch, tc.N, b, None, 2 * len(complete), (ch, "mixed"))
    assert int(got["crc32"][0]) == int(got["crc32"][-1]) != int(got["crc32"][len(complete) + 1])


# ---- 4. status words -----------------------------------------------------------------------------------------------------------------
def _ragged_cases():
    rng = np.random.default_rng(9)

    def sub(c, typ, parent, n):
        return (c, typ, parent, [], rng.integers(-5000, 5000, n).astype(np.int32))

    plain = _build_frame([sub(0, 0, 0, 300), sub(1, 0, 1, 300), sub(2, 0, 2, 300)])
    direct = _build_frame([sub(0, 0, 0, 300), sub(1, 1, 0, 200), sub(2, 0, 2, 300)])            # a direct layout, channel 1 shorter
    other = _build_frame([sub(0, 0, 0, 300), sub(1, 1, 0, 300), sub(2, 1, 1, 200)])             # a chain, channel 2 shorter
    yield "channels disagree, a direct layout", _stream([plain, direct, plain]), 3, 300, (0, 1)
    yield "channels disagree, a fallback layout", _stream([plain, other, plain]), 3, 300, (1, 1)
    yield "both", _stream([direct, plain, other, direct]), 3, 301, (1, 3)


@pytest.mark.parametrize("b", WIDTHS)
def test_status_words_are_decoder_pcms(gpu, b):  # noqa: F811
    seen = set()
    for label, (blob, offs), ch, stride, (fallback, refused) in _ragged_cases():
        n = len(offs) - 1
        _, _, dst = _decode_pcm(gpu, blob, offs, ch, stride, b)
        dev = _Device(gpu, n, ch, stride, b)
        _, _, st = dev.digest(blob, offs)
        assert st.tolist() == dst.tolist(), (label, st, dst)
        assert int(st[0]) & capi.FLAG_BAD_FRAME and int(st[1]) == refused and dev.fallback() == fallback, (label, st, dev.fallback())
        seen.add(codec.decode_pcm_status_error(st))
    for label, blob, offs, ch, stride in _status_cases():  # a malformed frame in the middle, a truncated one, a stride too small, ...
        n = len(offs) - 1
        _, _, dst = _decode_pcm(gpu, blob, offs, ch, stride, b)
        _, _, st = _Device(gpu, n, ch, stride, b).digest(blob, offs)
        assert st.tolist() == dst.tolist(), (label, st, dst)
        if label == "stride too small":
            assert int(st[0]) & capi.FLAG_STRIDE
        code = codec.decode_pcm_status_error(st)
        assert code == codec.decode_pcm_status_error(dst)
        seen.add(code)
    assert seen == {0, -4, -5}, seen


# ---- 5. streams ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", WIDTHS)
def test_frames_of_different_lengths(gpu, b):  # noqa: F811
    lengths = [2048, 2048, 2048 + 777, 128]
    made = [_frame(n, 2, b, 50 + k) for k, n in enumerate(lengths)]
    stream, offs = _stream([blob for blob, _ in made])
    for stride in (2825, 2828):
        got, _, _ = _check(gpu, stream, offs, 2, stride, b, np.concatenate([raw for _, raw in made]), 0, f"mixed lengths, stride {stride}")
        assert got["samples"].tolist() == lengths


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("tail", [1, 777, 2047])
def test_a_whole_track_stream(gpu, tail, b):  # noqa: F811
    """codec.encode_whole_pcm_host, lossless: frames of 2048 and a last frame of 2048 + tail; the track word is zlib's of the original"""
    n_samples = 3 * 2048 + tail
    raw = pack_interleaved(_music(np.random.default_rng(40 + tail), n_samples, 2, 23 if b == 3 else 28), b)
    frames, offs = codec.encode_whole_pcm_host(raw, 2, b, lossless=True)
    assert len(offs) - 1 == 3
    got, track, _ = _check(gpu, frames, offs, 2, 2048 + tail, b, raw, 0, f"whole track, tail {tail}")
    assert got["samples"].tolist() == [2048] * 2 + [2048 + tail]
    assert track == (zlib.crc32(raw.tobytes()), n_samples * 2 * b)


@pytest.mark.parametrize("b", WIDTHS)
def test_300_short_frames(gpu, b):  # noqa: F811
    """more than 256 frames: the track fold has more than one workgroup"""
    n = 128
    raw = pack_interleaved(_music(np.random.default_rng(300), 300 * n, 2, 22), b)
    frames, offs = codec.encode_pcm_host(raw, 2, n, b, lossless=True)
    assert len(offs) - 1 == 300
    _, track, _ = _check(gpu, frames, offs, 2, n, b, raw, 0, "300 frames")
    order = np.random.default_rng(3).permutation(300)
    blobs = [frames[int(offs[k]): int(offs[k + 1])].tobytes() for k in order]
    shuffled_raw = raw.reshape(300, -1)[order].reshape(-1)
    _, shuffled, _ = _check(gpu, *_stream(blobs), 2, n, b, shuffled_raw, 0, "300 frames, shuffled")
    assert shuffled[0] != track[0] and shuffled[1] == track[1]


@pytest.mark.parametrize("b", WIDTHS)
def test_a_frame_of_no_samples_between_two_others(gpu, b):  # noqa: F811
    """As for the 16-bit digest: the decode call itself refuses a frame of no samples (SELA_HIP_FLAG_SHORT_BLOCK), so the status words
    say so and the records are formally not defined; the call still leaves the empty frame's record at (0, 0), and its neighbours' at
    the CRC of what the decode call writes for them."""
    rng = np.random.default_rng(3)
    a = _build_frame([(0, 0, 0, [], rng.integers(-900000, 900000, 300)), (1, 0, 1, [], rng.integers(-900, 900, 300))])
    z = _build_frame([(0, 0, 0, [], np.zeros(0, np.int32)), (1, 0, 1, [], np.zeros(0, np.int32))])
    c = _build_frame([(0, 0, 0, [], rng.integers(-900, 900, 300)), (1, 0, 1, [], rng.integers(-900000, 900000, 300))])
    stream, offs = _stream([a, z, c])
    decoded, so, dst = _decode_pcm(gpu, stream, offs, 2, 300, b)
    assert so.tolist() == [0, 300, 300, 600]
    assert int(dst[0]) == capi.FLAG_SHORT_BLOCK and codec.decode_pcm_status_error(dst) == -6
    got, track, st = _Device(gpu, 3, 2, 300, b).digest(stream, offs)
    assert st.tolist() == dst.tolist()
    want, want_crc, want_bytes = _expect(decoded[: 600 * 2 * b], so, 2, b)
    _same(got, want, "an empty frame")
    assert got[1].tolist() == (0, 0) and track == (want_crc, want_bytes) and want_bytes == 1200 * b


# ---- 6. the payload form, no frames, no offsets -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", WIDTHS)
def test_a_payload_with_trailing_garbage(gpu, b):  # noqa: F811
    torch = gpu
    lengths = [2048] * 4 + [2048 + 777]
    made = [_frame(n, 2, b, 80 + k) for k, n in enumerate(lengths)]
    stream, offs = _stream([blob for blob, _ in made])
    raw = np.concatenate([r for _, r in made])
    so = np.cumsum([0] + lengths)
    n = len(lengths)
    payload = np.frombuffer(stream.tobytes() + b"\x11" * 40, np.uint8).copy()  # (no sync word in the garbage: the walk ends at it)
    max_frames = n + 5
    dig = codec.DigesterPcm(max_frames, 2, 2825, b)
    guarded = _Guarded(torch, max_frames, -7)
    dig.digests = guarded.view
    d_payload = torch.from_numpy(payload).cuda()
    before = d_payload.clone()
    records, track, count = dig.digest_payload(d_payload)
    dig.check()
    assert int(count.item()) == n and dig.wide_samples() == 0
    want, want_crc, want_bytes = _expect(raw, so, 2, b)
    _same(dig.records(records)[:n], want, "payload")
    assert dig.track_words() == (want_crc, want_bytes)
    assert guarded.intact() and (dig.digests[n:].cpu().numpy() == -7).all(), "frames from *d_n_frames on, and the guards round d_digests, are left alone"
    assert np.array_equal(dig.frame_offsets[: n + 1].cpu().numpy().view(np.uint64), offs)
    assert np.array_equal(dig.sample_offsets[: n + 1].cpu().numpy(), so)
    assert torch.equal(d_payload, before), "the payload was written"


@pytest.mark.parametrize("b", WIDTHS)
def test_no_frames(gpu, b):  # noqa: F811
    dev = _Device(gpu, 0, 2, 2048, b)
    got, track, st = dev.digest(b"", np.zeros(1, np.uint64))
    assert (st == 0).all() and got.shape == (0,) and track == (0, 0)
    assert int(dev.sample_offsets.view[0].item()) == 0


@pytest.mark.parametrize("b", WIDTHS)
def test_nothing_else_is_written_without_sample_offsets(gpu, b):  # noqa: F811
    made = [_frame(n, 2, b, 90 + k) for k, n in enumerate([2048, 500, 2049])]
    stream, offs = _stream([blob for blob, _ in made])
    want, want_crc, want_bytes = _expect(np.concatenate([r for _, r in made]), np.array([0, 2048, 2548, 4597]), 2, b)
    for stride in (2049, 2052):
        dev = _Device(gpu, 3, 2, stride, b)
        dev.ws.fill_(0xFF)  # (no initialisation is needed)
        got, track, st = dev.digest(stream, offs, with_offsets=False)
        assert (dev.sample_offsets.view.cpu().numpy() == -1).all()
        _same(got, want, stride)
        assert track == (want_crc, want_bytes) and st.tolist() == [0, 0, 2049, 0]


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("form", ["digest", "digest_payload"])
def test_in_a_graph(gpu, form, b):  # noqa: F811
    torch = gpu
    n = 12
    inputs = []
    for seed in (2, 5):
        raw = pack_interleaved(_music(np.random.default_rng(seed), n * 2048, 2, 23 if b == 3 else 28), b)
        frames, offs = codec.encode_pcm_host(raw, 2, 2048, b, lossless=True)
        inputs.append((frames, offs, _expect(raw, np.arange(n + 1) * 2048, 2, b)))
    assert inputs[0][2][1] != inputs[1][2][1]
    room = max(len(i[0]) for i in inputs) + 4
    d_frames = torch.zeros(room, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

    def load(k):
        frames, offs, _ = inputs[k]
        d_frames.zero_()
        d_frames[: len(frames)].copy_(torch.from_numpy(frames))
        d_offs.copy_(torch.from_numpy(offs.view(np.int64).copy()))

    dig = codec.DigesterPcm(n, 2, 2048, b)
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
        assert dig.status.cpu().numpy().tolist() == [0, 0, 2048, 0], (form, k)
        # the direct kernel took every frame (the payload form's own workspace lies behind its index part)
        own = dig.workspace.data_ptr() if form == "digest" else dig.payload_workspace.data_ptr() + int(capi.lib().sela_hip_index_workspace_bytes(d_frames.numel(), n))
        assert int(capi.lib().sela_hip_debug_digest_pcm_fallback_frames(own, n, 2, 2048)) == 0, (form, k)
        if form == "digest_payload":
            assert int(out[2].item()) == n


# ---- 8. the host-pointer call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", WIDTHS)
def test_the_host_pointer_call_equals_the_device_call(gpu, b):  # noqa: F811
    n_samples = 6 * 2048 + 777
    x = _music(np.random.default_rng(77), n_samples, 2, 23)
    x[5, 0], x[3 * 2048 + 9, 1], x[n_samples - 1, 0] = 1 << 23, -(1 << 23) - 1, 1 << 27   # (three samples beyond 24 bits, in three chunks of two frames)
    stream, o = codec.encode_whole_pcm_host(pack_interleaved(x, 4), 2, 4, lossless=True)
    raw = pack_interleaved(x, b)
    want, track, st = _Device(gpu, 6, 2, 2825, b).digest(stream, o)
    assert codec.decode_pcm_status_error(st) == 0 and track == (zlib.crc32(raw.tobytes()), raw.size)
    for chunk in (0, 1, 2, 5):
        capi.lib().sela_hip_debug_pcm_chunk_frames(chunk)
        try:
            got, crc, total, wide = codec.digest_pcm_host(stream, o, 2, b)
        finally:
            capi.lib().sela_hip_debug_pcm_chunk_frames(0)
        _same(got, want, ("chunk", chunk))
        assert (crc, total) == track and wide == (3 if b == 3 else 0), ("chunk", chunk, wide)
    # each output may be missing
    lib = capi.lib()
    fr, offs = np.ascontiguousarray(stream, np.uint8), np.ascontiguousarray(o, np.uint64)
    assert lib.sela_hip_digest_pcm(fr.ctypes.data, offs.ctypes.data, 6, 2, b, None, None, None, None) == 0
    # a malformed stream: the decode call's code
    bad = stream.copy()
    bad[int(o[3])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as e:
        codec.digest_pcm_host(bad, o, 2, b)
    assert e.value.code == -5
    with pytest.raises(capi.SelaHipError) as e:
        codec.decode_pcm_host(bad, o, 2, b)
    assert e.value.code == -5
    assert codec.digest_pcm_host(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2, b)[1:] == (0, 0, 0)


def test_the_host_pointer_call_leaves_an_open_job_alone(gpu):  # noqa: F811
    import ctypes as C

    from sela_amd.synth import synth_frames

    lib = capi.lib()
    pcm = synth_frames(12, 2, 5)
    frames, offs = codec.encode_host(pcm)
    back = np.zeros(pcm.size, np.int16)
    job = C.c_void_p()
    ff = C.c_uint32(0)
    capi.check(lib.sela_hip_decode_begin(C.byref(job), 2, 12, back.ctypes.data))
    o = np.ascontiguousarray(offs[:6])
    capi.check(lib.sela_hip_decode_feed(job, frames.ctypes.data, o.ctypes.data, 5, C.byref(ff)))
    got, crc, total, wide = codec.digest_pcm_host(frames, offs, 2, 3)
    o = np.ascontiguousarray(offs[5:] - offs[5])
    capi.check(lib.sela_hip_decode_feed(job, frames[int(offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12
    assert np.array_equal(back, codec.decode_host(frames, offs, 2).reshape(-1)), "the job's output"
    raw, _ = codec.decode_pcm_host(frames, offs, 2, 3)
    want, want_crc, want_bytes = _expect(raw, np.arange(13) * 2048, 2, 3)
    _same(got, want, "beside an open job")
    assert (crc, total, wide) == (want_crc, want_bytes, 0)
