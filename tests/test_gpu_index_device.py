"""sela_hip_index_frames_device and sela_hip_decode_payload_device: the frames of a payload found on the device are the host
walk's (sela_hip_index_frames) bit for bit, on every input, and a payload decoded on the device alone is the offset decode."""
import os
import struct

import numpy as np
import pytest

from gpu_common import gpu  # noqa: F401
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

SYNC = struct.pack("<I", 0xAA55FF00)


def _host_walk(payload, max_frames, channels):
    fr = np.frombuffer(bytes(payload), np.uint8).copy() if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, np.uint8)
    offs = np.zeros(max_frames + 1, np.uint64)
    found = capi.lib().sela_hip_index_frames(fr.ctypes.data, fr.nbytes, max_frames, channels, offs.ctypes.data)
    return offs[: found + 1], int(found)


class _Indexer:
    """One device buffer of `capacity` bytes, its workspace and outputs; index() takes any prefix of it."""

    def __init__(self, torch, capacity, max_frames):
        self.torch = torch
        self.buf = torch.zeros(max(capacity, 4), dtype=torch.uint8, device="cuda")
        self.ws = torch.empty(codec.index_workspace_bytes(capacity, max_frames), dtype=torch.uint8, device="cuda")
        self.offsets = torch.empty(max_frames + 1, dtype=torch.int64, device="cuda")
        self.count = torch.empty(1, dtype=torch.int32, device="cuda")

    def load(self, payload):
        data = np.frombuffer(bytes(payload), np.uint8)
        if len(data):
            self.buf[: len(data)].copy_(self.torch.from_numpy(data.copy()))
        return len(data)

    def index(self, n_bytes, max_frames, channels):
        self.offsets.fill_(-1)  # (entries beyond [found] must stay as they are)
        capi.check(capi.lib().sela_hip_index_frames_device(
            self.buf.data_ptr(), n_bytes, max_frames, channels, self.offsets.data_ptr(), self.count.data_ptr(), self.ws.data_ptr(),
            self.ws.numel(), self.torch.cuda.current_stream().cuda_stream))
        n = int(self.count.item())
        offs = self.offsets.cpu().numpy()
        assert (offs[n + 1: max_frames + 1] == -1).all(), "written beyond [found]"
        return offs[: n + 1].view(np.uint64), n


def _same(gpu, payload, channels, caps, indexer=None):  # noqa: F811
    payload = bytes(payload)
    ix = indexer or _Indexer(gpu, len(payload), max(caps))
    n_bytes = ix.load(payload)
    for cap in caps:
        want, wn = _host_walk(payload, cap, channels)
        got, gn = ix.index(n_bytes, cap, channels)
        assert gn == wn and np.array_equal(got, want), (cap, len(payload), wn, gn, want[-3:], got[-3:])


def _stream(n_frames, channels, track=0):
    frames, offs = codec.encode_host(synth_frames(n_frames, channels, track))
    return frames.tobytes(), offs


# every max_frames below, at and above the true count, 0, and one above the one-workgroup limit (the device-wide rounds)
def _caps(n):
    return sorted({0, 1, max(n - 1, 0), n, n + 1, 2 * n + 3, 5000})


@pytest.mark.gpu
def test_bench_sized_stream(gpu):  # noqa: F811
    blob, offs = _stream(3875, 2, 0)
    want, n = _host_walk(blob, 3875, 2)
    assert n == 3875 and np.array_equal(want, offs)
    _same(gpu, blob, 2, [0, 1, 2, 3, 1000, 3874, 3875, 3876, 4096, 4097, 8000, 20000])


@pytest.mark.gpu
def test_golden_frames(gpu, kats):  # noqa: F811
    blobs = [kats["frame/stereo_same_sine/bytes"], kats["frame/stereo_synth_diff/bytes"], kats["frame/stereo_silence/bytes"]]
    stream = np.concatenate(blobs).tobytes()
    _same(gpu, stream, 2, [0, 1, 2, 3, 4, 9, 5000])


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 2, 6, 9, 255])
def test_channel_counts(gpu, channels):  # noqa: F811
    n = 3 if channels == 255 else 17
    blob, _ = _stream(n, channels, 1)
    _same(gpu, blob, channels, _caps(n))
    _same(gpu, blob, channels + 1 if channels < 255 else 1, _caps(n))  # (the same bytes read with another channel count)


@pytest.mark.gpu
def test_tiny_and_unaligned_lengths(gpu):  # noqa: F811
    blob, _ = _stream(3, 2, 2)
    ix = _Indexer(gpu, len(blob) + 64, 8)
    for payload in [b"", SYNC[:1], SYNC[:2], SYNC[:3], SYNC, SYNC + b"\0" * 7, blob + b"\x01", blob + b"\x01\x02\x03", blob[:-1], blob[:-2], blob[:-3]]:
        _same(gpu, payload, 2, [0, 1, 3, 8], ix)


@pytest.mark.gpu
def test_every_truncation_point(gpu):  # noqa: F811
    blob, offs = _stream(6, 2, 3)
    ix = _Indexer(gpu, len(blob), 8)
    ix.load(blob)
    for length in range(len(blob) + 1):
        for cap in (6, 8):
            want, wn = _host_walk(blob[:length], cap, 2)
            got, gn = ix.index(length, cap, 2)
            assert gn == wn and np.array_equal(got, want), (length, cap)


@pytest.mark.gpu
def test_bad_sync_word_and_trailing_garbage(gpu):  # noqa: F811
    blob, offs = _stream(6, 2, 4)
    for k in range(6):
        bad = bytearray(blob)
        bad[int(offs[k]) + 1] ^= 0x40
        _same(gpu, bad, 2, [3, 6, 7, 5000])
    rng = np.random.default_rng(5)
    for tail in (rng.integers(0, 256, 999, dtype=np.uint8).tobytes(), SYNC + rng.integers(0, 256, 64, dtype=np.uint8).tobytes(),
                 SYNC + struct.pack("<BBBBHB", 0, 0, 0, 0, 0, 0) + struct.pack("<BHH", 0, 0, 2048) + SYNC):
        _same(gpu, blob + tail, 2, [6, 7, 20, 5000])


def _frame_hiding_a_fake(channels, target_distance, gap_words=64):
    """A frame whose first residue stream holds, `gap_words` words in, a sync word and a fake header of `channels` subframes
    whose frame would end `target_distance` bytes after the end of this frame (0: on the frame right behind it).  The fake
    is a candidate and its `next` lands on a true frame: a chain that merges with the true one."""
    fake_at = 4 + 12 + 4 * gap_words  # from the start of this frame
    fake_fixed = 4 + 12 * channels
    res_words = gap_words + fake_fixed // 4 + 8
    own_len = 4 + 12 * channels + 4 * res_words + 4 * (channels - 1)
    rest = own_len + target_distance - fake_at - fake_fixed
    assert rest % 4 == 0 and 0 <= rest // 4 <= 65535
    fake = bytearray(SYNC)
    for c in range(channels):
        fake += struct.pack("<BBBBHB", c, 0, c, 0, 0, 0) + struct.pack("<BHH", 0, rest // 4 if c == channels - 1 else 0, 2048)
    rng = np.random.default_rng(channels)
    residue = bytearray(rng.integers(0, 256, 4 * res_words, dtype=np.uint8).tobytes())
    residue[4 * gap_words: 4 * gap_words + len(fake)] = fake
    out = bytearray(SYNC) + struct.pack("<BBBBHB", 0, 0, 0, 0, 0, 0) + struct.pack("<BHH", 3, res_words, 2048) + residue
    for c in range(1, channels):
        out += struct.pack("<BBBBHB", c, 0, c, 0, 0, 0) + struct.pack("<BHH", 0, 1, 2048) + b"\0\0\0\0"
    assert len(out) == own_len
    return bytes(out), fake_at, fake_at + fake_fixed + rest


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 2])
def test_merging_chain(gpu, channels):  # noqa: F811
    """A sync word in residue data whose crafted header points at a real later frame: ranked from the head, never reached."""
    blob, offs = _stream(4, channels, 6)
    frames = [blob[int(offs[i]): int(offs[i + 1])] for i in range(4)]
    for target in (0, len(frames[1]), len(frames[1]) + len(frames[2])):
        x, fake_at, fake_end = _frame_hiding_a_fake(channels, target)
        stream = frames[0] + x + b"".join(frames[1:])
        want, wn = _host_walk(stream, 16, channels)
        assert wn == 5
        start = len(frames[0])
        assert stream[start + fake_at: start + fake_at + 4] == SYNC and start + fake_end in want.tolist()  # (it merges)
        _same(gpu, stream, channels, [1, 2, 5, 6, 16, 5000])
        # ... and with the true frame in front of the fake corrupted, the fake is still not a frame
        bad = bytearray(stream)
        bad[start] ^= 1
        _same(gpu, bad, channels, [1, 5, 5000])


@pytest.mark.gpu
def test_only_sync_words_in_the_workspace_the_formula_gives(gpu):  # noqa: F811
    """The worst case of the workspace: every word a sync word, most of them candidates (a subframe that says 0xFF00
    coefficient words and as many residue words: about 1 MiB per channel), chains from every one of them."""
    lib = capi.lib()
    for n_bytes, caps in ((4 << 20, (1, 4, 5000)), ((1 << 16) + 2, (2, 5000))):
        payload = SYNC * (n_bytes // 4) + SYNC[: n_bytes % 4]
        for cap in caps:
            ix = _Indexer(gpu, n_bytes, cap)
            exact = int(lib.sela_hip_index_workspace_bytes(n_bytes, cap))
            assert ix.ws.numel() == exact
            for channels in (1, 2):
                _same(gpu, payload, channels, [cap], ix)


@pytest.mark.gpu
def test_header_field_mutations(gpu):  # noqa: F811
    """Single-byte mutations of the sync words and the subframe headers (the fields the walk reads and those it skips)."""
    trials = int(os.environ.get("SELA_INDEX_TRIALS", "300"))  # (a soak: SELA_INDEX_TRIALS=20000 SELA_INDEX_SEED=...)
    rng = np.random.default_rng(int(os.environ.get("SELA_INDEX_SEED", "20261015")))
    blob, offs = _stream(6, 2, 7)
    fields = []
    for f in range(6):
        p = int(offs[f])
        fields += range(p, p + 4)
        p += 4
        for _ in range(2):
            cw = blob[p + 4] | (blob[p + 5] << 8)
            fields += range(p, p + 7)
            p += 7 + 4 * cw
            rw = blob[p + 1] | (blob[p + 2] << 8)
            fields += range(p, p + 5)
            p += 5 + 4 * rw
    ix = _Indexer(gpu, len(blob), 5000)
    for _ in range(trials):
        bad = bytearray(blob)
        at = int(rng.choice(fields))
        bad[at] = int(rng.integers(0, 256)) if rng.random() < 0.5 else bad[at] ^ (1 << int(rng.integers(0, 8)))
        _same(gpu, bad, 2, [6, 5000], ix)


# ---- the payload decode -------------------------------------------------------------------------------------------
def _payload_decode(gpu, blob, max_frames, channels):  # noqa: F811
    dec = codec.Decoder(max_frames, channels)
    pcm, offs, count = dec.decode_payload(gpu.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda())
    gpu.cuda.synchronize()
    n = int(count.item())
    return pcm[:n].cpu().numpy(), offs[: n + 1].cpu().numpy().view(np.uint64), n, dec.status.cpu().numpy()


def _offset_decode(gpu, blob, offsets, channels):  # noqa: F811
    n = len(offsets) - 1
    dec = codec.Decoder(max(n, 1), channels)
    pcm = dec.decode(gpu.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda(), gpu.from_numpy(offsets.view(np.int64).copy()).cuda(), n)
    gpu.cuda.synchronize()
    return pcm.cpu().numpy(), dec.status.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [2, 9])
def test_payload_decode_is_the_offset_decode(gpu, channels):  # noqa: F811
    n = 40
    pcm_in = synth_frames(n, channels, 8)
    frames, offs = codec.encode_host(pcm_in)
    blob = frames.tobytes() + b"" * 5  # (trailing bytes that are no frame)
    for cap in (n - 3, n, n + 5):
        pcm, got_offs, found, status = _payload_decode(gpu, blob, cap, channels)
        want_offs, wn = _host_walk(blob, cap, channels)
        assert found == wn == min(cap, n) and np.array_equal(got_offs, want_offs)
        ref, ref_status = _offset_decode(gpu, blob, want_offs, channels)
        assert np.array_equal(pcm, ref) and np.array_equal(status, ref_status) and int(status[0]) == 0
        assert np.array_equal(pcm, pcm_in[:found])
        assert np.array_equal(pcm, codec.decode_host(frames, want_offs, channels))


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [2, 9])
def test_payload_decode_with_a_malformed_frame(gpu, channels):  # noqa: F811
    """A frame in the middle whose subframe says 1000 samples (the walk passes it; the 2048-sample decoder calls it malformed):
    the same status words and samples as the offset decode."""
    n = 12
    frames, offs = codec.encode_host(synth_frames(n, channels, 9))
    blob = bytearray(frames.tobytes())
    p = int(offs[5]) + 4
    cw = blob[p + 4] | (blob[p + 5] << 8)
    p += 7 + 4 * cw
    blob[p + 3: p + 5] = struct.pack("<H", 1000)
    blob = bytes(blob)
    pcm, got_offs, found, status = _payload_decode(gpu, blob, n, channels)
    want_offs, wn = _host_walk(blob, n, channels)
    assert found == wn == n and np.array_equal(got_offs, want_offs)
    ref, ref_status = _offset_decode(gpu, blob, want_offs, channels)
    assert int(status[0]) & capi.FLAG_BAD_FRAME and int(status[1]) == 1
    assert np.array_equal(status, ref_status) and np.array_equal(pcm, ref)


@pytest.mark.gpu
def test_payload_decode_in_a_graph_and_on_two_streams(gpu):  # noqa: F811
    torch = gpu
    a, _ = _stream(30, 2, 10)
    b, _ = _stream(21, 2, 11)
    assert len(b) <= len(a)
    dec = codec.Decoder(32, 2)
    buf = torch.from_numpy(np.frombuffer(a, np.uint8).copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.decode_payload(buf)  # (the workspace is allocated here, not under capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pcm, offs, count = dec.decode_payload(buf)
    buf.zero_()
    buf[: len(b)].copy_(torch.from_numpy(np.frombuffer(b, np.uint8).copy()))
    graph.replay()
    torch.cuda.synchronize()
    want_pcm, want_offs, wn, want_status = _payload_decode(gpu, b, 32, 2)
    n = int(count.item())
    assert n == wn == 21
    assert np.array_equal(pcm[:n].cpu().numpy(), want_pcm) and np.array_equal(offs[: n + 1].cpu().numpy().view(np.uint64), want_offs)
    assert np.array_equal(dec.status.cpu().numpy(), want_status)

    # two streams at once, each with its own decoder (workspace) and payload, each against its own host walk
    decs = [codec.Decoder(32, 2), codec.Decoder(32, 2)]
    blobs = [a, b]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    payloads = [torch.from_numpy(np.frombuffer(x, np.uint8).copy()).cuda() for x in blobs]
    torch.cuda.synchronize()
    outs = []
    for d, s, p in zip(decs, streams, payloads):
        with torch.cuda.stream(s):
            outs.append(d.decode_payload(p))
    torch.cuda.synchronize()
    for (pcm, offs, count), blob, d in zip(outs, blobs, decs):
        want_offs, wn = _host_walk(blob, 32, 2)
        n = int(count.item())
        assert n == wn and np.array_equal(offs[: n + 1].cpu().numpy().view(np.uint64), want_offs)
        ref, ref_status = _offset_decode(gpu, blob, want_offs, 2)
        assert np.array_equal(pcm[:n].cpu().numpy(), ref) and np.array_equal(d.status.cpu().numpy(), ref_status)


@pytest.mark.gpu
def test_argument_errors(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    blob, _ = _stream(4, 2, 12)
    buf = torch.from_numpy(np.frombuffer(blob + b"\0" * 4, np.uint8).copy()).cuda()
    n = len(blob)
    ws_bytes = int(lib.sela_hip_index_workspace_bytes(n, 4))
    dec_bytes = int(lib.sela_hip_decode_workspace_bytes(4, 2))
    ws = torch.empty(ws_bytes + dec_bytes, dtype=torch.uint8, device="cuda")
    offs = torch.empty(5, dtype=torch.int64, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    pcm = torch.empty((4, 2048, 2), dtype=torch.int16, device="cuda")
    status = torch.empty(4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def index(payload=buf.data_ptr(), channels=2, o=offs.data_ptr(), c=cnt.data_ptr(), w=ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_index_frames_device(payload, n, 4, channels, o, c, w, wb, stream)

    def decode(payload=buf.data_ptr(), channels=2, p=pcm.data_ptr(), s=status.data_ptr(), w=ws.data_ptr(), wb=ws_bytes + dec_bytes):
        return lib.sela_hip_decode_payload_device(payload, n, 4, channels, p, offs.data_ptr(), cnt.data_ptr(), s, w, wb, stream)

    for call, code in [(lambda: index(payload=buf.data_ptr() + 1), -2), (lambda: index(channels=0), -2), (lambda: index(channels=256), -2),
                       (lambda: index(wb=ws_bytes - 1), -4), (lambda: index(o=None), -2), (lambda: index(c=None), -2), (lambda: index(w=None), -2),
                       (lambda: index(payload=None), -2),
                       (lambda: decode(payload=buf.data_ptr() + 2), -2), (lambda: decode(channels=0), -2), (lambda: decode(channels=256), -2),
                       (lambda: decode(wb=ws_bytes + dec_bytes - 1), -4), (lambda: decode(p=None), -2), (lambda: decode(s=None), -2)]:
        assert call() == code
        assert lib.sela_hip_last_error().decode()
    assert index() == 0 and decode() == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == 4


def test_index_workspace_formula_needs_no_gpu():
    lib = capi.lib()
    for n in (0, 1, 3, 4, 4096, 16384, 16385, 23_000_001, 1 << 33):
        got = int(lib.sela_hip_index_workspace_bytes(n, 3875))
        assert got == int(lib.sela_hip_index_workspace_bytes(n, 1 << 20))
        assert 6 * (n // 4) * 4 <= got <= 6 * n + n // 4096 + 2560, (n, got)
