"""sela_hip_verify_device, sela_hip_verify_payload_device and sela_hip_verify: a stream held against the PCM it was
made from, frame by frame, on the device.  diff_counts[f] is the number of (sample, channel) values sela_hip_decode_n_device
would have written differently from the PCM, first_diff[f] the smallest such index in the frame (or 0xFFFFFFFF), status[2] the
number of frames with a difference; status[0], [1] and [3] are the decode call's.  The expectation for the reference's own
lossy frames comes from the CPU oracle (pinned to the reference by test_verify_cpu.py), everywhere else from the decode call's
output compared in torch."""
import ctypes as C
import zlib

import numpy as np
import pytest

import corpus
from gpu_common import _build_frame, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

NONE, FAST, ANY = 0, 1, 2
NO_DIFF = 0xFFFFFFFF
GUARD = 64          # words behind each output array that no call may write
SENTINEL = 0x5E1A5E1A


def _bytes(blob):
    return np.frombuffer(bytes(blob), np.uint8).copy() if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, np.uint8)


def _stream(blobs):
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)


def _per_frame(diff, so, ch):
    """diff: bool [total samples, ch]; so: sample offsets [n + 1] -> (counts uint32 [n], first uint32 [n]) as the calls define them."""
    n = len(so) - 1
    counts, first = np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32)
    flat = np.asarray(diff).reshape(-1)
    for f in range(n):
        d = flat[int(so[f]) * ch: int(so[f + 1]) * ch]
        counts[f] = int(d.sum())
        if counts[f]:
            first[f] = int(np.argmax(d))
    return counts, first


class _Device:
    """Buffers of one sela_hip_verify_device call, the raw C ABI: guard words behind both output arrays, the inputs kept for a
    look afterwards."""

    def __init__(self, torch, n, ch, stride):
        self.torch, self.n, self.ch, self.stride = torch, n, ch, stride
        self.counts = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.first = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.sample_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_verify_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")

    def verify(self, blob, offs, pcm, with_offsets=True):
        torch = self.torch
        data = _bytes(blob)
        frames = torch.zeros(max(len(data), 4), dtype=torch.uint8, device="cuda")
        if len(data):
            frames[: len(data)].copy_(torch.from_numpy(data))
        o = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).cuda()
        p_host = np.ascontiguousarray(pcm, np.int16).reshape(-1)
        p = torch.from_numpy(p_host.copy() if len(p_host) else np.zeros(1, np.int16)).cuda()
        frames_before, pcm_before = frames.clone(), p.clone()
        capi.check(capi.lib().sela_hip_verify_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, p.data_ptr(), self.counts.data_ptr(), self.first.data_ptr(),
            self.sample_offsets.data_ptr() if with_offsets else None, self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(frames, frames_before), "d_frames was written"
        assert torch.equal(p, pcm_before), "d_pcm was written"
        return self.results()

    def results(self):
        n = self.n
        c = self.counts.cpu().numpy().view(np.uint32)
        f = self.first.cpu().numpy().view(np.uint32)
        assert (c[n:] == SENTINEL).all() and (f[n:] == SENTINEL).all(), "written past the per-frame arrays"
        return c[:n].copy(), f[:n].copy(), self.status.cpu().numpy().view(np.uint32).copy()


def _decode_n(torch, blob, offs, ch, stride):
    """sela_hip_decode_n_device -> (pcm int16 [samples, ch], sample offsets, status)."""
    n = len(offs) - 1
    dec = codec.DecoderN(max(n, 1), ch, stride)
    data = _bytes(blob)
    frames = torch.zeros(max(len(data), 4), dtype=torch.uint8, device="cuda")
    if len(data):
        frames[: len(data)].copy_(torch.from_numpy(data))
    o = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).cuda()
    pcm, so = dec.decode(frames, o, n)
    torch.cuda.synchronize()
    return pcm, so.cpu().numpy().view(np.uint64), dec.status.cpu().numpy().view(np.uint32).copy()


def _against_decode(torch, blob, offs, ch, stride, pcm, route=None, label=""):
    """The verify call on (stream, pcm) == compare(DecoderN output, pcm) in torch, frame by frame -> (counts, first)."""
    n = len(offs) - 1
    back, so, dst = _decode_n(torch, blob, offs, ch, stride)
    assert codec.decode_n_status_error(dst) == 0, (label, dst)
    total = int(so[n])
    p = np.ascontiguousarray(pcm, np.int16).reshape(-1, ch)
    assert len(p) == total, (label, len(p), total)
    diff = (back[:total] != torch.from_numpy(p).cuda()).cpu().numpy()
    want_counts, want_first = _per_frame(diff, so, ch)
    counts, first, st = _Device(torch, n, ch, stride).verify(blob, offs, p)
    assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (label, st, dst)
    if route is not None:
        assert int(st[3]) == route, (label, st)
    assert np.array_equal(counts, want_counts), (label, np.flatnonzero(counts != want_counts)[:8])
    assert np.array_equal(first, want_first), (label, np.flatnonzero(first != want_first)[:8])
    assert int(st[2]) == int((want_counts != 0).sum()), (label, st)
    return counts, first


def _plant(pcm, positions):
    """A copy of pcm ([frames or samples ..., ch] int16) with the values at the flat `positions` changed."""
    out = np.ascontiguousarray(pcm, np.int16).copy()
    flat = out.reshape(-1)
    flat[np.asarray(positions, np.int64)] ^= 1
    return out


# ---- 1. the reference's own lossy frames ----------------------------------------------------------------------------------------
def _oracle_expectation(frames, offs, pcm):
    back, _ = oracle().decode_frames(frames, offs, pcm.shape[2], threads=8)
    diff = back != pcm
    n = len(pcm)
    counts = diff.reshape(n, -1).sum(1).astype(np.uint32)
    first = np.where(counts != 0, diff.reshape(n, -1).argmax(1), NO_DIFF).astype(np.uint32)
    return counts, first


def _encoded(torch, pcm):
    n, _, ch = pcm.shape
    enc = codec.Encoder(n, ch)
    out = enc.encode(torch.from_numpy(np.ascontiguousarray(pcm)).cuda())
    torch.cuda.synchronize()
    frames, offs = out.to_host()
    return frames, offs, out


def test_the_references_own_lossy_frames_are_found_exactly(gpu):  # noqa: F811
    torch = gpu
    pcm = corpus.build(3000, 20260927)
    frames, offs, out = _encoded(torch, pcm)
    want_frames, want_offs, _ = oracle().encode_frames(pcm, threads=8)
    assert np.array_equal(offs, want_offs) and np.array_equal(frames, want_frames), "the encoder's bytes are not the oracle's"
    want_counts, want_first = _oracle_expectation(frames, offs, pcm)
    lossy = np.flatnonzero(want_counts)
    print("lossy frames of corpus.build(3000, 20260927):", [(int(f), int(want_counts[f]), int(want_first[f])) for f in lossy])
    assert len(lossy) >= 3, "the expectation is vacuous: the oracle finds fewer than three lossy frames"
    ver = codec.Verifier(3000, 2, 2048)
    counts, first = ver.verify(out.frames, out.offsets, 3000, torch.from_numpy(pcm).cuda())
    ver.check()
    assert ver.route() == FAST
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want_counts)
    assert np.array_equal(first.cpu().numpy().view(np.uint32), want_first)
    assert ver.lossy_frames() == len(lossy) and int(ver.status[2].item()) == len(lossy)
    # ... and through the raw call with guards, and the payload form
    c2, f2, st = _Device(torch, 3000, 2, 2048).verify(frames, offs, pcm)
    assert np.array_equal(c2, want_counts) and np.array_equal(f2, want_first) and int(st[2]) == len(lossy) and int(st[3]) == FAST
    c3, f3, count = ver.verify_payload(out.frames[: len(frames)], torch.from_numpy(pcm).cuda())
    ver.check()
    assert int(count.item()) == 3000 and ver.lossy_frames() == len(lossy)
    assert np.array_equal(c3.cpu().numpy().view(np.uint32), want_counts) and np.array_equal(f3.cpu().numpy().view(np.uint32), want_first)


@pytest.mark.parametrize("seed, lossy_frames", [(2, 2), (0, 0)])
def test_the_bench_track(gpu, seed, lossy_frames):  # noqa: F811
    torch = gpu
    pcm = synth_frames(3875, 2, seed)
    frames, offs, out = _encoded(torch, pcm)
    want_counts, want_first = _oracle_expectation(frames, offs, pcm)
    assert int((want_counts != 0).sum()) == lossy_frames, "the oracle's count of lossy frames of this track has changed"
    ver = codec.Verifier(3875, 2, 2048)
    counts, first = ver.verify(out.frames, out.offsets, 3875, torch.from_numpy(pcm).cuda())
    ver.check()
    counts, first = counts.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32)
    assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first)
    assert ver.lossy_frames() == lossy_frames and ver.route() == FAST
    if lossy_frames == 0:
        assert (counts == 0).all() and (first == NO_DIFF).all()


# ---- 2. one planted difference, found where it is ---------------------------------------------------------------------------------
def test_one_planted_difference_is_found_where_it_is(gpu):  # noqa: F811
    torch = gpu
    n = 24
    pcm = synth_frames(n, 2, 0)
    frames, offs, _ = _encoded(torch, pcm)
    base_counts, _ = _oracle_expectation(frames, offs, pcm)
    assert (base_counts == 0).all(), "this batch is meant to be lossless"
    rng = np.random.default_rng(11)
    places = [(f, i, c) for f in (0, n - 1) for i in (0, 1, 2047) for c in (0, 1)]
    places += [(int(rng.integers(n)), int(rng.integers(2048)), int(rng.integers(2))) for _ in range(50)]
    dev = _Device(torch, n, 2, 2048)
    for f, i, c in places:
        changed = pcm.copy()
        changed.view(np.uint16)[f, i, c] ^= np.uint16(1 << int(rng.integers(16)))
        counts, first, st = dev.verify(frames, offs, changed)
        want_counts, want_first = np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32)
        want_counts[f], want_first[f] = 1, i * 2 + c
        assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first), (f, i, c)
        assert int(st[2]) == 1 and int(st[0]) == 0 and int(st[1]) == 0 and int(st[3]) == FAST
    # 2 .. 2048 * channels differences in one frame
    for k in (2, 3, 64, 1000, 4095, 4096):
        f = int(rng.integers(n))
        where = np.sort(rng.choice(4096, size=k, replace=False))
        changed = _plant(pcm, f * 4096 + where)
        counts, first, st = dev.verify(frames, offs, changed)
        assert int(counts[f]) == k and int(first[f]) == int(where[0]) and int(counts.sum()) == k and int(st[2]) == 1, (k, f)
        assert (np.delete(first, f) == NO_DIFF).all()


# ---- 3. every route ---------------------------------------------------------------------------------------------------------------
def _planted_positions(rng, so, ch, n_random):
    """First and last value of the first and last frame, and random ones."""
    n = len(so) - 1
    spots = [int(so[0]) * ch, int(so[1]) * ch - 1, int(so[n - 1]) * ch, int(so[n]) * ch - 1]
    spots += [int(x) for x in rng.integers(0, int(so[n]) * ch, n_random)]
    return np.unique(spots)


def _route_checks(torch, blob, offs, ch, stride, pcm, route, label):
    """Tests 1 and 2 in reduced form on one stream: against the decode call with the PCM as it is, then with planted differences."""
    rng = np.random.default_rng(zlib.crc32(repr(label).encode()))
    _against_decode(torch, blob, offs, ch, stride, pcm, route, label)
    _, so, _ = _decode_n(torch, blob, offs, ch, stride)
    flat = np.ascontiguousarray(pcm, np.int16).reshape(-1)
    for n_random in (0, 40):
        where = _planted_positions(rng, so, ch, n_random)
        counts, _ = _against_decode(torch, blob, offs, ch, stride, _plant(flat, where), route, (label, n_random))
        assert int(counts.sum()) >= 1
    # one difference alone, at the very last value of the stream
    last = int(so[-1]) * ch - 1
    base_counts, _ = _against_decode(torch, blob, offs, ch, stride, flat, route, label)
    counts, first = _against_decode(torch, blob, offs, ch, stride, _plant(flat, [last]), route, (label, "last"))
    if base_counts[-1] == 0:
        assert int(counts[-1]) == 1 and int(first[-1]) == last - int(so[-2]) * ch


def _channels_pcm(n, ch, seed):
    return np.ascontiguousarray(np.concatenate([synth_frames(n, 1, seed + c) for c in range(ch)], axis=2))


@pytest.mark.parametrize("ch", [1, 3, 8, 12])
def test_2048_sample_frames_of_other_channel_counts(gpu, ch):  # noqa: F811
    """mono, 3 and 8 channels: k_verify_frames; 12: k_decode_frames_wide into the workspace, then k_verify_compare"""
    pcm = _channels_pcm(9, ch, 30 + ch)
    frames, offs = codec.encode_i32(np.ascontiguousarray(pcm.transpose(0, 2, 1)).astype(np.int32))
    _route_checks(gpu, frames, offs, ch, 2048, pcm, FAST, f"{ch} channels")
    _route_checks(gpu, frames, offs, ch, 3000, pcm, FAST, f"{ch} channels, a larger stride")


@pytest.mark.parametrize("n", [1000, 5000])
def test_frames_of_other_lengths_from_the_device_encoder(gpu, n):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(n)
    pcm = np.stack([np.stack([_signal(rng, "tone", n, 15), _signal(rng, "noise", n, 12)], axis=1) for _ in range(5)]).astype(np.int16)
    enc = codec.Encoder32(5, 2, n)
    enc.encode(torch.from_numpy(np.ascontiguousarray(pcm)).cuda())  # (sela_hip_encode_n_device)
    frames, offs = enc.to_host()
    _route_checks(torch, frames, offs, 2, n, pcm, ANY, f"length {n}")
    _route_checks(torch, frames, offs, 2, n + 123, pcm, ANY, f"length {n}, a larger stride")
    for mode in (0, 2):
        capi.lib().sela_hip_debug_standard_first(mode)
        try:
            _against_decode(torch, frames, offs, 2, n, _plant(pcm, [0, 7, n * 2 * 5 - 1]), ANY, (n, "mode", mode))
        finally:
            capi.lib().sela_hip_debug_standard_first(-1)


def test_a_stream_that_mixes_2048_with_another_length(gpu):  # noqa: F811
    pcm = synth_frames(12, 2, 3)
    frames, offs = codec.encode_host(pcm)
    blobs = [frames[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(12)]
    odd_pcm = np.stack([_signal(np.random.default_rng(1), "tone", 777, 15), _signal(np.random.default_rng(2), "noise", 777, 12)], axis=1).astype(np.int16)
    odd = codec.encode_host(odd_pcm[None])[0].tobytes()
    stream, so = _stream(blobs[:7] + [odd] + blobs[7:])
    flat = np.concatenate([pcm[:7].reshape(-1, 2), odd_pcm, pcm[7:].reshape(-1, 2)])
    _route_checks(gpu, stream, so, 2, 2048, flat, ANY, "mixed lengths")


def test_a_frame_on_the_serial_parse_fallback(gpu, kats):  # noqa: F811
    """A Rice stream beyond the parser's plan (kStreamCap words): the serial parse into the workspace, then the same compare."""
    rng = np.random.default_rng(77)
    q_sine = kats["blk/sine_deg/q"]
    big = _build_frame([(0, 0, 0, q_sine, rng.integers(-120000, 120000, 2048))])
    small = _build_frame([(0, 0, 0, q_sine, rng.integers(-200, 200, 2048))])
    assert (len(big) - 16) // 4 + 2 > 1072 + 50, "the subframe's words (coefficients + 2 + residues) are meant to exceed kStreamCap"
    for blobs, ch in (([small, big, small], 1),):
        stream, offs = _stream(blobs)
        back, so, st = _decode_n(gpu, stream, offs, ch, 2048)
        assert codec.decode_n_status_error(st) == 0 and int(st[3]) == FAST
        pcm = back[: int(so[-1])].cpu().numpy()
        _route_checks(gpu, stream, offs, ch, 2048, pcm, FAST, "serial parse")
    # ... and as one channel of a stereo frame beside a subframe that fits the plan (the whole frame takes the fallback)
    two = _build_frame([(0, 0, 0, q_sine, rng.integers(-120000, 120000, 2048)), (1, 0, 1, q_sine, rng.integers(-50, 50, 2048))])
    stream, offs = _stream([two, two])
    back, so, st = _decode_n(gpu, stream, offs, 2, 2048)
    assert codec.decode_n_status_error(st) == 0 and int(st[3]) == FAST
    _route_checks(gpu, stream, offs, 2, 2048, back[: int(so[-1])].cpu().numpy(), FAST, "serial parse, stereo")


# ---- 4. status, no frames, argument errors ------------------------------------------------------------------------------------------
def _status_cases(kats):
    pcm = synth_frames(4, 2, 6)
    frames, offs = codec.encode_host(pcm)
    bad_sync = frames.copy()
    bad_sync[int(offs[2])] ^= 0xFF
    cut = offs.copy()
    cut[1] -= 8
    decreasing = offs.copy()
    decreasing[2] = decreasing[1] - 4
    outside = _build_frame([(0, 0, 0, [5, 100, -3], np.zeros(2048, np.int32))])  # (a coefficient index outside the tables)
    odd = codec.encode_i32(np.stack([_signal(np.random.default_rng(3), "tone", 700, 15)] * 2)[None])
    odd_cut = odd[1].copy()
    odd_cut[1] -= 6
    yield "bad sync", bad_sync, offs, 2, 2048, pcm
    yield "truncated frame", frames, cut, 2, 2048, pcm
    yield "decreasing offsets", frames, decreasing, 2, 2048, pcm
    yield "coefficient outside the tables", _bytes(outside), np.array([0, len(outside)], np.uint64), 1, 2048, np.zeros((2048, 1), np.int16)
    yield "stride too small", frames, offs, 2, 2047, pcm
    yield "stride too small, another length", odd[0], odd[1], 2, 699, np.zeros((700, 2), np.int16)
    yield "truncated frame, another length", odd[0], odd_cut, 2, 700, np.zeros((700, 2), np.int16)
    yield "clean", frames, offs, 2, 2048, pcm


def test_status_words_are_the_decode_calls(gpu, kats):  # noqa: F811
    seen = set()
    for label, blob, offs, ch, stride, pcm in _status_cases(kats):
        n = len(offs) - 1
        _, _, dst = _decode_n(gpu, blob, offs, ch, stride)
        room = np.zeros(max(n * stride * ch, 1), np.int16)  # (whatever the stream says, nothing beyond n * stride * channels is read)
        flat = np.ascontiguousarray(pcm, np.int16).reshape(-1)
        room[: min(len(flat), len(room))] = flat[: len(room)]
        _, _, st = _Device(gpu, n, ch, stride).verify(blob, offs, room)
        assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (label, st, dst)
        code = codec.decode_n_status_error(st)
        assert code == codec.decode_n_status_error(dst), (label, st, dst)
        seen.add(code)
        if label == "clean":
            assert code == 0 and int(st[2]) == 0
    assert {0, -4, -5, -6} <= seen, seen


def test_no_frames(gpu):  # noqa: F811
    torch = gpu
    dev = _Device(torch, 0, 2, 2048)
    dev.status.fill_(-1)
    counts, first, st = dev.verify(b"", np.zeros(1, np.uint64), np.zeros(0, np.int16))
    assert (st == 0).all() and len(counts) == 0
    assert int(dev.sample_offsets[0].item()) == 0


def test_argument_errors_enqueue_nothing(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    pcm = synth_frames(2, 2, 1)
    blob, o = codec.encode_host(pcm)
    n = len(blob)
    buf = torch.from_numpy(np.concatenate([blob, np.zeros(4, np.uint8)])).cuda()
    offs = torch.from_numpy(o.view(np.int64).copy()).cuda()
    p = torch.from_numpy(pcm.reshape(-1).copy()).cuda()
    ws_bytes = int(lib.sela_hip_verify_workspace_bytes(2, 2, 2048))
    ix_bytes = int(lib.sela_hip_index_workspace_bytes(n, 2))
    ws = torch.empty(ws_bytes + ix_bytes, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    first = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    so = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    fo = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    nf = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def dev(frames=buf.data_ptr(), fo_=offs.data_ptr(), nfr=2, channels=2, stride=2048, pcm_=p.data_ptr(), c=counts.data_ptr(), f=first.data_ptr(),
            st=status.data_ptr(), w=ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_verify_device(frames, fo_, nfr, channels, stride, pcm_, c, f, so.data_ptr(), st, w, wb, stream)

    def pay(payload=buf.data_ptr(), channels=2, stride=2048, pcm_=p.data_ptr(), c=counts.data_ptr(), f=first.data_ptr(), st=status.data_ptr(),
            o_=fo.data_ptr(), k=nf.data_ptr(), w=ws.data_ptr(), wb=ws_bytes + ix_bytes):
        return lib.sela_hip_verify_payload_device(payload, n, 2, channels, stride, pcm_, c, f, so.data_ptr(), o_, k, st, w, wb, stream)

    for call, code in [(lambda: dev(frames=buf.data_ptr() + 1), -2), (lambda: dev(channels=0), -2), (lambda: dev(channels=256), -2),
                       (lambda: dev(stride=0), -2), (lambda: dev(pcm_=None), -2), (lambda: dev(c=None), -2), (lambda: dev(f=None), -2),
                       (lambda: dev(st=None), -2), (lambda: dev(w=None), -2), (lambda: dev(fo_=None), -2), (lambda: dev(frames=None), -2),
                       (lambda: dev(pcm_=p.data_ptr() + 1), -2), (lambda: dev(c=counts.data_ptr() + 2), -2), (lambda: dev(f=first.data_ptr() + 1), -2),
                       (lambda: dev(wb=ws_bytes - 1), -4), (lambda: dev(nfr=0x40000000), -2),
                       (lambda: pay(payload=buf.data_ptr() + 2), -2), (lambda: pay(channels=0), -2), (lambda: pay(stride=0), -2),
                       (lambda: pay(pcm_=None), -2), (lambda: pay(c=None), -2), (lambda: pay(f=None), -2), (lambda: pay(st=None), -2),
                       (lambda: pay(o_=None), -2), (lambda: pay(k=None), -2), (lambda: pay(w=None), -2),
                       (lambda: pay(wb=ws_bytes + ix_bytes - 1), -4)]:
        assert call() == code
    torch.cuda.synchronize()  # nothing was enqueued: every output is as it was
    for t in (counts, first, so, fo, nf, status):
        assert (t.cpu().numpy() == -1).all()
    # a workspace of the size asked for is enough, and no initialisation is needed
    ws.fill_(0xFF)
    assert dev() == 0
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert codec.decode_n_status_error(st) == 0 and int(st[2]) == 0 and int(st[3]) == FAST and (counts.cpu().numpy() == 0).all()
    assert pay() == 0
    torch.cuda.synchronize()
    assert int(nf.item()) == 2 and int(status[2].item()) == 0 and (first.cpu().numpy() == -1).all()


# ---- 5. nothing else is written: _Device.verify checks d_frames, d_pcm and the guards on every call above; here also without
#         d_sample_offsets, on both kinds of route ---------------------------------------------------------------------------------
def test_nothing_else_is_written(gpu):  # noqa: F811
    pcm = synth_frames(6, 2, 4)
    frames, offs = codec.encode_host(pcm)
    changed = _plant(pcm, [5, 4096 * 3 + 17])
    for stride in (2048, 2500):
        dev = _Device(gpu, 6, 2, stride)
        counts, first, st = dev.verify(frames, offs, changed, with_offsets=False)
        assert (dev.sample_offsets.cpu().numpy() == -1).all()
        assert counts.tolist() == [1, 0, 0, 1, 0, 0] and first[0] == 5 and first[3] == 17 and int(st[2]) == 2
    odd = np.stack([_signal(np.random.default_rng(4), "tone", 900, 15)] * 2, axis=1).astype(np.int16)
    blob, o = codec.encode_host(odd[None])
    dev = _Device(gpu, 1, 2, 900)
    counts, first, st = dev.verify(blob, o, _plant(odd, [1799]), with_offsets=False)
    assert counts.tolist() == [1] and first.tolist() == [1799] and int(st[3]) == ANY


def test_a_stereo_pcm_that_is_only_2_byte_aligned(gpu):  # noqa: F811
    """The ABI asks int16 alignment of d_pcm, no more: a stereo PCM two bytes off a 16-byte boundary takes the kernel's loop
    without the 16-byte loads.  Planted differences at the frame's ends and inside, found where they are."""
    torch = gpu
    n = 7
    pcm = synth_frames(n, 2, 0)
    frames, offs = codec.encode_host(pcm)
    base_counts, _ = _oracle_expectation(frames, offs, pcm)
    assert (base_counts == 0).all(), "this batch is meant to be lossless"
    where = [0, 1, 4095, 4096 * 3 + 8, 4096 * 3 + 9, 4096 * 3 + 2000, 4096 * 6 + 4094, 4096 * 6 + 4095]
    changed = _plant(pcm, where).reshape(-1)
    lib = capi.lib()
    d_frames = torch.from_numpy(frames).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    for shift in (1, 3, 0):  # int16 elements off the allocation's start
        room = torch.zeros(len(changed) + 8, dtype=torch.int16, device="cuda")
        room[shift: shift + len(changed)].copy_(torch.from_numpy(changed))
        before = room.clone()
        assert room.data_ptr() % 16 == 0
        counts = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
        first = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
        status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(lib.sela_hip_verify_workspace_bytes(n, 2, 2048)), dtype=torch.uint8, device="cuda")
        capi.check(lib.sela_hip_verify_device(d_frames.data_ptr(), d_offs.data_ptr(), n, 2, 2048, room.data_ptr() + 2 * shift, counts.data_ptr(),
                                              first.data_ptr(), None, status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(room, before)
        assert counts.cpu().numpy()[:n].tolist() == [3, 0, 0, 3, 0, 0, 2], shift
        assert first.cpu().numpy().view(np.uint32)[:n].tolist() == [0, NO_DIFF, NO_DIFF, 8, NO_DIFF, NO_DIFF, 4094], shift
        assert (counts.cpu().numpy()[n:] == -1).all() and (first.cpu().numpy()[n:] == -1).all()
        assert status.cpu().numpy().tolist() == [0, 0, 3, FAST], shift


# ---- 6. capture -------------------------------------------------------------------------------------------------------------------
def _eager(torch, frames, offs, ch, stride, pcm):
    c, f, st = _Device(torch, len(offs) - 1, ch, stride).verify(frames, offs, pcm)
    return c, f, st


@pytest.mark.parametrize("form", ["verify", "verify_payload"])
def test_in_a_graph(gpu, form):  # noqa: F811
    torch = gpu
    n = 40
    inputs = []
    for seed, where in ((2, [3, 4096 * 11 + 9, 4096 * 39 + 4095]), (5, [4096 * 2, 4096 * 20 + 1])):
        pcm = synth_frames(n, 2, seed)
        frames, offs = codec.encode_host(pcm)
        inputs.append((frames, offs, _plant(pcm, where)))
    room = max(len(i[0]) for i in inputs)
    d_frames = torch.zeros(room, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_pcm = torch.zeros(n * 2048 * 2, dtype=torch.int16, device="cuda")

    def load(k):
        frames, offs, pcm = inputs[k]
        d_frames.zero_()
        d_frames[: len(frames)].copy_(torch.from_numpy(frames))
        d_offs.copy_(torch.from_numpy(offs.view(np.int64).copy()))
        d_pcm.copy_(torch.from_numpy(pcm.reshape(-1)))

    ver = codec.Verifier(n, 2, 2048)
    call = (lambda: ver.verify(d_frames, d_offs, n, d_pcm)) if form == "verify" else (lambda: ver.verify_payload(d_frames, d_pcm))
    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # (the workspace is allocated here, not under capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for k in (0, 1, 0):
        load(k)
        ver.diff_counts.fill_(-7)
        ver.first_diff.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        want_counts, want_first, want_st = _eager(torch, *inputs[k][:2], 2, 2048, inputs[k][2])
        assert int(want_st[2]) >= 2
        assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want_counts), (form, k)
        assert np.array_equal(out[1].cpu().numpy().view(np.uint32), want_first), (form, k)
        assert np.array_equal(ver.status.cpu().numpy().view(np.uint32), want_st), (form, k)
        if form == "verify_payload":
            assert int(out[2].item()) == n


# ---- 7. the host-pointer call -----------------------------------------------------------------------------------------------------
def test_the_host_pointer_call_equals_the_device_call(gpu):  # noqa: F811
    pcm = synth_frames(50, 2, 2)
    frames, offs = codec.encode_host(pcm)
    changed = _plant(pcm, [0, 4096 * 17 + 100, 4096 * 17 + 101, 4096 * 50 - 1])
    want_counts, want_first, st = _eager(gpu, frames, offs, 2, 2048, changed)
    counts, first, lossy = codec.verify_host(frames, offs, 2, changed)
    assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first) and lossy == int(st[2]) >= 3
    # another length, and a mix
    odd = np.stack([np.stack([_signal(np.random.default_rng(s), "tone", 1500, 15)] * 2, axis=1) for s in (1, 2, 3)]).astype(np.int16)
    blob, o = codec.encode_host(odd)
    changed = _plant(odd, [2999, 3000, 8999])
    want_counts, want_first, st = _eager(gpu, blob, o, 2, 1500, changed)
    counts, first, lossy = codec.verify_host(blob, o, 2, changed)
    assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first) and lossy == int(st[2]) == 3
    assert counts.tolist() == [1, 1, 1] and first.tolist() == [2999, 0, 2999]
    # a malformed stream: the decode call's code
    bad = frames.copy()
    bad[int(offs[3])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as e:
        codec.verify_host(bad, offs, 2, pcm)
    assert e.value.code == -5
    assert codec.verify_host(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2, np.zeros(0, np.int16))[2] == 0


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
    changed = _plant(pcm, [4096 * 4 + 33])
    counts, first, lossy = codec.verify_host(frames, offs, 2, changed)
    assert lossy == 1 and int(counts[4]) == 1 and int(first[4]) == 33 and int(counts.sum()) == 1
    o = np.ascontiguousarray(offs[5:] - offs[5])
    capi.check(lib.sela_hip_decode_feed(job, frames[int(offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12 and np.array_equal(back, pcm.reshape(-1))
