"""sela_hip_salvage_frames_device and sela_hip_salvage_payload_device: the records and totals of a damaged
payload found on the device are the host walk's (sela_hip_salvage_frames, itself held to a model in tests/test_salvage_cpu.py)
word for word on every damage case, across every threshold of the implementation; the compacted payload is the taken frames
back to back, decodes to the surviving frames' PCM, and never writes behind out_cap."""
import struct

import numpy as np
import pytest

from gpu_common import gpu  # noqa: F401
from salvage_cases import SYNC_BYTES, Stream, as_tuples, crafted_frame, damage_cases, damaged, frame_end, singles_and_pairs
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

EINVAL, ECAPACITY = -2, -4
GUARD = 0xC3


class _Device:
    """One device buffer of `capacity` bytes with its outputs and a workspace of exactly the public size; the calls take any
    prefix of it and any cap up to max_frames."""

    def __init__(self, torch, capacity, max_frames, misalign=0):
        self.torch, self.capacity, self.max_frames = torch, capacity, max_frames
        # (misalign: payload and out both that many bytes past a 16-byte line)
        self.buf = torch.zeros(capacity + 32, dtype=torch.uint8, device="cuda")[misalign:]
        self.out = torch.zeros(capacity + 32, dtype=torch.uint8, device="cuda")[misalign:]
        self.ws = torch.empty(codec.salvage_workspace_bytes(capacity, max_frames), dtype=torch.uint8, device="cuda")
        self.records = torch.zeros((max_frames, 3), dtype=torch.int64, device="cuda")
        self.totals = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.offsets = torch.zeros(max_frames + 1, dtype=torch.int64, device="cuda")

    def load(self, payload):
        data = np.ascontiguousarray(payload, np.uint8)
        assert len(data) <= self.capacity
        if len(data):
            self.buf[: len(data)].copy_(self.torch.from_numpy(data.copy()))
        return len(data)

    def _results(self, cap):
        totals = [int(t) for t in self.totals.cpu().numpy().view(np.uint64)]
        rec = self.records.cpu().numpy()
        assert (rec[totals[0]:cap] == -1).all(), "records written beyond totals[0]"
        return np.ascontiguousarray(rec[:totals[0]]).view(codec.SALVAGED_DTYPE).reshape(totals[0]), totals

    def frames(self, n_bytes, cap, channels):
        self.records.fill_(-1)
        self.totals.fill_(-1)
        capi.check(capi.lib().sela_hip_salvage_frames_device(
            self.buf.data_ptr(), n_bytes, cap, channels, self.records.data_ptr(), self.totals.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            self.torch.cuda.current_stream().cuda_stream))
        return self._results(cap)

    def payload(self, n_bytes, cap, channels, out_cap=None, records=True):
        out_cap = self.capacity // 4 * 4 if out_cap is None else out_cap
        self.records.fill_(-1)
        self.totals.fill_(-1)
        self.offsets.fill_(-1)
        self.out.fill_(GUARD)
        capi.check(capi.lib().sela_hip_salvage_payload_device(
            self.buf.data_ptr(), n_bytes, cap, channels, self.out.data_ptr(), out_cap, self.offsets.data_ptr(),
            self.records.data_ptr() if records else None, self.totals.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            self.torch.cuda.current_stream().cuda_stream))
        rec, totals = self._results(cap if records else 0)
        offs = self.offsets.cpu().numpy()
        assert (offs[totals[0] + 1:cap + 1] == -1).all(), "offsets written beyond [totals[0]]"
        return rec, totals, offs[:totals[0] + 1].view(np.uint64), self.out.cpu().numpy()


def _packed(payload, records):
    parts = [payload[int(r["offset"]):int(r["offset"]) + int(r["bytes"])] for r in records]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def _same(dev, payload, channels, caps, copy=True):
    """The device's records and totals are the host walk's; the payload call's too, with the frames back to back."""
    payload = np.ascontiguousarray(payload, np.uint8)
    n_bytes = dev.load(payload)
    for cap in caps:
        want, want_totals = codec.salvage_frames(payload, channels, cap)
        got, totals = dev.frames(n_bytes, cap, channels)
        assert totals == [int(t) for t in want_totals] and got.tobytes() == want.tobytes(), (cap, n_bytes, totals, want_totals.tolist(), as_tuples(got)[:8], as_tuples(want)[:8])
        if not copy:
            continue
        got, totals, offs, out = dev.payload(n_bytes, cap, channels)
        assert totals == [int(t) for t in want_totals] and got.tobytes() == want.tobytes(), (cap, n_bytes, "payload call")
        assert offs.tolist() == np.concatenate([[0], np.cumsum(want["bytes"], dtype=np.uint64)]).tolist()
        packed = _packed(payload, want)
        assert out[:len(packed)].tobytes() == packed.tobytes() and (out[len(packed):] == GUARD).all(), (cap, n_bytes, "compacted payload")


def _encoded(n_frames, channels, track):
    pcm = synth_frames(n_frames, channels, track)
    frames, offs = codec.encode_host(pcm)
    blob = frames.tobytes()
    return Stream([blob[int(offs[f]):int(offs[f + 1])] for f in range(n_frames)], channels), pcm


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [2, 1, 3])
def test_every_damage_singly_and_in_pairs_is_the_host_walk(gpu, channels):  # noqa: F811
    base, _ = _encoded(12, channels, 20 + channels)
    assert channels != 2 or len(base.buf) > 2 * 4096 * 4, "the stereo stream spans three candidate workgroups"
    ops = damage_cases(has_rice=True)
    dev = _Device(gpu, len(base.buf) + 64, 64)
    _same(dev, base.payload(), channels, [0, 1, 11, 12, 13, 64])
    for case in singles_and_pairs(ops):
        s = damaged(base, ops, case)
        try:
            _same(dev, s.payload(), channels, [64])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (case, e)) from e
    # the cap inside a clean run, right at the gap and behind it, and on both sides of 4096 (where the index changes its form)
    s = damaged(base, ops, ("sync_middle", "cut_rice_2"))
    big = _Device(gpu, len(base.buf) + 64, 4097)
    _same(big, s.payload(), channels, [0, 1, 3, 5, 6, 8, 9, 4096, 4097])


def _mono_stream(n_frames, bad):
    frames = [crafted_frame(1, tag=f) for f in range(n_frames)]
    s = Stream(frames, 1)
    for f in bad:
        s.buf[s.offs[f]] ^= 0xFF
    return s


def _candidates(payload, channels):
    buf = payload.tobytes()
    words = np.frombuffer(buf, "<u4", count=len(buf) // 4)
    return sum(1 for w in np.flatnonzero(words == 0xAA55FF00) if frame_end(buf, 4 * int(w), channels))


@pytest.mark.gpu
@pytest.mark.parametrize("candidates", [4095, 4096, 4097, 5119, 5120, 5121])
def test_both_sides_of_a_links_workgroup_and_of_the_index_node_limit(gpu, candidates):  # noqa: F811
    """16-byte mono frames, five of them damaged: exactly `candidates` candidates.  A links workgroup covers 4096 CANDIDATES, and
    "the next confirmed one" behind its last comes from the scan over the workgroups: frame 4097 is candidate 4095, intact but
    between two damaged frames, so the search that starts on it finds nothing in its workgroup.  5120 is the index's own limit
    for its chain on LDS (the salvage has none: its chain always runs device-wide)."""
    n = candidates + 5
    s = _mono_stream(n, [7, n - 40, n - 38] + ([4096, 4098] if n > 4200 else [n // 2, n // 2 + 1]))
    payload = s.payload()
    assert _candidates(payload, 1) == candidates
    dev = _Device(gpu, len(payload), 8192)
    _same(dev, payload, 1, [4096, 4097, 8192])
    found = codec.salvage_frames(payload, 1, 8192)[0]["offset"].tolist()
    assert s.offs[n - 39] not in found and (n <= 4200 or s.offs[4097] not in found)  # (the intact frames between two damaged ones: missed)
    assert len(found) == candidates - (2 if n > 4200 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("words", [4095, 4096, 4097, 8192, 8193])
def test_both_sides_of_the_candidate_chunk(gpu, words):  # noqa: F811
    """Payloads that end just before, at and just behind a candidates workgroup's 4096 words; a damaged frame at each edge."""
    n = words // 4 + 1
    edge = 4096 // 4
    s = _mono_stream(n, [f for f in (edge - 1, edge, 2 * edge - 1) if f < n])
    payload = s.payload()[:4 * words]
    dev = _Device(gpu, len(payload) + 3, 4097)
    _same(dev, payload, 1, [4096, 4097])
    for extra in (1, 2, 3):  # payload_bytes no multiple of 4
        _same(dev, np.concatenate([payload, np.full(extra, 0xAA, np.uint8)]), 1, [4096, 4097])


@pytest.mark.gpu
def test_small_payloads_and_a_lone_sync_word(gpu):  # noqa: F811
    dev = _Device(gpu, 4096, 8)
    frame = crafted_frame(2, rice_words=3)
    for blob in (b"", SYNC_BYTES[:1], SYNC_BYTES[:3], SYNC_BYTES, frame, frame + SYNC_BYTES, frame * 3 + SYNC_BYTES, b"\0" * 8 + frame + SYNC_BYTES[:3],
                 frame[:-1], frame + frame[:-4] + frame + SYNC_BYTES):
        _same(dev, np.frombuffer(blob, np.uint8), 2, [0, 1, 8])


@pytest.mark.gpu
def test_only_sync_words_in_the_workspace_the_formula_gives(gpu):  # noqa: F811
    """The worst case of the workspace: every word a sync word and most of them candidates that chain into each other."""
    for n_bytes, caps in ((4 << 20, (4, 5000)), ((1 << 16) + 2, (2, 5000))):
        payload = np.frombuffer(SYNC_BYTES * (n_bytes // 4) + SYNC_BYTES[: n_bytes % 4], np.uint8)
        for cap in caps:
            dev = _Device(gpu, n_bytes, cap)
            assert dev.ws.numel() == int(capi.lib().sela_hip_salvage_workspace_bytes(n_bytes, cap))
            _same(dev, payload, 1, [cap])


@pytest.mark.gpu
def test_on_an_intact_payload_the_salvage_is_the_device_index(gpu):  # noqa: F811
    base, _ = _encoded(12, 2, 31)
    payload = base.payload()
    dev = _Device(gpu, len(payload), 16)
    n_bytes = dev.load(payload)
    for cap in (11, 12, 13):
        offs, count = codec.index_frames_device(dev.buf[:n_bytes], cap, 2)
        found = int(count.item())
        offs = offs.cpu().numpy()[:found + 1]
        got, totals = dev.frames(n_bytes, cap, 2)
        assert found == min(cap, 12) == totals[0] and got["offset"].tolist() == offs[:-1].tolist() and (got["offset"] + got["bytes"]).tolist() == offs[1:].tolist()
        assert not np.any(got["skipped_before"]) and totals[1] == 0 and totals[3] == offs[-1]


@pytest.mark.gpu
def test_out_cap_cuts_at_a_frame_and_nothing_behind_it_is_written(gpu):  # noqa: F811
    base, _ = _encoded(12, 2, 32)
    s = damaged(base, damage_cases(True), ("sync_middle", "garbage_prefix"))
    payload = s.payload()
    dev = _Device(gpu, len(payload), 16)
    n_bytes = dev.load(payload)
    want, want_totals = codec.salvage_frames(payload, 2, 16)
    packed = _packed(payload, want)
    ends = np.cumsum(want["bytes"], dtype=np.uint64).tolist()
    assert len(want) == 11
    for out_cap, kept in ((ends[6], 7), (ends[6] - 1, 6), (ends[6] + 1, 7), (ends[0], 1), (ends[0] - 4, 0), (0, 0), (3, 0), (ends[-1], 11), (ends[-1] - 1, 10)):
        got, totals, offs, out = dev.payload(n_bytes, 16, 2, out_cap=out_cap)
        assert totals == [int(t) for t in want_totals] and got.tobytes() == want.tobytes() and offs.tolist() == [0] + ends, "a frame that does not fit is still counted"
        limit = ends[kept - 1] if kept else 0
        assert out[:limit].tobytes() == packed[:limit].tobytes() and (out[limit:] == GUARD).all(), (out_cap, kept)
    # without records: the same frames
    _, totals, offs, out = dev.payload(n_bytes, 16, 2, records=False)
    assert totals == [int(t) for t in want_totals] and offs.tolist() == [0] + ends and out[:len(packed)].tobytes() == packed.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [2, 3])
def test_the_compacted_payload_decodes_to_the_surviving_frames(gpu, channels):  # noqa: F811
    torch = gpu
    base, pcm = _encoded(12, channels, 33)
    ops = damage_cases(True)
    salvager = codec.Salvager(len(base.buf) + 64, 16, channels)
    dec = codec.Decoder(16, channels)
    for case in (("sync_first",), ("sync_middle",), ("sync_last",), ("adjacent_headers", "cut_rice_3"), ("intact_between_damaged", "garbage_prefix"), ()):
        s = damaged(base, ops, case)
        payload = s.payload()
        out, offsets, _, totals = salvager.payload(torch.from_numpy(payload).cuda())
        n = int(totals.cpu()[0])
        records = salvager.records()
        want, _ = codec.salvage_frames(payload, channels, 16)
        assert records.tobytes() == want.tobytes() and n == len(want)
        back = dec.decode(out, offsets, n)
        torch.cuda.synchronize()
        survivors = [s.offs.index(int(o) - len(s.prefix)) for o in records["offset"]]
        assert len(survivors) >= 7 and survivors == sorted(set(survivors))
        assert int(dec.status.cpu()[0]) == 0 and int(dec.status.cpu()[1]) == 0, (case, "a flag")
        assert np.array_equal(back.cpu().numpy(), pcm[survivors]), case


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [0, 4])
@pytest.mark.parametrize("prefix_words", [0, 1, 4])
def test_one_frame_far_longer_than_its_neighbours(gpu, prefix_words, misalign):  # noqa: F811
    """A mono frame of 65535 zero Rice words (256 KiB: 64 copy workgroups) among frames of 16 to 56 bytes, with a gap in front
    of it and one behind.  The shift between source and destination grows at each gap: for the long frame it is 11 words with
    no prefix (dwords), 12 with one garbage word in front (16 bytes per lane), 15 with four.  misalign: both pointers 4 bytes
    past a 16-byte line (they still agree modulo 16: dwords up to the line, then 16 bytes per lane)."""
    small = [crafted_frame(1, rice_words=f % 11, tag=f) for f in range(40)]
    long_frame = crafted_frame(1, rice_words=65535, tag=99, fill=0)
    frames = small[:20] + [long_frame] + small[20:]
    s = Stream(frames, 1)
    for f in (18, 22):
        s.buf[s.offs[f]] ^= 0xFF
    s.prefix = b"\x11" * (4 * prefix_words)
    payload = s.payload()
    dev = _Device(gpu, len(payload), 64, misalign)
    assert dev.buf.data_ptr() % 16 == misalign == dev.out.data_ptr() % 16
    _same(dev, payload, 1, [64])
    want, _ = codec.salvage_frames(payload, 1, 64)
    assert len(want) == 39 and int(want["bytes"].max()) == len(long_frame)


@pytest.mark.gpu
def test_argument_refusals_come_before_anything_is_enqueued(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    base, _ = _encoded(4, 2, 34)
    payload = base.payload()
    n = len(payload)
    dev = _Device(gpu, n, 4)
    dev.load(payload)
    dev.payload(n, 4, 2)
    torch.cuda.synchronize()
    before = [t.clone() for t in (dev.records, dev.totals, dev.offsets, dev.out)]
    stream = torch.cuda.current_stream().cuda_stream
    ws_bytes = dev.ws.numel()

    def frames(p=dev.buf.data_ptr(), channels=2, r=dev.records.data_ptr(), t=dev.totals.data_ptr(), w=dev.ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_salvage_frames_device(p, n, 4, channels, r, t, w, wb, stream)

    def copy(p=dev.buf.data_ptr(), channels=2, o=dev.out.data_ptr(), cap=n, f=dev.offsets.data_ptr(), r=dev.records.data_ptr(), t=dev.totals.data_ptr(),
             w=dev.ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_salvage_payload_device(p, n, 4, channels, o, cap, f, r, t, w, wb, stream)

    inside = dev.buf.data_ptr() + 8  # d_out inside the payload
    for call, code in [(lambda: frames(p=dev.buf.data_ptr() + 1), EINVAL), (lambda: frames(channels=0), EINVAL), (lambda: frames(channels=256), EINVAL),
                       (lambda: frames(p=None), EINVAL), (lambda: frames(r=None), EINVAL), (lambda: frames(t=None), EINVAL), (lambda: frames(w=None), EINVAL),
                       (lambda: frames(wb=ws_bytes - 1), ECAPACITY),
                       (lambda: copy(p=dev.buf.data_ptr() + 2), EINVAL), (lambda: copy(o=dev.out.data_ptr() + 1), EINVAL), (lambda: copy(channels=0), EINVAL),
                       (lambda: copy(channels=256), EINVAL), (lambda: copy(p=None), EINVAL), (lambda: copy(o=None), EINVAL), (lambda: copy(f=None), EINVAL),
                       (lambda: copy(t=None), EINVAL), (lambda: copy(w=None), EINVAL), (lambda: copy(wb=ws_bytes - 1), ECAPACITY),
                       (lambda: copy(o=inside), EINVAL), (lambda: copy(o=dev.buf.data_ptr() + n - 4, cap=8), EINVAL)]:
        assert call() == code
        assert lib.sela_hip_last_error().decode()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (dev.records, dev.totals, dev.offsets, dev.out))), "a refused call wrote something"
    assert frames() == 0 and copy(r=None) == 0 and copy(o=None, cap=0) == 0  # (no records wanted; no room given: no out needed)
    torch.cuda.synchronize()
    assert int(dev.totals.cpu()[0]) == 4
    # the same codes as the index call's
    offs, cnt = torch.empty(5, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    assert lib.sela_hip_index_frames_device(dev.buf.data_ptr() + 1, n, 4, 2, offs.data_ptr(), cnt.data_ptr(), dev.ws.data_ptr(), ws_bytes, stream) == EINVAL
    assert lib.sela_hip_index_frames_device(dev.buf.data_ptr(), n, 4, 2, offs.data_ptr(), cnt.data_ptr(), dev.ws.data_ptr(), 16, stream) == ECAPACITY


@pytest.mark.gpu
def test_one_capture_replayed_over_payloads_damaged_differently(gpu):  # noqa: F811
    torch = gpu
    base, _ = _encoded(12, 2, 35)
    ops = damage_cases(True)
    capacity = len(base.buf) + 64
    salvager = codec.Salvager(capacity, 16, 2)
    buf = torch.zeros(capacity, dtype=torch.uint8, device="cuda")
    first = base.payload()
    buf[:len(first)].copy_(torch.from_numpy(first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        salvager.payload(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, offsets, records, totals = salvager.payload(buf)
    for case in (("sync_middle",), ("adjacent_headers", "sync_last"), ("garbage_prefix", "zero_header"), ()):
        payload = damaged(base, ops, case).payload()
        buf.zero_()
        buf[:len(payload)].copy_(torch.from_numpy(payload))
        graph.replay()
        torch.cuda.synchronize()
        whole = np.concatenate([payload, np.zeros(capacity - len(payload), np.uint8)])  # (the call was captured over the whole buffer)
        want, want_totals = codec.salvage_frames(whole, 2, 16)
        assert totals.cpu().numpy().view(np.uint64).tolist() == want_totals.tolist() and salvager.records().tobytes() == want.tobytes(), case
        packed = _packed(whole, want)
        assert out[:len(packed)].cpu().numpy().tobytes() == packed.tobytes()
        assert offsets[:len(want) + 1].cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(want["bytes"], dtype=np.int64)]).tolist()
