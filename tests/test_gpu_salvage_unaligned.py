"""sela_hip_salvage_frames_unaligned_device and sela_hip_salvage_payload_unaligned_device: the records, totals
and offsets of a damaged payload found on the device are the host walk's (sela_hip_salvage_frames_unaligned, itself held to a
model in tests/test_salvage_unaligned_cpu.py) byte for byte on every damage case, with frames at every phase and across every
edge of the implementation; the compacted payload is the taken frames back to back, decodes to the PCM of every frame behind an
insertion, and nothing behind its end is written."""
import numpy as np
import pytest

import salvage_unaligned_cases as ua
from gpu_common import gpu  # noqa: F401
from salvage_cases import SYNC_BYTES, Stream, as_tuples, crafted_frame, damage_cases, damaged, singles_and_pairs
from sela_amd import capi, codec
from test_gpu_salvage import GUARD, _Device, _encoded, _packed

EINVAL, ECAPACITY = -2, -4
CHUNK = 4096  # words a candidates workgroup covers, candidates a links workgroup covers, words a copy workgroup writes


class _UaDevice(_Device):
    """tests/test_gpu_salvage.py's buffers, the *_unaligned calls on them.  What lies BEHIND a loaded payload in the buffer
    continues a sync word and a frame's headers: a read past payload_bytes would find a frame the host does not."""
    POISON = (SYNC_BYTES + crafted_frame(1)[4:]) * 2

    def load(self, payload):
        n = super().load(payload)
        tail = np.frombuffer((SYNC_BYTES[n % 4:] if n % 4 else b"") + self.POISON, np.uint8)[:self.buf.numel() - n]
        self.buf[n:n + len(tail)].copy_(self.torch.from_numpy(tail.copy()))
        return n

    def frames(self, n_bytes, cap, channels):
        self.records.fill_(-1)
        self.totals.fill_(-1)
        capi.check(capi.lib().sela_hip_salvage_frames_unaligned_device(
            self.buf.data_ptr(), n_bytes, cap, channels, self.records.data_ptr(), self.totals.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            self.torch.cuda.current_stream().cuda_stream))
        return self._results(cap)

    def payload(self, n_bytes, cap, channels, out_cap=None, records=True):
        out_cap = self.capacity // 4 * 4 if out_cap is None else out_cap
        self.records.fill_(-1)
        self.totals.fill_(-1)
        self.offsets.fill_(-1)
        self.out.fill_(GUARD)
        capi.check(capi.lib().sela_hip_salvage_payload_unaligned_device(
            self.buf.data_ptr(), n_bytes, cap, channels, self.out.data_ptr(), out_cap, self.offsets.data_ptr(),
            self.records.data_ptr() if records else None, self.totals.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            self.torch.cuda.current_stream().cuda_stream))
        rec, totals = self._results(cap if records else 0)
        offs = self.offsets.cpu().numpy()
        assert (offs[totals[0] + 1:cap + 1] == -1).all(), "offsets written beyond [totals[0]]"
        return rec, totals, offs[:totals[0] + 1].view(np.uint64), self.out.cpu().numpy()


def _same(dev, payload, channels, caps, copy=True):
    """The device's records and totals are the host walk's; the payload call's too, with the frames back to back and the canary
    behind them."""
    payload = np.ascontiguousarray(payload, np.uint8)
    n_bytes = dev.load(payload)
    want = None
    for cap in caps:
        want, want_totals = codec.salvage_frames(payload, channels, cap, unaligned=True)
        got, totals = dev.frames(n_bytes, cap, channels)
        assert totals == [int(t) for t in want_totals] and got.tobytes() == want.tobytes(), (cap, n_bytes, totals, want_totals.tolist(), as_tuples(got)[:8], as_tuples(want)[:8])
        if not copy:
            continue
        got, totals, offs, out = dev.payload(n_bytes, cap, channels)
        assert totals == [int(t) for t in want_totals] and got.tobytes() == want.tobytes(), (cap, n_bytes, "payload call")
        assert offs.tolist() == np.concatenate([[0], np.cumsum(want["bytes"], dtype=np.uint64)]).tolist()
        packed = _packed(payload, want)
        assert out[:len(packed)].tobytes() == packed.tobytes() and (out[len(packed):] == GUARD).all(), (cap, n_bytes, "compacted payload")
    return want


def _unaligned_cases(s):
    """name -> payload: the damages of tests/test_salvage_unaligned_cpu.py on the 12-frame stream s."""
    ch, base = s.channels, s.payload()
    out = {"intact": base}
    for extra in (1, 2, 3, 5, 15):
        for f in (1, 5, 11):
            out["insert_%d_before_%d" % (extra, f)] = ua.insert(base, s.offs[f], ua.garbage(extra, f))
    for a, b in ((1, 2), (3, 3), (2, 5), (1, 3)):
        out["insert_%d_and_%d" % (a, b)] = ua.insert(ua.insert(base, s.offs[8], ua.garbage(b, 1)), s.offs[3], ua.garbage(a))
    for n in (1, 2, 3):
        out["prefix_%d" % n] = ua.insert(base, 0, ua.garbage(n))
        out["delete_%d" % n] = ua.delete(base, s.rice(4)[0] + 1, n)
        out["fake_confirmed_%d" % n] = ua.fake_at_odd_phase(s, 8, True, n)[0]
        out["fake_unconfirmed_%d" % n] = ua.fake_at_odd_phase(s, 8, False, n)[0]
    out["concatenated"] = ua.concatenated(s, ua.rice_stream(ch, 7, words=(2, 4)), ch)
    for shift in range(4):
        whole = ua.insert(base, s.offs[2], ua.garbage(shift))
        whole[s.offs[8] + shift] ^= 0xFF
        for tail in range(6):
            out["cut_shift_%d_tail_%d" % (shift, tail)] = np.concatenate([whole[:s.offs[10] + shift], np.frombuffer(ua.garbage(tail), np.uint8)]).astype(np.uint8)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [2, 1, 3])
def test_every_case_is_the_host_walk(gpu, channels):  # noqa: F811
    s = ua.rice_stream(channels)
    dev = _UaDevice(gpu, 2 * len(s.buf) + 64, 64)
    _same(dev, s.payload(), channels, [0, 1, 11, 12, 13, 64])
    for name, payload in _unaligned_cases(s).items():
        try:
            _same(dev, payload, channels, [64])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from e
    # the word salvage's damages, singly and in pairs, as they are and with 1 .. 3 bytes inserted in front of frame 3
    ops = damage_cases(has_rice=True)
    for k, case in enumerate(singles_and_pairs(ops)):
        d = damaged(s, ops, case)
        payload = d.payload()
        shifted = ua.insert(payload, min(len(payload), len(d.prefix) + d.offs[3]), ua.garbage(1 + k % 3, k))
        try:
            _same(dev, payload, channels, [64], copy=False)
            _same(dev, shifted, channels, [64])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (case, e)) from e
    # the cap inside a clean run, right at a gap and behind it
    _same(dev, ua.insert(ua.insert(s.payload(), s.offs[8], ua.garbage(2)), s.offs[3], ua.garbage(1)), channels, [0, 1, 3, 4, 8, 9, 12])


@pytest.mark.gpu
def test_small_payloads_and_a_lone_sync_word(gpu):  # noqa: F811
    dev = _UaDevice(gpu, 4096, 8)
    for n in range(20):
        _same(dev, np.zeros(n, np.uint8), 1, [8])
        _same(dev, np.frombuffer((SYNC_BYTES * 5)[:n], np.uint8), 1, [8])
    for back in range(1, 8):  # a sync word, or what fits of it, at each of the last 7 byte positions
        for n in (16, 17, 18, 19, 40):
            body = bytearray(n)
            body[n - back:] = SYNC_BYTES[:back]
            assert len(_same(dev, np.frombuffer(bytes(body[:n]), np.uint8), 1, [8])) == 0
    frame = crafted_frame(2, rice_words=3)
    for blob in (b"\x11" + frame, b"\x11\x12" + frame + SYNC_BYTES, b"\x11" * 3 + frame * 3 + SYNC_BYTES[:3], frame + b"\x11" + frame[:-1], b"\x11" * 7 + frame + frame[:-4] + b"\x12" + frame):
        _same(dev, np.frombuffer(blob, np.uint8), 2, [0, 1, 8])


@pytest.mark.gpu
@pytest.mark.parametrize("phase", [1, 2, 3])
def test_a_sync_word_across_every_boundary_of_the_candidates_kernel(gpu, phase):  # noqa: F811
    """Frames that start `phase` bytes into the last word of a lane's, a wave's (64 words) and a workgroup's (4096 words) stretch:
    the sync word lies across the boundary and is seen once, by the word it starts in.  Then payloads of a chunk - 1, a chunk, a
    chunk + 1 and two chunks + 1 words whose last frame ends at the payload's last byte, inside its last PARTIAL word."""
    s = ua.rice_stream(1, 12)
    frames = bytes(s.buf)
    dev = _UaDevice(gpu, 4 * (2 * CHUNK + 2) + 512, 64)
    for word in (0, 1, 63, 64, 255, 256, CHUNK - 1, CHUNK, 2 * CHUNK - 1):
        payload = np.frombuffer(ua.garbage(4 * word + phase, word) + frames, np.uint8)
        want = _same(dev, payload, 1, [64])
        assert want["offset"].tolist() == [4 * word + phase + o for o in s.offs[:12]], word
    for words in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        total = 4 * words + phase  # payload_bytes % 4 == phase, and the last frame ends there
        payload = np.frombuffer(ua.garbage(total - len(frames), words) + frames, np.uint8)
        want = _same(dev, payload, 1, [64])
        assert len(payload) == total and len(want) == 12 and int(want["offset"][-1] + want["bytes"][-1]) == total, words
        # ... and with its last 1 .. 4 bytes gone, the last frame is not one
        for short in (1, 2, 3, 4):
            assert len(_same(dev, payload[:total - short], 1, [64], copy=False)) == 11  # (frame 10 is trusted: it needs no confirmation)


@pytest.mark.gpu
@pytest.mark.parametrize("candidates", [4095, 4096, 4097])
def test_both_sides_of_a_links_workgroup_at_phase_1(gpu, candidates):  # noqa: F811
    """16-byte mono frames one byte off the word grid, five of them damaged: exactly `candidates` candidates.  A links workgroup
    covers 4096 CANDIDATES, and "the next confirmed one" behind its last comes from the scan over the workgroups."""
    n = candidates + 5
    frames = [crafted_frame(1, tag=f) for f in range(n)]
    s = Stream(frames, 1)
    for f in [7, n - 40, n - 38] + ([4096, 4098] if n > 4100 else [n // 2, n // 2 + 1]):
        s.buf[s.offs[f]] ^= 0xFF
    payload = ua.insert(s.payload(), 0, ua.garbage(1))
    assert len(ua.candidates(payload.tobytes(), 1)) == candidates
    dev = _UaDevice(gpu, len(payload), 8192)
    want = _same(dev, payload, 1, [4096, 8192])
    assert np.all(want["offset"] % 4 == 1) and s.offs[n - 39] + 1 not in want["offset"].tolist()
    assert len(want) == candidates - (2 if n > 4100 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 2, 3, 4, 16, 17])
def test_one_frame_far_longer_than_its_neighbours_at_every_shift(gpu, shift):  # noqa: F811
    """A mono frame of 65535 zero Rice words (256 KiB: 64 copy workgroups) among small ones, all of them `shift` bytes behind their
    place in the compacted payload: the straight copy by funnel shift (1, 2, 3, 17), by dwords (4) and by 16-byte lines (16).  The
    payload ends with the last frame, so the funnel's second word is the payload's partial one at its very end."""
    small = [crafted_frame(1, rice_words=f % 11, tag=f) for f in range(10)]
    s = Stream(small[:5] + [crafted_frame(1, rice_words=65535, tag=99, fill=0)] + small[5:], 1)
    payload = ua.insert(s.payload(), 0, ua.garbage(shift))
    dev = _UaDevice(gpu, len(payload), 16)
    want = _same(dev, payload, 1, [16])
    assert len(want) == 11 and int(want["skipped_before"][0]) == shift and int(want["bytes"].max()) == 4 + 12 + 4 * 65535
    # out_cap cuts at a frame: the long one does not fit, and nothing of it or behind it is written
    n_bytes = dev.load(payload)
    ends = np.cumsum(want["bytes"], dtype=np.uint64).tolist()
    packed = _packed(payload, want)
    for out_cap, kept in ((ends[5] - 1, 5), (ends[5], 6), (ends[4] + 3, 5), (ends[-1] - 4, 10), (3, 0)):
        got, totals, offs, out = dev.payload(n_bytes, 16, 1, out_cap=out_cap)
        assert got.tobytes() == want.tobytes() and offs.tolist() == [0] + ends, "a frame that does not fit is still counted"
        limit = ends[kept - 1] if kept else 0
        assert out[:limit].tobytes() == packed[:limit].tobytes() and (out[limit:] == GUARD).all(), (out_cap, kept)


@pytest.mark.gpu
def test_a_copy_workgroup_with_two_gaps_of_different_phases_inside(gpu):  # noqa: F811
    """Frames of a few hundred bytes, so that one copy workgroup's 4096 destination words hold many of them, with 1 byte inserted
    in front of one and 2 in front of another (shifts 0, 1 and 3 inside one workgroup), and then a run long enough for the
    workgroups behind to copy straight at shift 3."""
    frames = [crafted_frame(2, rice_words=60 + f % 7, tag=f) for f in range(150)]
    s = Stream(frames, 2)
    assert s.offs[9] < 4 * CHUNK < s.offs[149]
    payload = ua.insert(ua.insert(s.payload(), s.offs[9], ua.garbage(2)), s.offs[4], ua.garbage(1))
    dev = _UaDevice(gpu, len(payload), 256)
    want = _same(dev, payload, 2, [256])
    assert len(want) == 150 and want["skipped_before"][[4, 9]].tolist() == [1, 2]
    _, _, _, out = dev.payload(dev.load(payload), 256, 2, records=False)
    assert out[:len(s.buf)].tobytes() == bytes(s.buf)


@pytest.mark.gpu
def test_every_frame_behind_two_insertions_decodes(gpu):  # noqa: F811
    """12 real stereo frames, 3 bytes inserted before frame 4 and 1 byte before frame 9: sela_hip_decode_payload_device on the
    compacted payload gives the PCM of all 12 frames, byte for byte the decode of the intact stream.  The word salvage of the same
    bytes takes the 4 frames in front of the first insertion and loses frames 4 .. 8; 3 + 1 bytes put frames 9 .. 11 back on the
    word grid, where its rule finds them again."""
    torch = gpu
    base, pcm = _encoded(12, 2, 36)
    intact = base.payload()
    payload = ua.insert(ua.insert(intact, base.offs[9], ua.garbage(1)), base.offs[4], ua.garbage(3))
    dec = codec.Decoder(16, 2)
    clean, _, count = dec.decode_payload(torch.from_numpy(intact).cuda(), 16)
    torch.cuda.synchronize()
    assert int(count.item()) == 12
    clean = clean[:12].cpu().numpy().copy()
    assert np.array_equal(clean, pcm)
    salvager = codec.Salvager(len(payload), 16, 2, unaligned=True)
    out, offsets, _, totals = salvager.payload(torch.from_numpy(payload).cuda())
    totals = totals.cpu().numpy().view(np.uint64).tolist()
    assert totals == [12, 2, len(intact), len(payload)]
    assert out[:len(intact)].cpu().numpy().tobytes() == intact.tobytes()
    back, _, count = dec.decode_payload(out[:totals[2]], 16)
    torch.cuda.synchronize()
    dec.check()
    assert int(count.item()) == 12 and back[:12].cpu().numpy().tobytes() == clean.tobytes()
    word = codec.Salvager(len(payload), 16, 2)
    word.frames(torch.from_numpy(payload).cuda())
    lost = word.records()
    assert lost.tobytes() == codec.salvage_frames(payload, 2, 16)[0].tobytes()
    assert lost["offset"].tolist() == base.offs[:4] + [o + 4 for o in base.offs[9:12]], "frames 4 .. 8 are lost to the word salvage"


@pytest.mark.gpu
def test_refusals_come_before_anything_is_enqueued_and_the_formula_suffices(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    s = ua.rice_stream(2, 4)
    payload = ua.insert(s.payload(), s.offs[2], ua.garbage(1))
    n = len(payload)
    dev = _UaDevice(gpu, n, 4)
    dev.payload(dev.load(payload), 4, 2)
    torch.cuda.synchronize()
    before = [t.clone() for t in (dev.records, dev.totals, dev.offsets, dev.out)]
    stream = torch.cuda.current_stream().cuda_stream
    ws_bytes = dev.ws.numel()
    assert ws_bytes == int(lib.sela_hip_salvage_unaligned_workspace_bytes(n, 4))

    def frames(p=dev.buf.data_ptr(), size=n, channels=2, r=dev.records.data_ptr(), t=dev.totals.data_ptr(), w=dev.ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_salvage_frames_unaligned_device(p, size, 4, channels, r, t, w, wb, stream)

    def copy(p=dev.buf.data_ptr(), size=n, channels=2, o=dev.out.data_ptr(), cap=n // 4 * 4, f=dev.offsets.data_ptr(), r=dev.records.data_ptr(),
             t=dev.totals.data_ptr(), w=dev.ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_salvage_payload_unaligned_device(p, size, 4, channels, o, cap, f, r, t, w, wb, stream)

    for call, code in [(lambda: frames(p=dev.buf.data_ptr() + 1), EINVAL), (lambda: frames(channels=0), EINVAL), (lambda: frames(channels=256), EINVAL),
                       (lambda: frames(p=None), EINVAL), (lambda: frames(r=None), EINVAL), (lambda: frames(t=None), EINVAL), (lambda: frames(w=None), EINVAL),
                       (lambda: frames(wb=ws_bytes - 1), ECAPACITY), (lambda: frames(size=1 << 32, wb=1 << 60), EINVAL),
                       (lambda: copy(p=dev.buf.data_ptr() + 2), EINVAL), (lambda: copy(o=dev.out.data_ptr() + 1), EINVAL), (lambda: copy(channels=0), EINVAL),
                       (lambda: copy(p=None), EINVAL), (lambda: copy(o=None), EINVAL), (lambda: copy(f=None), EINVAL), (lambda: copy(t=None), EINVAL),
                       (lambda: copy(w=None), EINVAL), (lambda: copy(wb=ws_bytes - 1), ECAPACITY), (lambda: copy(size=1 << 32, wb=1 << 60), EINVAL),
                       (lambda: copy(o=dev.buf.data_ptr() + 8), EINVAL), (lambda: copy(o=dev.buf.data_ptr() + n // 4 * 4 - 4, cap=8), EINVAL)]:
        assert call() == code
        assert lib.sela_hip_last_error().decode()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (dev.records, dev.totals, dev.offsets, dev.out))), "a refused call wrote something"
    assert frames() == 0 and copy(r=None) == 0 and copy(o=None, cap=0) == 0  # (no records wanted; no room given: no out needed)
    torch.cuda.synchronize()
    assert int(dev.totals.cpu()[0]) == 4
    # the worst case of the workspace, in exactly the bytes the formula gives: nothing but sync words, on and off the grid
    for n_bytes, lead in ((1 << 20, 0), ((1 << 20) + 3, 1), ((1 << 16) + 2, 3)):
        body = (b"\x11" * lead + SYNC_BYTES * (n_bytes // 4 + 1))[:n_bytes]
        for cap in (4, 5000):
            big = _UaDevice(gpu, n_bytes, cap)
            assert big.ws.numel() == int(lib.sela_hip_salvage_unaligned_workspace_bytes(n_bytes, cap))
            _same(big, np.frombuffer(body, np.uint8), 1, [cap])


@pytest.mark.gpu
def test_one_capture_replayed_over_payloads_damaged_at_different_phases(gpu):  # noqa: F811
    torch = gpu
    s = ua.rice_stream(2, 12)
    capacity = len(s.buf) + 64
    salvager = codec.Salvager(capacity, 16, 2, unaligned=True)
    buf = torch.zeros(capacity, dtype=torch.uint8, device="cuda")
    first = s.payload()
    buf[:len(first)].copy_(torch.from_numpy(first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        salvager.payload(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, offsets, records, totals = salvager.payload(buf)
    for payload in (ua.insert(first, s.offs[5], ua.garbage(1)), ua.insert(ua.insert(first, s.offs[8], ua.garbage(3)), s.offs[2], ua.garbage(2)),
                    ua.delete(first, s.rice(4)[0] + 1, 3), first):
        buf.zero_()
        buf[:len(payload)].copy_(torch.from_numpy(payload))
        graph.replay()
        torch.cuda.synchronize()
        whole = np.concatenate([payload, np.zeros(capacity - len(payload), np.uint8)])  # (the call was captured over the whole buffer)
        want, want_totals = codec.salvage_frames(whole, 2, 16, unaligned=True)
        assert len(want) >= 10 and totals.cpu().numpy().view(np.uint64).tolist() == want_totals.tolist() and salvager.records().tobytes() == want.tobytes()
        packed = _packed(whole, want)
        assert out[:len(packed)].cpu().numpy().tobytes() == packed.tobytes()
        assert offsets[:len(want) + 1].cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(want["bytes"], dtype=np.int64)]).tolist()
