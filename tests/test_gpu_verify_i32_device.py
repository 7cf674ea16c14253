"""sela_hip_verify_i32_device, sela_hip_verify_payload_i32_device and sela_hip_verify_i32: a stream held against
the int32 samples it was made from, frame by frame, on the device.  With m the count sela_hip_decode_i32_device reports for
(frame, channel) and L the original's length, diff_counts[f] is the sum over the channels of the values below min(m, L) that
differ plus |m - L|, first_diff[f] the smallest c * stride + i (or 0xFFFFFFFF), status[2] the number of frames with a
difference; status[0] and [1] are the decode call's.  The expectation is always one of two things: the fixture
tests/golden/verify_wide.json (made from the unmodified reference, held against the oracle by test_verify32_cpu.py), or
compare(Decoder32's output and counts, the original and its lengths) computed here in numpy by those definitions."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

import generic_cases as gc
import topology_cases as tc
import wide_cases as wc
from gpu_common import _build_frame, _rice_words, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DIFF = 0xFFFFFFFF
GUARD = 64          # words in front of and behind each output array that no call may write
SENTINEL = 0x5E1A5E1A


def _bytes(blob):
    return np.frombuffer(bytes(blob), np.uint8).copy() if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, np.uint8)


def _stream(blobs):
    return np.frombuffer(b"".join(bytes(b) for b in blobs), np.uint8).copy(), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)


def _on_device(torch, blob, offs):
    data = _bytes(blob)
    frames = torch.zeros(max(len(data), 4), dtype=torch.uint8, device="cuda")
    if len(data):
        frames[: len(data)].copy_(torch.from_numpy(data))
    return frames, torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).cuda()


def _decode32(torch, blob, offs, ch, stride):
    """sela_hip_decode_i32_device -> (samples int32 [n, ch, stride], counts uint32 [n, ch], status uint32 [4])."""
    n = len(offs) - 1
    dec = codec.Decoder32(max(n, 1), ch, stride)
    dec.samples.zero_()
    frames, o = _on_device(torch, blob, offs)
    samples, counts, _ = dec.decode(frames, o, n)
    torch.cuda.synchronize()
    return samples.cpu().numpy().copy(), counts.cpu().numpy().view(np.uint32).copy(), dec.status.cpu().numpy().view(np.uint32).copy()


def _expect(dec, counts, orig, lengths, stride):
    """The definitions of include/sela_hip.h, in numpy -> (diff_counts uint32 [n], first_diff uint32 [n])."""
    n, ch = counts.shape
    out_c, out_f = np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32)
    for f in range(n):
        total, first = 0, NO_DIFF
        for c in range(ch):
            m = int(counts[f, c])
            L = stride if lengths is None else min(int(lengths[f, c]), stride)
            k = min(m, L)
            d = np.flatnonzero(dec[f, c, :k] != orig[f, c, :k])
            total += len(d) + abs(m - L)
            i = int(d[0]) if len(d) else (k if m != L else None)
            if i is not None:
                first = min(first, c * stride + i)
        out_c[f], out_f[f] = total, first
    return out_c, out_f


class _Device:
    """Buffers of one sela_hip_verify_i32_device call, the raw C ABI: guard words around both output arrays, the inputs kept for
    a look afterwards."""

    def __init__(self, torch, n, ch, stride):
        self.torch, self.n, self.ch, self.stride = torch, n, ch, stride
        self.counts = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.first = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.sample_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_verify_i32_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")
        self.ws.fill_(0xA5)  # (no initialisation is needed: whatever lies there)

    def verify(self, blob, offs, orig, lengths=None, with_offsets=True):
        torch = self.torch
        frames, o = _on_device(torch, blob, offs)
        s_host = np.ascontiguousarray(orig, np.int32).reshape(-1)
        assert len(s_host) == self.n * self.ch * self.stride
        s = torch.from_numpy(s_host.copy() if len(s_host) else np.zeros(1, np.int32)).cuda()
        ln = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, np.uint32).reshape(-1).view(np.int32).copy()).cuda()
        before = frames.clone(), s.clone(), None if ln is None else ln.clone()
        capi.check(capi.lib().sela_hip_verify_i32_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, s.data_ptr(), None if ln is None else ln.data_ptr(),
            self.counts.data_ptr() + 4 * GUARD, self.first.data_ptr() + 4 * GUARD, self.sample_offsets.data_ptr() if with_offsets else None,
            self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(frames, before[0]), "d_frames was written"
        assert torch.equal(s, before[1]), "d_samples was written"
        assert ln is None or torch.equal(ln, before[2]), "d_lengths was written"
        return self.results()

    def results(self):
        n = self.n
        c = self.counts.cpu().numpy().view(np.uint32)
        f = self.first.cpu().numpy().view(np.uint32)
        for a in (c, f):
            assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + n:] == SENTINEL).all(), "written outside the per-frame arrays"
        return c[GUARD: GUARD + n].copy(), f[GUARD: GUARD + n].copy(), self.status.cpu().numpy().view(np.uint32).copy()

    def fallback_frames(self):
        return int(capi.lib().sela_hip_debug_verify_i32_fallback_frames(self.ws.data_ptr(), self.n, self.ch, self.stride))


def _against_decode(torch, blob, offs, ch, stride, orig=None, lengths=None, plant=(), fallback=None, label=""):
    """The verify call == compare(Decoder32 output, original) by the definitions.  orig None: the decoder's own output (an exact
    stream); plant: (frame, channel, i) values of the original to change -> (counts, first, status, decoded counts)."""
    n = len(offs) - 1
    lengths = None if lengths is None else np.asarray(lengths, np.uint32)
    dec, m, dst = _decode32(torch, blob, offs, ch, stride)
    orig = dec.copy() if orig is None else np.ascontiguousarray(orig, np.int32).copy()
    for f, c, i in plant:
        orig[f, c, i] ^= 1 << ((f + c + i) % 31)
    want_counts, want_first = _expect(dec, m, orig, lengths, stride)
    dev = _Device(torch, n, ch, stride)
    counts, first, st = dev.verify(blob, offs, orig, lengths)
    assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), 0), (label, st, dst)
    if codec.decode_status_error(dst) == 0:
        assert np.array_equal(counts, want_counts), (label, np.flatnonzero(counts != want_counts)[:8], counts[:8], want_counts[:8])
        assert np.array_equal(first, want_first), (label, np.flatnonzero(first != want_first)[:8], first[:8], want_first[:8])
        assert int(st[2]) == int((want_counts != 0).sum()), (label, st)
    if fallback is not None:
        assert dev.fallback_frames() == fallback, (label, dev.fallback_frames(), fallback)
    return counts, first, st, m


# ---- 1. the reference's own lossy frames of 24-bit audio ----------------------------------------------------------------------------
def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "verify_wide.json")) as fh:
        fx = json.load(fh)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        from make_verify_wide import wide_frames
    finally:
        sys.path.pop(0)
    return fx, wide_frames(fx["frames"], fx["seed"], fx["noise_seed"], fx["bits"])


def _fixture_arrays(fx, n):
    counts, first = np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32)
    for e in fx["lossy"]:
        if e["frame"] < n:
            counts[e["frame"]], first[e["frame"]] = e["count"], e["first"]
    return counts, first


def test_the_references_own_lossy_wide_frames_are_found_exactly(gpu):  # noqa: F811
    torch = gpu
    fx, x = _fixture()
    n = fx["frames"]
    want_counts, want_first = _fixture_arrays(fx, n)
    d_x = torch.from_numpy(x).cuda()
    enc = codec.Encoder32(n, 2, 2048)
    frames, offsets, _ = enc.encode(d_x)
    enc.check()
    ver = codec.Verifier32(n, 2, 2048)
    counts, first = ver.verify(frames, offsets, n, d_x)
    ver.check()
    counts, first = counts.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32)
    print("lossy frames found:", [(int(f), int(counts[f]), int(first[f])) for f in np.flatnonzero(counts)])
    assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first)
    assert ver.lossy_frames() == len(fx["lossy"]) and ver.status.cpu().numpy().tolist() == [0, 0, len(fx["lossy"]), 0]
    assert ver.fallback_frames() == 0
    # ... through the payload call (the stream's bytes alone: the index takes whatever follows for more frames or for the end)
    ver.diff_counts.fill_(-7), ver.first_diff.fill_(-7)
    c2, f2, count = ver.verify_payload(frames[: enc.needed_bytes()], d_x)
    ver.check()
    assert int(count.item()) == n and ver.lossy_frames() == len(fx["lossy"])
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), want_counts) and np.array_equal(f2.cpu().numpy().view(np.uint32), want_first)
    # ... and through the raw call with guards
    blob, offs = enc.to_host()
    c3, f3, st = _Device(torch, n, 2, 2048).verify(blob, offs, x)
    assert np.array_equal(c3, want_counts) and np.array_equal(f3, want_first) and st.tolist() == [0, 0, len(fx["lossy"]), 0]


# ---- 2. planted differences in an exact stream ------------------------------------------------------------------------------------
def _wide_stereo_stream(n):
    """Frames of 25- to 31-bit audio the encoder takes: (stream, offsets, names)."""
    sig = dict(wc.wide_signals(n, 5))
    pairs = [("tone 25-bit", "noise 25-bit"), ("tone 28-bit", "tone 27-bit"), ("tone 30-bit", "sparse 28-bit"), ("sparse 30-bit", "tone 26-bit"),
             ("tone 31-bit", "sparse 31-bit"), ("dc 2^29 + sine", "tone 29-bit")]
    blobs, names = [], []
    for a, b in pairs:
        try:
            blobs.append(codec.encode_i32(np.stack([sig[a], sig[b]])[None])[0].tobytes())
            names.append((a, b))
        except capi.SelaHipError:  # (a residue beyond the zig-zag, or a difference that wraps: no encoder codes it)
            continue
    assert len(blobs) >= 3, names
    return _stream(blobs) + (names,)


def test_planted_differences_are_found_where_they_are(gpu):  # noqa: F811
    torch = gpu
    n = 9000  # (three slices of 4096 samples)
    stream, offs, names = _wide_stereo_stream(n)
    frames = len(offs) - 1
    dec, m, dst = _decode32(torch, stream, offs, 2, n)
    assert codec.decode_status_error(dst) == 0 and (m == n).all()
    print("wide frames taken:", names, "largest sample: 2^%.1f" % np.log2(float(np.abs(dec.astype(np.int64)).max())))
    assert int(np.abs(dec.astype(np.int64)).max()) >= 1 << 24, "no frame beyond 24 bits"
    last = frames - 1
    cases = {
        "channel 0, sample 0": [(0, 0, 0)],
        "the last sample": [(last, 1, n - 1)],
        "before a slice boundary": [(1, 0, 4095)],
        "behind a slice boundary": [(1, 0, 4096)],
        "both sides of it": [(1, 0, 4095), (1, 0, 4096)],
        "the second channel only": [(0, 1, 4097)],
        "one per channel": [(2, 0, 8191), (2, 1, 8192)],
        "in every frame": [(f, f & 1, 1000 * f + 3) for f in range(frames)],
    }
    for label, plant in cases.items():
        counts, first, st, _ = _against_decode(torch, stream, offs, 2, n, plant=plant, fallback=0, label=label)
        want_counts, want_first = np.zeros(frames, np.uint32), np.full(frames, NO_DIFF, np.uint32)
        for f, c, i in plant:
            want_counts[f] += 1
            want_first[f] = min(int(want_first[f]), c * n + i)
        assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first), label
        assert st.tolist() == [0, 0, len({p[0] for p in plant}), 0], (label, st)
    # nothing planted: an exact stream gives zeros
    counts, first, st, _ = _against_decode(torch, stream, offs, 2, n, label="exact")
    assert not counts.any() and (first == NO_DIFF).all() and int(st[2]) == 0
    # a stride that is no multiple of four (sample by sample) and a roomy one; a d_samples that is only 4-byte aligned
    for stride in (9001, 9004, 10000):
        _against_decode(torch, stream, offs, 2, stride, plant=[(0, 0, 0), (1, 1, 4096), (last, 1, n - 1)], lengths=np.full((frames, 2), n), fallback=0,
                        label=("stride", stride))
    lib = capi.lib()
    d_frames, d_offs = _on_device(torch, stream, offs)
    orig = dec.copy()
    orig[0, 0, 1] += 1
    orig[last, 1, n - 1] -= 1
    for shift in (1, 3):
        room = torch.zeros(orig.size + 8, dtype=torch.int32, device="cuda")
        room[shift: shift + orig.size].copy_(torch.from_numpy(orig.reshape(-1)))
        assert room.data_ptr() % 16 == 0
        dev = _Device(torch, frames, 2, n)
        capi.check(lib.sela_hip_verify_i32_device(d_frames.data_ptr(), d_offs.data_ptr(), frames, 2, n, room.data_ptr() + 4 * shift, None,
                                                  dev.counts.data_ptr() + 4 * GUARD, dev.first.data_ptr() + 4 * GUARD, None, dev.status.data_ptr(),
                                                  dev.ws.data_ptr(), dev.ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        counts, first, st = dev.results()
        assert counts.tolist() == [1] + [0] * (frames - 2) + [1] and int(first[0]) == 1 and int(first[last]) == 2 * n - 1 and int(st[2]) == 2


# ---- 3. lengths and channel counts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [127, 4095, 4096, 4097, 9000, 65535])
def test_lengths(gpu, n):  # noqa: F811
    rng = np.random.default_rng(n)
    frames = 1 if n == 65535 else 3
    x = np.stack([np.stack([_signal(rng, "tone", n, 20), _signal(rng, "noise", n, 17)]) for _ in range(frames)]).astype(np.int32)
    blob, offs = codec.encode_i32(x)
    # against the audio itself, then an exact stream with differences at the ends and around every slice boundary
    _against_decode(gpu, blob, offs, 2, n, orig=x, fallback=0, label=(n, "the audio"))
    spots = sorted({0, n - 1} | {i for b in range(4096, n, 4096) for i in (b - 1, b)})
    plant = [(f, (f + k) & 1, i) for f in range(frames) for k, i in enumerate(spots)]
    counts, first, _, _ = _against_decode(gpu, blob, offs, 2, n, plant=plant, fallback=0, label=(n, "planted"))
    assert counts.tolist() == [len(spots)] * frames
    assert first.tolist() == [min(((f + k) & 1) * n + i for k, i in enumerate(spots)) for f in range(frames)]


def test_one_sample_mono(gpu):  # noqa: F811
    blob = _build_frame([(0, 0, 0, np.zeros(0, np.int32), np.array([-77], np.int32))])
    offs = np.array([0, len(blob)], np.uint64)
    dec, m, dst = _decode32(gpu, blob, offs, 1, 1)
    assert codec.decode_status_error(dst) == 0 and m.tolist() == [[1]] and dec.tolist() == [[[-77]]]
    counts, first, st, _ = _against_decode(gpu, blob, offs, 1, 1, fallback=0, label="one sample")
    assert counts.tolist() == [0] and first.tolist() == [NO_DIFF]
    counts, first, st, _ = _against_decode(gpu, blob, offs, 1, 1, plant=[(0, 0, 0)], fallback=0, label="one sample, changed")
    assert counts.tolist() == [1] and first.tolist() == [0] and st.tolist() == [0, 0, 1, 0]


@pytest.mark.parametrize("ch, n", [(1, 2048), (2, 2048), (3, 1000), (8, 2049), (255, 300)])
def test_channel_counts(gpu, ch, n):  # noqa: F811
    rng = np.random.default_rng(ch)
    x = np.stack([np.stack([_signal(rng, ("tone", "noise", "sparse")[c % 3], n, 12 + c % 9) for c in range(ch)]) for _ in range(2)]).astype(np.int32)
    blob, offs = codec.encode_i32(x)
    _against_decode(gpu, blob, offs, ch, n, orig=x, fallback=0, label=(ch, "the audio"))
    plant = [(0, 0, 0), (0, ch - 1, n - 1), (1, ch // 2, n // 2), (1, ch - 1, 0)]
    counts, first, st, _ = _against_decode(gpu, blob, offs, ch, n, plant=plant, fallback=0, label=(ch, "planted"))
    assert counts.tolist() == [2, 2] and int(first[0]) == 0 and int(first[1]) == min((ch // 2) * n + n // 2, (ch - 1) * n) and int(st[2]) == 2


# ---- 4. frames whose channels differ in length ------------------------------------------------------------------------------------
def test_ragged_frames(gpu):  # noqa: F811
    for label, chans in gc.ragged_cases():
        ch, lens = len(chans), [len(c) for c in chans]
        stride = max(lens)
        blob = codec.encode_ragged(chans)
        offs = np.array([0, len(blob)], np.uint64)
        dec, m, dst = _decode32(gpu, blob, offs, ch, stride)
        assert codec.decode_status_error(dst) == 0 and m[0].tolist() == lens, label
        orig = np.zeros((1, ch, stride), np.int32)
        for c, x in enumerate(chans):
            orig[0, c, : len(x)] = x
        exact = np.array([lens], np.uint32)
        # the audio itself with its lengths, then the decoder's own output: exact lengths give zero
        _against_decode(gpu, blob, offs, ch, stride, orig=orig, lengths=exact, fallback=0, label=(label, "the audio"))
        counts, first, st, _ = _against_decode(gpu, blob, offs, ch, stride, lengths=exact, fallback=0, label=(label, "exact"))
        assert counts.tolist() == [0] and first.tolist() == [NO_DIFF] and int(st[2]) == 0
        # one shorter and one longer than the decoded count: one difference, at min(m, L)
        for c in range(ch):
            shorter = exact.copy()
            shorter[0, c] -= 1
            counts, first, _, _ = _against_decode(gpu, blob, offs, ch, stride, lengths=shorter, fallback=0, label=(label, c, "shorter"))
            assert counts.tolist() == [1] and first.tolist() == [c * stride + lens[c] - 1], (label, c)
            if lens[c] < stride:
                longer = exact.copy()
                longer[0, c] += 1
                counts, first, _, _ = _against_decode(gpu, blob, offs, ch, stride, lengths=longer, fallback=0, label=(label, c, "longer"))
                assert counts.tolist() == [1] and first.tolist() == [c * stride + lens[c]], (label, c)
        # no lengths: every channel is stride long, the missing samples count; a length above stride counts as stride
        missing = sum(stride - k for k in lens)
        where = min([c * stride + k for c, k in enumerate(lens) if k < stride], default=NO_DIFF)
        for lengths in (None, np.full((1, ch), stride + 1000, np.uint32), np.full((1, ch), 0xFFFFFFFF, np.uint32)):
            counts, first, _, _ = _against_decode(gpu, blob, offs, ch, stride, lengths=lengths, fallback=0, label=(label, "no lengths"))
            assert counts.tolist() == [missing] and first.tolist() == [where], label
        # a planted value behind a shorter channel's end is not looked at; one in front of it is
        c = int(np.argmin(lens))
        changed = dec.copy()
        changed[0, c, lens[c] - 1] ^= 4
        if lens[c] < stride:
            changed[0, c, lens[c]] ^= 4
        counts, first, _, _ = _against_decode(gpu, blob, offs, ch, stride, orig=changed, lengths=exact, fallback=0, label=(label, "behind the end"))
        assert counts.tolist() == [1] and first.tolist() == [c * stride + lens[c] - 1]


# ---- 5. subframe layouts ----------------------------------------------------------------------------------------------------------
def _layout_blob(o, layout, seed):
    return wc.frame_bytes(o, tc.subframes(layout, tc.ORDINARY, seed))


def _fallback_layouts(ch):
    refused = dict(tc.refused_layouts(ch))
    out = [("channel 0 twice, channel 1 never", refused["channel 0 twice, channel 1 never"]), ("type 2", refused["type 2"])]
    if ch == 3:
        out.append(("a chain in stream order", tc.CHAIN_IN_STREAM_ORDER))
    return out


@pytest.mark.parametrize("ch", sorted(tc.ACCEPTED_LAYOUTS))
def test_every_accepted_layout_takes_the_direct_kernel(gpu, ch):  # noqa: F811
    o = oracle()
    blobs = [_layout_blob(o, layout, 100 * ch + k) for k, (_, layout) in enumerate(tc.ACCEPTED_LAYOUTS[ch])]
    stream, offs = _stream(blobs)
    n = len(blobs)
    counts, _, st, m = _against_decode(gpu, stream, offs, ch, tc.N, fallback=0, label=(ch, "exact"))
    assert not counts.any() and (m == tc.N).all() and st.tolist() == [0, 0, 0, 0]
    plant = [(f, c, (37 * f + 501 * c) % tc.N) for f in range(n) for c in range(ch)] + [(0, ch - 1, tc.N - 1)]
    counts, _, _, _ = _against_decode(gpu, stream, offs, ch, tc.N, plant=plant, fallback=0, label=(ch, "planted"))
    assert counts.tolist() == [ch + 1] + [ch] * (n - 1)
    _against_decode(gpu, stream, offs, ch, tc.N + 3, plant=plant, lengths=np.full((n, ch), tc.N), fallback=0, label=(ch, "an odd stride"))


@pytest.mark.parametrize("ch", [2, 3, 5])
def test_other_layouts_take_the_fallback(gpu, ch):  # noqa: F811
    o = oracle()
    good = [_layout_blob(o, layout, 7 * ch + k) for k, (_, layout) in enumerate(tc.ACCEPTED_LAYOUTS[ch][:2])]
    others = [(name, _layout_blob(o, layout, 900 + 10 * ch + k)) for k, (name, layout) in enumerate(_fallback_layouts(ch))]
    for name, blob in others:  # each alone
        offs = np.array([0, len(blob)], np.uint64)
        _against_decode(gpu, blob, offs, ch, tc.N, fallback=1, label=(ch, name))
        plant = [(0, c, (11 + 700 * c) % tc.N) for c in range(ch)]
        _against_decode(gpu, blob, offs, ch, tc.N, plant=plant, fallback=1, label=(ch, name, "planted"))
    # direct and fallback frames in one stream
    blobs = [good[0]] + [b for _, b in others[:1]] + [good[1]] + [b for _, b in others[1:]] + [good[0]]
    stream, offs = _stream(blobs)
    n = len(blobs)
    counts, first, st, m = _against_decode(gpu, stream, offs, ch, tc.N, fallback=len(others), label=(ch, "mixed"))
    assert int(counts[0]) == 0 and int(counts[2]) == 0 and int(counts[n - 1]) == 0
    if ch == 3:  # the chain's three channels are all there
        assert m[n - 2].tolist() == [tc.N] * 3 and int(counts[n - 2]) == 0
    assert int(m[1, 1]) == 0 and int(counts[1]) == tc.N and int(first[1]) == tc.N  # (channel 1 never named: all of it is missing)
    plant = [(f, c, (5 * f + 300 * c) % tc.N) for f in range(n) for c in range(ch) if m[f, c]]
    _against_decode(gpu, stream, offs, ch, tc.N, plant=plant, lengths=m, fallback=len(others), label=(ch, "mixed, planted, the decoder's lengths"))
    _against_decode(gpu, stream, offs, ch, tc.N + 2, plant=plant, fallback=len(others), label=(ch, "mixed, an odd stride"))


# ---- 6. sela_hip_debug_standard_first ---------------------------------------------------------------------------------------------
def test_the_three_decode_routes_give_the_same(gpu):  # noqa: F811
    v, _, _ = gc.long_rice_stream()  # (its first 65535 values: a subframe far beyond the parser's plan)
    rng = np.random.default_rng(3)
    frame = _build_frame([(0, 0, 0, rng.integers(-4, 5, 2).astype(np.int32), v[:65535])])
    small = codec.encode_i32(np.stack([_signal(rng, "tone", 3000, 18)])[None])[0].tobytes()
    stream, offs = _stream([small, frame, small])
    seen = []
    for mode in (0, 1, 2):
        capi.lib().sela_hip_debug_standard_first(mode)
        try:
            counts, first, st, m = _against_decode(gpu, stream, offs, 1, 65535, plant=[(0, 0, 2999), (1, 0, 0), (1, 0, 65534)], lengths=[[3000], [65535], [2999]],
                                                   fallback=0, label=("mode", mode))
        finally:
            capi.lib().sela_hip_debug_standard_first(-1)
        assert counts.tolist() == [1, 2, 1] and first.tolist() == [2999, 0, 2999] and st.tolist() == [0, 0, 3, 0], (mode, counts, first, st)
        seen.append((counts.tolist(), first.tolist(), st.tolist(), m.tolist()))
    assert seen[0] == seen[1] == seen[2]


# ---- 7. status words --------------------------------------------------------------------------------------------------------------
def _sub(c, typ, parent, order, q, ck, res, rk, n=None):
    cw = _rice_words(np.asarray(q, np.int32), ck) if order else np.zeros(0, np.uint32)
    rw = _rice_words(np.asarray(res, np.int32), rk)
    return (struct.pack("<BBBBHB", c, typ, parent, ck, len(cw), order) + cw.tobytes()
            + struct.pack("<BHH", rk, len(rw), len(res) if n is None else n) + rw.tobytes())


def _status_cases():
    rng = np.random.default_rng(6)
    x = np.stack([np.stack([_signal(rng, "tone", 700, 19), _signal(rng, "noise", 700, 14)]) for _ in range(4)]).astype(np.int32)
    frames, offs = codec.encode_i32(x)
    bad_sync = frames.copy()
    bad_sync[int(offs[2])] ^= 0xFF
    cut = offs.copy()
    cut[1] -= 8
    sync = bytes.fromhex("00ff55aa")
    good = sync + _sub(0, 0, 0, 2, [-40, 10], 4, rng.integers(-300, 301, 500), 8)
    dry = sync + _sub(0, 0, 0, 2, [-40, 10], 4, np.full(400, 1000), 2, n=4000)
    dry_stream, dry_offs = _stream([good, dry, good])
    yield "bad sync word", bad_sync, offs, 2, 700
    yield "truncated frame", frames, cut, 2, 700
    yield "stride too small", frames, offs, 2, 699
    yield "a Rice stream that runs dry", dry_stream, dry_offs, 1, 4096
    yield "clean", frames, offs, 2, 700


def test_status_words_are_the_decode_calls(gpu):  # noqa: F811
    lib = capi.lib()
    seen = set()
    for label, blob, offs, ch, stride in _status_cases():
        n = len(offs) - 1
        _, _, dst = _decode32(gpu, blob, offs, ch, stride)
        orig = np.zeros((n, ch, stride), np.int32)
        _, _, st = _Device(gpu, n, ch, stride).verify(blob, offs, orig)
        assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), 0), (label, st, dst)
        # ... and their code is the host call's, from both host calls
        fr, o = _bytes(blob), np.ascontiguousarray(offs, np.uint64)
        out, cnt = np.zeros((n, ch, stride), np.int32), np.zeros((n, ch), np.uint32)
        rc = lib.sela_hip_decode_i32(fr.ctypes.data, o.ctypes.data, n, ch, out.ctypes.data, stride, cnt.ctypes.data)
        status = st.copy()
        status[2] = 0
        assert codec.decode_status_error(status) == rc == codec.decode_status_error(dst), (label, rc, st, dst)
        c, f = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        assert lib.sela_hip_verify_i32(fr.ctypes.data, o.ctypes.data, n, ch, stride, orig.ctypes.data, None, c.ctypes.data, f.ctypes.data, None) == rc, label
        seen.add(rc)
        if label == "stride too small":
            assert int(st[0]) & capi.FLAG_STRIDE
    assert seen == {0, -4, -5}, seen


# ---- 8. nothing else is written ---------------------------------------------------------------------------------------------------
def test_no_frames_no_offsets_and_the_payload_calls_tail(gpu):  # noqa: F811
    torch = gpu
    dev = _Device(torch, 0, 2, 2048)
    counts, first, st = dev.verify(b"", np.zeros(1, np.uint64), np.zeros(0, np.int32))
    assert (st == 0).all() and len(counts) == 0 and int(dev.sample_offsets[0].item()) == 0
    # without d_sample_offsets (_Device.verify looks at the guards, d_frames and d_samples on every call of this file)
    rng = np.random.default_rng(12)
    x = np.stack([np.stack([_signal(rng, "tone", 900, 18)] * 2) for _ in range(4)]).astype(np.int32)
    blob, offs = codec.encode_i32(x)
    dec, _, _ = _decode32(torch, blob, offs, 2, 900)
    changed = dec.copy()
    changed[1, 1, 899] += 1
    changed[3, 0, 5] -= 1
    dev = _Device(torch, 4, 2, 900)
    counts, first, st = dev.verify(blob, offs, changed, with_offsets=False)
    assert (dev.sample_offsets.cpu().numpy() == -1).all()
    assert counts.tolist() == [0, 1, 0, 1] and first.tolist() == [NO_DIFF, 1799, NO_DIFF, 5] and st.tolist() == [0, 0, 2, 0]
    # the payload call with room for more frames than the stream has: entries from the count on are not written
    ver = codec.Verifier32(7, 2, 900)
    ver.diff_counts.fill_(-7), ver.first_diff.fill_(-7)
    payload = torch.from_numpy(blob).cuda()
    c, f, count = ver.verify_payload(payload, torch.from_numpy(np.concatenate([changed, np.zeros((3, 2, 900), np.int32)])).cuda())
    ver.check()
    assert int(count.item()) == 4 and ver.lossy_frames() == 2
    assert c.cpu().numpy().tolist() == [0, 1, 0, 1, -7, -7, -7] and f.cpu().numpy().tolist() == [-1, 1799, -1, 5, -7, -7, -7]


def test_argument_errors_enqueue_nothing(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    x = np.stack([np.stack([_signal(np.random.default_rng(1), "tone", 500, 18)] * 2)] * 2).astype(np.int32)
    blob, o = codec.encode_i32(x)
    nb = len(blob)
    buf = torch.from_numpy(np.concatenate([blob, np.zeros(4, np.uint8)])).cuda()
    offs = torch.from_numpy(o.view(np.int64).copy()).cuda()
    s = torch.from_numpy(x.reshape(-1).copy()).cuda()
    ln = torch.full((4,), 500, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.sela_hip_verify_i32_workspace_bytes(2, 2, 500))
    ix_bytes = int(lib.sela_hip_index_workspace_bytes(nb, 2))
    ws = torch.empty(ws_bytes + ix_bytes, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    first = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    so = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    fo = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    nf = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def dev(frames=buf.data_ptr(), fo_=offs.data_ptr(), nfr=2, channels=2, stride=500, s_=s.data_ptr(), l_=ln.data_ptr(), c=counts.data_ptr(),
            f=first.data_ptr(), st=status.data_ptr(), w=ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_verify_i32_device(frames, fo_, nfr, channels, stride, s_, l_, c, f, so.data_ptr(), st, w, wb, stream)

    def pay(payload=buf.data_ptr(), channels=2, stride=500, s_=s.data_ptr(), c=counts.data_ptr(), f=first.data_ptr(), st=status.data_ptr(),
            o_=fo.data_ptr(), k=nf.data_ptr(), w=ws.data_ptr(), wb=ws_bytes + ix_bytes):
        return lib.sela_hip_verify_payload_i32_device(payload, nb, 2, channels, stride, s_, None, c, f, so.data_ptr(), o_, k, st, w, wb, stream)

    for call, code in [(lambda: dev(frames=buf.data_ptr() + 1), -2), (lambda: dev(channels=0), -2), (lambda: dev(channels=256), -2),
                       (lambda: dev(stride=0), -2), (lambda: dev(s_=None), -2), (lambda: dev(c=None), -2), (lambda: dev(f=None), -2),
                       (lambda: dev(st=None), -2), (lambda: dev(w=None), -2), (lambda: dev(fo_=None), -2), (lambda: dev(frames=None), -2),
                       (lambda: dev(s_=s.data_ptr() + 2), -2), (lambda: dev(l_=ln.data_ptr() + 1), -2), (lambda: dev(c=counts.data_ptr() + 2), -2),
                       (lambda: dev(f=first.data_ptr() + 1), -2), (lambda: dev(wb=ws_bytes - 1), -4), (lambda: dev(nfr=0x40000000), -2),
                       (lambda: pay(payload=buf.data_ptr() + 2), -2), (lambda: pay(channels=0), -2), (lambda: pay(stride=0), -2),
                       (lambda: pay(s_=None), -2), (lambda: pay(c=None), -2), (lambda: pay(f=None), -2), (lambda: pay(st=None), -2),
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
    assert codec.decode_status_error([int(st[0]), int(st[1]), 0, 0]) == 0 and int(st[3]) == 0 and so.cpu().numpy().tolist() == [0, 500, 1000]
    assert pay() == 0
    torch.cuda.synchronize()
    assert int(nf.item()) == 2 and fo.cpu().numpy().tolist() == o.tolist()


# ---- 9. capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["verify", "verify_payload"])
def test_encode_and_verify_in_one_graph(gpu, form):  # noqa: F811
    torch = gpu
    n, spc = 24, 3000
    inputs = []
    for seed, where in ((2, [(0, 0, 3), (11, 1, 9), (23, 1, 2999)]), (5, [(2, 0, 0), (20, 0, 2048)])):
        rng = np.random.default_rng(seed)
        x = np.stack([np.stack([_signal(rng, "tone", spc, 21), _signal(rng, "noise", spc, 18)]) for _ in range(n)]).astype(np.int32)
        held = x.copy()
        for f, c, i in where:
            held[f, c, i] += 1
        inputs.append((x, held))
    d_x = torch.zeros((n, 2, spc), dtype=torch.int32, device="cuda")
    d_held = torch.zeros((n, 2, spc), dtype=torch.int32, device="cuda")
    enc = codec.Encoder32(n, 2, spc)
    ver = codec.Verifier32(n, 2, spc)

    def load(k):
        d_x.copy_(torch.from_numpy(inputs[k][0]))
        d_held.copy_(torch.from_numpy(inputs[k][1]))
        enc.frames.zero_()  # (the payload form: what follows the stream must not look like a frame)

    def call():
        frames, offsets, _ = enc.encode(d_x)
        return ver.verify(frames, offsets, n, d_held) if form == "verify" else ver.verify_payload(frames, d_held)

    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # (the payload workspace is allocated here, not under capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for k in (0, 1, 0):
        load(k)
        ver.diff_counts.fill_(-7), ver.first_diff.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        enc.check()
        blob, offs = enc.to_host()
        want_counts, want_first, want_st = _Device(torch, n, 2, spc).verify(blob, offs, inputs[k][1])
        assert int(want_st[2]) >= 2
        assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want_counts), (form, k)
        assert np.array_equal(out[1].cpu().numpy().view(np.uint32), want_first), (form, k)
        assert np.array_equal(ver.status.cpu().numpy().view(np.uint32), want_st), (form, k)
        if form == "verify_payload":
            assert int(out[2].item()) == n


# ---- 10. the host-pointer call ----------------------------------------------------------------------------------------------------
def test_the_host_pointer_call_equals_the_device_call(gpu):  # noqa: F811
    fx, x = _fixture()
    x = x[:300]
    blob, offs = codec.encode_i32(x)
    want_counts, want_first = _fixture_arrays(fx, 300)
    assert want_counts.any()
    counts, first, lossy = codec.verify_i32(blob, offs, 2, x)
    assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first) and lossy == int((want_counts != 0).sum())
    c2, f2, st = _Device(gpu, 300, 2, 2048).verify(blob, offs, x)
    assert np.array_equal(c2, counts) and np.array_equal(f2, first) and int(st[2]) == lossy
    # ragged frames, with and without lengths
    for label, chans in gc.ragged_cases():
        ch, lens = len(chans), [len(c) for c in chans]
        stride = max(lens)
        b = codec.encode_ragged(chans)
        o = np.array([0, len(b)], np.uint64)
        orig = np.zeros((1, ch, stride), np.int32)
        for c, v in enumerate(chans):
            orig[0, c, : len(v)] = v
        orig[0, ch - 1, lens[ch - 1] - 1] ^= 2
        for lengths in (np.array([lens], np.uint32), None):
            want = _Device(gpu, 1, ch, stride).verify(b, o, orig, lengths)
            got = codec.verify_i32(_bytes(b), o, ch, orig, lengths)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == int(want[2][2]) == 1, (label, lengths is None)
    # a malformed stream: sela_hip_decode_i32's code
    bad = blob.copy()
    bad[int(offs[3])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as e:
        codec.verify_i32(bad, offs, 2, x)
    with pytest.raises(capi.SelaHipError) as d:
        codec.decode_i32(bad, offs, 2, 2048)
    assert e.value.code == d.value.code == -5
    with pytest.raises(capi.SelaHipError) as e:  # a stride below the stream's largest length
        codec.verify_i32(blob, offs, 2, x[:, :, :2047])
    assert e.value.code == -4
    assert codec.verify_i32(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2, np.zeros((0, 2, 2048), np.int32))[2] == 0


def test_the_host_pointer_call_leaves_an_open_job_alone(gpu):  # noqa: F811
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
    held = np.ascontiguousarray(pcm.transpose(0, 2, 1)).astype(np.int32)
    held[4, 1, 33] += 1
    counts, first, lossy = codec.verify_i32(frames, offs, 2, held)
    assert lossy == 1 and int(counts[4]) == 1 and int(first[4]) == 2048 + 33 and int(counts.sum()) == 1
    o = np.ascontiguousarray(offs[5:] - offs[5])
    capi.check(lib.sela_hip_decode_feed(job, frames[int(offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12 and np.array_equal(back, pcm.reshape(-1))
