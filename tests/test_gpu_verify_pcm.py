"""sela_hip_verify_pcm_device, sela_hip_verify_payload_pcm_device and sela_hip_verify_pcm: a 24- or 32-bit stream
held against the packed interleaved PCM it was made from, frame by frame, on the device.  With so the stream's sample offsets,
n_f = so[f + 1] - so[f], L_f = min(n_f, max(pcm_samples - so[f], 0)) and m_c the count sela_hip_decode_i32_device reports for
(f, c): diff_counts[f] is the sum over the channels of the values below min(m_c, L_f) that differ plus |m_c - L_f|, first_diff[f]
the smallest i * channels + c (or 0xFFFFFFFF), status[2] the number of frames with a difference; status[0] and [1] are the decode
call's.  The expectation is always one of two things: the fixture tests/golden/verify_wide.json (made from the unmodified
reference), or _expect(Decoder32's output and counts, the unpacked original) computed here in numpy by those definitions --
never the call under test."""
import ctypes as C

import numpy as np
import pytest

import generic_cases as gc
import topology_cases as tc
from gpu_common import _build_frame, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from test_gpu_pcm import GUARD as PCM_GUARD
from test_gpu_pcm import LENGTHS, Guarded, pack_interleaved
from test_gpu_verify_i32_device import NO_DIFF, _bytes, _decode32, _fallback_layouts, _fixture, _layout_blob, _on_device, _status_cases, _stream

pytestmark = pytest.mark.gpu

GUARD = 64          # words in front of and behind each output array that no call may write
SENTINEL = 0x5E1A5E1A
SUBSET = list(range(185, 190)) + list(range(640, 645)) + list(range(904, 909)) + list(range(937, 942))
# frame -> (count, first): the counts are the fixture's (the unmodified reference), the firsts the interleaved order of the same differences
LOSSY = {187: (9, 3), 642: (27, 2), 906: (56, 3), 939: (1, 3)}


def _unpack(raw, ch, b):
    """packed bytes -> int32 [samples, ch], sign-extended"""
    n = len(raw) // (ch * b)
    v = np.asarray(raw[: n * ch * b], np.uint8).reshape(n, ch, b).astype(np.uint32)
    x = sum(v[..., k] << np.uint32(8 * k) for k in range(b)).astype(np.uint32)
    if b == 3:
        x = (x ^ np.uint32(0x800000)) - np.uint32(0x800000)
    return x.astype(np.uint32).view(np.int32)


def _pack(x, b):
    """int32 [frames, ch, n] (planar) -> the packed interleaved bytes, frames back to back"""
    return pack_interleaved(np.ascontiguousarray(np.asarray(x, np.int32).transpose(0, 2, 1)), b)


def _expect(dec, m, so, raw, pcm_samples, ch, b):
    """The definitions of include/sela_hip.h, in numpy -> (diff_counts uint32 [n], first_diff uint32 [n])."""
    n = m.shape[0]
    org = _unpack(raw, ch, b)
    assert pcm_samples <= len(org)
    out_c, out_f = np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32)
    for f in range(n):
        s0, n_f = int(so[f]), int(so[f + 1]) - int(so[f])
        L = min(n_f, max(pcm_samples - s0, 0))
        total, first = 0, NO_DIFF
        for c in range(ch):
            mc = int(m[f, c])
            k = min(mc, L)
            d = np.flatnonzero(dec[f, c, :k] != org[s0: s0 + k, c])
            total += len(d) + abs(mc - L)
            i = int(d[0]) if len(d) else (k if mc != L else None)
            if i is not None:
                first = min(first, i * ch + c)
        out_c[f], out_f[f] = total, first
    return out_c, out_f


class _Device:
    """Buffers of one sela_hip_verify_pcm_device call, the raw C ABI: guard words around both output arrays, the original an
    exact-size view with 0xA5 guard bytes around it."""

    def __init__(self, torch, n, ch, stride, b):
        self.torch, self.n, self.ch, self.stride, self.b = torch, n, ch, stride, b
        self.counts = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.first = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.sample_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_verify_pcm_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")
        self.ws.fill_(0xA5)  # (no initialisation is needed: whatever lies there)

    def verify(self, blob, offs, raw, pcm_samples, with_offsets=True):
        torch = self.torch
        frames, o = _on_device(torch, blob, offs)
        nbytes = pcm_samples * self.ch * self.b
        pcm = Guarded(torch, nbytes, np.asarray(raw[:nbytes], np.uint8) if nbytes else None)
        before = frames.clone(), pcm.big.clone()
        capi.check(capi.lib().sela_hip_verify_pcm_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, pcm.big.data_ptr() + PCM_GUARD, self.b, pcm_samples,
            self.counts.data_ptr() + 4 * GUARD, self.first.data_ptr() + 4 * GUARD, self.sample_offsets.data_ptr() if with_offsets else None,
            self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(frames, before[0]), "d_frames was written"
        assert torch.equal(pcm.big, before[1]) and pcm.intact(), "d_pcm or its guard bytes were written"
        return self.results()

    def results(self):
        n = self.n
        c = self.counts.cpu().numpy().view(np.uint32)
        f = self.first.cpu().numpy().view(np.uint32)
        for a in (c, f):
            assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + n:] == SENTINEL).all(), "written outside the per-frame arrays"
        return c[GUARD: GUARD + n].copy(), f[GUARD: GUARD + n].copy(), self.status.cpu().numpy().view(np.uint32).copy()

    def fallback_frames(self):
        return int(capi.lib().sela_hip_debug_verify_pcm_fallback_frames(self.ws.data_ptr(), self.n, self.ch, self.stride))


def _against_decode(torch, blob, offs, ch, stride, b, raw, pcm_samples=None, fallback=None, label=""):
    """The verify call == _expect(Decoder32's output, the unpacked original) -> (counts, first, status, decoded counts)."""
    n = len(offs) - 1
    raw = np.asarray(raw, np.uint8)
    if pcm_samples is None:
        pcm_samples = len(raw) // (ch * b)
    dec, m, dst = _decode32(torch, blob, offs, ch, stride)
    so, _ = codec.index_samples(_bytes(blob), offs, ch)
    dev = _Device(torch, n, ch, stride, b)
    counts, first, st = dev.verify(blob, offs, raw, pcm_samples)
    assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), 0), (label, st, dst)
    if codec.decode_status_error(dst) == 0:
        want_counts, want_first = _expect(dec, m, so, raw, pcm_samples, ch, b)
        print(label, "counts", counts[:8].tolist(), "want", want_counts[:8].tolist(), "first", first[:8].tolist(), "want", want_first[:8].tolist())
        assert np.array_equal(counts, want_counts), (label, np.flatnonzero(counts != want_counts)[:8], counts[:8], want_counts[:8])
        assert np.array_equal(first, want_first), (label, np.flatnonzero(first != want_first)[:8], first[:8], want_first[:8])
        assert int(st[2]) == int((want_counts != 0).sum()), (label, st)
        assert np.array_equal(dev.sample_offsets.cpu().numpy().view(np.uint64), so), label
    if fallback is not None:
        assert dev.fallback_frames() == fallback, (label, dev.fallback_frames(), fallback)
    return counts, first, st, m


# ---- 1. the reference's own lossy frames of 24-bit audio ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_subset():
    fx, x = _fixture()
    assert {e["frame"]: e["count"] for e in fx["lossy"]} == {f: c for f, (c, _) in LOSSY.items()}, "the counts are the fixture's"
    return np.ascontiguousarray(x[SUBSET])


def _subset_arrays():
    counts, first = np.zeros(len(SUBSET), np.uint32), np.full(len(SUBSET), NO_DIFF, np.uint32)
    for f, (c, i) in LOSSY.items():
        counts[SUBSET.index(f)], first[SUBSET.index(f)] = c, i
    return counts, first


@pytest.mark.parametrize("lossless", [False, True])
def test_the_references_own_lossy_wide_frames_are_found_exactly(gpu, wide_subset, lossless):  # noqa: F811
    torch = gpu
    x, n = wide_subset, len(SUBSET)
    want_counts, want_first = _subset_arrays()
    if lossless:
        want_counts, want_first = np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32)
    lossy = int((want_counts != 0).sum())
    raw = _pack(x, 3)
    d_pcm = torch.from_numpy(raw).cuda()
    enc = codec.EncoderPcm(n, 2, 2048, 3, lossless=lossless)
    frames, offsets, _ = enc.encode(d_pcm)
    enc.check()
    ver = codec.VerifierPcm(n, 2, 2048, 3)
    counts, first = ver.verify(frames, offsets, n, d_pcm)
    ver.check()
    counts, first = counts.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32)
    print("lossy frames found:", [(SUBSET[f], int(counts[f]), int(first[f])) for f in np.flatnonzero(counts)])
    assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first)
    assert ver.lossy_frames() == lossy and ver.status.cpu().numpy().tolist() == [0, 0, lossy, 0]
    assert ver.fallback_frames() == 0
    # ... through the payload call (the stream's bytes alone)
    ver.diff_counts.fill_(-7), ver.first_diff.fill_(-7)
    c2, f2, count = ver.verify_payload(frames[: enc.needed_bytes()], d_pcm)
    ver.check()
    assert int(count.item()) == n and ver.lossy_frames() == lossy
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), want_counts) and np.array_equal(f2.cpu().numpy().view(np.uint32), want_first)
    # ... through the raw call with guards, against Decoder32 and numpy
    blob, offs = enc.to_host()
    c3, f3, st, _ = _against_decode(torch, blob, offs, 2, 2048, 3, raw, fallback=0, label=("fixture", lossless))
    assert np.array_equal(c3, want_counts) and np.array_equal(f3, want_first) and st.tolist() == [0, 0, lossy, 0]
    # ... and through the host call
    c4, f4, l4 = codec.verify_pcm_host(blob, offs, 2, 3, raw)
    assert np.array_equal(c4, want_counts) and np.array_equal(f4, want_first) and l4 == lossy


# ---- 2. planted differences in a lossless stream ----------------------------------------------------------------------------------
def _music(rng, frames, ch, n, bits):
    return np.stack([np.stack([_signal(rng, ("tone", "noise", "sparse")[(c + f) % 3], n, bits - c % 5) for c in range(ch)]) for f in range(frames)]).astype(np.int32)


def _exact_stream(x):
    """A stream that decodes to x (int32 [frames, ch, n]) exactly: the lossless encoder's or, where a frame is no longer than the
    predictor order the encoder would take (it refuses those: ERANGE) or wide noise codes to more than the host call's bound
    (ECAPACITY), subframes of order 0 assembled by hand."""
    try:
        return codec.encode_i32(x, lossless=True)
    except capi.SelaHipError as e:
        if e.code not in (-6, -4):
            raise
    return _stream([_build_frame([(c, 0, c, np.zeros(0, np.int32), frame[c]) for c in range(x.shape[1])]) for frame in x])


def _planted(torch, ch, n, b, frames, spots, label):
    """spots: (frame, channel, sample, bit) of the original to flip -> checked against numpy and against the spots themselves"""
    rng = np.random.default_rng(1000 * ch + n)
    x = _music(rng, frames, ch, n, 22)
    blob, offs = _exact_stream(x)
    raw = _pack(x, b)
    counts, first, st, _ = _against_decode(torch, blob, offs, ch, n, b, raw, fallback=0, label=(label, "exact"))
    assert not counts.any() and (first == NO_DIFF).all() and st.tolist() == [0, 0, 0, 0], label
    changed = raw.copy()
    want_counts, want_first = np.zeros(frames, np.uint32), np.full(frames, NO_DIFF, np.uint32)
    for f, c, i, bit in spots:
        changed[((f * n + i) * ch + c) * b + bit // 8] ^= 1 << (bit % 8)
        want_counts[f] += 1
        want_first[f] = min(int(want_first[f]), i * ch + c)
    counts, first, st, _ = _against_decode(torch, blob, offs, ch, n, b, changed, fallback=0, label=(label, "planted"))
    assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first), (label, counts, first)
    assert st.tolist() == [0, 0, int((want_counts != 0).sum()), 0]


@pytest.mark.parametrize("b", [3, 4])
def test_planted_differences_are_found_where_they_are(gpu, b):  # noqa: F811
    top = 8 * b - 1  # the sign bit: a flip in the sign byte only
    n = 4100  # stereo: tiles of 2048 samples
    for label, spots in {
        "the first value": [(0, 0, 0, 0)],
        "the last value": [(1, 1, n - 1, 5)],
        "before a tile boundary": [(0, 1, 2047, 9)],
        "behind a tile boundary": [(0, 0, 2048, 1)],
        "both sides of it, both channels": [(1, 0, 2047, 3), (1, 1, 2047, 3), (1, 0, 2048, 3), (1, 1, 2048, 3)],
        "the second boundary": [(0, 1, 4095, 0), (0, 1, 4096, 0)],
        "the sign byte only": [(0, 1, 17, top), (1, 0, 2048, top)],
        "every frame": [(0, 1, 33, 2), (1, 0, 4099, 7)],
    }.items():
        _planted(gpu, 2, n, b, 2, spots, (b, "stereo", label))
    n = 40  # 255 channels: tiles of 16 samples
    for label, spots in {
        "the first and the last value": [(0, 0, 0, 0), (0, 254, n - 1, 4)],
        "both sides of a tile boundary": [(0, 7, 15, 1), (0, 3, 16, 1)],
        "the second boundary, the last channel": [(0, 254, 31, 6), (0, 254, 32, 6)],
        "the sign byte only": [(0, 128, 16, top)],
    }.items():
        _planted(gpu, 255, n, b, 1, spots, (b, "255 channels", label))


# ---- 3. a 3-byte container that cannot hold the stream ------------------------------------------------------------------------------
def test_samples_beyond_24_bits_never_equal_their_low_bytes(gpu):  # noqa: F811
    rng = np.random.default_rng(25)
    n = 2500
    x = _music(rng, 2, 2, n, 24)  # (amplitudes up to 2^24 - 1: 25-bit samples)
    wide = (x < -(1 << 23)) | (x >= (1 << 23))
    assert wide.any() and not wide.all()
    blob, offs = codec.encode_i32(x, lossless=True)
    dec, m, dst = _decode32(gpu, blob, offs, 2, n)
    assert codec.decode_status_error(dst) == 0 and np.array_equal(dec, x)
    raw = _pack(x, 3)  # (the low three bytes of every sample)
    counts, first, st, _ = _against_decode(gpu, blob, offs, 2, n, 3, raw, fallback=0, label="25-bit in 3 bytes")
    assert counts.tolist() == [int(wide[f].sum()) for f in range(2)] and int(st[2]) == 2
    inter = wide.transpose(0, 2, 1).reshape(2, -1)
    assert first.tolist() == [int(np.flatnonzero(inter[f])[0]) for f in range(2)]
    # the same stream in a 4-byte container: nothing differs
    counts, first, st, _ = _against_decode(gpu, blob, offs, 2, n, 4, _pack(x, 4), fallback=0, label="25-bit in 4 bytes")
    assert not counts.any() and st.tolist() == [0, 0, 0, 0]


# ---- 4. shapes --------------------------------------------------------------------------------------------------------------------
def _shape_case(torch, ch, n, frames, b):
    rng = np.random.default_rng(ch * 100000 + n * 10 + frames)
    x = _music(rng, frames, ch, n, 22 if b == 3 else 27)
    blob, offs = _exact_stream(x)
    raw = _pack(x, b)
    label = (b, ch, n, frames)
    _against_decode(torch, blob, offs, ch, n, b, raw, fallback=0, label=label)
    # the decoder's own output with one value changed at each end of every frame
    dec, m, dst = _decode32(torch, blob, offs, ch, n)
    changed = _pack(dec, b)
    for f in range(frames):
        changed[f * n * ch * b] ^= 1
        changed[(f + 1) * n * ch * b - 1] ^= 0x40
    counts, first, st, _ = _against_decode(torch, blob, offs, ch, n, b, changed, fallback=0, label=label + ("planted",))
    both = 1 if n * ch == 1 else 2
    assert counts.tolist() == [both] * frames and first.tolist() == [0] * frames and int(st[2]) == frames, label


@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("ch", [1, 2, 3, 5, 8])
def test_shapes(gpu, ch, b):  # noqa: F811
    for n in LENGTHS:
        for frames in (1, 3):
            _shape_case(gpu, ch, n, frames, b)


@pytest.mark.parametrize("b", [3, 4])
def test_shapes_of_255_channels(gpu, b):  # noqa: F811
    for n in (15, 16, 17, 33):
        for frames in (1, 3):
            _shape_case(gpu, 255, n, frames, b)


# ---- 5. and 6. frames of different lengths; pcm_samples -----------------------------------------------------------------------------
MIXED = [2048, 2048, 2048 + 777, 128]


def _mixed_stream(ch):
    rng = np.random.default_rng(777)
    xs = [_music(rng, 1, ch, n, 22) for n in MIXED]
    blobs = [_exact_stream(x)[0].tobytes() for x in xs]
    return _stream(blobs) + (xs,)


@pytest.mark.parametrize("b", [3, 4])
def test_a_stream_of_frames_of_different_lengths(gpu, b):  # noqa: F811
    stream, offs, xs = _mixed_stream(2)
    raw = np.concatenate([_pack(x, b) for x in xs])
    so, largest = codec.index_samples(stream, offs, 2)
    assert so.tolist() == np.cumsum([0] + MIXED).tolist() and largest == max(MIXED)
    counts, first, st, m = _against_decode(gpu, stream, offs, 2, max(MIXED), b, raw, fallback=0, label=("mixed", b))
    assert not counts.any() and st.tolist() == [0, 0, 0, 0] and m.tolist() == [[k, k] for k in MIXED]
    changed = raw.copy()
    spots = [(2, 1, 2048 + 776), (2, 0, 2048), (3, 1, 0), (3, 0, 127), (1, 1, 2047)]
    for f, c, i in spots:
        changed[((int(so[f]) + i) * 2 + c) * b] ^= 0x10
    counts, first, st, _ = _against_decode(gpu, stream, offs, 2, max(MIXED), b, changed, fallback=0, label=("mixed, planted", b))
    assert counts.tolist() == [0, 1, 2, 2] and first.tolist() == [NO_DIFF, 2047 * 2 + 1, 2048 * 2, 1] and int(st[2]) == 3
    # a roomy stride, and one that is no multiple of four (the decoded side sample by sample)
    for stride in (max(MIXED) + 3, 4096, max(MIXED) + 1):
        counts, _, _, _ = _against_decode(gpu, stream, offs, 2, stride, b, changed, fallback=0, label=("mixed", b, stride))
        assert counts.tolist() == [0, 1, 2, 2]
    # the host call: chunks of whole frames, whatever their lengths
    c, f, lossy = codec.verify_pcm_host(stream, offs, 2, b, changed)
    assert c.tolist() == [0, 1, 2, 2] and f.tolist() == [NO_DIFF, 2047 * 2 + 1, 2048 * 2, 1] and lossy == 3


@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("ch", [2, 3])
def test_pcm_samples(gpu, ch, b):  # noqa: F811
    stream, offs, xs = _mixed_stream(ch)
    raw = np.concatenate([_pack(x, b) for x in xs])
    total = sum(MIXED)
    for label, held, want in [
        ("exact", total, [0, 0, 0, 0]),
        ("one short", total - 1, [0, 0, 0, ch]),
        ("inside a middle frame", 2048 + 1000, [0, 1048 * ch, MIXED[2] * ch, 128 * ch]),
        ("at a frame's start", 4096, [0, 0, MIXED[2] * ch, 128 * ch]),
        ("nothing", 0, [k * ch for k in MIXED]),
    ]:
        counts, first, st, _ = _against_decode(gpu, stream, offs, ch, max(MIXED), b, raw, pcm_samples=held, fallback=0, label=(label, ch, b))
        assert counts.tolist() == want, (label, counts)
        so = np.cumsum([0] + MIXED)
        assert first.tolist() == [NO_DIFF if not w else max(min(held - int(so[f]), MIXED[f]), 0) * ch for f, w in enumerate(want)], (label, first)
        c, f, lossy = codec.verify_pcm_host(stream, offs, ch, b, raw, pcm_samples=held)
        assert c.tolist() == want and np.array_equal(f, first) and lossy == int(st[2]), label


# ---- 7. subframe layouts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [2, 3, 5, 8])
def test_every_accepted_layout_takes_the_direct_kernel(gpu, ch):  # noqa: F811
    o = oracle()
    blobs = [_layout_blob(o, layout, 100 * ch + k) for k, (_, layout) in enumerate(tc.ACCEPTED_LAYOUTS[ch])]
    stream, offs = _stream(blobs)
    n = len(blobs)
    dec, m, dst = _decode32(gpu, stream, offs, ch, tc.N)
    assert codec.decode_status_error(dst) == 0 and (m == tc.N).all()
    for b in (3, 4):
        raw = _pack(dec, b)
        counts, _, st, _ = _against_decode(gpu, stream, offs, ch, tc.N, b, raw, fallback=0, label=(ch, b, "exact"))
        assert not counts.any() and st.tolist() == [0, 0, 0, 0]
        changed = raw.copy()
        for f in range(n):
            for c in range(ch):
                changed[((f * tc.N + (37 * f + 501 * c) % tc.N) * ch + c) * b + 1] ^= 0x08
        counts, _, _, _ = _against_decode(gpu, stream, offs, ch, tc.N, b, changed, fallback=0, label=(ch, b, "planted"))
        assert counts.tolist() == [ch] * n
        _against_decode(gpu, stream, offs, ch, tc.N + 3, b, changed, fallback=0, label=(ch, b, "an odd stride"))


@pytest.mark.parametrize("ch", [2, 3, 5])
def test_other_layouts_take_the_fallback(gpu, ch):  # noqa: F811
    o = oracle()
    good = [_layout_blob(o, layout, 7 * ch + k) for k, (_, layout) in enumerate(tc.ACCEPTED_LAYOUTS[ch][:2])]
    others = [(name, _layout_blob(o, layout, 900 + 10 * ch + k)) for k, (name, layout) in enumerate(_fallback_layouts(ch))]
    assert {name for name, _ in others} >= {"channel 0 twice, channel 1 never", "type 2"} and (ch != 3 or len(others) == 3)
    blobs = [good[0]] + [b for _, b in others[:1]] + [good[1]] + [b for _, b in others[1:]] + [good[0]]
    stream, offs = _stream(blobs)
    n = len(blobs)
    dec, m, dst = _decode32(gpu, stream, offs, ch, tc.N)
    for b in (3, 4):
        for name, blob in others:  # each alone: which way it went
            o1 = np.array([0, len(blob)], np.uint64)
            d1, _, _ = _decode32(gpu, blob, o1, ch, tc.N)
            _against_decode(gpu, blob, o1, ch, tc.N, b, _pack(d1, b), fallback=1, label=(ch, b, name))
        # direct and fallback frames in one stream: the missing channel's samples are all differences
        raw = _pack(dec, b)
        counts, first, st, m2 = _against_decode(gpu, stream, offs, ch, tc.N, b, raw, fallback=len(others), label=(ch, b, "mixed"))
        assert int(counts[0]) == 0 and int(counts[2]) == 0 and int(counts[n - 1]) == 0
        assert int(m2[1, 1]) == 0 and int(counts[1]) == tc.N and int(first[1]) == 1  # (channel 1 never named: |0 - 2048|, found at sample 0)
        changed = raw.copy()
        for f in range(n):
            for c in range(ch):
                if m[f, c]:
                    changed[((f * tc.N + (5 * f + 300 * c) % tc.N) * ch + c) * b] ^= 0x01
        _against_decode(gpu, stream, offs, ch, tc.N, b, changed, fallback=len(others), label=(ch, b, "mixed, planted"))
        _against_decode(gpu, stream, offs, ch, tc.N + 2, b, changed, fallback=len(others), label=(ch, b, "mixed, an odd stride"))


def test_channels_that_disagree_about_the_length(gpu):  # noqa: F811
    for label, chans in gc.ragged_cases():
        ch, lens = len(chans), [len(c) for c in chans]
        stride = max(lens)
        blob = _bytes(codec.encode_ragged(chans, lossless=True))
        offs = np.array([0, len(blob)], np.uint64)
        so, _ = codec.index_samples(blob, offs, ch)
        n_f = int(so[1])  # (the frame's first subframe says how long the frame is)
        dec, m, dst = _decode32(gpu, blob, offs, ch, stride)
        assert codec.decode_status_error(dst) == 0 and m[0].tolist() == lens, label
        for b in (3, 4):
            raw = _pack(dec[:, :, :n_f], b)
            counts, first, st, _ = _against_decode(gpu, blob, offs, ch, stride, b, raw, fallback=0, label=(label, b))
            assert counts.tolist() == [sum(abs(k - n_f) for k in lens)], (label, counts, lens, n_f)
            where = [min(k, n_f) * ch + c for c, k in enumerate(lens) if k != n_f]
            assert first.tolist() == [min(where, default=NO_DIFF)], (label, first)


# ---- 8. status words --------------------------------------------------------------------------------------------------------------
def test_status_words_are_the_decode_calls(gpu):  # noqa: F811
    lib = capi.lib()
    seen = set()
    for label, blob, offs, ch, stride in _status_cases():
        n = len(offs) - 1
        _, _, dst = _decode32(gpu, blob, offs, ch, stride)
        for b in (3, 4):
            raw = np.zeros(n * stride * ch * b, np.uint8)
            counts, first, st = _Device(gpu, n, ch, stride, b).verify(blob, offs, raw, n * stride)
            assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), 0), (label, st, dst)
            if label == "stride too small":
                assert int(st[0]) & capi.FLAG_STRIDE and int(st[2]) == 0 and not counts.any() and (first == NO_DIFF).all(), "nothing is compared"
        status = st.copy()
        status[2] = 0
        rc = codec.decode_status_error(dst)
        assert codec.decode_status_error(status) == rc, (label, st, dst)
        seen.add(rc)
        if label != "stride too small":  # (the host call takes the stream's own largest frame for its stride)
            fr, o = _bytes(blob), np.ascontiguousarray(offs, np.uint64)
            c, f = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            assert lib.sela_hip_verify_pcm(fr.ctypes.data, o.ctypes.data, n, ch, 3, raw.ctypes.data, n * stride, c.ctypes.data, f.ctypes.data, None) == rc, label
    assert seen == {0, -4, -5}, seen


def test_no_frames_no_offsets_and_the_payload_calls_tail(gpu):  # noqa: F811
    torch = gpu
    dev = _Device(torch, 0, 2, 2048, 3)
    counts, first, st = dev.verify(b"", np.zeros(1, np.uint64), np.zeros(0, np.uint8), 0)
    assert (st == 0).all() and len(counts) == 0 and int(dev.sample_offsets[0].item()) == 0
    # without d_sample_offsets: the workspace's copy
    rng = np.random.default_rng(12)
    x = _music(rng, 4, 2, 900, 20)
    blob, offs = codec.encode_i32(x, lossless=True)
    raw = _pack(x, 3)
    raw[((1 * 900 + 899) * 2 + 1) * 3] ^= 1
    raw[((3 * 900 + 5) * 2 + 0) * 3 + 2] ^= 0x80
    dev = _Device(torch, 4, 2, 900, 3)
    counts, first, st = dev.verify(blob, offs, raw, 3600, with_offsets=False)
    assert (dev.sample_offsets.cpu().numpy() == -1).all()
    assert counts.tolist() == [0, 1, 0, 1] and first.tolist() == [NO_DIFF, 1799, NO_DIFF, 10] and st.tolist() == [0, 0, 2, 0]
    # the payload call with room for more frames than the stream has: entries from the count on are not written
    ver = codec.VerifierPcm(7, 2, 900, 3)
    ver.diff_counts.fill_(-7), ver.first_diff.fill_(-7)
    c, f, count = ver.verify_payload(torch.from_numpy(blob).cuda(), torch.from_numpy(raw).cuda())
    ver.check()
    assert int(count.item()) == 4 and ver.lossy_frames() == 2
    assert c.cpu().numpy().tolist() == [0, 1, 0, 1, -7, -7, -7] and f.cpu().numpy().tolist() == [-1, 1799, -1, 10, -7, -7, -7]


# ---- 9. capture; the host-pointer call --------------------------------------------------------------------------------------------
def test_encode_and_verify_in_one_graph(gpu):  # noqa: F811
    torch = gpu
    n, spc, b = 12, 3000, 3
    rng = np.random.default_rng(9)
    x = _music(rng, n, 2, spc, 22)
    raw = _pack(x, b)
    d_pcm = torch.from_numpy(raw).cuda()       # what is encoded
    d_held = torch.from_numpy(raw).cuda()      # what the stream is held against: changed in place between the replays
    enc = codec.EncoderPcm(n, 2, spc, b, lossless=True)
    ver = codec.VerifierPcm(n, 2, spc, b)

    def call():
        frames, offsets, _ = enc.encode(d_pcm)
        return ver.verify(frames, offsets, n, d_held)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for spots in ([], [(0, 0, 3), (5, 1, 9), (11, 1, 2999)], [(2, 0, 0), (7, 0, 2048)], []):
        held = raw.copy()
        for f, c, i in spots:
            held[((f * spc + i) * 2 + c) * b + 1] ^= 0x20
        d_held.copy_(torch.from_numpy(held))
        ver.diff_counts.fill_(-7), ver.first_diff.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        enc.check(), ver.check()
        want_counts, want_first = np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32)
        for f, c, i in spots:
            want_counts[f], want_first[f] = 1, i * 2 + c
        assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want_counts), spots
        assert np.array_equal(out[1].cpu().numpy().view(np.uint32), want_first), spots
        assert ver.status.cpu().numpy().tolist() == [0, 0, len(spots), 0]


def test_the_host_pointer_call_equals_the_device_call(gpu, wide_subset):  # noqa: F811
    x = wide_subset
    blob, offs = codec.encode_i32(x)
    want_counts, want_first = _subset_arrays()
    for b in (3, 4):
        raw = _pack(x, b)
        counts, first, lossy = codec.verify_pcm_host(blob, offs, 2, b, raw)
        assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first) and lossy == len(LOSSY)
        c2, f2, st = _Device(gpu, len(SUBSET), 2, 2048, b).verify(blob, offs, raw, len(SUBSET) * 2048)
        assert np.array_equal(c2, counts) and np.array_equal(f2, first) and int(st[2]) == lossy
        # an original that is nowhere aligned on the host
        room = np.zeros(len(raw) + 8, np.uint8)
        for shift in (1, 2, 3):
            room[shift: shift + len(raw)] = raw
            c3, f3, l3 = codec.verify_pcm_host(blob, offs, 2, b, room[shift: shift + len(raw)])
            assert np.array_equal(c3, counts) and np.array_equal(f3, first) and l3 == lossy
    # small chunks: every chunk's packed bytes are staged from its own first frame, and pcm_samples ends inside a later chunk
    lib = capi.lib()
    raw = _pack(x, 3)
    for chunk in (1, 3, 7):
        lib.sela_hip_debug_pcm_chunk_frames(chunk)
        try:
            c5, f5, l5 = codec.verify_pcm_host(blob, offs, 2, 3, raw)
            c6, f6, l6 = codec.verify_pcm_host(blob, offs, 2, 3, raw, pcm_samples=8 * 2048 + 5)
        finally:
            lib.sela_hip_debug_pcm_chunk_frames(0)
        assert np.array_equal(c5, want_counts) and np.array_equal(f5, want_first) and l5 == len(LOSSY), chunk
        # (frame 8 of the subset is not lossy: 5 of its samples are held, the rest and every later frame are missing)
        assert SUBSET[8] not in LOSSY
        assert np.array_equal(c6[:8], want_counts[:8]) and np.array_equal(f6[:8], want_first[:8]), chunk
        assert c6[8:].tolist() == [2043 * 2] + [4096] * (len(SUBSET) - 9) and f6[8:].tolist() == [10] + [0] * (len(SUBSET) - 9), chunk
        assert l6 == int((want_counts[:8] != 0).sum()) + len(SUBSET) - 8, chunk
    # a malformed stream: sela_hip_decode_i32's code
    bad = blob.copy()
    bad[int(offs[3])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as e:
        codec.verify_pcm_host(bad, offs, 2, 3, _pack(x, 3))
    with pytest.raises(capi.SelaHipError) as d:
        codec.decode_i32(bad, offs, 2, 2048)
    assert e.value.code == d.value.code == -5
    assert codec.verify_pcm_host(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2, 3, np.zeros(0, np.uint8))[2] == 0


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
    held = pack_interleaved(pcm.astype(np.int32), 3)
    held[((4 * 2048 + 33) * 2 + 1) * 3] ^= 1
    counts, first, lossy = codec.verify_pcm_host(frames, offs, 2, 3, held)
    assert lossy == 1 and int(counts[4]) == 1 and int(first[4]) == 33 * 2 + 1 and int(counts.sum()) == 1
    o = np.ascontiguousarray(offs[5:] - offs[5])
    capi.check(lib.sela_hip_decode_feed(job, frames[int(offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12 and np.array_equal(back, pcm.reshape(-1))
