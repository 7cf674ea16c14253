"""sela_hip_levels_i32_device, sela_hip_levels_payload_i32_device, sela_hip_levels_samples_i32_device and sela_hip_levels_i32
(DESIGN.md 5.27): per frame and channel the peak, the sample count, the sum and the 128-bit sum of squares of the int32 samples
sela_hip_decode_i32_device writes.  The expectation is always numpy over that call's samples_out[f][c][:counts] for the same stream
and stride (the energy in Python's integers), and every comparison is exact equality of all five fields.  status[0], [1] and [3]
are the decode call's; status[2] counts the frames that are not digital silence."""
import os

import numpy as np
import pytest

import generic_cases as gc
import topology_cases as tc
import wide_cases as wc
from gpu_common import _build_frame, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from test_gpu_pcm_cli import _samples
from test_gpu_verify_i32_device import _bytes, _decode32, _fallback_layouts, _layout_blob, _on_device, _stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16              # records behind d_levels that no call may write
SENTINEL = 0x5E1A5E1A5E1A5E1A
WORDS = 4               # 8-byte words of a record
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def _record(v):
    """one channel's samples -> (peak, samples, sum, energy) in Python's integers"""
    v = np.asarray(v, np.int32).astype(np.int64)
    a = np.abs(v).astype(np.uint64)
    sq = a * a  # (|v| <= 2^31: a square is at most 2^62)
    energy = int((sq & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64)) + (int((sq >> np.uint64(32)).sum(dtype=np.uint64)) << 32)
    return (int(a.max()) if len(v) else 0, len(v), int(v.sum()), energy)


def _expect(dec, counts):
    """dec: int32 [n, ch, stride] and counts [n, ch] as sela_hip_decode_i32_device writes them -> LEVEL32_DTYPE [n, ch]."""
    n, ch = counts.shape
    out = np.zeros((n, ch), codec.LEVEL32_DTYPE)
    for f in range(n):
        for c in range(ch):
            peak, samples, total, energy = _record(dec[f, c, : int(counts[f, c])])
            out[f, c] = (peak, samples, total, energy & ((1 << 64) - 1), energy >> 64)
    return out


def _same(got, want, label=""):
    for name in codec.LEVEL32_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (label, name, np.argwhere(got[name] != want[name])[:6].tolist(), got[name].ravel()[:4], want[name].ravel()[:4])


def _loud(rec):
    return int((rec["peak"] != 0).any(1).sum()) if rec.size else 0


class _Device:
    """Buffers of one sela_hip_levels_i32_device call, the raw C ABI: guard records behind d_levels, d_frames kept for a look afterwards."""

    def __init__(self, torch, n, ch, stride):
        self.torch, self.n, self.ch, self.stride = torch, n, ch, stride
        self.levels = torch.full(((n * ch + GUARD) * WORDS,), SENTINEL, dtype=torch.int64, device="cuda")
        self.sample_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_levels_i32_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")
        self.ws.fill_(0xA5)  # (no initialisation is needed: whatever lies there)

    def call(self, frames, o, with_offsets=True):
        torch = self.torch
        assert self.levels.data_ptr() % 8 == 0
        capi.check(capi.lib().sela_hip_levels_i32_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, self.levels.data_ptr(),
            self.sample_offsets.data_ptr() if with_offsets else None, self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream))

    def measure(self, blob, offs, with_offsets=True):
        torch = self.torch
        frames, o = _on_device(torch, blob, offs)
        before = frames.clone()
        self.call(frames, o, with_offsets)
        torch.cuda.synchronize()
        assert torch.equal(frames, before), "d_frames was written"
        return self.results()

    def results(self):
        words = self.levels.cpu().numpy()
        k = self.n * self.ch * WORDS
        assert (words[k:] == np.int64(SENTINEL)).all(), "written past d_levels"
        return words[:k].copy().view(codec.LEVEL32_DTYPE).reshape(self.n, self.ch), self.status.cpu().numpy().view(np.uint32).copy()

    def fallback_frames(self):
        return int(capi.lib().sela_hip_debug_levels_i32_fallback_frames(self.ws.data_ptr(), self.n, self.ch, self.stride))


def _check(torch, blob, offs, ch, stride, fallback=None, label="", clean=True):
    """The records of (stream) == numpy on what the decode call writes; status and sample offsets as that call leaves them
    -> (records, status, decoded samples, counts)."""
    n = len(offs) - 1
    dec, m, dst = _decode32(torch, blob, offs, ch, stride)
    if clean:
        assert codec.decode_status_error(dst) == 0, (label, dst)
    want = _expect(dec, m)
    dev = _Device(torch, n, ch, stride)
    got, st = dev.measure(blob, offs)
    assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (label, st, dst)
    if not int(dst[0]) & capi.FLAG_STRIDE:
        _same(got, want, label)
        assert int(st[2]) == _loud(want), (label, st)
    so = codec.Decoder32(max(n, 1), ch, stride)
    frames, o = _on_device(torch, blob, offs)
    so.decode(frames, o, n)
    torch.cuda.synchronize()
    assert np.array_equal(dev.sample_offsets.cpu().numpy()[: n + 1], so.sample_offsets.cpu().numpy()[: n + 1]), label
    if fallback is not None:
        assert dev.fallback_frames() == fallback, (label, dev.fallback_frames(), fallback)
    return got, st, dec, m


# ---- 1. direct layouts ----------------------------------------------------------------------------------------------------------------
def _wide_frames(ch, n, seed):
    """3 frames of `ch` channels from wide_signals (25 to 31 bits), those an encoder accepts -> (stream, offsets)"""
    pool = [s for name, s in wc.wide_signals(n, seed) if int(np.abs(s.astype(np.int64)).max()) >= 1 << 24]
    taken = []
    for s in pool:  # (a signal no encoder codes -- a residue beyond the zig-zag -- is left out)
        try:
            codec.encode_i32(s[None, None])
            taken.append(s)
        except capi.SelaHipError:
            continue
    assert len(taken) >= 3, len(taken)
    blobs = []
    for f in range(3):
        chans = np.stack([taken[(f + 2 * c) % len(taken)] for c in range(ch)])
        if ch == 2:  # (the stereo difference may wrap: then the second channel is the first one, halved)
            try:
                codec.encode_i32(chans[None])
            except capi.SelaHipError:
                chans[1] = chans[0] >> 1
        blobs.append(codec.encode_i32(chans[None])[0].tobytes())
    return _stream(blobs)


@pytest.mark.parametrize("ch", [1, 2, 3, 8, 9])
def test_direct_layouts_at_a_vector_and_a_scalar_stride(gpu, ch):  # noqa: F811
    x = _samples(ch, 24, 60 + ch)[: 3 * 2048].reshape(3, 2048, ch).transpose(0, 2, 1)
    for label, (blob, offs) in (("24-bit", codec.encode_i32(np.ascontiguousarray(x))), ("25 to 31 bits", _wide_frames(ch, 2048, 9 + ch))):
        got, st, dec, m = _check(gpu, blob, offs, ch, 2048, fallback=0, label=(ch, label, 2048))
        assert (m == 2048).all() and (got["peak"] > 0).all() and int(st[2]) == 3
        print(ch, label, "largest |v| 2^%.1f" % np.log2(float(got["peak"].max())), "largest energy 2^%.1f" % np.log2(float(int(got["sum_squares_lo"].max()) + (int(got["sum_squares_hi"].max()) << 64))))
        if label != "24-bit":
            assert int(got["peak"].max()) >= 1 << 24
        odd, _, _, _ = _check(gpu, blob, offs, ch, 2050, fallback=0, label=(ch, label, 2050))
        _same(odd, got, "both strides give the same records")


# ---- 2. lengths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 63, 64, 65, 777, 4095, 4096, 4097])
def test_lengths_at_every_edge(gpu, n):  # noqa: F811
    rng = np.random.default_rng(n)
    for ch in (1, 2):
        x = np.stack([np.stack([_signal(rng, ("tone", "noise")[c], n, 23 - 3 * c) for c in range(ch)]) for _ in range(2)]).astype(np.int32)
        if n < 100:  # (hand-built, order 0: an encoder's block must be longer than its order)
            blob, offs = _stream([_build_frame([(c, 0, 0, np.zeros(0, np.int32), x[f, c]) for c in range(ch)]) for f in range(2)])
        else:
            blob, offs = codec.encode_i32(x)
        got, _, _, m = _check(gpu, blob, offs, ch, n, fallback=0, label=(n, ch))
        assert (m == n).all() and (got["samples"] == n).all()
        _check(gpu, blob, offs, ch, n + 5, fallback=0, label=(n, ch, "a roomy stride"))


def test_a_65535_sample_mono_frame(gpu):  # noqa: F811
    rng = np.random.default_rng(65535)
    x = _signal(rng, "tone", 65535, 23).astype(np.int32)[None, None]
    blob, offs = codec.encode_i32(x)
    got, _, _, m = _check(gpu, blob, offs, 1, 65535, fallback=0, label="65535")
    assert m.tolist() == [[65535]] and int(got["samples"][0, 0]) == 65535


def test_the_references_own_17_bit_frames(gpu):  # noqa: F811
    z = np.load(os.path.join(ROOT, "tests", "golden", "generic_kats.npz"))
    for name, ch in (("n2049_mono_i17", 1), ("n2049_stereo_diff_i17", 2), ("n1000_three_i17", 3), ("n128_stereo_indep_i17", 2)):
        blob = z[name + "/bytes"].tobytes()
        offs = np.array([0, len(blob)], np.uint64)
        n = int(name[1:].split("_")[0])
        got, _, dec, m = _check(gpu, blob, offs, ch, n, fallback=0, label=name)
        assert (m == n).all() and int(got["peak"].max()) > 32768, (name, got["peak"])


# ---- 3. ragged frames -----------------------------------------------------------------------------------------------------------------
def test_ragged_frames(gpu):  # noqa: F811
    for label, chans in gc.ragged_cases():
        ch, lens = len(chans), [len(c) for c in chans]
        blob = codec.encode_ragged(chans)
        offs = np.array([0, len(blob)], np.uint64)
        for stride in (max(lens), max(lens) + 3):
            got, _, _, m = _check(gpu, blob, offs, ch, stride, fallback=0, label=(label, stride))
            assert m[0].tolist() == lens and got["samples"][0].tolist() == lens, label


# ---- 4. the fallback ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [2, 3, 5])
def test_other_layouts_take_the_fallback(gpu, ch):  # noqa: F811
    o = oracle()
    good = [_layout_blob(o, layout, 7 * ch + k) for k, (_, layout) in enumerate(tc.ACCEPTED_LAYOUTS[ch][:2])]
    others = [(name, _layout_blob(o, layout, 900 + 10 * ch + k)) for k, (name, layout) in enumerate(_fallback_layouts(ch))]
    for name, blob in others:  # each alone
        _check(gpu, blob, np.array([0, len(blob)], np.uint64), ch, tc.N, fallback=1, label=(ch, name), clean=False)
    # direct frames alone leave the fallback idle
    stream, offs = _stream(good)
    _check(gpu, stream, offs, ch, tc.N, fallback=0, label=(ch, "direct alone"))
    # direct and fallback frames in one stream
    blobs = [good[0]] + [b for _, b in others[:1]] + [good[1]] + [b for _, b in others[1:]] + [good[0]]
    stream, offs = _stream(blobs)
    for stride in (tc.N, tc.N + 2):
        got, _, _, m = _check(gpu, stream, offs, ch, stride, fallback=len(others), label=(ch, "mixed", stride), clean=False)
        assert int(m[1, 1]) == 0 and got[1, 1].tolist() == (0, 0, 0, 0, 0)  # (channel 1 never named: an all-zero record)
        assert (got["samples"][[0, 2, len(blobs) - 1]] == tc.N).all()


# ---- 5. faults in the stream ----------------------------------------------------------------------------------------------------------
def test_a_malformed_frame_in_the_middle_and_a_small_stride(gpu):  # noqa: F811
    rng = np.random.default_rng(6)
    x = np.stack([np.stack([_signal(rng, "tone", 700, 23), _signal(rng, "noise", 700, 20)]) for _ in range(4)]).astype(np.int32)
    frames, offs = codec.encode_i32(x)
    bad = frames.copy()
    bad[int(offs[2])] ^= 0xFF
    got, st, _, m = _check(gpu, bad, offs, 2, 700, label="bad sync word", clean=False)
    assert codec.decode_status_error([int(st[0]), int(st[1]), 0, 0]) != 0
    clean, _, _, _ = _check(gpu, frames, offs, 2, 700, fallback=0, label="clean")
    _same(got[[0, 1, 3]], clean[[0, 1, 3]], "the other frames")
    # a stride that is too small: the flag, and nothing past the guards (_Device.results looks)
    _, st, _, _ = _check(gpu, frames, offs, 2, 699, label="stride too small", clean=False)
    assert int(st[0]) & capi.FLAG_STRIDE


# ---- 6. wrap-around -------------------------------------------------------------------------------------------------------------------
def test_a_difference_subframe_at_the_ends_of_int32(gpu):  # noqa: F811
    n = 100
    parent, diff = np.full(n, (1 << 30) - 1, np.int32), np.full(n, -(1 << 30), np.int32)
    blob = _build_frame([(0, 0, 0, np.zeros(0, np.int32), parent), (1, 1, 0, np.zeros(0, np.int32), diff)])
    got, _, dec, m = _check(gpu, blob, np.array([0, len(blob)], np.uint64), 2, n, fallback=0, label="INT32_MAX")
    assert m.tolist() == [[n, n]] and (dec[0, 1, :n] == INT32_MAX).all()
    assert got[0, 1].tolist() == (INT32_MAX, n, n * INT32_MAX, (n * INT32_MAX * INT32_MAX) & ((1 << 64) - 1), (n * INT32_MAX * INT32_MAX) >> 64)
    assert int(got["sum_squares_hi"][0, 1]) > 0
    # ... and a crafted frame whose parent - difference wraps int32 on the decoder's side
    o = oracle()
    subs, _ = wc.stereo_wrap_subframes(o, 600, 4)
    blob = wc.frame_bytes(o, subs)
    for stride in (600, 601):
        _check(gpu, blob, np.array([0, len(blob)], np.uint64), 2, stride, fallback=0, label=("wrap", stride))


# ---- 7. the number range, on samples that already lie in device memory ------------------------------------------------------------------
def _measure_samples(torch, x, counts=None, shift=0):
    """sela_hip_levels_samples_i32_device, the raw C ABI with guard records -> (records, status); shift: d_samples that many
    int32s behind a 16-byte boundary."""
    x = np.ascontiguousarray(x, np.int32)
    n, ch, stride = x.shape
    lib = capi.lib()
    room = torch.zeros(x.size + 8, dtype=torch.int32, device="cuda")
    room[shift: shift + x.size].copy_(torch.from_numpy(x.reshape(-1)))
    before = room.clone()
    cnt = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts, np.uint32).reshape(-1).view(np.int32).copy()).cuda()
    levels = torch.full(((n * ch + GUARD) * WORDS,), SENTINEL, dtype=torch.int64, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sela_hip_levels_samples_i32_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")
    ws.fill_(0xA5)
    capi.check(lib.sela_hip_levels_samples_i32_device(room.data_ptr() + 4 * shift, None if cnt is None else cnt.data_ptr(), n, ch, stride, levels.data_ptr(),
                                                      status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(room, before), "d_samples was written"
    words = levels.cpu().numpy()
    assert (words[n * ch * WORDS:] == np.int64(SENTINEL)).all(), "written past d_levels"
    return words[: n * ch * WORDS].copy().view(codec.LEVEL32_DTYPE).reshape(n, ch), status.cpu().numpy().view(np.uint32).copy()


def _samples_case(torch, x, counts=None, label=""):
    x = np.ascontiguousarray(x, np.int32)
    n, ch, stride = x.shape
    m = np.full((n, ch), stride, np.uint32) if counts is None else np.minimum(np.asarray(counts, np.uint32).reshape(n, ch), stride)
    want = _expect(x, m)
    for shift in (0, 1):  # (rows at 16 bytes: four samples a load; rows behind: one)
        got, st = _measure_samples(torch, x, counts, shift)
        _same(got, want, (label, shift))
        assert st.tolist() == [0, 0, _loud(want), 0], (label, st)
    return want


def test_full_scale_samples_pass_64_bits(gpu):  # noqa: F811
    # 2048 x INT32_MIN: eight per thread, 2^65 in a lane -- a bare 64-bit accumulator wraps to 0
    want = _samples_case(gpu, np.full((1, 1, 2048), INT32_MIN, np.int32), label="2048 x INT32_MIN")
    assert want[0, 0].tolist() == (1 << 31, 2048, -2048 << 31, 0, 2048 << 62 >> 64)
    # 65535 x INT32_MIN: 65535 * 2^62, sixteen slices
    want = _samples_case(gpu, np.full((1, 1, 65535), INT32_MIN, np.int32), label="65535 x INT32_MIN")
    energy = 65535 << 62
    assert want[0, 0].tolist() == (1 << 31, 65535, -65535 << 31, energy & ((1 << 64) - 1), energy >> 64) and energy >> 64 == 16383
    alt = np.where(np.arange(4100) % 2 == 0, INT32_MIN, INT32_MAX).astype(np.int32)
    want = _samples_case(gpu, np.stack([alt, alt[::-1]])[None], label="alternating")
    assert int(want["sum"][0, 0]) == -2050 and int(want["peak"][0, 1]) == 1 << 31


def test_silence_single_samples_and_counts(gpu):  # noqa: F811
    want = _samples_case(gpu, np.zeros((2, 2, 4097), np.int32), label="silence")
    assert _loud(want) == 0 and (want["samples"] == 4097).all()
    n = 8195
    spots = [0, 63, 64, 4095, 4096, n - 1]
    x = np.zeros((len(spots), 2, n), np.int32)
    for f, i in enumerate(spots):
        x[f, f & 1, i] = INT32_MIN if f % 3 == 0 else -(f + 1)
    want = _samples_case(gpu, x, label="single samples")
    assert _loud(want) == len(spots) and (np.count_nonzero(want["peak"], axis=1) == 1).all()
    # counts: NULL is stride for every channel; an explicit array of the same says the same; shorter ones, 0 and beyond stride
    rng = np.random.default_rng(2)
    y = rng.integers(INT32_MIN, INT32_MAX, (3, 3, 5000), dtype=np.int64, endpoint=True).astype(np.int32)
    full = _samples_case(gpu, y, label="counts NULL")
    _same(_samples_case(gpu, y, np.full((3, 3), 5000), label="counts = stride"), full, "NULL against an explicit array")
    want = _samples_case(gpu, y, [[0, 1, 4096], [4097, 5000, 70000], [0, 0, 0]], label="counts")
    assert want["samples"].tolist() == [[0, 1, 4096], [4097, 5000, 5000], [0, 0, 0]] and want[2].tolist() == [(0, 0, 0, 0, 0)] * 3
    assert _loud(want) == 2


def test_levels_samples_i32_of_codec(gpu):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(8)
    y = rng.integers(INT32_MIN, INT32_MAX, (2, 2, 3000), dtype=np.int64, endpoint=True).astype(np.int32)
    levels, status = codec.levels_samples_i32(torch.from_numpy(y).cuda())
    _same(codec.Leveler32.records(levels), _expect(y, np.full((2, 2), 3000)), "levels_samples_i32")
    assert status.cpu().numpy().tolist() == [0, 0, 2, 0]


# ---- 8. the payload form --------------------------------------------------------------------------------------------------------------
def test_a_payload_with_trailing_garbage(gpu):  # noqa: F811
    torch = gpu
    x = _samples(2, 24, 71)[: 3 * 2048].reshape(3, 2048, 2).transpose(0, 2, 1)
    blob, offs = codec.encode_i32(np.ascontiguousarray(x))
    want, _, _, _ = _check(torch, blob, offs, 2, 2048, fallback=0, label="the frames call")
    payload = np.frombuffer(blob.tobytes() + b"\x11" * 40, np.uint8).copy()  # (no sync word in the garbage: the walk ends at it)
    lev = codec.Leveler32(5, 2, 2048)
    lev.levels.fill_(-7)
    records, count = lev.measure_payload(torch.from_numpy(payload).cuda())
    lev.check()
    assert int(count.item()) == 3 and lev.loud_frames() == 3
    _same(lev.records(records[:3]), want, "the payload call")
    assert (records[3:].cpu().numpy() == -7).all(), "records of frames beyond the count were written"
    assert lev.frame_offsets.cpu().numpy()[:4].tolist() == offs.tolist()


# ---- 9. capture -----------------------------------------------------------------------------------------------------------------------
def test_one_capture_and_one_replay(gpu):  # noqa: F811
    torch = gpu
    x = _samples(2, 24, 72)[: 3 * 2048].reshape(3, 2048, 2).transpose(0, 2, 1)
    blob, offs = codec.encode_i32(np.ascontiguousarray(x))
    want, want_st, _, _ = _check(torch, blob, offs, 2, 2048, fallback=0, label="eager")
    frames, o = _on_device(torch, blob, offs)
    lev = codec.Leveler32(3, 2, 2048)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lev.measure(frames, o, 3)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lev.measure(frames, o, 3)
    lev.levels.fill_(-7), lev.status.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    _same(lev.records(out), want, "the replay")
    assert np.array_equal(lev.status.cpu().numpy().view(np.uint32), want_st)


# ---- 10. the host-pointer call and the Python classes ------------------------------------------------------------------------------------
def test_the_host_pointer_call_and_the_track_fold(gpu):  # noqa: F811
    torch = gpu
    x = _samples(2, 32, 73)[: 3 * 2048].reshape(3, 2048, 2).transpose(0, 2, 1)
    tail = np.stack([_signal(np.random.default_rng(1), "tone", 777, 27), _signal(np.random.default_rng(2), "noise", 777, 24)]).astype(np.int32)
    blobs = [codec.encode_i32(np.ascontiguousarray(x[f: f + 1]))[0].tobytes() for f in range(3)] + [codec.encode_i32(tail[None])[0].tobytes()]
    stream, offs = _stream(blobs)
    want, _, dec, m = _check(torch, stream, offs, 2, 2048, fallback=0, label="the device call")
    assert m[3].tolist() == [777, 777]
    got = codec.levels_i32_host(stream, offs, 2)
    _same(got, want, "sela_hip_levels_i32")
    lev = codec.Leveler32(4, 2, 2048)
    frames, o = _on_device(torch, stream, offs)
    _same(lev.records(lev.measure(frames, o, 4)), want, "Leveler32")
    lev.check()
    assert lev.loud_frames() == 4 and lev.fallback_frames() == 0
    track = codec.track_levels32(got)
    for c in range(2):
        peak, samples, total, energy = _record(np.concatenate([dec[f, c, : int(m[f, c])] for f in range(4)]))
        assert track[c] == {"peak": peak, "samples": samples, "sum": total, "sum_squares": energy}, c
    # a fold that passes 2^64: Python's integers carry it
    big = np.zeros((3, 1), codec.LEVEL32_DTYPE)
    big["sum_squares_lo"], big["sum_squares_hi"], big["peak"] = (1 << 64) - 1, 5, [[3], [9], [1]]
    assert codec.track_levels32(big)[0]["sum_squares"] == 3 * ((1 << 64) - 1) + (15 << 64) and codec.track_levels32(big)[0]["peak"] == 9
    # a malformed stream: sela_hip_decode_i32's code; no frames: no device
    bad = stream.copy()
    bad[int(offs[1])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as e:
        codec.levels_i32_host(bad, offs, 2)
    with pytest.raises(capi.SelaHipError) as d:
        codec.decode_i32(bad, offs, 2, 2048)
    assert e.value.code == d.value.code == -5
    assert codec.levels_i32_host(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2).shape == (0, 2)
