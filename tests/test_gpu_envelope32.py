"""sela_hip_envelope_i32_device, sela_hip_envelope_payload_i32_device, sela_hip_envelope_samples_i32_device and
sela_hip_envelope_i32: per frame, bucket of 32 .. 2048 samples and channel the smallest and the largest value,
the sum and the 128-bit sum of squares of the int32 samples sela_hip_decode_i32_device writes.  The expectation is always numpy
over that call's samples_out[f][c][:counts] for the same stream and stride (the energy in Python's integers), and every
comparison is exact equality of all five fields.  status[0], [1] and [3] are the decode call's; status[2] is 0."""
import numpy as np
import pytest

import generic_cases as gc
import topology_cases as tc
import wide_cases as wc
from gpu_common import _build_frame, _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from test_gpu_digest_pcm import _music
from test_gpu_levels32 import INT32_MAX, INT32_MIN, _record, _wide_frames
from test_gpu_pcm import pack_interleaved
from test_gpu_pcm_cli import _samples
from test_gpu_verify_i32_device import _bytes, _decode32, _fallback_layouts, _layout_blob, _on_device, _stream

pytestmark = pytest.mark.gpu

GUARD = 16              # records behind d_env that no call may write
SENTINEL = 0x5E1A5E1A5E1A5E1A
WORDS = 4               # 8-byte words of a record
MASK64 = (1 << 64) - 1


def _slots(stride, bucket):
    return -(-stride // bucket)


def _bucket_record(v):
    """the samples of one bucket of one channel (at least one) -> the record's five fields"""
    _, _, total, energy = _record(v)
    return (int(np.min(v)), int(np.max(v)), total, energy & MASK64, energy >> 64)


def _expect(dec, counts, bucket, stride=None):
    """dec: int32 [n, ch, stride] and counts [n, ch] as sela_hip_decode_i32_device writes them -> ENVELOPE32_DTYPE [n, slots, ch]."""
    n, ch = counts.shape
    slots = _slots(dec.shape[2] if stride is None else stride, bucket)
    out = np.zeros((n, slots, ch), codec.ENVELOPE32_DTYPE)
    for f in range(n):
        for c in range(ch):
            m = int(counts[f, c])
            for b in range(_slots(m, bucket)):
                out[f, b, c] = _bucket_record(dec[f, c, b * bucket: min((b + 1) * bucket, m)])
    return out


def _zero(rec):
    """are these records all-zero records"""
    return all(not np.asarray(rec[name]).any() for name in codec.ENVELOPE32_DTYPE.names)


def _same(got, want, label=""):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    for name in codec.ENVELOPE32_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (label, name, np.argwhere(got[name] != want[name])[:6].tolist(), got[name][got[name] != want[name]][:4],
                                                       want[name][got[name] != want[name]][:4])


class _Device:
    """Buffers of one sela_hip_envelope_i32_device call, the raw C ABI: guard records behind d_env, d_frames kept for a look afterwards."""

    def __init__(self, torch, n, ch, stride, bucket):
        self.torch, self.n, self.ch, self.stride, self.bucket = torch, n, ch, stride, bucket
        self.slots = int(capi.lib().sela_hip_envelope_slots(stride, bucket))
        assert self.slots == _slots(stride, bucket)
        self.env = torch.full(((n * self.slots * ch + GUARD) * WORDS,), SENTINEL, dtype=torch.int64, device="cuda")
        self.sample_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_envelope_i32_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")
        self.ws.fill_(0xA5)  # (no initialisation is needed: whatever lies there)

    def measure(self, blob, offs, with_offsets=True):
        torch = self.torch
        frames, o = _on_device(torch, blob, offs)
        before = frames.clone()
        assert self.env.data_ptr() % 8 == 0
        capi.check(capi.lib().sela_hip_envelope_i32_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, self.bucket, self.env.data_ptr(),
            self.sample_offsets.data_ptr() if with_offsets else None, self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(frames, before), "d_frames was written"
        return self.results()

    def results(self):
        words = self.env.cpu().numpy()
        k = self.n * self.slots * self.ch * WORDS
        assert (words[k:] == np.int64(SENTINEL)).all(), "written past d_env"
        return words[:k].copy().view(codec.ENVELOPE32_DTYPE).reshape(self.n, self.slots, self.ch), self.status.cpu().numpy().view(np.uint32).copy()

    def fallback_frames(self):
        return int(capi.lib().sela_hip_debug_envelope_i32_fallback_frames(self.ws.data_ptr(), self.n, self.ch, self.stride))


_DECODED = {}


def _decoded(torch, blob, offs, ch, stride):
    """what sela_hip_decode_i32_device writes for (stream, stride): computed once a stream and shared, never changed"""
    key = (_bytes(blob).tobytes(), tuple(int(x) for x in offs), ch, stride)
    if key not in _DECODED:
        if len(_DECODED) > 8:
            _DECODED.clear()
        dec, m, dst = _decode32(torch, blob, offs, ch, stride)
        so = codec.Decoder32(max(len(offs) - 1, 1), ch, stride)
        frames, o = _on_device(torch, blob, offs)
        so.decode(frames, o, len(offs) - 1)
        torch.cuda.synchronize()
        _DECODED[key] = (dec, m, dst, so.sample_offsets.cpu().numpy()[: len(offs)].copy())
    return _DECODED[key]


def _check(torch, blob, offs, ch, stride, bucket, fallback=None, label="", clean=True):
    """The records of (stream) == numpy on what the decode call writes; status and sample offsets as that call leaves them
    -> (records, status, decoded samples, counts)."""
    n = len(offs) - 1
    dec, m, dst, want_so = _decoded(torch, blob, offs, ch, stride)
    if clean:
        assert codec.decode_status_error(dst) == 0, (label, dst)
    dev = _Device(torch, n, ch, stride, bucket)
    got, st = dev.measure(blob, offs)  # (results() looks behind d_env whatever the status says)
    assert (int(st[0]), int(st[1]), int(st[2]), int(st[3])) == (int(dst[0]), int(dst[1]), 0, int(dst[3])), (label, st, dst)
    if not int(dst[0]) & capi.FLAG_STRIDE:
        assert not (got.view(np.int64) == np.int64(SENTINEL)).any(), (label, "a record was not written")
        _same(got, _expect(dec, m, bucket), label)
    assert np.array_equal(dev.sample_offsets.cpu().numpy()[: n + 1], want_so), label
    if fallback is not None:
        assert dev.fallback_frames() == fallback, (label, dev.fallback_frames(), fallback)
    return got, st, dec, m


# ---- 1. direct layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2, 3, 8, 9])
def test_direct_layouts_at_a_vector_and_a_scalar_stride(gpu, ch):  # noqa: F811
    x = _samples(ch, 24, 60 + ch)[: 3 * 2048].reshape(3, 2048, ch).transpose(0, 2, 1)
    streams = [("24-bit", codec.encode_i32(np.ascontiguousarray(x)))] + ([("25 to 31 bits", _wide_frames(2, 2048, 11))] if ch == 2 else [])
    for label, (blob, offs) in streams:
        for bucket in (32, 256, 2048):
            got, st, dec, m = _check(gpu, blob, offs, ch, 2048, bucket, fallback=0, label=(ch, label, 2048, bucket))
            assert (m == 2048).all() and got.shape == (3, 2048 // bucket, ch) and (got["max"] >= got["min"]).all() and (got["max"] > got["min"]).any()
            odd, _, _, _ = _check(gpu, blob, offs, ch, 2050, bucket, fallback=0, label=(ch, label, 2050, bucket))
            assert odd.shape[1] == 2048 // bucket + 1 and _zero(odd[:, -1]), "the slot behind the frame is the zero record"
            _same(odd[:, :-1], got, "both strides give the same leading records")
        if label != "24-bit":
            assert int(np.abs(got["min"].astype(np.int64)).max()) >= 1 << 24 or int(got["max"].max()) >= 1 << 24


# ---- 2. lengths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 31, 32, 33, 63, 64, 65, 777, 4095, 4096, 4097])
def test_lengths_at_every_edge(gpu, n):  # noqa: F811
    rng = np.random.default_rng(n)
    for ch in (1, 2):
        x = np.stack([np.stack([_signal(rng, ("tone", "noise")[c], n, 23 - 3 * c) for c in range(ch)]) for _ in range(2)]).astype(np.int32)
        if n < 100:  # (hand-built, order 0: an encoder's block must be longer than its order)
            blob, offs = _stream([_build_frame([(c, 0, 0, np.zeros(0, np.int32), x[f, c]) for c in range(ch)]) for f in range(2)])
        else:
            blob, offs = codec.encode_i32(x)
        for bucket in (32, 1024):
            got, _, _, m = _check(gpu, blob, offs, ch, n, bucket, fallback=0, label=(n, ch, bucket))
            assert (m == n).all() and got.shape[1] == _slots(n, bucket)
            _check(gpu, blob, offs, ch, n + 5, bucket, fallback=0, label=(n, ch, bucket, "a roomy stride"))


# ---- 3. a partial bucket --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [-5, 7])
def test_a_partial_bucket_is_not_padded_with_zeros(gpu, value):  # noqa: F811
    n = 37
    v = np.full(n, value, np.int32)
    mono = _build_frame([(0, 0, 0, np.zeros(0, np.int32), v)])
    # the second channel a difference subframe: parent - difference = value
    stereo = _build_frame([(0, 0, 0, np.zeros(0, np.int32), np.full(n, 100, np.int32)), (1, 1, 0, np.zeros(0, np.int32), np.full(n, 100 - value, np.int32))])
    for ch, blob in ((1, mono), (2, stereo)):
        for stride in (40, 37):  # (40: int4 loads, the last one reaches past the end; 37: scalar loads)
            got, _, dec, m = _check(gpu, blob, np.array([0, len(blob)], np.uint64), ch, stride, 32, fallback=0, label=(value, ch, stride))
            assert (m == n).all() and (dec[0, ch - 1, :n] == value).all()
            assert got[0, 0, ch - 1].tolist() == (value, value, 32 * value, 32 * value * value, 0)
            assert got[0, 1, ch - 1].tolist() == (value, value, 5 * value, 5 * value * value, 0), got[0, 1]
            assert int(got["min"][0, 1, ch - 1]) != 0 and int(got["max"][0, 1, ch - 1]) != 0


# ---- 4. ragged frames -----------------------------------------------------------------------------------------------------------------
def test_ragged_frames(gpu):  # noqa: F811
    for label, chans in gc.ragged_cases():
        ch, lens = len(chans), [len(c) for c in chans]
        blob = codec.encode_ragged(chans)
        offs = np.array([0, len(blob)], np.uint64)
        for stride in (max(lens), max(lens) + 3):
            got, _, _, m = _check(gpu, blob, offs, ch, stride, 32, fallback=0, label=(label, stride))
            assert m[0].tolist() == lens, label
            for c, n in enumerate(lens):  # each channel's records end at its own count: zero records behind it
                assert _zero(got[0, _slots(n, 32):, c]), (label, c)


# ---- 5. the fallback ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [2, 3, 5])
def test_other_layouts_take_the_fallback(gpu, ch):  # noqa: F811
    o = oracle()
    good = [_layout_blob(o, layout, 7 * ch + k) for k, (_, layout) in enumerate(tc.ACCEPTED_LAYOUTS[ch][:2])]
    others = [(name, _layout_blob(o, layout, 900 + 10 * ch + k)) for k, (name, layout) in enumerate(_fallback_layouts(ch))]
    for name, blob in others:  # each alone
        _check(gpu, blob, np.array([0, len(blob)], np.uint64), ch, tc.N, 256, fallback=1, label=(ch, name), clean=False)
    # direct frames alone leave the fallback idle
    stream, offs = _stream(good)
    _check(gpu, stream, offs, ch, tc.N, 256, fallback=0, label=(ch, "direct alone"))
    # direct and fallback frames in one stream
    blobs = [good[0]] + [b for _, b in others[:1]] + [good[1]] + [b for _, b in others[1:]] + [good[0]]
    stream, offs = _stream(blobs)
    for stride in (tc.N, tc.N + 2):
        got, _, _, m = _check(gpu, stream, offs, ch, stride, 32, fallback=len(others), label=(ch, "mixed", stride), clean=False)
        assert int(m[1, 1]) == 0 and _zero(got[1, :, 1])  # (channel 1 never named: all zero records)
        assert (m[[0, 2, len(blobs) - 1]] == tc.N).all()


# ---- 6. faults in the stream ----------------------------------------------------------------------------------------------------------
def test_a_malformed_frame_in_the_middle_and_a_small_stride(gpu):  # noqa: F811
    rng = np.random.default_rng(6)
    x = np.stack([np.stack([_signal(rng, "tone", 700, 23), _signal(rng, "noise", 700, 20)]) for _ in range(4)]).astype(np.int32)
    frames, offs = codec.encode_i32(x)
    bad = frames.copy()
    bad[int(offs[2])] ^= 0xFF
    got, st, _, m = _check(gpu, bad, offs, 2, 700, 64, label="bad sync word", clean=False)
    assert codec.decode_status_error([int(st[0]), int(st[1]), 0, 0]) != 0
    clean, _, _, _ = _check(gpu, frames, offs, 2, 700, 64, fallback=0, label="clean")
    _same(got[[0, 1, 3]], clean[[0, 1, 3]], "the other frames")
    # a stride that is too small: the flag, and nothing past the guards (_Device.results looks)
    _, st, _, _ = _check(gpu, frames, offs, 2, 699, 64, label="stride too small", clean=False)
    assert int(st[0]) & capi.FLAG_STRIDE


# ---- 7. the ends of int32, from a stream ------------------------------------------------------------------------------------------------
def test_a_difference_subframe_at_the_ends_of_int32(gpu):  # noqa: F811
    n = 100
    parent, diff = np.full(n, (1 << 30) - 1, np.int32), np.full(n, -(1 << 30), np.int32)
    blob = _build_frame([(0, 0, 0, np.zeros(0, np.int32), parent), (1, 1, 0, np.zeros(0, np.int32), diff)])
    got, _, dec, m = _check(gpu, blob, np.array([0, len(blob)], np.uint64), 2, n, 32, fallback=0, label="INT32_MAX")
    assert m.tolist() == [[n, n]] and (dec[0, 1, :n] == INT32_MAX).all() and got.shape == (1, 4, 2)
    for b, k in enumerate((32, 32, 32, 4)):
        energy = k * INT32_MAX * INT32_MAX
        assert got[0, b, 1].tolist() == (INT32_MAX, INT32_MAX, k * INT32_MAX, energy & MASK64, energy >> 64), b
    assert (got["sum_squares_hi"][0, :3, 1] > 0).all() and int(got["sum_squares_hi"][0, 3, 1]) == 0
    # ... and a crafted frame whose parent - difference wraps int32 on the decoder's side
    o = oracle()
    subs, _ = wc.stereo_wrap_subframes(o, 600, 4)
    blob = wc.frame_bytes(o, subs)
    for stride in (600, 601):
        _check(gpu, blob, np.array([0, len(blob)], np.uint64), 2, stride, 32, fallback=0, label=("wrap", stride))


# ---- 8. the number range, on samples that already lie in device memory ------------------------------------------------------------------
def _measure_samples(torch, x, bucket, counts=None, shift=0):
    """sela_hip_envelope_samples_i32_device, the raw C ABI with guard records -> (records, status); shift: d_samples that many
    int32s behind a 16-byte boundary."""
    x = np.ascontiguousarray(x, np.int32)
    n, ch, stride = x.shape
    slots = _slots(stride, bucket)
    lib = capi.lib()
    room = torch.zeros(x.size + 8, dtype=torch.int32, device="cuda")
    room[shift: shift + x.size].copy_(torch.from_numpy(x.reshape(-1)))
    before = room.clone()
    cnt = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts, np.uint32).reshape(-1).view(np.int32).copy()).cuda()
    env = torch.full(((n * slots * ch + GUARD) * WORDS,), SENTINEL, dtype=torch.int64, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sela_hip_envelope_samples_i32_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")
    ws.fill_(0xA5)
    capi.check(lib.sela_hip_envelope_samples_i32_device(room.data_ptr() + 4 * shift, None if cnt is None else cnt.data_ptr(), n, ch, stride, bucket, env.data_ptr(),
                                                        status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(room, before), "d_samples was written"
    words = env.cpu().numpy()
    k = n * slots * ch * WORDS
    assert (words[k:] == np.int64(SENTINEL)).all(), "written past d_env"
    assert not (words[:k] == np.int64(SENTINEL)).any(), "a record was not written"
    return words[:k].copy().view(codec.ENVELOPE32_DTYPE).reshape(n, slots, ch), status.cpu().numpy().view(np.uint32).copy()


def _samples_case(torch, x, bucket, counts=None, label=""):
    x = np.ascontiguousarray(x, np.int32)
    n, ch, stride = x.shape
    m = np.full((n, ch), stride, np.uint32) if counts is None else np.minimum(np.asarray(counts, np.uint32).reshape(n, ch), stride)
    want = _expect(x, m, bucket)
    for shift in (0, 1):  # (rows at 16 bytes: four samples a load; rows behind: one)
        got, st = _measure_samples(torch, x, bucket, counts, shift)
        _same(got, want, (label, shift))
        assert st.tolist() == [0, 0, 0, 0], (label, st)
    return want


def test_full_scale_samples_pass_64_bits(gpu):  # noqa: F811
    full = np.full((1, 1, 2048), INT32_MIN, np.int32)
    # 2^73: 32 samples a lane, 2^67 in a lane -- a bare 64-bit accumulator gives 0
    want = _samples_case(gpu, full, 2048, label="2048 x INT32_MIN, bucket 2048")
    assert want.shape == (1, 1, 1) and want[0, 0, 0].tolist() == (INT32_MIN, INT32_MIN, -(1 << 42), 0, 512)
    # 32 x INT32_MIN a bucket: 2^67 -- a bare u64 energy gives 0, a 32-bit sum ladder wraps
    want = _samples_case(gpu, full, 32, label="2048 x INT32_MIN, bucket 32")
    assert want.shape == (1, 64, 1) and all(r.tolist() == (INT32_MIN, INT32_MIN, -(1 << 36), 0, 8) for r in want[0, :, 0])
    alt = np.where(np.arange(4100) % 2 == 0, INT32_MIN, INT32_MAX).astype(np.int32)
    for bucket in (32, 2048):
        want = _samples_case(gpu, np.stack([alt, alt[::-1]])[None], bucket, label=("alternating", bucket))
        assert (want["min"] == INT32_MIN).all() and (want["max"] == INT32_MAX).all()
        assert int(want["sum"][0, 0, 0]) == -(bucket // 2)


def test_silence_single_samples_and_counts(gpu):  # noqa: F811
    want = _samples_case(gpu, np.zeros((2, 2, 4097), np.int32), 64, label="silence")
    assert _zero(want)
    n = 8195
    spots = [0, 31, 32, 4095, 4096, n - 1]
    x = np.zeros((len(spots), 2, n), np.int32)
    for f, i in enumerate(spots):
        x[f, f & 1, i] = INT32_MIN if f % 3 == 0 else (f + 1) * (-1) ** f
    for bucket in (32, 2048):
        want = _samples_case(gpu, x, bucket, label=("single samples", bucket))
        for f, i in enumerate(spots):  # exactly one record of the frame is not silent: the spot's
            loud = np.argwhere((want["min"][f] != 0) | (want["max"][f] != 0)).tolist()
            assert loud == [[i // bucket, f & 1]], (bucket, f, loud)
    # counts: NULL is stride for every channel; an explicit array of the same says the same; shorter ones, 0 and beyond stride
    rng = np.random.default_rng(2)
    y = rng.integers(INT32_MIN, INT32_MAX, (3, 3, 5000), dtype=np.int64, endpoint=True).astype(np.int32)
    full = _samples_case(gpu, y, 256, label="counts NULL")
    _same(_samples_case(gpu, y, 256, np.full((3, 3), 5000), label="counts = stride"), full, "NULL against an explicit array")
    want = _samples_case(gpu, y, 256, [[0, 1, 4096], [4097, 5000, 70000], [0, 0, 0]], label="counts")
    assert _zero(want[2]) and _zero(want[0, :, 0])
    assert want[0, 0, 1].tolist() == (int(y[0, 1, 0]), int(y[0, 1, 0]), int(y[0, 1, 0]), (int(y[0, 1, 0]) ** 2) & MASK64, (int(y[0, 1, 0]) ** 2) >> 64)
    assert _zero(want[0, 16:, 2]) and not _zero(want[1, 16, 0]) and _zero(want[1, 17:, 0])
    _same(want[1, :, 2], full[1, :, 2], "a count beyond stride is stride")


def test_envelope_samples_i32_of_codec(gpu):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(8)
    y = rng.integers(INT32_MIN, INT32_MAX, (2, 2, 3000), dtype=np.int64, endpoint=True).astype(np.int32)
    env, status = codec.envelope_samples_i32(torch.from_numpy(y).cuda(), 128)
    _same(codec.Enveloper32.records(env), _expect(y, np.full((2, 2), 3000), 128), "envelope_samples_i32")
    assert status.cpu().numpy().tolist() == [0, 0, 0, 0]


# ---- 9. consistency with what is already shipped ---------------------------------------------------------------------------------------
def test_the_records_fold_to_the_level_call_s_and_to_a_coarser_bucket(gpu):  # noqa: F811
    torch = gpu
    x = _samples(2, 32, 74)[: 3 * 2048].reshape(3, 2048, 2).transpose(0, 2, 1)
    blob, offs = codec.encode_i32(np.ascontiguousarray(x))
    fine, _, _, _ = _check(torch, blob, offs, 2, 2048, 32, fallback=0, label="bucket 32")
    coarse, _, _, _ = _check(torch, blob, offs, 2, 2048, 256, fallback=0, label="bucket 256")
    _same(codec.fold_envelope32(fine, 8), coarse, "bucket 32 folded by 8 is bucket 256")
    frames, o = _on_device(torch, blob, offs)
    lev = codec.Leveler32(3, 2, 2048)
    levels = lev.records(lev.measure(frames, o, 3))
    lev.check()
    whole = codec.fold_envelope32(fine, 64)[:, 0]
    assert np.array_equal(np.maximum(np.abs(whole["min"].astype(np.int64)), np.abs(whole["max"].astype(np.int64))), levels["peak"].astype(np.int64))
    assert (levels["samples"] == 2048).all()
    for name in ("sum", "sum_squares_lo", "sum_squares_hi"):
        assert np.array_equal(whole[name], levels[name]), name


def test_a_16_bit_stream_gives_the_16_bit_envelope_s_records(gpu):  # noqa: F811
    torch = gpu
    x = _samples(2, 16, 75)[: 3 * 2048].reshape(3, 2048, 2).transpose(0, 2, 1)
    blob, offs = codec.encode_i32(np.ascontiguousarray(x))
    frames, o = _on_device(torch, blob, offs)
    for bucket in (32, 512):
        got, _, _, _ = _check(torch, blob, offs, 2, 2048, bucket, fallback=0, label=("16-bit", bucket))
        narrow = codec.Enveloper(3, 2, 2048, bucket)
        want = narrow.records(narrow.measure(frames, o, 3))
        narrow.check()
        for name in ("min", "max", "sum"):
            assert np.array_equal(got[name].astype(np.int64), want[name].astype(np.int64)), (bucket, name)
        assert np.array_equal(got["sum_squares_lo"], want["sum_squares"]) and not got["sum_squares_hi"].any()


# ---- 10. a long frame -----------------------------------------------------------------------------------------------------------------
def test_a_65535_sample_mono_frame(gpu):  # noqa: F811
    rng = np.random.default_rng(65535)
    x = _signal(rng, "tone", 65535, 23).astype(np.int32)[None, None]
    blob, offs = codec.encode_i32(x)
    got, _, _, m = _check(gpu, blob, offs, 1, 65535, 2048, fallback=0, label="65535")
    assert m.tolist() == [[65535]] and got.shape == (1, 32, 1) and capi.lib().sela_hip_envelope_i32_workspace_bytes(1, 1, 65535) == capi.lib().sela_hip_verify_i32_workspace_bytes(1, 1, 65535)


# ---- 11. the payload form -------------------------------------------------------------------------------------------------------------
def test_a_payload_with_trailing_garbage(gpu):  # noqa: F811
    torch = gpu
    x = _samples(2, 24, 71)[: 3 * 2048].reshape(3, 2048, 2).transpose(0, 2, 1)
    blob, offs = codec.encode_i32(np.ascontiguousarray(x))
    want, _, _, _ = _check(torch, blob, offs, 2, 2048, 128, fallback=0, label="the frames call")
    payload = np.frombuffer(blob.tobytes() + b"\x11" * 40, np.uint8).copy()  # (no sync word in the garbage: the walk ends at it)
    env = codec.Enveloper32(5, 2, 2048, 128)
    env.envelope.fill_(-7)
    records, count = env.measure_payload(torch.from_numpy(payload).cuda())
    env.check()
    assert int(count.item()) == 3 and int(env.status[2].item()) == 0
    _same(env.records(records[:3]), want, "the payload call")
    assert (records[3:].cpu().numpy() == -7).all(), "records of frames beyond the count were written"
    assert env.frame_offsets.cpu().numpy()[:4].tolist() == offs.tolist()


# ---- 12. capture ----------------------------------------------------------------------------------------------------------------------
def test_one_capture_and_one_replay(gpu):  # noqa: F811
    torch = gpu
    x = _samples(2, 24, 72)[: 3 * 2048].reshape(3, 2048, 2).transpose(0, 2, 1)
    blob, offs = codec.encode_i32(np.ascontiguousarray(x))
    want, want_st, _, _ = _check(torch, blob, offs, 2, 2048, 256, fallback=0, label="eager")
    frames, o = _on_device(torch, blob, offs)
    env = codec.Enveloper32(3, 2, 2048, 256)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.measure(frames, o, 3)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = env.measure(frames, o, 3)
    env.envelope.fill_(-7), env.status.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    _same(env.records(out), want, "the replay")
    assert np.array_equal(env.status.cpu().numpy().view(np.uint32), want_st)


# ---- 13. the host-pointer call and whole tracks -----------------------------------------------------------------------------------------
def test_the_host_pointer_call_and_a_whole_track(gpu):  # noqa: F811
    torch = gpu
    n_samples, bucket = 3 * 2048 + 777, 256
    x = _music(np.random.default_rng(47), n_samples, 2, 23)
    stream, offs = codec.encode_whole_pcm_host(pack_interleaved(x, 3), 2, 3, lossless=True)
    assert len(offs) - 1 == 3
    stride = 2048 + 777
    want, _, dec, m = _check(torch, stream, offs, 2, stride, bucket, fallback=0, label="the device call")
    assert m.tolist() == [[2048, 2048], [2048, 2048], [stride, stride]]
    got = codec.envelope_i32_host(stream, offs, 2, bucket)
    _same(got, want, "sela_hip_envelope_i32")
    env = codec.Enveloper32(3, 2, stride, bucket)
    frames, o = _on_device(torch, stream, offs)
    _same(env.records(env.measure(frames, o, 3)), want, "Enveloper32")
    env.check()
    assert env.fallback_frames() == 0
    # on the track's grid: numpy over the original samples
    track = codec.track_envelope32(got, env.sample_offsets.cpu().numpy()[:4], bucket)
    assert track.shape == (_slots(n_samples, bucket), 2)
    _same(track[None], _expect(np.ascontiguousarray(x.T)[None].astype(np.int32), np.full((1, 2), n_samples), bucket).reshape(1, -1, 2), "the track")
    # a malformed stream: sela_hip_decode_i32's code; no frames: no device
    bad = stream.copy()
    bad[int(offs[1])] ^= 0xFF
    with pytest.raises(capi.SelaHipError) as e:
        codec.envelope_i32_host(bad, offs, 2, bucket, stride)
    with pytest.raises(capi.SelaHipError) as d:
        codec.decode_i32(bad, offs, 2, stride)
    assert e.value.code == d.value.code == -5
    assert codec.envelope_i32_host(np.zeros(4, np.uint8), np.zeros(1, np.uint64), 2, bucket, 2048).shape == (0, 8, 2)
