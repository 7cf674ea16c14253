"""The second pass of frame::FrameDecoder as the four fused 16-bit kernels consume it -- k_level_frames, k_digest_frames,
k_envelope_frames and k_window_frames, each with its own copy of the frame loop -- and the cold routes of levels, digest and
envelope behind k_decode_frames_wide, on every subframe layout of topology_cases.py: subframes out of channel order (position
!= channel), a difference in front of its parent, a parent with the higher channel number, two differences under one parent,
parent - difference beyond int16 (the +-12000 frames: a reduction taken before the mod 2^16 has another peak), the refused
layouts, and a subframe on the serial parse between two frames on the fast plan, in both recurrence forms.

Every expectation is numpy or zlib on the CPU oracle's PCM (topology_cases.accepted_stream and its kin, pinned to the reference
by test_oracle_topologies.py), never another GPU call; only the status words of a stream with refused frames are compared with
sela_hip_decode_n_device's.  All comparisons are exact.  All frames of one channel count are one stream: one launch per call
on at most 16 frames (19 where every refused layout stands between two accepted ones)."""
import functools

import numpy as np
import pytest

import test_gpu_decode_windows as tw
import test_gpu_digest as td
import test_gpu_envelope as te
import test_gpu_levels as tl
import topology_cases as tc
from gpu_common import gpu  # noqa: F401
from sela_amd import capi, codec
from test_gpu_decode_topologies import _serial_between_fast
from test_gpu_verify_device import _decode_n

pytestmark = pytest.mark.gpu

FAST = 1
EFORMAT = -5
BAD = capi.FLAG_BAD_FRAME
I16, F32 = capi.WINDOW_I16_INTERLEAVED, capi.WINDOW_F32_PLANAR
FUSED, COLD = (2, 3, 5, 8), (9, 12)  # up to eight channels the fused kernels; more: k_decode_frames_wide, then the *_channels / _pcm kernels
BUCKETS = (32, 256, 2048)            # one bucket inside a wave step, one of several steps for the non-stereo shape, one per frame
STRIDES = (tc.N, 3000)


def _offsets(n):
    return np.arange(n + 1, dtype=np.uint64) * np.uint64(tc.N)


@functools.lru_cache(maxsize=None)
def _wanted(kind, ch):
    """(labels, stream, offsets, oracle PCM int16 [frames, 2048, ch], accepted mask) of one stream, and what numpy and zlib make of
    its PCM: levels, (digests, track crc, track bytes), {bucket: envelope at stride 2048}.  Computed once; treat as read-only."""
    if kind == "accepted":
        cs, stream, offs, pcm = tc.accepted_stream(ch)
        labels, mask = [c[0] for c in cs], np.ones(len(cs), bool)
    elif kind == "refused":
        cs, mask, stream, offs, pcm = tc.refused_stream(ch)
        labels = [c[0] for c in cs]
    else:
        _, stream, offs, pcm = _serial_between_fast(ch)
        labels, mask = ["fast", "serial", "fast"], np.ones(3, bool)
    n = len(labels)
    assert pcm.shape == (n, tc.N, ch) and n <= (16 if kind != "refused" else 20)
    flat, so = pcm.reshape(-1, ch), _offsets(n)
    return labels, stream, offs, pcm, mask, tl._expect(flat, so), td._expect(flat, so), {b: te._expect(flat, so, tc.N, b) for b in BUCKETS}


def _rows(got, want, names, labels, which, what):
    """the records of the frames `which` are the expectation's, field by field"""
    for f in which:
        for name in names:
            g, w = np.atleast_1d(got[name][f]), np.atleast_1d(want[name][f])
            assert np.array_equal(g, w), (what, labels[f], name, g.reshape(-1)[:4].tolist(), w.reshape(-1)[:4].tolist())


def _levels(torch, kind, ch, stride, which=None):
    labels, stream, offs, _, _, want, _, _ = _wanted(kind, ch)
    dev = tl._Device(torch, len(labels), ch, stride)
    got, st = dev.measure(np.array(stream), np.array(offs))
    _rows(got, want, codec.LEVEL_DTYPE.names, labels, range(len(labels)) if which is None else which, ("levels", ch, stride))
    assert np.array_equal(dev.sample_offsets.cpu().numpy().view(np.uint64), _offsets(len(labels)))
    return st, want


def _digest(torch, kind, ch, stride, which=None):
    labels, stream, offs, _, _, _, (want, crc, total), _ = _wanted(kind, ch)
    dev = td._Device(torch, len(labels), ch, stride)
    got, track, st = dev.digest(np.array(stream), np.array(offs))
    _rows(got, want, codec.DIGEST_DTYPE.names, labels, range(len(labels)) if which is None else which, ("digest", ch, stride))
    if which is None:
        assert track == (crc, total), ("digest, the track", ch, stride, [hex(track[0]), track[1]], [hex(crc), total])
    assert np.array_equal(dev.sample_offsets.cpu().numpy().view(np.uint64), _offsets(len(labels)))
    return st


def _envelope(torch, kind, ch, stride, bucket, which=None):
    labels, stream, offs, _, _, _, _, wants = _wanted(kind, ch)
    n, filled = len(labels), tc.N // bucket
    dev = te._Device(torch, n, ch, stride, bucket)
    dev.env[: n * dev.slots * ch * 2] = te.SENTINEL + 1  # (nothing is pre-cleared: every record of a frame that ran is written)
    got, st = dev.measure(np.array(stream), np.array(offs))
    assert got.shape == (n, te._slots(stride, bucket), ch)
    which = range(n) if which is None else which
    _rows(got[:, :filled], wants[bucket], codec.ENVELOPE_DTYPE.names, labels, which, ("envelope", ch, stride, bucket))
    assert all(r == te.ZERO for f in which for r in got[f, filled:].reshape(-1).tolist()), "the slots behind the frame's end are zero records"
    assert np.array_equal(dev.sample_offsets.cpu().numpy().view(np.uint64), _offsets(n))
    return st


def test_the_streams_are_what_the_issue_counted():
    """... and every stream has a +-12000 frame with a dependent channel: topology_cases.cases() asserts that such a channel leaves
    int16, so a reduction taken before the mod 2^16 has another peak than the PCM's."""
    assert [len(_wanted("accepted", ch)[0]) for ch in FUSED + COLD] == [16, 6, 7, 6, 4, 5]
    for ch in FUSED + COLD:
        assert any(f"+-{tc.WRAPPING}" in c[0] and tc.dependent_channels(c[2]) for c in tc.accepted(ch))


# ---- a. accepted layouts: levels, digest, envelope ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", FUSED + COLD)
def test_levels_of_accepted_layouts(gpu, ch):  # noqa: F811
    for stride in STRIDES:
        st, want = _levels(gpu, "accepted", ch, stride)
        assert st.tolist() == [0, 0, int((want["peak"] != 0).any(1).sum()), FAST], (stride, st)


@pytest.mark.parametrize("ch", FUSED + COLD)
def test_digests_of_accepted_layouts(gpu, ch):  # noqa: F811
    for stride in STRIDES:
        st = _digest(gpu, "accepted", ch, stride)
        assert st.tolist() == [0, 0, 0, FAST], (stride, st)


@pytest.mark.parametrize("bucket", BUCKETS)
@pytest.mark.parametrize("ch", FUSED + COLD)
def test_envelopes_of_accepted_layouts(gpu, ch, bucket):  # noqa: F811
    for stride in STRIDES:
        st = _envelope(gpu, "accepted", ch, stride, bucket)
        assert st.tolist() == [0, 0, 0, FAST], (stride, bucket, st)


@pytest.mark.parametrize("ch", FUSED + COLD)
def test_the_payload_and_the_host_pointer_forms(gpu, ch):  # noqa: F811
    """sela_hip_levels_payload_device, _digest_payload_device, _envelope_payload_device and the three host-pointer calls, once each
    at stride 2048 (the host calls choose it themselves)."""
    torch = gpu
    labels, stream, offs, _, _, levels, (digests, crc, total), envelopes = _wanted("accepted", ch)
    stream, offs = np.array(stream), np.array(offs)
    n = len(labels)
    payload = torch.from_numpy(stream).cuda()
    every = range(n)
    lev = codec.Leveler(n, ch, tc.N)
    records, count = lev.measure_payload(payload)
    lev.check()
    assert int(count.item()) == n and lev.route() == FAST and lev.loud_frames() == int((levels["peak"] != 0).any(1).sum())
    _rows(lev.records(records), levels, codec.LEVEL_DTYPE.names, labels, every, "levels, payload")
    assert np.array_equal(lev.frame_offsets[: n + 1].cpu().numpy().view(np.uint64), offs)
    dig = codec.Digester(n, ch, tc.N)
    records, track, count = dig.digest_payload(payload)
    dig.check()
    assert int(count.item()) == n and dig.route() == FAST and dig.track_words() == (crc, total)
    _rows(dig.records(records), digests, codec.DIGEST_DTYPE.names, labels, every, "digest, payload")
    env = codec.Enveloper(n, ch, tc.N, 256)
    records, count = env.measure_payload(payload)
    env.check()
    assert int(count.item()) == n and env.route() == FAST
    _rows(env.records(records), envelopes[256], codec.ENVELOPE_DTYPE.names, labels, every, "envelope, payload")
    _rows(codec.levels_host(stream, offs, ch), levels, codec.LEVEL_DTYPE.names, labels, every, "levels, host")
    got, got_crc, got_total = codec.digest_host(stream, offs, ch)
    _rows(got, digests, codec.DIGEST_DTYPE.names, labels, every, "digest, host")
    assert (got_crc, got_total) == (crc, total)
    got = codec.envelope_host(stream, offs, ch, 256)
    assert got.shape == (n, 8, ch)
    _rows(got, envelopes[256], codec.ENVELOPE_DTYPE.names, labels, every, "envelope, host")


# ---- b. accepted layouts: windows ---------------------------------------------------------------------------------------------------
class _Table:
    """what test_gpu_decode_windows.device_call asks of a table, without its GPU decode: the expectation here is the oracle's"""

    def __init__(self, torch, stream, offs, ch):
        self.torch, self.ch, self.n = torch, ch, len(offs) - 1
        self.stream, self.offs = np.array(stream), np.array(offs)
        self.d_frames = torch.from_numpy(self.stream).cuda()
        self.d_offs = torch.from_numpy(self.offs.view(np.int64).copy()).cuda()


def _cut(flat, windows, ws):
    """flat: [samples of the one stream, ch]; windows of that stream -> [n, ws, ch], zeros behind the stream's end"""
    out = np.zeros((len(windows), ws) + flat.shape[1:], flat.dtype)
    for w, (start, _, _) in enumerate(windows):
        seg = flat[start: start + ws]
        out[w, : len(seg)] = seg
    return out


def _touched(windows, ws, n):
    """per window the frames of the stream (0 .. n - 1) it decodes: the window geometry alone"""
    return [range(s // tc.N, min((s + ws - 1) // tc.N + 1, n)) for s, _, _ in windows]


def _window_batches(n):
    """(windows, length): one per frame from its sample 0; three samples across every seam, so that two frames of different
    layouts share a window; the whole stream"""
    return [([(f * tc.N, 0, n) for f in range(n)], tc.N), ([(f * tc.N + tc.N - 1, 0, n) for f in range(n - 1)], 3), ([(0, 0, n)], n * tc.N)]


@pytest.mark.parametrize("fmt", [I16, F32], ids=["i16", "f32"])
@pytest.mark.parametrize("ch", FUSED)
def test_windows_of_accepted_layouts(gpu, ch, fmt):  # noqa: F811
    labels, stream, offs, pcm, _, _, _, _ = _wanted("accepted", ch)
    n = len(labels)
    t = _Table(gpu, stream, offs, ch)
    for windows, ws in _window_batches(n):
        want = tw.as_format(_cut(pcm.reshape(-1, ch), windows, ws), fmt)
        _, out, flags, status = tw.device_call(t, windows, ws, fmt)
        bad = np.argwhere(out != want)
        assert tw.same_bits(out, want), (ws, len(bad), bad[:6].tolist(), [labels[k] for k in sorted({int(b[0]) for b in bad[:50]})] if ws == tc.N else "")
        assert not flags.any() and status.tolist() == [0, 0, 0, 0], (ws, flags, status)


@pytest.mark.parametrize("ch", FUSED)
def test_windows_through_the_host_pointer_call(gpu, ch):  # noqa: F811
    """sela_hip_decode_windows stages the covering frames onto a compacted table: windows into every other frame and across the
    seams behind them, so that the layouts meet renumbered frames."""
    labels, stream, offs, pcm, _, _, _, _ = _wanted("accepted", ch)
    n = len(labels)
    windows = [(f * tc.N + 5, 0, n) for f in range(1, n, 2)] + [(f * tc.N + tc.N - 300, 0, n) for f in range(1, n - 1, 3)]
    ws = 700
    packed = codec.WindowDecoder.pack([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])
    out, flags, rc = codec.decode_windows_host(np.array(stream), np.array(offs), ch, packed, ws)
    staged = sorted({f for r in _touched(windows, ws, n) for f in r})
    assert 0 not in staged and len(staged) < n  # (the table is compacted: staged frame k is not frame k)
    assert int(capi.lib().sela_hip_debug_windows_staged_bytes()) == sum(int(offs[f + 1] - offs[f]) for f in staged)
    assert rc == 0 and not flags.any() and tw.same_bits(out, _cut(pcm.reshape(-1, ch), windows, ws))


# ---- c. refused layouts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", tc.REFUSED_CHANNELS)
def test_refused_layouts_cost_their_own_records_and_no_others(gpu, ch):  # noqa: F811
    """status[0], [1] and [3] are sela_hip_decode_n_device's on the same stream -- BAD_FRAME, the refused frames counted once each,
    the fast route -- and the records of every accepted frame are exact.  Nothing is asserted about a refused frame's own record,
    nor about the track word that contains it."""
    labels, stream, offs, _, mask, _, _, _ = _wanted("refused", ch)
    good, n_bad = np.flatnonzero(mask), int((~mask).sum())
    _, _, dst = _decode_n(gpu, np.array(stream), np.array(offs), ch, tc.N)
    assert (int(dst[0]), int(dst[1]), int(dst[3])) == (BAD, n_bad, FAST) and codec.decode_n_status_error(dst) == EFORMAT, dst
    runs = [("levels", _levels(gpu, "refused", ch, tc.N, good)[0]), ("digest", _digest(gpu, "refused", ch, tc.N, good))]
    runs += [(("envelope", b), _envelope(gpu, "refused", ch, tc.N, b, good)) for b in (32, 2048)]
    for what, st in runs:
        assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (what, st, dst)
        assert codec.decode_n_status_error(st) == EFORMAT, (what, st)


@pytest.mark.parametrize("fmt", [I16, F32], ids=["i16", "f32"])
@pytest.mark.parametrize("ch", [c for c in tc.REFUSED_CHANNELS if c <= 8])
def test_windows_on_refused_layouts(gpu, ch, fmt):  # noqa: F811
    """One window per frame: BAD_FRAME exactly on the windows of refused frames, status[1] the (window, frame) decodes of refused
    frames, status[2] the flagged windows -- both from the window geometry -- and the accepted frames' windows exact."""
    labels, stream, offs, pcm, mask, _, _, _ = _wanted("refused", ch)
    n = len(labels)
    t = _Table(gpu, stream, offs, ch)
    windows, ws = _window_batches(n)[0]
    touched = _touched(windows, ws, n)
    want_flags = np.array([BAD if any(not mask[f] for f in r) else 0 for r in touched], np.uint32)
    decodes = sum(1 for r in touched for f in r if not mask[f])
    assert decodes == int((~mask).sum()) == int((want_flags != 0).sum()) >= 7
    want = tw.as_format(_cut(pcm.reshape(-1, ch), windows, ws), fmt)
    _, out, flags, status = tw.device_call(t, windows, ws, fmt)
    assert np.array_equal(flags, want_flags), [(labels[w], int(flags[w])) for w in np.flatnonzero(flags != want_flags)]
    assert status.tolist() == [BAD, decodes, int((want_flags != 0).sum()), 0], status
    for w in np.flatnonzero(want_flags == 0):
        assert tw.same_bits(out[w], want[w]), (labels[w], np.argwhere(out[w] != want[w])[:4].tolist())


# ---- d. the serial parse between two frames on the fast plan ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("ch", [2, 8, 9])
def test_a_serial_parse_between_two_fast_frames(gpu, ch, form):  # noqa: F811
    """The long subframe has a dependant (2, 9 channels) or is one (8): the serial parse of these kernels with a type-1 subframe
    in the frame.  Two windows share the serial frame: each has its own residue slot in the workspace."""
    labels, stream, offs, pcm, _, levels, _, _ = _wanted("serial", ch)
    lib = capi.lib()
    lib.sela_hip_debug_decode_recurrence(form)
    try:
        st, _ = _levels(gpu, "serial", ch, tc.N)
        assert st.tolist() == [0, 0, int((levels["peak"] != 0).any(1).sum()), FAST], st
        assert _digest(gpu, "serial", ch, tc.N).tolist() == [0, 0, 0, FAST]
        assert _envelope(gpu, "serial", ch, tc.N, 256).tolist() == [0, 0, 0, FAST]
        if ch <= 8:
            t = _Table(gpu, stream, offs, ch)
            windows, ws = [(0, 0, 3), (1000, 0, 3), (tc.N + 100, 0, 3), (tc.N + 100, 0, 3), (2 * tc.N - 1, 0, 3)], 3000
            assert sum(1 for r in _touched(windows, ws, 3) if 1 in r) == 5
            for fmt in (I16, F32):
                _, out, flags, status = tw.device_call(t, windows, ws, fmt)
                want = tw.as_format(_cut(pcm.reshape(-1, ch), windows, ws), fmt)
                assert tw.same_bits(out, want), (fmt, np.argwhere(out != want)[:6].tolist())
                assert not flags.any() and status.tolist() == [0, 0, 0, 0]
    finally:
        lib.sela_hip_debug_decode_recurrence(-1)
