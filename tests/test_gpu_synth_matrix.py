"""Every compiled copy of the decoder's synthesis (sela_synth.h and sela_decode_core.inc are compiled into each kernel's own
translation unit) on the hard cases of tests/synth_cases.py, in both recurrence forms: every order across the step-up's seams,
the three ring / group classes, the hand-over from the folded to the exact form in block 0, in an odd and an even block and in
the last one, samples that leave the folded range, a predictor that never fits the fold -- each parsed just in time and parked in
the workspace, at 2048 samples and at run-time lengths.

  kernel                   forms                        how the form is set
  k_decode_frames          0, 1                         sela_hip_debug_decode_recurrence
  k_decode_frames_wide     0, 1                         the same hook (9 and 10 channels)
  k_verify_frames          0, 1                         the same hook (device pointers and the host call)
  k_window_frames          0, 1                         the same hook (int16 interleaved and float32 planar)
  k_tailwin_decode         one form (<true>)            whole-track windows: the long last frame, always parked by segments
  k_decode_subframes32     <true> (= 1), <false> (= 0)  by the launch's subframes alone: at most 2560, and above
  k_stage_lpc_decode, k_lpc_decode_any   one form       the control: a wrong case fails here too, a wrong kernel does not

Every expectation is the oracle's (tests/test_synth_cases.py shows what each case is); no GPU decoder is a reference here, and
every comparison is exact."""
import contextlib

import numpy as np
import pytest

import synth_cases as sc
from gpu_common import gpu  # noqa: F401
from sela_amd import capi, codec
from test_gpu_decode_windows import as_format, same_bits

pytestmark = pytest.mark.gpu

N = sc.N
FAST = 1
NO_DIFF = 0xFFFFFFFF
I16, F32 = capi.WINDOW_I16_INTERLEAVED, capi.WINDOW_F32_PLANAR
LONELY = 2560  # kLonelyWaves (sela_decode_core.inc)


@contextlib.contextmanager
def recurrence(form):
    lib = capi.lib()
    lib.sela_hip_debug_decode_recurrence(form)
    try:
        yield
    finally:
        lib.sela_hip_debug_decode_recurrence(-1)


def _on_device(torch, stream, offs):
    d_frames = torch.zeros(max(len(stream), 4), dtype=torch.uint8, device="cuda")
    d_frames[: len(stream)].copy_(torch.from_numpy(np.array(stream)))
    return d_frames, torch.from_numpy(np.array(offs).view(np.int64)).cuda()


def _decode16(torch, frames, ch):
    """sela_hip_decode_device on one launch -> (int16 [n, 2048, ch], status uint32 [4])"""
    stream, offs = sc.stream_of(frames)
    d_frames, d_offs = _on_device(torch, stream, offs)
    dec = codec.Decoder(len(frames), ch)
    pcm = dec.decode(d_frames, d_offs, len(frames))
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), dec.status.cpu().numpy().view(np.uint32)


def _same_pcm(got, frames, who):
    for i, f in enumerate(frames):
        bad = np.argwhere(got[i] != f.pcm)
        assert len(bad) == 0, (who, i, f.label, f.mode, len(bad), bad[:4].tolist())


# ---- k_decode_frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
def test_k_decode_frames(gpu, form):  # noqa: F811
    """All 2048-sample cases as stereo frames in ONE launch, a different hard subframe on either channel, every workspace-mode
    frame between two just-in-time frames: the oracle's int16 PCM, its flags as the launch's status (the extreme seam kinds
    raise COEF_OVERFLOW and nothing else does: the same launch without them reports nothing)."""
    frames = sc.stereo_frames()
    flags = 0
    for f in frames:
        flags |= f.flags
    assert flags == sc.COEF_OVERFLOW
    clean = [f for f in frames if f.flags == 0]
    with recurrence(form):
        got, status = _decode16(gpu, frames, 2)
        got_clean, status_clean = _decode16(gpu, clean, 2)
    _same_pcm(got, frames, ("k_decode_frames", form))
    _same_pcm(got_clean, clean, ("k_decode_frames, clean frames", form))
    assert status[:2].tolist() == [flags, 0] and status_clean[:2].tolist() == [0, 0], (status, status_clean)


# ---- k_decode_frames_wide -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("ch", sc.WIDE_CHANNELS)
def test_k_decode_frames_wide(gpu, ch, form):  # noqa: F811
    """Frames of 9 and 10 channels whose subframes cycle through the class x hand-over cases, two difference subframes under
    hand-over parents in the first, the last one parked in the workspace."""
    frames = sc.wide_frames(ch)
    with recurrence(form):
        got, status = _decode16(gpu, frames, ch)
    _same_pcm(got, frames, ("k_decode_frames_wide", ch, form))
    assert status[:2].tolist() == [0, 0], status


# ---- k_verify_frames ------------------------------------------------------------------------------------------------------------------
def _clean_stereo():
    return [f for f in sc.stereo_frames() if f.flags == 0]


def _plant_at(frame, i, where):
    """(sample, channel) of the value to change in frame i: in the channel of one of its cases, at that case's hand-over sample
    (a case without one: any sample), at the last lane of that block, at the frame's last sample"""
    c = i % frame.channels
    case = frame.cases[c]
    at = case.at if case.at is not None else (37 * case.order + i) % N
    return {"hand-over": at, "last lane": 64 * (at // 64) + 63, "last sample": N - 1}[where], c


def _planted(frames, want, where, parity):
    changed = want.copy()
    counts, first = np.zeros(len(frames), np.uint32), np.full(len(frames), NO_DIFF, np.uint32)
    for i, f in enumerate(frames):
        if i % 2 == parity:
            s, c = _plant_at(f, i // 2, where)
            changed[i, s, c] ^= 1
            counts[i], first[i] = 1, s * f.channels + c
    return changed, counts, first


@pytest.mark.parametrize("form", [0, 1])
def test_k_verify_frames(gpu, form):  # noqa: F811
    """Against the oracle's PCM no frame reports a difference.  One changed value in every other frame -- at the hand-over's
    sample, at that block's last lane, at sample 2047 -- is counted once and found at its index, and the frames between report
    nothing: the compare looks at the samples the hard block produced.  Device pointers, and once the host call."""
    torch = gpu
    frames = _clean_stereo()
    n = len(frames)
    stream, offs = sc.stream_of(frames)
    d_frames, d_offs = _on_device(torch, stream, offs)
    want = np.stack([f.pcm for f in frames])
    runs = [("the oracle's PCM", want, np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32))]
    for where in ("hand-over", "last lane", "last sample"):
        for parity in (0, 1):
            runs.append(((where, parity),) + _planted(frames, want, where, parity))
    with recurrence(form):
        ver = codec.Verifier(n, 2, N)
        for label, pcm, want_counts, want_first in runs:
            counts, first = ver.verify(d_frames, d_offs, n, torch.from_numpy(pcm).cuda())
            ver.check()
            counts, first = counts.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32)
            wrong = np.flatnonzero((counts != want_counts) | (first != want_first))
            assert len(wrong) == 0, (label, form, [(frames[i].label, int(counts[i]), int(first[i]), int(want_first[i])) for i in wrong[:4]])
            assert ver.status.cpu().numpy().view(np.uint32).tolist() == [0, 0, int((want_counts != 0).sum()), FAST], label
        for label, pcm, want_counts, want_first in runs[:2]:
            counts, first, lossy = codec.verify_host(stream, offs, 2, pcm)
            assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first) and lossy == int((want_counts != 0).sum()), (label, form, "host")


# ---- k_window_frames ------------------------------------------------------------------------------------------------------------------
def _expected_windows(pcm, windows, ws, bounds):
    """pcm int16 [samples of the table, ch], windows (start, first frame, frames), bounds: the table's sample offsets
    -> int16 [n, ws, ch]: the stream's samples from `start` on, zero behind its end"""
    out = np.zeros((len(windows), ws, pcm.shape[1]), np.int16)
    for w, (start, first, count) in enumerate(windows):
        stream = pcm[bounds[first]: bounds[first + count]]
        seg = stream[start: start + ws]
        out[w, : len(seg)] = seg
    return out


def _pack(windows):
    return codec.WindowDecoder.pack([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])


def _check_windows(torch, table, windows, ws, fmt, whole, who):
    stream, offs, d_frames, d_offs, pcm, bounds, ch = table
    n_table = len(offs) - 1
    want = as_format(_expected_windows(pcm, windows, ws, bounds), fmt)
    wd = codec.WindowDecoder(len(windows), ws, ch, planar_float=fmt == F32, whole=whole)
    got = wd.decode(d_frames, d_offs, n_table, torch.from_numpy(_pack(windows)).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert same_bits(got, want), (who, "device", np.argwhere(got != want)[:4].tolist())
    assert not wd.flags.cpu().numpy().any() and wd.status.cpu().numpy().tolist() == [0, 0, 0, 0], (who, wd.status)
    out, flags, rc = codec.decode_windows_host(stream, offs, ch, _pack(windows), ws, planar_float=fmt == F32, whole=whole)
    assert same_bits(out, want), (who, "host", np.argwhere(out != want)[:4].tolist())
    assert rc == 0 and not flags.any(), (who, rc)


def _table(torch, frames):
    stream, offs = sc.stream_of(frames)
    pcm = np.concatenate([f.pcm for f in frames])
    bounds = np.cumsum([0] + [f.n for f in frames])
    return (stream, offs) + _on_device(torch, stream, offs) + (pcm, bounds, frames[0].channels)


@pytest.mark.parametrize("fmt", [I16, F32], ids=["i16", "f32"])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("ch", [2, 1, 3])
def test_k_window_frames(gpu, ch, form, fmt):  # noqa: F811
    """The table is the hard frames (stereo; mono and three channels from the same cases), one stream.  Per frame: the whole
    frame; a crop from 7 samples in front of the hand-over block through the rest of the frame and 2050 samples and more into
    the frames behind; the hand-over sample alone.  The oracle's PCM, sliced on the host; float32 is int16 / 32768 by bytes."""
    frames = sc.hard_frames() if ch == 2 else sc.narrow_frames(ch)
    assert all(f.flags == 0 for f in frames)
    table = _table(gpu, frames)
    n = len(frames)
    spots = [_plant_at(f, i, "hand-over")[0] for i, f in enumerate(frames)]
    whole_frames = [(N * f, 0, n) for f in range(n)]
    crops = [(max(N * f + 64 * (spots[f] // 64) - 7, 0), 0, n) for f in range(n)]
    ones = [(N * f + spots[f], 0, n) for f in range(n)]
    with recurrence(form):
        for label, windows, ws in (("whole frames", whole_frames, N), ("crops", crops, 7 + N + 2050), ("one sample", ones, 1)):
            _check_windows(gpu, table, windows, ws, fmt, False, ("k_window_frames", ch, form, label))


# ---- k_tailwin_decode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [I16, F32], ids=["i16", "f32"])
@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo_diff"])
def test_k_tailwin_decode(gpu, ch, fmt):  # noqa: F811
    """Whole-track streams in one table: two ordinary 2048-sample frames and a hand-built last frame of 2049, 2113 and 4095
    samples, and single frames of 191 -- orders 61 and 100, folded throughout and with samples that leave the range in an odd
    and in an even block; mono, and stereo with a difference channel under the hard one.  All of the tail, a window across
    2048 (n - 1), and one inside the block of the departure.  The expectation for the last frame is the oracle's any-length
    decode, narrowed.  (The kernel is synthesize_by_order<true, true> on residues parked by segments: one form, one mode; the
    hook reaches only the 2048-sample frames in front, which k_window_frames decodes.)"""
    streams = sc.tail_streams(ch)
    stream = np.frombuffer(b"".join(b for s in streams for b in s.blobs), np.uint8).copy()
    offs = np.cumsum([0] + [len(b) for s in streams for b in s.blobs]).astype(np.uint64)
    pcm = np.concatenate([s.pcm for s in streams])
    firsts = np.cumsum([0] + [len(s.blobs) for s in streams])
    bounds = np.zeros(len(offs), np.int64)  # sample offsets of the table's frames
    tails, inside = [], []
    for i, s in enumerate(streams):
        first, count, n_last = int(firsts[i]), len(s.blobs), len(s.case.residues)
        base = N * (count - 1)
        bounds[first + 1: first + count + 1] = bounds[first] + np.array([N * (k + 1) for k in range(count - 1)] + [base + n_last])
        tails += [(b, first, count) for b in sorted({base, max(base - 10, 0)})]
        block = s.case.block if s.case.block is not None else (n_last - 1) // 64
        inside.append((min(base + 64 * block + 5, base + n_last - 1), first, count))
    assert bounds[-1] == len(pcm)
    table = (stream, offs) + _on_device(gpu, stream, offs) + (pcm, bounds, ch)
    _check_windows(gpu, table, tails, 4095, fmt, True, ("k_tailwin_decode", ch, "tails"))
    _check_windows(gpu, table, inside, 40, fmt, True, ("k_tailwin_decode", ch, "inside the block"))


# ---- k_decode_subframes32 -------------------------------------------------------------------------------------------------------------
STRIDE32 = 4095


def _frames32():
    """the clean stereo frames: 2048 samples and the run-time lengths"""
    return _clean_stereo() + list(sc.length_frames())


def _same32(samples, counts, frames, copies, who):
    """samples int32 [copies * n, 2, stride], counts [copies * n, 2]: every copy of every frame is the oracle's"""
    n = len(frames)
    samples, counts = samples.reshape(copies, n, 2, -1), counts.reshape(copies, n, 2)
    for i, f in enumerate(frames):
        assert (counts[:, i] == f.n).all(), (who, i, f.label)
        for c in range(2):
            wrong = np.argwhere(samples[:, i, c, : f.n] != f.wide[c][None])
            assert len(wrong) == 0, (who, i, f.label, c, len(wrong), wrong[:4].tolist())


@pytest.mark.parametrize("mode", [1, 2], ids=["product_parse", "by_segments"])
@pytest.mark.parametrize("tiled", [False, True], ids=["vec_shift", "scalar_shift"])
def test_k_decode_subframes32(gpu, tiled, mode):  # noqa: F811
    """launch_decode_subframes32 (sela_decode32.hip) picks <true> for at most 2560 subframes and <false> above, and no hook
    forces either.  The count it sees is n_frames * channels of ITS caller: on device pointers launch_any_length_subframes
    hands it the call's n_frames (FramesForm passes the argument of sela_hip_decode_i32_device, not a capacity); on host
    pointers generic_decode hands it one chunk, min(n_frames, 768 MiB / per-frame scratch) frames, which at this stride is
    every frame of the call (asserted below).  So the stream as it is runs <true>, and as many copies of it as make 2562
    subframes or more -- its bytes repeated, its offsets extended; the oracle decodes the distinct frames only -- run <false>:
    both counts are asserted against 2560.
    mode 1 is the product's parse (one piece for up to 2048 samples in up to 1072 words, segments for the rest), mode 2 every
    subframe by segments, the workspace mode of this kernel; on the host call the library's own counters say that the fast
    kernel decoded the chunk alone and how many subframes it parsed by segments."""
    torch, lib = gpu, capi.lib()
    frames = _frames32()
    copies = -(-(LONELY + 2) // (2 * len(frames))) if tiled else 1
    n = len(frames) * copies
    subframes = 2 * n
    assert (subframes >= LONELY + 2) if tiled else (subframes <= LONELY), subframes
    assert (768 << 20) // (2 * STRIDE32 * 8 + 2 * 64 + 16) >= n  # (the host call's chunk holds them all)
    one, one_offs = sc.stream_of(frames)
    stream = np.tile(one, copies)
    offs = np.concatenate([one_offs[:-1] + np.uint64(i * len(one)) for i in range(copies)] + [np.array([copies * len(one)], np.uint64)])
    by_segments = sum(1 for f in frames for w in sc._subframe_words(f.blob, 2) if mode == 2 or f.n > N or w > sc.PLAN_WORDS) * copies
    assert 0 < by_segments and (mode == 2 or by_segments < subframes)
    d_frames, d_offs = _on_device(torch, stream, offs)
    try:
        lib.sela_hip_debug_standard_first(mode)
        dec = codec.Decoder32(n, 2, STRIDE32)
        samples, counts, _ = dec.decode(d_frames, d_offs, n)
        dec.check()
        _same32(samples.cpu().numpy(), counts.cpu().numpy(), frames, copies, ("Decoder32", copies, mode))
        del samples, counts, dec
        chunks0, segs0 = lib.sela_hip_debug_standard_chunks(), lib.sela_hip_debug_segment_subframes()
        host = codec.decode_i32(stream, offs, 2, stride=STRIDE32)
        assert lib.sela_hip_debug_standard_chunks() - chunks0 == 1 and lib.sela_hip_debug_segment_subframes() - segs0 == by_segments
        for k in range(copies):
            for i, f in enumerate(frames):
                for c in range(2):
                    assert np.array_equal(host[k * len(frames) + i][c], f.wide[c]), ("decode_i32", copies, mode, k, i, f.label, c)
    finally:
        lib.sela_hip_debug_standard_first(-1)


# ---- the control ----------------------------------------------------------------------------------------------------------------------
def test_the_stage_kernels_on_the_same_cases(gpu):  # noqa: F811
    """k_stage_lpc_decode (sela_hip_lpc_decode) and k_lpc_decode_any (sela_hip_lpc_decode_n) have one form only: the subframes
    of the clean stereo frames, one block each.  A case that fails here as well is a wrong case, not a wrong frame kernel."""
    subs = [(f, c) for f in _clean_stereo() for c in range(2) if f.cases[c].res_k is None]  # (the workspace cases are the same subframes)
    orders = np.array([f.cases[c].order for f, c in subs], np.int32)
    q = np.zeros((len(subs), 100), np.int32)
    for b, (f, c) in enumerate(subs):
        q[b, : orders[b]] = f.cases[c].q
    res = np.stack([f.cases[c].residues for f, c in subs])
    for label, call in (("lpc_decode", codec.lpc_decode), ("lpc_decode_n", codec.lpc_decode_n)):
        got = call(orders, q, res)
        for b, (f, c) in enumerate(subs):
            assert np.array_equal(got[b], f.wide[c]), (label, f.label, c, int(np.flatnonzero(got[b] != f.wide[c])[0]))
