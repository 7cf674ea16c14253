"""sela_hip_decode_windows_whole_device and sela_hip_decode_windows_whole: sample windows of whole-track streams,
whose last frame L says 1 .. 4095 samples.  In front of L a window holds what sela_hip_decode_windows_device writes; inside L exactly
the int16 sela_hip_decode_n_device writes for that frame decoded alone; zero behind the stream's end S = 2048 (n - 1) + n_L.

Streams are built on the CPU with the oracle as tests/test_gpu_encode_whole.py builds them (encode_frames for the 2048-sample frames,
frame_encode for the last).  The expectation for a well-formed stream is codec.DecoderN on that stream alone, sliced and zero-padded
on the host, and for its last frame also the reference's (or the oracle's) frame_decode_i32, narrowed; all comparisons are exact.
Every case goes through the raw device call (guard elements around d_out, behind the flags and behind the status words, the
inputs compared afterwards), through codec.WindowDecoder(whole=True) and through the host call."""
import os
import struct
import subprocess

import numpy as np
import pytest

from gpu_common import HOST, _build, _build_frame, _write_wav, gpu  # noqa: F401
from oracle_lib import oracle, reference
from sela_amd import capi, codec
from sela_amd.synth import synth_frames
from test_gpu_decode_windows import Table, _encoded_blobs, _stereo_kinds, as_format, same_bits
from test_gpu_encode_whole import _expected, _layout, _track

pytestmark = pytest.mark.gpu

BLOCK = 2048
I16, F32 = capi.WINDOW_I16_INTERLEAVED, capi.WINDOW_F32_PLANAR
EFORMAT, ERANGE = -5, -6
BAD, DRY = capi.FLAG_BAD_FRAME, capi.FLAG_RICE_OVERRUN
GUARD = 63
SENT16, SENTF, SENT32 = 0x5E1A, 12345.0, 0x5E1A5E1A
ARGS = ("d_frames", "d_frame_offsets", "n_frames_total", "channels", "d_windows", "n_windows", "window_samples", "format", "d_out", "d_window_flags", "d_status",
        "d_workspace", "workspace_bytes", "stream")


def says(blob):
    """what a frame says its length is: its first subframe's samplesPerChannel (0: too short to hold that header)"""
    if len(blob) < 4 + 12:
        return 0
    cw = struct.unpack_from("<H", blob, 4 + 4)[0]
    at = 4 + 7 + 4 * cw
    return struct.unpack_from("<H", blob, at + 3)[0] if at + 5 <= len(blob) else 0


def tailed(n):
    return 1 <= n <= 4095 and n != BLOCK


def patch_n(blob, n, sub=0):
    """the frame with samplesPerChannel of subframe `sub` replaced"""
    b, p = bytearray(blob), 4
    for _ in range(sub):
        cw = struct.unpack_from("<H", b, p + 4)[0]
        rw = struct.unpack_from("<H", b, p + 7 + 4 * cw + 1)[0]
        p += 12 + 4 * (cw + rw)
    cw = struct.unpack_from("<H", b, p + 4)[0]
    struct.pack_into("<H", b, p + 7 + 4 * cw + 3, n)
    return bytes(b)


class WholeTable(Table):
    """A frame table, what the 2048-sample decoder makes of every frame (Table), and what sela_hip_decode_n_device makes of every
    frame that says a tail's length, decoded alone.  declined: {frame: flags} for the hostile frames, whose share is zeros."""

    def __init__(self, torch, blobs, ch, declined=None):
        super().__init__(torch, blobs, ch)
        self.blobs = [bytes(b) for b in blobs]
        self.says = [says(b) for b in self.blobs]
        self.declined = dict(declined or {})
        self.tail = {}
        one = codec.DecoderN(1, ch, 4095)
        for f, n in enumerate(self.says):
            if not tailed(n) or f in self.declined:
                continue
            pcm, so = one.decode(self.d_frames, self.d_offs[f: f + 2], 1)
            torch.cuda.synchronize()
            st = one.status.cpu().numpy().view(np.uint32)
            if int(st[0]) == 0 and int(st[3]) == 2 and int(so.cpu().numpy()[1]) == n:  # route 2, nothing flagged
                self.tail[f] = pcm.cpu().numpy()[:n].copy()
            # (anything else must not be a stream's last frame in a test, unless the test says what it is declined for: stream_of)

    def stream_of(self, first, n_frames):
        """-> (pcm int16 [S, ch], L or None when the stream has no long last frame, frames inside the table)"""
        n = min(n_frames, self.n - first) if first < self.n else 0
        if n == 0:
            return np.zeros((0, self.ch), np.int16), None, 0
        last = first + n - 1
        if not tailed(self.says[last]):
            return self.pcm[first * BLOCK: (first + n) * BLOCK], None, n
        assert last in self.tail or last in self.declined, last
        tail = self.tail.get(last, np.zeros((self.says[last], self.ch), np.int16))
        return np.concatenate([self.pcm[first * BLOCK: last * BLOCK], tail]), last, n

    def expect_whole(self, windows, ws):
        out = np.zeros((len(windows), ws, self.ch), np.int16)
        flags = np.zeros(len(windows), np.uint32)
        bad = 0
        for w, (start, first, n_frames) in enumerate(windows):
            pcm, last, n = self.stream_of(first, n_frames)
            if start < len(pcm):
                seg = pcm[start: start + ws]
                out[w, : len(seg)] = seg
            for f in self.touched(start, first, n - 1 if last is not None else n, ws):
                flags[w] |= self.frame_flags[f]
                bad += self.frame_bad[f]
            if last is not None and last in self.declined and start < len(pcm) and start + ws > (n - 1) * BLOCK:
                flags[w] |= self.declined[last]
                bad += 1 if self.declined[last] & BAD else 0
        return out, flags, (int(np.bitwise_or.reduce(flags)) if len(flags) else 0, bad, int((flags != 0).sum()))


def pack(windows):
    return codec.WindowDecoder.pack([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])


def device_call(table, windows, ws, fmt=I16, whole=True, with_flags=True):
    """The raw C ABI on fresh buffers full of sentinels -> (out, flags or None, status uint32 [4]); guards and inputs checked here."""
    torch, lib = table.torch, capi.lib()
    n, ch = len(windows), table.ch
    elems = n * ws * ch
    buf = torch.full((GUARD + elems + GUARD,), SENTF if fmt == F32 else SENT16, dtype=torch.float32 if fmt == F32 else torch.int16, device="cuda")
    d_flags = torch.full((n + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    d_status = torch.full((4 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    d_windows = torch.from_numpy(pack(windows)).cuda()
    sizing = lib.sela_hip_decode_windows_whole_workspace_bytes if whole else lib.sela_hip_decode_windows_workspace_bytes
    need = int(sizing(n, ws, ch))
    d_ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    frames_before, offs_before, windows_before = table.d_frames.clone(), table.d_offs.clone(), d_windows.clone()
    args = dict(d_frames=table.d_frames.data_ptr(), d_frame_offsets=table.d_offs.data_ptr(), n_frames_total=table.n, channels=ch, d_windows=d_windows.data_ptr(),
                n_windows=n, window_samples=ws, format=fmt, d_out=buf.data_ptr() + GUARD * buf.element_size(), d_window_flags=d_flags.data_ptr() if with_flags else None,
                d_status=d_status.data_ptr(), d_workspace=d_ws.data_ptr(), workspace_bytes=need, stream=torch.cuda.current_stream().cuda_stream)
    rc = (lib.sela_hip_decode_windows_whole_device if whole else lib.sela_hip_decode_windows_device)(*[args[k] for k in ARGS])
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.sela_hip_last_error())
    assert torch.equal(table.d_frames, frames_before) and torch.equal(table.d_offs, offs_before) and torch.equal(d_windows, windows_before), "an input was written"
    host = buf.cpu().numpy()
    sent = np.float32(SENTF) if fmt == F32 else np.int16(SENT16)
    assert (host[:GUARD] == sent).all() and (host[GUARD + elems:] == sent).all(), "written around d_out"
    flags, status = d_flags.cpu().numpy().view(np.uint32), d_status.cpu().numpy().view(np.uint32)
    assert (flags[n:] == SENT32).all() and (status[4:] == SENT32).all(), "written behind d_window_flags or d_status"
    assert (d_ws[need:].cpu().numpy() == 0xA5).all(), "written behind the workspace"
    if not with_flags:
        assert (flags == SENT32).all()
    body = host[GUARD: GUARD + elems]
    out = body.reshape(n, ch, ws) if fmt == F32 else body.reshape(n, ws, ch)
    return out.copy(), (flags[:n].copy() if with_flags else None), status[:4].copy()


def check(table, windows, ws, fmt=I16):
    """The three ways in against the expectation -> the expectation's (flags, status[0..2])."""
    torch = table.torch
    want16, want_flags, want_status = table.expect_whole(windows, ws)
    want = as_format(want16, fmt)
    out, flags, status = device_call(table, windows, ws, fmt)
    assert same_bits(out, want), np.argwhere(out != want)[:8]
    assert np.array_equal(flags, want_flags), (flags, want_flags)
    assert tuple(int(x) for x in status) == want_status + (0,), (status, want_status)
    wd = codec.WindowDecoder(len(windows), ws, table.ch, planar_float=fmt == F32, whole=True)
    got = wd.decode(table.d_frames, table.d_offs, table.n, torch.from_numpy(pack(windows)).cuda())
    torch.cuda.synchronize()
    assert same_bits(got.cpu().numpy(), want)
    assert np.array_equal(wd.flags.cpu().numpy().view(np.uint32), want_flags)
    assert tuple(int(x) for x in wd.status.cpu().numpy().view(np.uint32)) == want_status + (0,)
    if want_status[0] == 0:
        wd.check()
    else:
        with pytest.raises(capi.SelaHipError):
            wd.check()
    hout, hflags, rc = codec.decode_windows_host(table.stream, table.offs, table.ch, pack(windows), ws, planar_float=fmt == F32, whole=True)
    assert same_bits(hout, want) and np.array_equal(hflags, want_flags), np.argwhere(hout != want)[:8]
    assert rc == (0 if want_status[0] == 0 else EFORMAT if want_status[0] & (BAD | DRY) else ERANGE), (rc, want_status)
    return want_flags, want_status


def blobs_of(n, ch, k):
    data, offs = _expected(n, ch, k)
    return [data[int(offs[f]): int(offs[f + 1])] for f in range(len(offs) - 1)]


def second_subframe_type(frame):
    cw = struct.unpack_from("<H", frame, 4 + 4)[0]
    rw = struct.unpack_from("<H", frame, 4 + 7 + 4 * cw + 1)[0]
    return frame[4 + 12 + 4 * (cw + rw) + 1]


# ---- well-formed tailed streams -----------------------------------------------------------------------------------------------------
# 2 frames + a tail of t (a last frame of 2048 + t); one long frame alone; one short frame alone; whole frames only (t = 0)
SHAPES = [3 * BLOCK + 1, 3 * BLOCK + 77, 3 * BLOCK + 2047, BLOCK + 5, 700, 3 * BLOCK]
# (channels, k of test_gpu_encode_whole._track: for odd k the second channel follows the first and the difference wins)
TRACKS = [(1, 0), (2, 0), (2, 1), (3, 0)]


@pytest.mark.parametrize("ch,k", TRACKS, ids=["mono", "stereo", "stereo_diff", "three"])
@pytest.mark.parametrize("n", SHAPES)
def test_windows_of_a_well_formed_whole_track_stream(gpu, n, ch, k):  # noqa: F811
    blobs = blobs_of(n, ch, k)
    whole, last = _layout(n)
    t = WholeTable(gpu, blobs, ch)
    assert not any(t.frame_flags[:whole])
    pcm, L, frames = t.stream_of(0, len(blobs))
    assert len(pcm) == n and frames == len(blobs) and (L is None) == (last == 0)
    # the expectation is the any-length decoder on the stream alone (route 2 for a tailed stream, the 2048-sample decoder for t = 0) ...
    dn = codec.DecoderN(len(blobs), ch, 4095)
    alone, so = dn.decode(t.d_frames, t.d_offs, len(blobs))
    gpu.cuda.synchronize()
    dn.check()
    assert int(so.cpu().numpy()[len(blobs)]) == n and np.array_equal(alone.cpu().numpy()[:n], pcm)
    if last:  # ... and for the last frame the reference's frame decoder, narrowed
        dec, used = (reference() or oracle()).frame_decode_i32(blobs[-1], ch, stride=last)
        assert used == len(blobs[-1]) and np.array_equal(np.stack(dec, axis=1).astype(np.int16), pcm[whole * BLOCK:])
        assert np.array_equal(pcm[whole * BLOCK:], _track(n, ch, k)[whole * BLOCK:])  # (none of these frames has a rounding tie)
        if ch == 2:
            assert second_subframe_type(blobs[-1]) == k
    base = whole * BLOCK if last else (whole - 1) * BLOCK  # 2048 (n - 1)
    starts = sorted({0, max(base - 300, 0), max(base - 1, 0), base, base + 1, max(n - 40, 0), max(n - 2, 0), n - 1, n, n + 1, n + 5000, 2 ** 40 + base, 2 ** 64 - 1})
    for ws in (1, 777, 2050, 5000):
        for fmt in (I16, F32):
            flags, status = check(t, [(s, 0, len(blobs)) for s in starts], ws, fmt)
            assert status == (0, 0, 0)
    want, _, _ = t.expect_whole([(n - 1, 0, len(blobs)), (n, 0, len(blobs))], 5)
    assert not want[0, 1:].any() and not want[1].any() and np.array_equal(want[0, 0], _track(n, ch, k)[n - 1])


# ---- several streams in one table ---------------------------------------------------------------------------------------------------
def test_a_tailed_stream_a_plain_one_and_one_that_runs_past_the_table(gpu):  # noqa: F811
    a = blobs_of(3 * BLOCK + 77, 2, 1)        # frames 0 .. 2: two of 2048 and a last one of 2125
    b = blobs_of(3 * BLOCK, 2, 0)             # frames 3 .. 5: plain
    c = blobs_of(BLOCK + 5, 2, 0)             # frame 6: one long frame alone
    t = WholeTable(gpu, a + b + c, 2)
    sa, sb = 2 * BLOCK + 2125, 3 * BLOCK
    rng = np.random.default_rng(520)
    windows = [(int(s), 0, 3) for s in rng.integers(0, sa + 300, 12)] + [(int(s), 3, 3) for s in rng.integers(0, sb + 300, 12)]
    windows += [(2 * BLOCK - 10, 0, 3), (2 * BLOCK - 10, 0, 3), (sa - 1, 0, 3), (sa, 0, 3), (0, 6, 1), (2000, 6, 1), (2052, 6, 1), (2053, 6, 1)]
    windows += [(3 * BLOCK - 100, 3, 0xFFFFFFFF), (BLOCK - 5, 5, 9), (3 * BLOCK + 3, 3, 4), (0, 7, 1), (5, 0xFFFFFFFF, 0xFFFFFFFF), (0, 2, 0)]  # cut at the table's end: frame 6 is the last
    windows += [(BLOCK + 700, 0, 2), (2 * BLOCK + 5, 0, 6), (2 * BLOCK + 5, 2, 1), (100, 2, 1)]  # the long frame mid-stream is no tail: BAD_FRAME; alone it is one
    order = rng.permutation(len(windows))
    windows = [windows[i] for i in order]
    for fmt in (I16, F32):
        flags, status = check(t, windows, 1000, fmt)
    mid = windows.index((2 * BLOCK + 5, 0, 6))
    assert int(flags[mid]) & BAD and status[1:] == (1, 1)
    alone = windows.index((100, 2, 1))
    want, _, _ = t.expect_whole(windows, 1000)
    assert want[alone].any() and not flags[alone]
    past = windows.index((3 * BLOCK - 100, 3, 0xFFFFFFFF))  # frames 3 .. 6: the plain stream and the long frame behind it make one whole-track stream
    assert want[past, 100:].any()
    check(t, windows[:9], 2050)


# ---- tables of 2048-sample frames only: every word is the existing call's -----------------------------------------------------------
def identical(table, windows, ws, fmt):
    for with_flags in (True, False):
        a = device_call(table, windows, ws, fmt, whole=True, with_flags=with_flags)
        b = device_call(table, windows, ws, fmt, whole=False, with_flags=with_flags)
        assert same_bits(a[0], b[0]) and a[2].tobytes() == b[2].tobytes() and (a[1] is None or a[1].tobytes() == b[1].tobytes()), (a[1:], b[1:])
    return a


@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_a_table_of_2048_sample_frames_gives_the_existing_call_s_words(gpu, ch):  # noqa: F811
    t = Table(gpu, _encoded_blobs(gpu, synth_frames(5, ch, 40 + ch)), ch)
    windows = [(s, 0, 5) for s in (0, 1, 777, 2047, 2048, 4095, 9000, 10239, 10240, 2 ** 64 - 1)] + [(3, 1, 3), (2 * BLOCK - 2, 1, 3), (0, 4, 9), (0, 5, 1), (7, 2, 0)]
    for ws, fmt in ((1, I16), (777, I16), (777, F32), (2050, I16), (5000, F32)):
        identical(t, windows, ws, fmt)


@pytest.mark.parametrize("kind", ["sync", "short"])
def test_malformed_2048_sample_tables_give_the_existing_call_s_words(gpu, kats, kind):  # noqa: F811
    """tests/test_gpu_decode_windows.py's construction: a broken sync word, and a frame whose second subframe says 1000 samples."""
    indep, dep0, diff = _stereo_kinds(kats)
    if kind == "sync":
        bad = bytearray(indep)
        bad[0] ^= 0xFF
        bad = bytes(bad)
    else:
        rng = np.random.default_rng(9)
        q = kats["blk/sine_deg/q"]
        bad = _build_frame([(0, 0, 0, q, rng.integers(-60, 60, BLOCK)), (1, 0, 1, q, rng.integers(-60, 60, 1000))])
    for blobs in ([indep, diff, dep0, bad, indep], [indep, diff, bad]):  # the bad frame inside a stream, and as its last frame
        t = Table(gpu, blobs, 2)
        n = len(blobs)
        windows = [(0, 0, n), (2 * BLOCK + 1900, 0, n), (3 * BLOCK - 1, 0, n), (3 * BLOCK + 5, 0, n), (2 * BLOCK - 150, 0, n), (BLOCK, 0, 3), (0, n - 1, 1), (2047, 1, 4)]
        out, flags, status = identical(t, windows, 150, I16)
        identical(t, windows, 2050, F32)
        assert status[0] & BAD and status[2] >= 2


# ---- hostile last frames ------------------------------------------------------------------------------------------------------------
def hostile_table(gpu, last, declined=None, ch=2, patch_mid=None):  # noqa: F811
    """frames 0, 1: a good stream's 2048-sample frames; 2: `last`; 3 .. 5: a good tailed stream beside it"""
    good = blobs_of(3 * BLOCK + 77, ch, 1)
    head = list(good[:2])
    if patch_mid is not None:
        head[1] = patch_n(head[1], patch_mid)
    return WholeTable(gpu, head + [last] + good, ch, declined={2: declined} if declined else None), good


HOSTILE_WINDOWS = [(2 * BLOCK - 100, 0, 3), (2 * BLOCK + 10, 0, 3), (2 * BLOCK + 2100, 0, 3), (100, 0, 3), (BLOCK + 100, 0, 3),
                   (2 * BLOCK - 100, 3, 3), (2 * BLOCK + 2100, 3, 3), (2 * BLOCK + 10, 0, 3), (2 ** 64 - 1, 0, 3)]
GOOD = [5, 6]  # the good stream's windows into its tail


def run_hostile(t):
    """-> (flags, status[0..2]) of the batch at 300 samples a window"""
    for ws, fmt in ((2050, I16), (300, F32), (300, I16)):
        want, want_flags, want_status = t.expect_whole(HOSTILE_WINDOWS, ws)
        assert all(want[w].any() and want_flags[w] == 0 for w in GOOD)  # the good windows beside the hostile ones come out exact
        flags, status = check(t, HOSTILE_WINDOWS, ws, fmt)
    return flags, status


@pytest.mark.parametrize("n_last", [0, 4096, 65535])
def test_a_last_frame_that_says_no_tail_s_length_gets_what_the_existing_call_writes(gpu, n_last):  # noqa: F811
    good = blobs_of(3 * BLOCK + 77, 2, 1)
    t, _ = hostile_table(gpu, patch_n(good[2], n_last))
    assert t.says[2] == n_last and t.frame_flags[2] & BAD
    flags, status = run_hostile(t)
    assert [int(f) & BAD for f in flags[:3]] == [BAD, BAD, 0] and status[2] == 3  # (the third starts behind 2048 n: it touches nothing)
    # ... which is, word for word, the existing call's on the hostile stream's windows
    for fmt in (I16, F32):
        identical(t, [w for w in HOSTILE_WINDOWS if w[1] == 0], 300, fmt)


def test_a_frame_in_front_of_the_last_that_says_2049(gpu):  # noqa: F811
    good = blobs_of(3 * BLOCK + 77, 2, 1)
    t, _ = hostile_table(gpu, good[2], patch_mid=2049)
    assert t.says[1] == 2049 and t.frame_flags[1] & BAD and 2 in t.tail
    flags, status = run_hostile(t)
    # frame 1 costs the windows that touch it; the last frame is decoded all the same
    assert [bool(f) for f in flags] == [True, False, False, False, True, False, False, False, False]
    want, _, _ = t.expect_whole(HOSTILE_WINDOWS, 300)
    assert not want[0, :100, 0].any() and want[0, 100:].any() and want[1].any() and want[2, :25].any() and not want[2, 25:].any()


def test_channels_that_disagree_about_the_length(gpu):  # noqa: F811
    good = blobs_of(3 * BLOCK + 77, 2, 1)
    t, _ = hostile_table(gpu, patch_n(good[2], 2124, sub=1), declined=BAD)
    flags, status = run_hostile(t)
    assert [int(f) for f in flags] == [BAD, BAD, BAD, 0, 0, 0, 0, BAD, 0] and status[1:] == (4, 4)
    want, _, _ = t.expect_whole(HOSTILE_WINDOWS, 300)
    assert want[0, :100].any() and not want[0, 100:].any() and not want[1].any()


def test_a_last_frame_cut_short_in_the_table(gpu):  # noqa: F811
    good = blobs_of(3 * BLOCK + 77, 2, 1)
    t, _ = hostile_table(gpu, good[2][:-8], declined=BAD)
    flags, status = run_hostile(t)
    assert [int(f) for f in flags] == [BAD, BAD, BAD, 0, 0, 0, 0, BAD, 0]
    # the same frame as the table's last: nothing behind its bytes is read (the device buffer ends with it)
    t2 = WholeTable(gpu, blobs_of(3 * BLOCK + 77, 2, 1) + good[:2] + [good[2][:-8]], 2, declined={5: BAD})
    flags, status = check(t2, [(2 * BLOCK + 10, 3, 3), (2 * BLOCK + 10, 0, 3), (BLOCK, 3, 9)], 300)
    assert [int(f) for f in flags] == [BAD, 0, 0]
    # ... and one too short to hold a header says nothing: the existing call's zeros and BAD_FRAME
    t3 = WholeTable(gpu, blobs_of(3 * BLOCK + 77, 2, 1) + good[:2] + [good[2][:12]], 2)
    assert t3.says[5] == 0
    check(t3, [(2 * BLOCK + 10, 3, 3), (2 * BLOCK + 10, 0, 3), (2 * BLOCK - 10, 3, 3)], 300)
    identical(t3, [(2 * BLOCK + 10, 3, 3), (2 * BLOCK - 10, 3, 3)], 300, I16)


def test_a_residue_stream_that_runs_dry(gpu, kats):  # noqa: F811
    rng = np.random.default_rng(77)
    q = kats["blk/sine_deg/q"]
    frame = _build_frame([(0, 0, 0, q, rng.integers(-60, 60, 3000)), (1, 0, 1, q, rng.integers(-60, 60, 2900))])
    frame = patch_n(frame, 3000, sub=1)  # 2900 codewords and the padding of the last word for 3000 values
    t, _ = hostile_table(gpu, frame, declined=DRY)
    assert t.says[2] == 3000
    flags, status = run_hostile(t)
    assert [int(f) for f in flags] == [DRY, DRY, DRY, 0, 0, 0, 0, DRY, 0] and status[1] == 0 and status[2] == 4
    # with the stream whole the frame is a tail like any other
    ok = WholeTable(gpu, [_build_frame([(0, 0, 0, q, rng.integers(-60, 60, 3000)), (1, 0, 1, q, rng.integers(-60, 60, 3000))])], 2)
    flags, status = check(ok, [(0, 0, 1), (2500, 0, 1), (2999, 0, 1), (3000, 0, 1)], 777)
    assert status == (0, 0, 0)


# ---- capture ------------------------------------------------------------------------------------------------------------------------
def test_a_captured_whole_call_reads_the_descriptors_at_replay(gpu):  # noqa: F811
    torch = gpu
    t = WholeTable(gpu, blobs_of(3 * BLOCK + 77, 2, 1), 2)
    first = [(0, 0, 3), (BLOCK + 100, 0, 3), (500, 0, 3), (2 * BLOCK - 5, 0, 2)]
    second = [(0, 0, 3), (2 * BLOCK + 1500, 0, 3), (2 * BLOCK - 5, 0, 3), (2 * BLOCK - 5, 0, 2)]  # the second window moves from the middle into the tail
    wd = codec.WindowDecoder(4, 777, 2, whole=True)
    d_windows = torch.from_numpy(pack(first)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wd.decode(t.d_frames, t.d_offs, t.n, d_windows)  # one plain call: what the library asks the runtime once per kernel is asked here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = wd.decode(t.d_frames, t.d_offs, t.n, d_windows)
    for windows in (first, second):
        d_windows.copy_(torch.from_numpy(pack(windows)))
        wd.out.fill_(SENT16), wd.window_flags.fill_(-1), wd.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.cpu().numpy().copy(), wd.flags.cpu().numpy().copy(), wd.status.cpu().numpy().copy()
        eager, eflags, estatus = device_call(t, windows, 777)
        assert same_bits(replayed[0], eager) and np.array_equal(replayed[1].view(np.uint32), eflags) and np.array_equal(replayed[2].view(np.uint32), estatus)
        assert same_bits(eager, t.expect_whole(windows, 777)[0])
    assert eager[1, :600].any() and not eager[1, 702:].any()


# ---- the host call stages the covering frames ---------------------------------------------------------------------------------------
def test_host_call_stages_the_last_frame_for_windows_inside_the_tail(gpu):  # noqa: F811
    lib = capi.lib()
    blobs = blobs_of(3 * BLOCK + 77, 2, 1)
    t = WholeTable(gpu, _encoded_blobs(gpu, synth_frames(6, 2, 77)) + blobs, 2)
    for windows, frames in (([(2 * BLOCK + 2100, 6, 3)], [8]), ([(2 * BLOCK + 2125, 6, 3)], [8]), ([(2 * BLOCK - 5, 6, 3)], [7, 8]), ([(100, 6, 3), (3 * BLOCK, 0, 6)], [3, 6]),
                            ([(2 * BLOCK + 2100, 6, 3), (2 * BLOCK + 100, 6, 3), (5, 2, 2)], [2, 8])):
        want, want_flags, _ = t.expect_whole(windows, 300)
        out, flags, rc = codec.decode_windows_host(t.stream, t.offs, 2, pack(windows), 300, whole=True)
        assert rc == 0 and same_bits(out, want) and not flags.any()
        assert int(lib.sela_hip_debug_windows_staged_bytes()) == sum(t.sizes[f] for f in frames), (windows, frames)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def test_cli_decodes_ranges_in_and_around_the_tail_of_a_keep_tail_file(gpu, tmp_path):  # noqa: F811
    _build()
    cli = os.path.join(HOST, "sela_mi355x")
    n = 4 * BLOCK + 777
    pcm = np.ascontiguousarray(_track(n, 2, 1))
    wav, sela = tmp_path / "in.wav", tmp_path / "in.sela"
    _write_wav(wav, pcm)
    r = subprocess.run([cli, "-e", "--keep-tail", "--lossless", str(wav), str(sela)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    base = 3 * BLOCK  # the last frame holds samples 3 * 2048 .. n
    for k, (start, count) in enumerate(((base - 500, 1000), (base - 1, 2), (base, 2825), (base + 2000, 700), (n - 1, 1), (n - 100, 100), (0, n), (BLOCK + 5, n), (n - 3, 10 ** 9))):
        out = tmp_path / f"r{k}.wav"
        r = subprocess.run([cli, "-d", "--start", str(start), "--count", str(count), str(sela), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, (start, count, r.stdout, r.stderr)
        data = open(out, "rb").read()
        got = np.frombuffer(data[44:], np.int16).reshape(-1, 2)
        want = pcm[start: min(start + count, n)]  # a count past the end is cut at S
        assert struct.unpack_from("<I", data, 40)[0] == want.size * 2 and np.array_equal(got, want), (start, count, got.shape)
    for start in (n, n + 1, 5 * BLOCK):
        out = tmp_path / "past.wav"
        r = subprocess.run([cli, "-d", "--start", str(start), "--count", "10", str(sela), str(out)], capture_output=True, text=True)
        assert r.returncode == 1 and "past the end" in (r.stdout + r.stderr) and str(n) in (r.stdout + r.stderr) and not out.exists(), (start, r.stdout, r.stderr)
