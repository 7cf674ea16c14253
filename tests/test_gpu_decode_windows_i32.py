"""sela_hip_decode_windows_i32_device and sela_hip_decode_windows_i32: sample windows of streams whose samples are
wider than 16 bits, in int32 planar, int32 interleaved, packed 3-byte and float.

Tables of 3 .. 5 frames of 2048 samples are built on the host.  The expectation for a healthy frame is the reference's (or the
oracle's) frame_decode_i32 of that frame alone, cross-checked against codec.Decoder32 at stride 2048 -- never the new call; for a
malformed frame it is zeros and the flag the header names.  Every case goes through the raw device call (0xA5 guards round every
buffer, the inputs compared afterwards), through codec.WindowDecoder32 and through the host call; all comparisons are exact.

The combine's rule is that a difference's parent is WRITTEN before it: independent subframes first, then dependent ones in subframe
order, as frame::FrameDecoder combines them.  So a difference subframe that merely stands in front of its independent parent is
a layout the reference decodes, and the window holds the reference's values
(test_a_difference_in_front_of_its_parent_is_the_reference_s_frame); the layout that is refused is a difference whose parent is a
difference that is written behind it ("difference_before_its_parent" among the malformed frames)."""
import struct

import numpy as np
import pytest

from gpu_common import _build_frame, _signal, _subframe_words, gpu  # noqa: F401
from oracle_lib import oracle, reference
from sela_amd import capi, codec
from sela_amd.synth import synth_frames
from test_gpu_pcm import _music24, pack_interleaved

pytestmark = pytest.mark.gpu

BLOCK = 2048
F32, I32, PCM24, PCM32 = capi.WINDOW_F32_PLANAR, capi.WINDOW_I32_PLANAR, capi.WINDOW_PCM24_INTERLEAVED, capi.WINDOW_PCM32_INTERLEAVED
FORMATS = (I32, PCM32, PCM24, F32)
EFORMAT, ERANGE = -5, -6
BAD, DRY, QRANGE, COEF = capi.FLAG_BAD_FRAME, capi.FLAG_RICE_OVERRUN, capi.FLAG_Q_RANGE, capi.FLAG_COEF_OVERFLOW
GUARD = 64  # bytes of 0xA5 in front of and behind every buffer (a multiple of 8: the views keep their alignment)
STREAM_CAP = 1072  # words: a subframe of at most this many is parsed in one piece, a longer one by segments
ARGS = ("d_frames", "d_frame_offsets", "n_frames_total", "channels", "d_windows", "n_windows", "window_samples", "format", "sample_bits", "d_out", "d_window_flags",
        "d_status", "d_workspace", "workspace_bytes", "stream")


def _ref():
    return reference() or oracle()


def cover(ws):
    return (ws + 2046) // 2048 + 1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def guarded(torch, data_or_bytes):
    """-> (the whole tensor, the exact-size view inside 0xA5 guards); data: a numpy array copied in, or a byte count left as 0xA5"""
    nbytes = data_or_bytes if isinstance(data_or_bytes, int) else data_or_bytes.nbytes
    big = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    view = big[GUARD: GUARD + nbytes]
    if not isinstance(data_or_bytes, int) and nbytes:
        view.copy_(torch.from_numpy(np.ascontiguousarray(data_or_bytes).view(np.uint8).reshape(-1)))
    return big, view


def guards_intact(big, nbytes):
    g = big.cpu().numpy()
    return bool((g[:GUARD] == 0xA5).all() and (g[GUARD + nbytes:] == 0xA5).all())


class Table32:
    """A frame table on the device inside guards, and per frame what a window holds of it: the reference's decode of a healthy
    frame, zeros and `declined[f]` (its flags) for a malformed one.  pad[f]: junk bytes behind frame f inside its table entry."""

    def __init__(self, torch, blobs, ch, declined=None, pad=None):
        self.torch, self.ch, self.n = torch, ch, len(blobs)
        self.declined = dict(declined or {})
        pad = dict(pad or {})
        self.blobs = [bytes(b) for b in blobs]
        entries = [b + b"\xEE" * pad.get(f, 0) for f, b in enumerate(self.blobs)]
        self.sizes = [len(e) for e in entries]
        self.stream = np.frombuffer(b"".join(entries), np.uint8).copy()
        self.offs = np.cumsum([0] + self.sizes).astype(np.uint64)
        self.big_frames, self.d_frames = guarded(torch, self.stream)
        self.big_offs, d_offs = guarded(torch, self.offs)
        self.d_offs = d_offs.view(torch.int64)
        self.frames = np.zeros((self.n, ch, BLOCK), np.int32)
        for f, b in enumerate(self.blobs):
            if f in self.declined:
                continue
            dec, used = _ref().frame_decode_i32(b, ch)
            assert used == len(b) and all(len(d) == BLOCK for d in dec), f
            self.frames[f] = np.stack(dec)
        self.pcm = np.ascontiguousarray(self.frames.transpose(0, 2, 1)).reshape(self.n * BLOCK, ch)  # [sample, channel] of the whole table

    def cross_check(self):
        """codec.Decoder32 at stride 2048 writes the same values for the healthy frames (one frame at a time: a malformed one beside
        them must not cost them their route)."""
        torch = self.torch
        one = codec.Decoder32(1, self.ch, BLOCK)
        for f in range(self.n):
            if f in self.declined:
                continue
            samples, counts, _ = one.decode(self.d_frames, self.d_offs[f: f + 2], 1)
            torch.cuda.synchronize()
            one.check()
            assert (counts.cpu().numpy() == BLOCK).all() and np.array_equal(samples.cpu().numpy()[0], self.frames[f]), f

    def words(self):
        """cw + 2 + rw of every subframe of the healthy frames"""
        return [w for f, b in enumerate(self.blobs) if f not in self.declined for w in _subframe_words(b, self.ch)]

    def touched(self, start, first, n, ws):
        n_eff = min(n, self.n - first) if first < self.n else 0
        q = start // BLOCK
        if q >= n_eff:
            return range(0)
        last = q + (start % BLOCK + ws - 1) // BLOCK
        return range(first + q, first + min(last + 1, n_eff))

    def expect(self, windows, ws):
        """-> (int32 [n, ws, ch], flags uint32 [n], status[0..2])"""
        out = np.zeros((len(windows), ws, self.ch), np.int32)
        flags = np.zeros(len(windows), np.uint32)
        bad = 0
        for w, (start, first, n) in enumerate(windows):
            n_eff = min(n, self.n - first) if first < self.n else 0
            stream = self.pcm[first * BLOCK: (first + n_eff) * BLOCK]
            if start < len(stream):
                seg = stream[start: start + ws]
                out[w, : len(seg)] = seg
            for f in self.touched(start, first, n, ws):
                flags[w] |= self.declined.get(f, 0)
                bad += 1 if self.declined.get(f, 0) & BAD else 0
        return out, flags, (int(np.bitwise_or.reduce(flags)) if len(flags) else 0, bad, int((flags != 0).sum()))


def as_format(want, fmt, bits):
    """int32 [n, ws, ch] -> what the format holds"""
    if fmt == PCM32:
        return want
    if fmt == PCM24:
        return pack_interleaved(want, 3).reshape(want.shape + (3,))
    planar = np.ascontiguousarray(want.transpose(0, 2, 1))
    if fmt == I32:
        return planar
    return planar.astype(np.float32) * np.float32(2.0 ** -(bits - 1))  # (int32 -> float32 rounds to nearest-even)


def wide_count(want, fmt):
    return int(((want < -(1 << 23)) | (want >= (1 << 23))).sum()) if fmt == PCM24 else 0


def pack(windows):
    return codec.WindowDecoder32.pack([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])


def device_call(table, windows, ws, fmt=I32, bits=24, with_flags=True, expect_rc=0, **override):
    """The raw C ABI on fresh buffers inside 0xA5 guards -> (out in the format's shape, flags or None, status uint32 [4]); after a
    refusal (expect_rc) every buffer still holds its sentinel.  Guards and inputs are checked here."""
    torch, lib = table.torch, capi.lib()
    n, ch = len(windows), table.ch
    shape, dtype = codec._window32_shape(n, ws, ch, fmt)
    out_bytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    big_out, d_out = guarded(torch, out_bytes)
    big_flags, d_flags = guarded(torch, 4 * n)
    big_status, d_status = guarded(torch, 16)
    big_win, d_windows = guarded(torch, pack(windows))
    need = int(lib.sela_hip_decode_windows_i32_workspace_bytes(n, ws, ch))
    big_ws, d_ws = guarded(torch, need)
    frames_before, offs_before, windows_before = table.big_frames.clone(), table.big_offs.clone(), big_win.clone()
    args = dict(d_frames=table.d_frames.data_ptr(), d_frame_offsets=table.d_offs.data_ptr(), n_frames_total=table.n, channels=ch, d_windows=d_windows.data_ptr(),
                n_windows=n, window_samples=ws, format=fmt, sample_bits=bits, d_out=d_out.data_ptr(), d_window_flags=d_flags.data_ptr() if with_flags else None,
                d_status=d_status.data_ptr(), d_workspace=d_ws.data_ptr(), workspace_bytes=need, stream=torch.cuda.current_stream().cuda_stream)
    args.update(override)
    rc = lib.sela_hip_decode_windows_i32_device(*[args[k] for k in ARGS])
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.sela_hip_last_error())
    assert torch.equal(table.big_frames, frames_before) and torch.equal(table.big_offs, offs_before) and torch.equal(big_win, windows_before), "an input was written"
    for big, nbytes, name in ((big_out, out_bytes, "d_out"), (big_flags, 4 * n, "d_window_flags"), (big_status, 16, "d_status"), (big_ws, need, "the workspace")):
        assert guards_intact(big, nbytes), "written around " + name
    if rc != 0:
        for big in (big_out, big_flags, big_status, big_ws):
            assert (big.cpu().numpy() == 0xA5).all(), "a refused call wrote"
        return None
    if not with_flags:
        assert (d_flags.cpu().numpy() == 0xA5).all()
    out = d_out.cpu().numpy().view(dtype).reshape(shape).copy()
    return out, (d_flags.cpu().numpy().view(np.uint32).copy() if with_flags else None), d_status.cpu().numpy().view(np.uint32).copy()


def check(table, windows, ws, fmt=I32, bits=24):
    """The three ways in against the expectation -> the expectation's (flags, status[0..2])."""
    torch = table.torch
    want32, want_flags, want_status = table.expect(windows, ws)
    want = as_format(want32, fmt, bits)
    full_status = want_status + (wide_count(want32, fmt),)
    for with_flags in (True, False):
        out, flags, status = device_call(table, windows, ws, fmt, bits, with_flags=with_flags)
        assert same_bits(out, want), (fmt, ws, np.argwhere(out != want)[:8])
        assert flags is None or np.array_equal(flags, want_flags), (flags, want_flags)
        assert tuple(int(x) for x in status) == full_status, (status, full_status)
    wd = codec.WindowDecoder32(len(windows), ws, table.ch, fmt, sample_bits=bits)
    got = wd.decode(table.d_frames, table.d_offs, table.n, torch.from_numpy(pack(windows)).cuda())
    torch.cuda.synchronize()
    assert same_bits(got.cpu().numpy(), want)
    assert np.array_equal(wd.flags.cpu().numpy().view(np.uint32), want_flags)
    assert tuple(int(x) for x in wd.status.cpu().numpy().view(np.uint32)) == full_status and wd.wide_samples() == full_status[3]
    if want_status[0] == 0:
        wd.check()
    else:
        with pytest.raises(capi.SelaHipError):
            wd.check()
    hout, hflags, rc = codec.decode_windows_i32_host(table.stream, table.offs, table.ch, pack(windows), ws, fmt, sample_bits=bits)
    assert same_bits(hout, want) and np.array_equal(hflags, want_flags), np.argwhere(hout != want)[:8]
    assert rc == (0 if want_status[0] == 0 else EFORMAT if want_status[0] & (BAD | DRY) else ERANGE), (rc, want_status)
    return want_flags, want_status


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def _blobs(planar, paired=False):
    """int32 [n_frames, ch, 2048] -> the frames' bytes: the reference's encoder per frame, or the library's paired encode"""
    if paired:
        frames, offs = codec.encode_i32(planar, paired=True)
        return [frames[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(len(offs) - 1)]
    return [_ref().frame_encode_i32(p) for p in planar]


def _planar(interleaved):
    return np.ascontiguousarray(np.asarray(interleaved, np.int32).transpose(0, 2, 1))


def _signals():
    rng = np.random.default_rng(523)
    same = _music24(4, 1, 9)
    same = np.concatenate([same, same - rng.integers(-2, 3, same.shape).astype(np.int32)], axis=2)  # the second channel follows the first: the difference is stored
    tones28 = np.stack([np.stack([_signal(rng, "tone", BLOCK, 27), _signal(rng, "tone", BLOCK, 27)], axis=1) for _ in range(3)])
    three = np.stack([np.stack([_signal(rng, k, BLOCK, 21) for k in ("tone", "noise", "sparse")], axis=1) for _ in range(3)])
    eight = _music24(3, 8, 4)
    eight[:, :, 1::2] = eight[:, :, 0::2] + rng.integers(-40, 41, eight[:, :, 1::2].shape).astype(np.int32)  # pairs worth pairing
    return {
        "mono24": (_planar(_music24(5, 1, 5)), 1, 24, False), "stereo24": (_planar(_music24(5, 2, 6)), 2, 24, False), "same24": (_planar(same), 2, 24, False),
        "tones28": (_planar(tones28), 2, 28, False), "three": (_planar(three), 3, 24, False), "eight_paired": (_planar(eight), 8, 24, True),
        "range16": (_planar(synth_frames(4, 2, 8).astype(np.int32)), 2, 16, False),
    }


SIGNALS = _signals()
_TABLES = {}


@pytest.fixture(scope="module")
def tables(gpu):  # noqa: F811
    def get(name):
        if name not in _TABLES:
            planar, ch, bits, paired = SIGNALS[name]
            t = Table32(gpu, _blobs(planar, paired), ch)
            t.cross_check()
            t.bits = bits
            _TABLES[name] = t
        return _TABLES[name]

    return get


def edge_windows(n):
    """starts at 0, 1, 2047, 2048, 2049, the last sample, the end, the end + 1 and 2^63 of the table's one stream; streams that
    start inside the table, run past its end, hold no frame; windows that overlap, repeat and come in no order"""
    end = n * BLOCK
    w = [(s, 0, n) for s in (0, 1, 2047, 2048, 2049, end - 1, end, end + 1, 2 ** 63)]
    w += [(5, 1, n - 1), (2047, 1, 2), (BLOCK + 3, 1, 0xFFFFFFFF), (0, n - 1, 9), (7, 2, 0), (0, n, 1), (5, 0xFFFFFFFF, 0xFFFFFFFF)]
    w += [(2047, 0, n), (2040, 0, n), (0, 0, n), (2 ** 64 - 1, 0, n), (end - 2, 0, n)]
    return w


def subframe_types(blob, ch):
    """the type byte (1: a difference) of every subframe of one frame"""
    out, p = [], 4
    for _ in range(ch):
        out.append(blob[p + 1])
        cw = struct.unpack_from("<H", blob, p + 4)[0]
        rw = struct.unpack_from("<H", blob, p + 7 + 4 * cw + 1)[0]
        p += 12 + 4 * (cw + rw)
    return out


def test_the_tables_hold_subframes_on_both_sides_of_the_parser_s_plan(tables):
    words = [w for name in SIGNALS for w in tables(name).words()]
    assert min(words) <= STREAM_CAP < max(words), (min(words), max(words))
    assert all(subframe_types(b, 2) == [0, 1] for b in tables("same24").blobs)  # the difference subframe is stored
    assert any(1 in subframe_types(b, 8) for b in tables("eight_paired").blobs)  # ... and so is a pair's


@pytest.mark.parametrize("ws", [1, 2, 3, 5, 2047, 2048, 2049, 4097])
def test_every_window_length_and_every_format_on_stereo_music(tables, ws):
    t = tables("stereo24")
    for fmt in FORMATS:
        flags, status = check(t, edge_windows(t.n), ws, fmt, 24)
        assert status == (0, 0, 0)


@pytest.mark.parametrize("name", ["mono24", "same24", "tones28", "three", "eight_paired", "range16"])
def test_every_table_in_every_format(tables, name):
    t = tables(name)
    for ws, fmt in ((5, I32), (2049, I32), (2049, PCM32), (777, PCM24), (2049, F32)):
        flags, status = check(t, edge_windows(t.n), ws, fmt, t.bits)
        assert status == (0, 0, 0)
    if name == "tones28":  # samples beyond 24 bits: counted where they go out as three bytes, and only there
        want32, _, _ = t.expect(edge_windows(t.n), 777)
        assert wide_count(want32, PCM24) > 1000
        check(t, edge_windows(t.n), 777, F32, 32)
        check(t, edge_windows(t.n), 777, F32, 28)


@pytest.mark.parametrize("name", list(SIGNALS))
def test_every_subframe_by_segments(tables, name):
    """sela_hip_debug_standard_first(2): no subframe is parsed in one piece, and the windows are the same."""
    t = tables(name)
    lib = capi.lib()
    lib.sela_hip_debug_standard_first(2)
    try:
        check(t, edge_windows(t.n), 2049, I32, t.bits)
        check(t, edge_windows(t.n), 5, PCM24, t.bits)
    finally:
        lib.sela_hip_debug_standard_first(-1)


@pytest.mark.parametrize("name,ws", [("mono24", 1), ("mono24", 3), ("mono24", 5), ("three", 5)])
def test_packed_windows_start_at_all_four_byte_phases(tables, name, ws):
    t = tables(name)
    windows = edge_windows(t.n)
    assert {(w * ws * t.ch * 3) % 4 for w in range(len(windows))} == {0, 1, 2, 3}
    check(t, windows, ws, PCM24, 24)


def test_no_windows_and_refusals_leave_every_buffer_alone(tables):
    t = tables("stereo24")
    for fmt in FORMATS:
        out, flags, status = device_call(t, [], 777, fmt)  # n_windows = 0: zero status words and nothing else
        assert out.size == 0 and len(flags) == 0 and not status.any()
    out, flags, rc = codec.decode_windows_i32_host(t.stream, t.offs, 2, np.zeros((0, 2), np.int64), 777, PCM24)
    assert rc == 0 and out.shape == (0, 777, 2, 3) and len(flags) == 0
    windows = edge_windows(t.n)[:4]
    for override in (dict(channels=9), dict(format=capi.WINDOW_I16_INTERLEAVED), dict(format=5), dict(format=F32, sample_bits=0), dict(format=F32, sample_bits=33),
                     dict(window_samples=0), dict(window_samples=(1 << 24) + 1), dict(workspace_bytes=1000)):
        device_call(t, windows, 777, expect_rc=-4 if "workspace_bytes" in override else -2, **override)
    big, view = guarded(t.torch, 4 * 777 * 2 * 4 + 8)  # d_out two bytes off a dword
    device_call(t, windows, 777, expect_rc=-2, d_out=view.data_ptr() + 2)
    assert (big.cpu().numpy() == 0xA5).all()


# ---- malformed frames in the middle of a healthy table --------------------------------------------------------------------------------
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


def patch_header(blob, sub, **fields):
    """the frame with the channel / type / parent byte of subframe `sub` replaced"""
    b, p = bytearray(blob), 4
    for _ in range(sub):
        cw = struct.unpack_from("<H", b, p + 4)[0]
        rw = struct.unpack_from("<H", b, p + 7 + 4 * cw + 1)[0]
        p += 12 + 4 * (cw + rw)
    for name, value in fields.items():
        b[p + ("channel", "type", "parent").index(name)] = value
    return bytes(b)


def _crafted(kats):
    """name -> (the malformed frame for a stereo table, its flags)"""
    rng = np.random.default_rng(77)
    q = kats["blk/sine_deg/q"]
    res = lambda n=BLOCK: rng.integers(-60000, 60000, n)  # noqa: E731
    good = _build_frame([(0, 0, 0, q, res()), (1, 0, 1, q, res())])
    sync = bytearray(good)
    sync[0] ^= 0xFF
    dry = patch_n(_build_frame([(0, 0, 0, q, res()), (1, 0, 1, q, res(BLOCK - 100))]), BLOCK, sub=1)  # 1948 codewords and the last word's padding for 2048 values
    return {
        "bad_sync": (bytes(sync), BAD), "cut_short": (good[:-8], BAD), "says_2047": (patch_n(good, 2047, sub=1), BAD),
        "channel_8": (patch_header(good, 1, channel=8), BAD), "missing_parent": (patch_header(good, 1, type=1, parent=5), BAD),
        # both are differences, each against the other: whichever is combined first, its parent has not been written
        "difference_before_its_parent": (patch_header(patch_header(good, 0, type=1, parent=1), 1, type=1, parent=0), BAD),
        "dry_rice": (dry, DRY), "q_out_of_range": (_build_frame([(0, 0, 0, q, res()), (1, 0, 1, np.array([100, -3, 7], np.int32), res())]), QRANGE),
    }


MALFORMED = ["bad_sync", "cut_short", "says_2047", "channel_8", "missing_parent", "difference_before_its_parent", "dry_rice", "q_out_of_range"]
# the bad frame is frame 2 of five: windows into it, across its two borders, beside it, and twice the same
BAD_WINDOWS = [(2 * BLOCK + 100, 0, 5), (2 * BLOCK - 50, 0, 5), (3 * BLOCK - 50, 0, 5), (BLOCK - 10, 0, 5), (3 * BLOCK + 10, 0, 5), (2 * BLOCK + 100, 0, 5), (0, 2, 1),
               (BLOCK + 1000, 0, 2), (2047, 1, 3), (4 * BLOCK, 0, 5)]


@pytest.mark.parametrize("kind", MALFORMED)
def test_one_malformed_frame_costs_its_share_and_no_other(tables, kats, kind):
    good = tables("stereo24")
    frame, flag = _crafted(kats)[kind]
    t = Table32(good.torch, good.blobs[:2] + [frame] + good.blobs[3:], 2, declined={2: flag})
    t.cross_check()
    for ws, fmt in ((300, I32), (2049, PCM24), (300, PCM32), (5, F32)):
        want32, want_flags, want_status = t.expect(BAD_WINDOWS, ws)
        if ws == 300:
            assert not want32[0].any() and want32[1, :50].any() and not want32[1, 50:].any() and not want32[2, :50].any() and want32[2, 50:].any()
            assert want32[3].any() and want32[4].any() and [int(f) for f in want_flags] == [flag, flag, flag, 0, 0, flag, flag, 0, flag, 0]
            assert want_status == (flag, 6 if flag == BAD else 0, 6)
        check(t, BAD_WINDOWS, ws, fmt, 24)


def test_a_frame_at_an_offset_that_is_no_multiple_of_four(tables, kats):
    """Frame 1 (a bad sync word) has two junk bytes behind it, so its entry is 4m + 2 bytes and frames 2 and 3 -- healthy frames of
    whole words, sync word and all -- sit at offsets of 4k + 2.  Nothing but the offset is wrong with them: they are not walked,
    their shares are zeros and each (window, frame) decode raises BAD_FRAME.  The device call, WindowDecoder32 and a host call
    whose batch stages frames 0 .. 3 (the offsets stay what they are) agree.  A host call whose batch stages frame 2 ALONE puts it
    at offset 0 of the staged table, where it is a healthy frame: include/sela_hip.h says so, and this holds it to that."""
    good = tables("stereo24")
    sync, _ = _crafted(kats)["bad_sync"]
    t = Table32(good.torch, [good.blobs[0], sync, good.blobs[2], good.blobs[3]], 2, declined={1: BAD, 2: BAD, 3: BAD}, pad={1: 2})
    assert all(len(b) % 4 == 0 for b in t.blobs) and t.sizes[1] % 4 == 2 and t.sizes[2] % 4 == 0 and t.sizes[3] % 4 == 0
    assert [int(o) % 4 for o in t.offs] == [0, 0, 2, 2, 2]
    t.cross_check()
    windows = [(0, 0, 4), (BLOCK - 50, 0, 4), (2 * BLOCK + 100, 0, 4), (3 * BLOCK - 50, 0, 4), (0, 2, 1), (0, 3, 1), (3 * BLOCK + 10, 0, 9)]
    for ws, fmt in ((300, I32), (300, PCM24)):
        want32, want_flags, want_status = t.expect(windows, ws)
        assert [int(f) for f in want_flags] == [0, BAD, BAD, BAD, BAD, BAD, BAD] and want32[0].any() and want32[1, :50].any() and not want32[1:, 50:].any()
        assert want_status == (BAD, 7, 6)
        check(t, windows, ws, fmt, 24)  # (the host call stages frames 0 .. 3: windows 0 and 1 cover frames 0 and 1)
    out, flags, rc = codec.decode_windows_i32_host(t.stream, t.offs, 2, pack([(0, 2, 1), (BLOCK - 300, 2, 1)]), 300, PCM32)
    assert int(capi.lib().sela_hip_debug_windows_staged_bytes()) == t.sizes[2]
    assert rc == 0 and not flags.any() and same_bits(out[0], good.pcm[2 * BLOCK: 2 * BLOCK + 300]) and same_bits(out[1], good.pcm[3 * BLOCK - 300: 3 * BLOCK])


def test_a_difference_in_front_of_its_parent_is_the_reference_s_frame(tables, kats):
    """Subframe 0 is channel 1 as a difference against channel 0, subframe 1 is channel 0: frame::FrameDecoder combines independent
    subframes first, so the parent is written before the difference is resolved, and the window holds the reference's values."""
    good = tables("stereo24")
    rng = np.random.default_rng(78)
    q = kats["blk/sine_deg/q"]
    frame = _build_frame([(1, 1, 0, q, rng.integers(-900, 900, BLOCK)), (0, 0, 0, q, rng.integers(-60000, 60000, BLOCK))])
    t = Table32(good.torch, [good.blobs[0], frame, good.blobs[1]], 2)
    t.cross_check()
    assert t.frames[1].any() and not np.array_equal(t.frames[1][0], t.frames[1][1])
    flags, status = check(t, [(BLOCK - 5, 0, 3), (BLOCK + 700, 0, 3), (0, 1, 1), (2 * BLOCK - 3, 0, 3)], 300, I32)
    assert status == (0, 0, 0)


# ---- capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [I32, PCM24])
def test_a_captured_call_reads_the_descriptors_at_replay(tables, fmt):
    t = tables("stereo24")
    torch = t.torch
    first = [(0, 0, 5), (BLOCK + 100, 0, 5), (500, 1, 2), (5 * BLOCK - 5, 0, 5)]
    second = [(3, 0, 5), (4 * BLOCK + 1500, 0, 5), (2 * BLOCK - 5, 0, 3), (2 * BLOCK - 5, 3, 9)]
    wd = codec.WindowDecoder32(4, 777, 2, fmt)
    d_windows = torch.from_numpy(pack(first)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wd.decode(t.d_frames, t.d_offs, t.n, d_windows)  # one plain call first
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = wd.decode(t.d_frames, t.d_offs, t.n, d_windows)
    for windows in (first, second):
        d_windows.copy_(torch.from_numpy(pack(windows)))
        wd.out.fill_(0x5E), wd.window_flags.fill_(-1), wd.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want32, want_flags, want_status = t.expect(windows, 777)
        assert same_bits(out.cpu().numpy(), as_format(want32, fmt, 24))
        assert np.array_equal(wd.flags.cpu().numpy().view(np.uint32), want_flags)
        assert tuple(int(x) for x in wd.status.cpu().numpy().view(np.uint32)) == want_status + (0,)


# ---- the host call stages the covering frames ---------------------------------------------------------------------------------------
def test_host_call_stages_the_covering_frames_and_no_others(tables):
    lib = capi.lib()
    t = tables("stereo24")
    for windows, frames in (([(BLOCK + 100, 0, 5)], [1]), ([(2 * BLOCK - 5, 0, 5)], [1, 2]), ([(100, 3, 2), (100, 3, 2), (4 * BLOCK - 1, 0, 5)], [3, 4]),
                            ([(5 * BLOCK, 0, 5)], []), ([(0, 4, 1), (2047, 0, 1)], [0, 4])):
        want32, want_flags, _ = t.expect(windows, 300)
        out, flags, rc = codec.decode_windows_i32_host(t.stream, t.offs, 2, pack(windows), 300, PCM32)
        assert rc == 0 and same_bits(out, want32) and not flags.any()
        assert int(lib.sela_hip_debug_windows_staged_bytes()) == sum(t.sizes[f] for f in frames), (windows, frames)
