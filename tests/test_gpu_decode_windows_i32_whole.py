"""sela_hip_decode_windows_i32_whole_device and sela_hip_decode_windows_i32_whole: sample windows of 24- and 32-bit
whole-track streams -- 2048-sample frames and one last frame of 1 .. 4095 samples -- in the four formats of the 32-bit windows.

Streams are made by the reference (or the oracle), never by the code under test; expected samples are its frame_decode_i32 per
frame, concatenated and cut.  One table per channel count holds several streams: a 2048-sample frame followed by a tail of every
length at which the store's rounds of 256 change, and two one-frame streams.  Every case goes through the raw device call (0xA5
guards round every buffer, the whole output buffer compared: no byte outside a share is written), through codec.WindowDecoder32
and through the host call.  All comparisons are exact."""
import numpy as np
import pytest

import whole_pcm_cases as W
from gpu_common import _build_frame, gpu  # noqa: F401
from sela_amd import capi, codec
from test_gpu_decode_windows_i32 import (ARGS, BAD, BLOCK, DRY, EFORMAT, ERANGE, F32, FORMATS, I32, PCM24, PCM32, Table32, _crafted, as_format, edge_windows, guarded,
                                         guards_intact, pack, patch_n, same_bits, wide_count)
from test_gpu_decode_windows_i32 import device_call as plain_device_call

pytestmark = pytest.mark.gpu

TAILS = (2049, 2048 + 255, 2048 + 256, 2048 + 257, 4095)
SHORT = (300, 2047)


def tail_length(n):
    return 1 <= n <= 4095 and n != BLOCK


def says(blob):
    """what a frame says its length is: its first subframe's samplesPerChannel (0: no such header)"""
    import struct

    if len(blob) < 4 + 12:
        return 0
    cw = struct.unpack_from("<H", blob, 4 + 4)[0]
    at = 4 + 7 + 4 * cw + 3
    return struct.unpack_from("<H", blob, at)[0] if at + 2 <= len(blob) else 0


class WholeTable:
    """A frame table on the device inside guards.  Per frame: what it says its length is, the reference's decode of it (None for
    a frame given in `declined`: frame -> the flags it raises wherever it is met, as a 2048-sample frame or as a tail)."""

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
        self.says = [says(b) for b in self.blobs]
        self.dec = []
        for f, b in enumerate(self.blobs):
            if f in self.declined:
                self.dec.append(None)
                continue
            dec, used = W.ref().frame_decode_i32(b, ch, stride=4096)
            assert used == len(b) and all(len(d) == self.says[f] for d in dec), f
            self.dec.append(np.stack(dec, axis=1))  # [sample, channel]

    def body(self, f):
        """(2048 samples of frame f as the 2048-sample decoder hands them out, its flags)"""
        if self.dec[f] is not None and self.says[f] == BLOCK:
            return self.dec[f], 0
        return np.zeros((BLOCK, self.ch), np.int32), self.declined.get(f, BAD)  # (a healthy frame of another length: BAD_FRAME)

    def expect(self, windows, ws, whole=True):
        """-> (int32 [n, ws, ch], flags uint32 [n], status[0..2]) by the header's rule"""
        out = np.zeros((len(windows), ws, self.ch), np.int32)
        flags = np.zeros(len(windows), np.uint32)
        bad = 0
        for w, (start, first, n) in enumerate(windows):
            n_eff = min(n, self.n - first) if first < self.n else 0
            if n_eff == 0:
                continue
            last = first + n_eff - 1
            tail = whole and tail_length(self.says[last])
            n_body = n_eff - 1 if tail else n_eff
            q = start // BLOCK
            for f in range(first + q, first + min(q + (start % BLOCK + ws - 1) // BLOCK + 1, n_body)) if q < n_body else ():
                x, fl = self.body(f)
                at = (f - first) * BLOCK - start  # the frame's first sample in the window
                lo, hi = max(at, 0), min(at + BLOCK, ws)
                out[w, lo:hi] = x[lo - at: hi - at]
                flags[w] |= fl
                bad += 1 if fl & BAD else 0
            base = BLOCK * (n_eff - 1)
            if tail and start < base + self.says[last] and start + ws > base:
                at = base - start
                lo, hi = max(at, 0), min(at + self.says[last], ws)
                if self.dec[last] is not None:
                    out[w, lo:hi] = self.dec[last][lo - at: hi - at]
                else:
                    flags[w] |= self.declined[last]
                    bad += 1 if self.declined[last] & BAD else 0
        return out, flags, (int(np.bitwise_or.reduce(flags)) if len(flags) else 0, bad, int((flags != 0).sum()))


def device_call(table, windows, ws, fmt=I32, bits=24, with_flags=True):
    """The raw C ABI on fresh buffers inside 0xA5 guards -> (out in the format's shape, flags or None, status uint32 [4])"""
    torch, lib = table.torch, capi.lib()
    n, ch = len(windows), table.ch
    shape, dtype = codec._window32_shape(n, ws, ch, fmt)
    out_bytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    big_out, d_out = guarded(torch, out_bytes)
    big_flags, d_flags = guarded(torch, 4 * n)
    big_status, d_status = guarded(torch, 16)
    big_win, d_windows = guarded(torch, pack(windows))
    need = int(lib.sela_hip_decode_windows_i32_whole_workspace_bytes(n, ws, ch))
    big_ws, d_ws = guarded(torch, need)
    frames_before, offs_before, windows_before = table.big_frames.clone(), table.big_offs.clone(), big_win.clone()
    args = dict(d_frames=table.d_frames.data_ptr(), d_frame_offsets=table.d_offs.data_ptr(), n_frames_total=table.n, channels=ch, d_windows=d_windows.data_ptr(),
                n_windows=n, window_samples=ws, format=fmt, sample_bits=bits, d_out=d_out.data_ptr(), d_window_flags=d_flags.data_ptr() if with_flags else None,
                d_status=d_status.data_ptr(), d_workspace=d_ws.data_ptr(), workspace_bytes=need, stream=torch.cuda.current_stream().cuda_stream)
    rc = lib.sela_hip_decode_windows_i32_whole_device(*[args[k] for k in ARGS])
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.sela_hip_last_error())
    assert torch.equal(table.big_frames, frames_before) and torch.equal(table.big_offs, offs_before) and torch.equal(big_win, windows_before), "an input was written"
    for big, nbytes, name in ((big_out, out_bytes, "d_out"), (big_flags, 4 * n, "d_window_flags"), (big_status, 16, "d_status"), (big_ws, need, "the workspace")):
        assert guards_intact(big, nbytes), "written around " + name
    if not with_flags:
        assert (d_flags.cpu().numpy() == 0xA5).all()
    out = d_out.cpu().numpy().view(dtype).reshape(shape).copy()
    return out, (d_flags.cpu().numpy().view(np.uint32).copy() if with_flags else None), d_status.cpu().numpy().view(np.uint32).copy()


def check(table, windows, ws, fmt=I32, bits=24, host=True):
    """The three ways in against the expectation -> the expectation's (int32 windows, flags, status[0..2])."""
    torch = table.torch
    want32, want_flags, want_status = table.expect(windows, ws)
    want = as_format(want32, fmt, bits)
    full_status = want_status + (wide_count(want32, fmt),)
    for with_flags in (True, False):
        out, flags, status = device_call(table, windows, ws, fmt, bits, with_flags=with_flags)
        assert same_bits(out, want), (fmt, ws, np.argwhere(out != want)[:8])
        assert flags is None or np.array_equal(flags, want_flags), (flags, want_flags)
        assert tuple(int(x) for x in status) == full_status, (status, full_status)
    wd = codec.WindowDecoder32(len(windows), ws, table.ch, fmt, sample_bits=bits, whole=True)
    got = wd.decode(table.d_frames, table.d_offs, table.n, torch.from_numpy(pack(windows)).cuda())
    torch.cuda.synchronize()
    assert same_bits(got.cpu().numpy(), want)
    assert np.array_equal(wd.flags.cpu().numpy().view(np.uint32), want_flags)
    assert tuple(int(x) for x in wd.status.cpu().numpy().view(np.uint32)) == full_status and wd.wide_samples() == full_status[3]
    if host:
        hout, hflags, rc = codec.decode_windows_i32_host(table.stream, table.offs, table.ch, pack(windows), ws, fmt, sample_bits=bits, whole=True)
        assert same_bits(hout, want) and np.array_equal(hflags, want_flags), np.argwhere(hout != want)[:8]
        assert rc == (0 if want_status[0] == 0 else EFORMAT if want_status[0] & (BAD | DRY) else ERANGE), (rc, want_status)
    return want32, want_flags, want_status


# ---- the tables: per channel count [F, T2049, F, T2303, F, T2304, F, T2305, F, T4095, T300, T2047] -------------------------------------
def _frame(n, ch, b, k):
    return W.ref().frame_encode_i32(np.ascontiguousarray(W.track(n, ch, b, k).T))


_TABLES = {}


@pytest.fixture(scope="module")
def tables(gpu):  # noqa: F811
    def get(ch, b=3):
        if (ch, b) not in _TABLES:
            body = _frame(BLOCK, ch, b, 2)
            blobs = []
            for i, n_l in enumerate(TAILS):
                blobs += [body, _frame(n_l, ch, b, i)]
            blobs += [_frame(n, ch, b, 1) for n in SHORT]
            _TABLES[(ch, b)] = WholeTable(gpu, blobs, ch)
        return _TABLES[(ch, b)]

    return get


def tail_windows():
    """per stream of a body frame and a tail: windows that start in front of the tail and end inside it, lie wholly inside it, run
    past S, start at and past S and near 2^64; the same for the one-frame streams; streams cut at the table's end"""
    w = []
    for i, n_l in enumerate(TAILS):
        s = BLOCK + n_l
        w += [(x, 2 * i, 2) for x in (0, BLOCK - 5, BLOCK, BLOCK + 10, BLOCK + 255, s - 300, s - 3, s - 1, s, s + 5, 2 ** 64 - 1, 2 ** 64 - 777)]
    for j, n_l in enumerate(SHORT):
        w += [(x, 2 * len(TAILS) + j, 1) for x in (0, 100, n_l - 1, n_l, 2 ** 64 - 1)]
    w += [(BLOCK + 7, 8, 2), (3, 11, 0xFFFFFFFF), (0, 12, 1), (5, 0xFFFFFFFF, 0xFFFFFFFF), (9, 3, 0)]
    return w


@pytest.mark.parametrize("ws", [1, 777, 4097])
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_every_format_at_every_round_length(tables, ch, ws):
    t = tables(ch)
    windows = tail_windows()
    for fmt in FORMATS:
        want32, flags, status = check(t, windows, ws, fmt, 24)
        assert status == (0, 0, 0)
    if ws == 777:  # the windows do what their names say
        assert want32[1, :5].any() and want32[1, 5:].any() and want32[3].any() and want32[6, :3].any() and not want32[6, 3:].any() and not want32[8].any()
        assert not want32[10].any()


def test_a_frame_in_front_of_the_tail_that_says_another_length(tables):
    """One stream over the whole table: its last frame (2047 samples) is the tail; every frame in front that does not say 2048 is
    the 2048-sample decoder's to refuse -- among them one that says 2049."""
    t = tables(2)
    assert t.says[1] == 2049
    windows = [(0, 0, 12), (BLOCK - 5, 0, 12), (BLOCK + 100, 0, 4), (2 * BLOCK - 5, 0, 12), (11 * BLOCK - 5, 0, 12), (11 * BLOCK + 2040, 0, 100), (10 * BLOCK + 100, 9, 100)]
    for fmt in (I32, PCM24):
        want32, flags, status = check(t, windows, 300, fmt, 24)
        assert [int(f) for f in flags] == [0, BAD, BAD, BAD, BAD, 0, 0] and status == (BAD, 4, 4)
        assert want32[4, 5:].any() and not want32[4, :5].any() and want32[5, :7].any() and not want32[5, 7:].any()


def test_packed_shares_start_at_all_four_byte_phases(tables):
    """channels = 3 and an odd window length: window w starts at byte 9 * 777 * w, its share of the tail at byte 9 * (777 w + lo).
    The whole output buffer is compared, guards included: no byte outside a share is written."""
    t = tables(3)
    ws = 777
    windows = [(BLOCK - lo, 2 * i, 2) for i in range(len(TAILS)) for lo in (0, 1, 2, 3, 5, 776)] + [(BLOCK + TAILS[0] - k, 0, 2) for k in (1, 1, 1, 1, 2)]
    assert {(w * ws * 9) % 4 for w in range(len(windows))} == {0, 1, 2, 3}
    assert {((w * ws + BLOCK - s) * 9) % 4 for w, (s, _, _) in enumerate(windows) if s <= BLOCK} == {0, 1, 2, 3}
    assert {((w * ws + TAILS[0] + BLOCK - s) * 9) % 4 for w, (s, _, _) in enumerate(windows) if s > BLOCK} == {0, 1, 2, 3}  # ... and where it ends
    check(t, windows, ws, PCM24, 24)
    check(t, windows[::-1], 5, PCM24, 24)


def test_samples_beyond_24_bits_are_counted_in_the_tail_and_in_front(tables):
    t = tables(2, 4)  # 27-bit samples
    windows = [(BLOCK - 100, 0, 2), (BLOCK + 50, 2, 2), (0, 10, 1), (BLOCK + 3000, 8, 2)]
    want32, flags, status = check(t, windows, 777, PCM24, 32)
    wide = lambda x: int(((x < -(1 << 23)) | (x >= (1 << 23))).sum())  # noqa: E731
    assert wide(want32[0, :100]) > 0 and wide(want32[0, 100:]) > 0 and wide(want32[1]) > 0 and wide(want32[2]) > 0  # in front of the tail, and in it
    for fmt in (I32, PCM32, F32):
        check(t, windows, 777, fmt, 27)


def test_difference_coded_tails(tables, kats):
    """A tail whose second subframe is a difference against the first (the reference's stereo decision), and a hand-built one whose
    difference stands in front of its parent: independent subframes are combined first."""
    import struct

    t = tables(2)
    types = [W.second_subframe_type(t.blobs[2 * i + 1]) for i in range(len(TAILS))]
    assert set(types) == {0, 1}, types
    rng = np.random.default_rng(78)
    q = kats["blk/sine_deg/q"]
    n_l = 2500
    frame = _build_frame([(1, 1, 0, q, rng.integers(-900, 900, n_l)), (0, 0, 0, q, rng.integers(-60000, 60000, n_l))])
    assert struct.unpack_from("<BBB", frame, 4) == (1, 1, 0)
    t2 = WholeTable(t.torch, [t.blobs[0], frame], 2)
    assert t2.dec[1].any() and not np.array_equal(t2.dec[1][:, 0], t2.dec[1][:, 1])
    for fmt in (I32, PCM24):
        want32, flags, status = check(t2, [(BLOCK - 5, 0, 2), (BLOCK + 700, 0, 2), (0, 1, 1), (BLOCK + n_l - 3, 0, 2)], 300, fmt, 24)
        assert status == (0, 0, 0) and want32[1].any()


def _both_calls_agree(plain_table, windows, ws, fmt, bits=24):
    """word for word the existing i32 call's outputs, flags and status -- device and host"""
    p_out, p_flags, p_status = plain_device_call(plain_table, windows, ws, fmt, bits)
    out, flags, status = device_call(plain_table, windows, ws, fmt, bits)
    assert same_bits(out, p_out) and np.array_equal(flags, p_flags) and np.array_equal(status, p_status)
    h_plain = codec.decode_windows_i32_host(plain_table.stream, plain_table.offs, plain_table.ch, pack(windows), ws, fmt, sample_bits=bits)
    h_whole = codec.decode_windows_i32_host(plain_table.stream, plain_table.offs, plain_table.ch, pack(windows), ws, fmt, sample_bits=bits, whole=True)
    assert same_bits(h_whole[0], h_plain[0]) and np.array_equal(h_whole[1], h_plain[1]) and h_whole[2] == h_plain[2]
    return p_status


MALFORMED = ["bad_sync", "cut_short", "says_2047", "channel_8", "missing_parent", "difference_before_its_parent", "dry_rice", "q_out_of_range"]


def _plain_table(torch):
    x = W.track(4 * BLOCK, 2, 3, 3)
    return [W.ref().frame_encode_i32(np.ascontiguousarray(x[f * BLOCK: (f + 1) * BLOCK].T)) for f in range(4)]


def test_a_table_of_2048_sample_frames_gives_the_plain_call_s_words(gpu):  # noqa: F811
    t = Table32(gpu, _plain_table(gpu), 2)
    for ws, fmt in ((300, I32), (2049, PCM24), (777, PCM32), (5, F32)):
        status = _both_calls_agree(t, edge_windows(t.n), ws, fmt)
        assert not status[:3].any()


@pytest.mark.parametrize("kind", MALFORMED)
def test_malformed_tables_give_the_plain_call_s_words(gpu, kats, kind):  # noqa: F811
    """The malformed frame in the middle of the table, and as its last frame: each of them says 2048 in its first subframe (which
    is what a frame says), so none is a tail and the plain call's verdict holds."""
    good = _plain_table(gpu)
    frame, flag = _crafted(kats)[kind]
    for blobs, at in ((good[:2] + [frame] + good[3:], 2), (good[:3] + [frame], 3)):
        t = Table32(gpu, blobs, 2, declined={at: flag})
        windows = edge_windows(t.n) + [(at * BLOCK + 100, 0, 4), (at * BLOCK - 50, 0, 4), (0, at, 1)]
        for ws, fmt in ((300, I32), (2049, PCM24)):
            status = _both_calls_agree(t, windows, ws, fmt)
            assert int(status[0]) == flag


def test_tails_that_say_0_2048_and_4096_are_the_plain_call_s(gpu):  # noqa: F811
    good = _plain_table(gpu)
    for n_l in (0, 4096):  # (2048: every table above)
        t = Table32(gpu, good[:2] + [patch_n(patch_n(good[2], n_l, 0), n_l, 1)], 2, declined={2: BAD})
        status = _both_calls_agree(t, [(2 * BLOCK - 50, 0, 3), (2 * BLOCK + 10, 0, 3), (0, 2, 1), (100, 0, 3)], 300, I32)
        assert int(status[0]) == BAD and int(status[1]) == 3


def test_declined_tails(tables, kats):
    """Each leaves its share zero and raises its flag, once per (window, L) that has a share; the frames in front are untouched."""
    t = tables(2)
    body, tail = t.blobs[0], t.blobs[1]  # a tail of 2049 samples
    rng = np.random.default_rng(79)
    q = kats["blk/sine_deg/q"]
    dry = patch_n(_build_frame([(0, 0, 0, q, rng.integers(-60000, 60000, 2500)), (1, 0, 1, q, rng.integers(-60000, 60000, 2400))]), 2500, sub=1)
    windows = [(BLOCK - 50, 0, 2), (BLOCK + 10, 0, 2), (100, 0, 2), (0, 1, 1), (BLOCK + 5000, 0, 2), (BLOCK - 50, 0, 2)]
    cases = {"channels_disagree": (patch_n(tail, 2040, sub=1), BAD), "runs_dry": (dry, DRY)}
    for name, (frame, flag) in cases.items():
        d = WholeTable(t.torch, [body, frame], 2, declined={1: flag})
        for fmt in (I32, PCM24):
            want32, flags, status = check(d, windows, 300, fmt, 24)
            assert [int(f) for f in flags] == [flag, flag, 0, flag, 0, flag], name
            assert status == (flag, 4 if flag == BAD else 0, 4), name
            assert want32[0, :50].any() and not want32[0, 50:].any() and not want32[1].any() and want32[2].any()
    # a tail at an offset of 4k + 2 is not walked (the device calls: a host call that stages it alone puts it at offset 0)
    sync = bytearray(body)
    sync[0] ^= 0xFF
    d = WholeTable(t.torch, [body, bytes(sync), tail], 2, declined={1: BAD, 2: BAD}, pad={1: 2})
    assert int(d.offs[2]) % 4 == 2 and len(tail) % 4 == 0
    windows = [(2 * BLOCK - 50, 0, 3), (2 * BLOCK + 10, 0, 3), (100, 0, 3), (0, 2, 1)]
    want32, flags, status = check(d, windows, 300, I32, 24, host=False)
    assert [int(f) for f in flags] == [BAD, BAD, 0, BAD] and status == (BAD, 4, 3)


@pytest.mark.parametrize("fmt", [I32, PCM24])
def test_a_captured_call_reads_the_descriptors_at_replay(tables, fmt):
    t = tables(2)
    torch = t.torch
    first = [(0, 0, 2), (BLOCK + 100, 0, 2), (BLOCK - 5, 2, 2), (100, 10, 1)]
    second = [(BLOCK + 1000, 4, 2), (3, 0, 1), (BLOCK + 2300, 8, 2), (BLOCK - 700, 6, 2)]
    wd = codec.WindowDecoder32(4, 777, 2, fmt, whole=True)
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
        assert want32[-1].any()
        assert same_bits(out.cpu().numpy(), as_format(want32, fmt, 24))
        assert np.array_equal(wd.flags.cpu().numpy().view(np.uint32), want_flags)
        assert tuple(int(x) for x in wd.status.cpu().numpy().view(np.uint32)) == want_status + (0,)


def test_host_call_stages_the_tail_only_for_windows_that_reach_it(tables):
    lib = capi.lib()
    t = tables(2)
    for windows, frames in (([(100, 0, 2)], [0]), ([(BLOCK - 300, 0, 2)], [0]), ([(BLOCK - 299, 0, 2)], [0, 1]), ([(BLOCK + 100, 0, 2)], [1]),
                            ([(BLOCK + 2049, 0, 2)], [1]), ([(5, 10, 1), (BLOCK, 4, 2)], [5, 10]), ([(0, 12, 1)], [])):
        want32, want_flags, _ = t.expect(windows, 300)
        out, flags, rc = codec.decode_windows_i32_host(t.stream, t.offs, 2, pack(windows), 300, PCM32, whole=True)
        assert rc == 0 and same_bits(out, want32) and not flags.any()
        assert int(lib.sela_hip_debug_windows_staged_bytes()) == sum(t.sizes[f] for f in frames), (windows, frames)
