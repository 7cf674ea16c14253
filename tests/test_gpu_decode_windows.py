"""sela_hip_decode_windows_device and sela_hip_decode_windows: sample windows of streams of 2048-sample frames,
only the frames they touch decoded.  Output sample i of a window is exactly what sela_hip_decode_device writes for sample
(start + i) % 2048 of table frame first_frame + (start + i) / 2048 while that frame is in the window's stream, and zero behind it.
The expectation comes from codec.Decoder on the same frames (pinned to the reference elsewhere), sliced and zero-padded on the
host; all comparisons are exact.  Every case goes through the raw device call (guard words around d_out and behind
d_window_flags, the inputs compared afterwards), through codec.WindowDecoder and through the host call."""
import numpy as np
import pytest

from gpu_common import _build_frame, gpu  # noqa: F401
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

BLOCK = 2048
I16, F32 = capi.WINDOW_I16_INTERLEAVED, capi.WINDOW_F32_PLANAR
EINVAL, ECAPACITY, EFORMAT = -2, -4, -5
BAD = capi.FLAG_BAD_FRAME
GUARD = 63          # elements in front of and behind d_out (an odd count: the base has its element's alignment and no more), words behind the flags
SENT16, SENTF, SENT32 = 0x5E1A, 12345.0, 0x5E1A5E1A


def cover(window_samples):
    return (window_samples + 2046) // 2048 + 1


class Table:
    """A frame table on the device, what codec.Decoder makes of it, and the flags of every frame decoded alone."""

    def __init__(self, torch, blobs, ch):
        self.torch, self.ch, self.n = torch, ch, len(blobs)
        self.sizes = [len(b) for b in blobs]
        self.stream = np.frombuffer(b"".join(bytes(b) for b in blobs), np.uint8).copy()
        self.offs = np.cumsum([0] + self.sizes).astype(np.uint64)
        self.d_frames = torch.zeros(max(len(self.stream), 4), dtype=torch.uint8, device="cuda")
        self.d_frames[: len(self.stream)].copy_(torch.from_numpy(self.stream))
        self.d_offs = torch.from_numpy(self.offs.view(np.int64).copy()).cuda()
        dec = codec.Decoder(self.n, ch)
        pcm = dec.decode(self.d_frames, self.d_offs, self.n)
        torch.cuda.synchronize()
        self.pcm = pcm.cpu().numpy().reshape(self.n * BLOCK, ch).copy()  # (not checked: malformed frames are among the inputs)
        one = codec.Decoder(1, ch)
        self.frame_flags, self.frame_bad = [], []
        for f in range(self.n):
            alone = one.decode(self.d_frames, self.d_offs[f: f + 2], 1)
            torch.cuda.synchronize()
            st = one.status.cpu().numpy().view(np.uint32)
            assert np.array_equal(alone.cpu().numpy()[0], self.pcm[f * BLOCK: (f + 1) * BLOCK])
            self.frame_flags.append(int(st[0]))
            self.frame_bad.append(int(st[1]))

    def touched(self, start, first, n, ws):
        """the table frames a window decodes"""
        n_eff = min(n, self.n - first) if first < self.n else 0
        q = start // BLOCK
        if q >= n_eff:
            return range(0)
        last = q + (start % BLOCK + ws - 1) // BLOCK
        return range(first + q, first + min(last + 1, n_eff))

    def expect(self, windows, ws):
        """-> (int16 [n, ws, ch], flags uint32 [n], status[0..2])"""
        out = np.zeros((len(windows), ws, self.ch), np.int16)
        flags = np.zeros(len(windows), np.uint32)
        bad = 0
        for w, (start, first, n) in enumerate(windows):
            n_eff = min(n, self.n - first) if first < self.n else 0
            stream = self.pcm[first * BLOCK: (first + n_eff) * BLOCK]
            if start < len(stream):
                seg = stream[start: start + ws]
                out[w, : len(seg)] = seg
            for f in self.touched(start, first, n, ws):
                flags[w] |= self.frame_flags[f]
                bad += self.frame_bad[f]
        return out, flags, (int(np.bitwise_or.reduce(flags)) if len(flags) else 0, bad, int((flags != 0).sum()))


def as_format(want16, fmt):
    """int16 [n, ws, ch] -> what the format holds: itself, or float32 [n, ch, ws] of value / 32768"""
    if fmt == I16:
        return want16
    return np.ascontiguousarray((want16.astype(np.float32) / np.float32(32768)).transpose(0, 2, 1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_call(table, windows, ws, fmt=I16, with_flags=True, expect_rc=0, n_windows=None, **override):
    """The raw C ABI on fresh buffers full of sentinels -> (rc, out, flags or None, status uint32 [4]).  Guards and inputs are
    checked here; after a refusal every buffer must still hold its sentinel."""
    torch = table.torch
    lib = capi.lib()
    n = len(windows) if n_windows is None else n_windows
    ch = override.get("channels", table.ch)
    elems = len(windows) * ws * table.ch
    if fmt == F32:
        buf = torch.full((GUARD + elems + GUARD,), SENTF, dtype=torch.float32, device="cuda")
    else:
        buf = torch.full((GUARD + elems + GUARD,), SENT16, dtype=torch.int16, device="cuda")
    d_flags = torch.full((len(windows) + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    d_status = torch.full((4 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    packed = codec.WindowDecoder.pack([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows]) if windows else np.zeros((0, 2), np.int64)
    d_windows = torch.zeros((max(len(windows), 1), 2), dtype=torch.int64, device="cuda")
    if len(windows):
        d_windows[: len(windows)].copy_(torch.from_numpy(packed))
    need = int(lib.sela_hip_decode_windows_workspace_bytes(n, max(ws, 1) if ws <= 1 << 24 else 1, ch if 1 <= ch <= 8 else 1))
    d_ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    frames_before, windows_before = table.d_frames.clone(), d_windows.clone()
    out_ptr = buf.data_ptr() + GUARD * buf.element_size()
    args = dict(d_frames=table.d_frames.data_ptr(), d_frame_offsets=table.d_offs.data_ptr(), n_frames_total=table.n, channels=ch, d_windows=d_windows.data_ptr(),
                n_windows=n, window_samples=ws, format=fmt, d_out=out_ptr, d_window_flags=d_flags.data_ptr() if with_flags else None, d_status=d_status.data_ptr(),
                d_workspace=d_ws.data_ptr(), workspace_bytes=need, stream=torch.cuda.current_stream().cuda_stream)
    args.update({k: v for k, v in override.items() if k != "channels"})
    rc = lib.sela_hip_decode_windows_device(*[args[k] for k in ("d_frames", "d_frame_offsets", "n_frames_total", "channels", "d_windows", "n_windows", "window_samples",
                                                               "format", "d_out", "d_window_flags", "d_status", "d_workspace", "workspace_bytes", "stream")])
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.sela_hip_last_error())
    assert torch.equal(table.d_frames, frames_before), "d_frames was written"
    assert torch.equal(d_windows, windows_before), "d_windows was written"
    host = buf.cpu().numpy()
    sent = np.float32(SENTF) if fmt == F32 else np.int16(SENT16)
    assert (host[:GUARD] == sent).all() and (host[GUARD + elems:] == sent).all(), "written around d_out"
    flags = d_flags.cpu().numpy().view(np.uint32)
    status = d_status.cpu().numpy().view(np.uint32)
    assert (flags[len(windows):] == SENT32).all() and (status[4:] == SENT32).all(), "written behind d_window_flags or d_status"
    if rc != 0 or n == 0:
        assert (host == sent).all(), "d_out was written"
        assert (flags == SENT32).all(), "d_window_flags was written"
    if rc != 0:
        assert (status == SENT32).all(), "a refused call wrote d_status"
    if not with_flags:
        assert (flags == SENT32).all()
    body = host[GUARD: GUARD + elems]
    out = body.reshape(len(windows), table.ch, ws) if fmt == F32 else body.reshape(len(windows), ws, table.ch)
    return rc, out.copy(), (flags[: len(windows)].copy() if with_flags else None), status[:4].copy()


def host_call(table, windows, ws, fmt=I16):
    packed = codec.WindowDecoder.pack([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])
    out, flags, rc = codec.decode_windows_host(table.stream, table.offs, table.ch, packed, ws, planar_float=fmt == F32)
    return rc, out, flags


def check(table, windows, ws, fmt=I16):
    """The three ways in against the expectation -> the expectation's (flags, status[0..2])."""
    torch = table.torch
    want16, want_flags, want_status = table.expect(windows, ws)
    want = as_format(want16, fmt)
    # 1. the raw device call
    rc, out, flags, status = device_call(table, windows, ws, fmt)
    assert same_bits(out, want), np.argwhere(out != want)[:8]
    assert np.array_equal(flags, want_flags), (flags, want_flags)
    assert tuple(int(x) for x in status) == want_status + (0,), (status, want_status)
    # 2. codec.WindowDecoder
    wd = codec.WindowDecoder(len(windows), ws, table.ch, planar_float=fmt == F32)
    packed = codec.WindowDecoder.pack([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])
    got = wd.decode(table.d_frames, table.d_offs, table.n, torch.from_numpy(packed).cuda())
    torch.cuda.synchronize()
    assert same_bits(got.cpu().numpy(), want)
    assert np.array_equal(wd.flags.cpu().numpy().view(np.uint32), want_flags)
    assert tuple(int(x) for x in wd.status.cpu().numpy().view(np.uint32)) == want_status + (0,)
    if want_status[0] == 0:
        wd.check()
    else:
        with pytest.raises(capi.SelaHipError):
            wd.check()
    # 3. the host call: the same outputs and flags; its return code is the verdict on the flags
    rc, hout, hflags = host_call(table, windows, ws, fmt)
    assert same_bits(hout, want) and np.array_equal(hflags, want_flags)
    assert rc == (0 if want_status[0] == 0 else EFORMAT if want_status[0] & (BAD | capi.FLAG_RICE_OVERRUN) else -6), (rc, want_status)
    return want_flags, want_status


def _encoded_blobs(torch, pcm):
    enc = codec.Encoder(pcm.shape[0], pcm.shape[2])
    out = enc.encode(torch.from_numpy(np.ascontiguousarray(pcm)).cuda())
    torch.cuda.synchronize()
    frames, offs = out.to_host()
    return [frames[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(pcm.shape[0])]


@pytest.fixture(scope="module")
def tables(gpu):  # noqa: F811
    """five frames of synthetic audio for every channel count the tests use, encoded by the library"""
    cache = {}

    def get(ch):
        if ch not in cache:
            cache[ch] = Table(gpu, _encoded_blobs(gpu, synth_frames(5, ch, 40 + ch)), ch)
        return cache[ch]
    return get


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def test_edges_of_frames_streams_and_the_start(tables):
    t = tables(2)
    assert not any(t.frame_flags)
    ends = [0, 2047, 2048, 5 * BLOCK - 1, 5 * BLOCK, 2 ** 64 - 1]
    flags, status = check(t, [(s, 0, 5) for s in ends], 1)
    assert status == (0, 0, 0) and not flags.any()
    check(t, [(2047, 0, 5)], 2)
    assert cover(2049) == 2 and cover(2050) == 3 and cover(3 * BLOCK) == 4
    check(t, [(2047, 0, 5)], 2049)                                  # two frames
    check(t, [(2047, 0, 5), (5 * BLOCK + 7, 0, 5), (3 * BLOCK + 2047, 0, 5)], 2050)  # three frames = cover; wholly past the end; off the end
    check(t, [(0, 0, 5), (BLOCK, 0, 5), (3 * BLOCK, 0, 5)], 3 * BLOCK)  # a cover of 4 with the last workgroup empty
    want, _, _ = t.expect([(5 * BLOCK + 7, 0, 5)], 2050)
    assert not want.any()
    for fmt in (I16, F32):  # starts that only 64 bits hold, next to ones they could be taken for modulo 2^32 or 2^43
        check(t, [(2 ** 64 - 1, 0, 5), (2 ** 32, 0, 5), (2 ** 32 + 5, 0, 5), (2 ** 43, 0, 0xFFFFFFFF), (2 ** 64 - BLOCK, 0, 0xFFFFFFFF), (5, 0, 5)], 300, fmt)


# ---- channel counts and store alignment ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [I16, F32], ids=["i16", "f32"])
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_channel_counts_formats_and_every_alignment(tables, ch, fmt):
    """An odd length and odd and even starts: the windows' bases in d_out (itself at an odd element) fall on every alignment the
    element allows; eight channels run eight waves and more than 64 KiB of LDS."""
    t = tables(ch)
    starts = [0, 1, 777, 2047, 2048, 4095, 5001, 9000, 10000, 10239]
    check(t, [(s, 0, 5) for s in starts], 777, fmt)
    check(t, [(3, 1, 3), (2 * BLOCK - 2, 1, 3)], 2 * BLOCK + 5, fmt)


# ---- the second pass ------------------------------------------------------------------------------------------------------------------
def _stereo_kinds(kats):
    rng = np.random.default_rng(5)
    q = kats["blk/sine_deg/q"]
    r = lambda: rng.integers(-60, 60, BLOCK)  # noqa: E731
    indep = _build_frame([(0, 0, 0, q, r()), (1, 0, 1, q, r())])
    dep0 = _build_frame([(0, 1, 1, q, r()), (1, 0, 1, q, r())])  # channel 0 is parent (channel 1) - difference
    diff = bytes(kats["frame/stereo_synth_diff/bytes"])          # channel 1 is a difference subframe
    return indep, dep0, diff


def test_stereo_second_pass_across_frames_of_different_kinds(gpu, kats):  # noqa: F811
    indep, dep0, diff = _stereo_kinds(kats)
    t = Table(gpu, [indep, diff, dep0, indep, diff], 2)
    assert not any(t.frame_flags)
    assert not np.array_equal(t.pcm[BLOCK: 2 * BLOCK, 0], t.pcm[BLOCK: 2 * BLOCK, 1])
    windows = [(BLOCK - 100, 0, 5), (2 * BLOCK - 151, 0, 5), (3 * BLOCK - 1, 0, 5), (4 * BLOCK - 299, 0, 5), (BLOCK - 100, 1, 3), (0, 2, 1)]
    for fmt in (I16, F32):
        check(t, windows, 301, fmt)
    check(t, [(BLOCK - 1, 0, 5)], 3 * BLOCK + 2)


# ---- many windows -----------------------------------------------------------------------------------------------------------------------
def test_sixty_four_windows_in_two_streams_of_one_table(tables):
    t = tables(2)
    rng = np.random.default_rng(64)
    windows = [(int(s), 0, 2) for s in sorted(rng.integers(0, 2 * BLOCK + 500, 24), reverse=True)]      # decreasing starts, some past the stream's 2 frames
    windows += [(int(s), 2, 3) for s in rng.integers(0, 3 * BLOCK + 500, 24)]
    windows += [windows[0], windows[0], windows[30], (BLOCK + 1500, 0, 2), (BLOCK + 1500, 0, 2)]          # duplicates
    windows += [(2 * BLOCK - 10, 0, 2), (2 * BLOCK, 0, 2)]                                                # runs into / starts at the second stream: zeros, not its samples
    windows += [(BLOCK, 3, 7), (0, 4, 0xFFFFFFFF), (5, 5, 1), (5, 0xFFFFFFFF, 0xFFFFFFFF), (0, 2, 0)]     # cut at the table; outside it; empty
    windows += [(100, 0, 5)] * (64 - len(windows))
    assert len(windows) == 64
    want, _, _ = t.expect(windows, 1000)
    w = windows.index((2 * BLOCK - 10, 0, 2))
    assert want[w, :10].any() and not want[w, 10:].any() and t.pcm[2 * BLOCK: 2 * BLOCK + 990].any()
    for fmt in (I16, F32):
        check(t, windows, 1000, fmt)


# ---- one bad frame ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sync", "short"])
def test_one_bad_frame_costs_the_windows_that_touch_it_and_no_others(gpu, kats, kind):  # noqa: F811
    indep, dep0, diff = _stereo_kinds(kats)
    if kind == "sync":
        bad = bytearray(indep)
        bad[0] ^= 0xFF
        bad = bytes(bad)
    else:
        rng = np.random.default_rng(9)
        q = kats["blk/sine_deg/q"]
        bad = _build_frame([(0, 0, 0, q, rng.integers(-60, 60, BLOCK)), (1, 0, 1, q, rng.integers(-60, 60, 1000))])  # a subframe that says 1000 samples
    t = Table(gpu, [indep, diff, dep0, bad, indep], 2)
    assert [bool(f & BAD) for f in t.frame_flags] == [False, False, False, True, False] and t.frame_bad == [0, 0, 0, 1, 0]
    windows = [(0, 0, 5), (2 * BLOCK + 1900, 0, 5), (3 * BLOCK - 1, 0, 5), (3 * BLOCK + 5, 0, 5), (3 * BLOCK + 5, 0, 5), (4 * BLOCK - 150, 0, 5), (4 * BLOCK, 0, 5),
               (BLOCK, 0, 3), (2 * BLOCK + 1900, 0, 3), (0, 3, 1), (2047, 1, 4)]
    ws = 150
    flags, status = check(t, windows, ws)
    touching = [w for w, (s, f, n) in enumerate(windows) if 3 in t.touched(s, f, n, ws)]
    assert touching == [1, 2, 3, 4, 5, 9] and [int(x) for x in np.flatnonzero(flags)] == touching and all(int(flags[w]) & BAD for w in touching)
    assert status == (int(np.bitwise_or.reduce(flags)), len(touching), len(touching))
    flags, status = check(t, [(2047 + BLOCK, 0, 5), (0, 0, 5)], 2050, F32)  # frames 1, 2 and 3 in one window
    assert flags.tolist() == [t.frame_flags[3], 0] and status[1:] == (1, 1)
    # d_window_flags = NULL: the same output and status
    want16, _, want_status = t.expect(windows, ws)
    rc, out, none, st = device_call(t, windows, ws, with_flags=False)
    assert none is None and same_bits(out, want16) and tuple(int(x) for x in st) == want_status + (0,)


# ---- generic mode -----------------------------------------------------------------------------------------------------------------------
def test_two_windows_share_a_frame_that_takes_generic_mode(gpu, kats):  # noqa: F811
    """A Rice stream beyond the LDS plan sends its frame through the serial parse, the residues parked in the workspace by
    workgroup: two windows that decode the frame at once each get all of it."""
    rng = np.random.default_rng(31)
    indep, dep0, diff = _stereo_kinds(kats)
    q_sine, q_noise = kats["blk/sine_deg/q"], kats["blk/white_fullscale/q"]
    big = _build_frame([(0, 0, 0, q_sine, rng.integers(-50, 50, BLOCK)), (1, 1, 0, q_noise, rng.integers(-(1 << 20), 1 << 20, BLOCK))])
    assert len(big) > 4 * 1072 + 64
    t = Table(gpu, [indep, big, diff], 2)
    assert not any(t.frame_flags)
    windows = [(BLOCK - 50, 0, 3), (BLOCK + 3, 0, 3), (BLOCK - 50, 0, 3), (2 * BLOCK - 5, 0, 3), (0, 1, 1), (7, 0, 1)]
    for fmt in (I16, F32):
        check(t, windows, 1501, fmt)
    mono = Table(gpu, [_build_frame([(0, 0, 0, q_sine, rng.integers(-30000, 30000, BLOCK))]), _build_frame([(0, 0, 0, q_sine, rng.integers(-30, 30, BLOCK))])], 1)
    check(mono, [(0, 0, 2), (1, 0, 2), (1000, 0, 2), (BLOCK - 1, 0, 2)], 1501)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_every_buffer_alone(tables):
    t = tables(2)
    windows = [(5, 0, 5), (3000, 0, 5)]
    for override in (dict(channels=0), dict(channels=9)):
        device_call(t, windows, 100, expect_rc=EINVAL, **override)
    device_call(t, windows, 100, expect_rc=EINVAL, window_samples=0)
    device_call(t, windows, 100, expect_rc=EINVAL, window_samples=(1 << 24) + 1)
    device_call(t, windows, 100, expect_rc=EINVAL, format=2)
    device_call(t, windows, 100, expect_rc=EINVAL, d_frames=t.d_frames.data_ptr() + 2)
    device_call(t, windows, 100, expect_rc=EINVAL, d_windows=t.d_offs.data_ptr() + 4)
    odd = t.torch.zeros(1024, dtype=t.torch.uint8, device="cuda")
    device_call(t, windows, 100, expect_rc=EINVAL, d_out=odd.data_ptr() + 1)
    device_call(t, windows, 100, F32, expect_rc=EINVAL, d_out=odd.data_ptr() + 2)
    device_call(t, windows, 100, expect_rc=EINVAL, d_status=None)
    need = int(capi.lib().sela_hip_decode_windows_workspace_bytes(2, 100, 2))
    device_call(t, windows, 100, expect_rc=ECAPACITY, workspace_bytes=need - 1)
    assert not odd.any()
    # no windows: zero status words, nothing else
    rc, out, flags, status = device_call(t, windows, 100, n_windows=0)
    assert status.tolist() == [0, 0, 0, 0]
    # ... and with exactly what the sizing function says the call goes through
    rc, out, flags, status = device_call(t, windows, 100, workspace_bytes=need)
    assert same_bits(out, t.expect(windows, 100)[0])


# ---- capture ----------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_reads_the_descriptors_at_replay(tables):
    t = tables(2)
    torch = t.torch
    first = [(0, 0, 5), (2047, 0, 5), (9000, 0, 5), (4000, 2, 2)]
    second = [(3 * BLOCK + 1, 0, 5), (1, 1, 1), (2 ** 64 - 1, 0, 5), (BLOCK - 400, 0, 2)]
    pack = lambda ws: torch.from_numpy(codec.WindowDecoder.pack([w[0] for w in ws], [w[1] for w in ws], [w[2] for w in ws]))  # noqa: E731
    wd = codec.WindowDecoder(4, 777, 2)
    d_windows = pack(first).cuda()
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
        d_windows.copy_(pack(windows))
        wd.out.fill_(SENT16), wd.window_flags.fill_(-1), wd.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want, want_flags, want_status = t.expect(windows, 777)
        assert same_bits(out.cpu().numpy(), want)
        assert np.array_equal(wd.flags.cpu().numpy().view(np.uint32), want_flags)
        assert tuple(int(x) for x in wd.status.cpu().numpy().view(np.uint32)) == want_status + (0,)


# ---- the host call copies what the windows touch -------------------------------------------------------------------------------------------
def test_host_call_stages_the_covering_frames_and_no_others(gpu):  # noqa: F811
    lib = capi.lib()
    t = Table(gpu, _encoded_blobs(gpu, synth_frames(40, 2, 77)), 2)
    windows = [(3 * BLOCK + 100, 0, 40), (3 * BLOCK + 2000, 0, 40), (2 * BLOCK + 5, 20, 20)]   # frames 3 | 3, 4 | 22
    ws = 300
    distinct = sorted({f for s, a, n in windows for f in t.touched(s, a, n, ws)})
    assert distinct == [3, 4, 22]
    rc, out, flags = host_call(t, windows, ws)
    assert rc == 0 and same_bits(out, t.expect(windows, ws)[0]) and not flags.any()
    staged = int(lib.sela_hip_debug_windows_staged_bytes())
    assert staged == sum(t.sizes[f] for f in distinct) and staged * 5 < len(t.stream), (staged, len(t.stream))
    rc, out, flags = host_call(t, [(40 * BLOCK, 0, 40)], ws)   # nothing touched: nothing staged, zeros
    assert rc == 0 and not out.any() and int(lib.sela_hip_debug_windows_staged_bytes()) == 0
    rc, out, flags = host_call(t, [(0, 0, 40)], 40 * BLOCK, F32)   # the whole stream is one window
    assert rc == 0 and same_bits(out, as_format(t.pcm.reshape(1, 40 * BLOCK, 2), F32)) and int(lib.sela_hip_debug_windows_staged_bytes()) == len(t.stream)
    # a call that stages nothing says so, whatever the call before it staged: no windows, and a refused argument
    assert host_call(t, [], ws)[0] == 0 and int(lib.sela_hip_debug_windows_staged_bytes()) == 0
    assert host_call(t, [(0, 0, 40)], ws)[0] == 0 and int(lib.sela_hip_debug_windows_staged_bytes()) > 0
    assert lib.sela_hip_decode_windows(t.stream.ctypes.data, t.offs.ctypes.data, 40, 9, 0, 0, ws, I16, 0, 0) == -2
    assert int(lib.sela_hip_debug_windows_staged_bytes()) == 0
    # frame offsets that decrease are refused as the sibling host calls refuse them
    offs = t.offs.copy()
    offs[5] = offs[4] - 4
    packed = codec.WindowDecoder.pack([0], [0], [40])
    assert codec.decode_windows_host(t.stream, offs, 2, packed, ws)[2] == EFORMAT
