"""sela_hip_decode_n_device and sela_hip_decode_payload_n_device: the int16 decode of any length on device pointers is the
host-pointer sela_hip_decode byte for byte -- interleaved PCM at sela_hip_index_samples' sample offsets -- wherever the host call
returns 0, and sela_hip_decode_n_status_error(device status) is the host call's code on every input.  The route the device takes
(status[3]) is the host call's: the 2048-sample decoder for 2048 everywhere, the any-length kernels otherwise.  (The host calls
are pinned to the oracle and the reference by test_gpu_decode_any_length.py, test_gpu_wide_samples.py and the golden suites.)"""
import numpy as np
import pytest

import generic_cases as gc
import wide_cases as wc
from gpu_common import DECODE_LENGTHS, ENCODE_LENGTHS, _build_frame, _hostile_frame, _one, _signal, gpu  # noqa: F401
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

GUARD = 2048  # int16 behind the PCM that no call may write
SENTINEL = 0x5EA1
NONE, FAST, ANY = 0, 1, 2


def _bytes(blob):
    fr = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, np.uint8)
    return fr


def _host(blob, offs, ch):
    """sela_hip_decode and sela_hip_index_samples on host pointers -> (rc, pcm int16 [samples * ch], sample offsets, largest)."""
    lib = capi.lib()
    fr = _bytes(blob)
    fr = np.ascontiguousarray(fr if len(fr) else np.zeros(4, np.uint8))
    o = np.ascontiguousarray(offs, np.uint64)
    n = len(o) - 1
    so = np.zeros(n + 1, np.uint64)
    largest = int(lib.sela_hip_index_samples(fr.ctypes.data, o.ctypes.data, n, ch, so.ctypes.data))
    total = int(so[n]) if (o[1:] >= o[:-1]).all() else 0
    out = np.zeros(max(n * 2048, total, 1) * ch, np.int16)
    rc = lib.sela_hip_decode(fr.ctypes.data, o.ctypes.data, n, ch, out.ctypes.data)
    return rc, out[: total * ch], so, largest


class _Device:
    """Device buffers for one call of sela_hip_decode_n_device, with guard words behind the PCM and the sample offsets."""

    def __init__(self, torch, n, ch, stride):
        self.torch, self.n, self.ch, self.stride = torch, n, ch, stride
        self.pcm = torch.full((n * stride * ch + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
        self.sample_offsets = torch.full((n + 1 + 16,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_decode_n_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")

    def decode(self, blob, offs, with_offsets=True):
        torch = self.torch
        data = _bytes(blob)
        frames = torch.zeros(max(len(data), 4), dtype=torch.uint8, device="cuda")
        if len(data):
            frames[: len(data)].copy_(torch.from_numpy(data.copy()))
        o = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).cuda()
        capi.check(capi.lib().sela_hip_decode_n_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, self.pcm.data_ptr(),
            self.sample_offsets.data_ptr() if with_offsets else None, self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return self.results()

    def results(self):
        n, ch, stride = self.n, self.ch, self.stride
        p = self.pcm.cpu().numpy()
        so = self.sample_offsets.cpu().numpy()
        assert (p[n * stride * ch:] == SENTINEL).all(), "written past n_frames * stride * channels"
        assert (so[n + 1:] == -1).all(), "written past the sample offsets"
        st = self.status.cpu().numpy().view(np.uint32).copy()
        return p[: n * stride * ch], so[: n + 1].view(np.uint64), st


def _same(torch, blob, offs, ch, stride=None, mode=-1, route=None, label=""):
    """Device call == host call on (blob, offs) under debug mode `mode` -> (the host call's code, the route taken)."""
    lib = capi.lib()
    offs = np.ascontiguousarray(offs, np.uint64)
    n = len(offs) - 1
    if stride is None:
        fr = _bytes(blob)
        stride = max(codec.index_samples(fr if len(fr) else np.zeros(4, np.uint8), offs, ch)[1], 1)
    lib.sela_hip_debug_standard_first(mode)
    try:
        rc, pcm, so, largest = _host(blob, offs, ch)
        d_pcm, d_so, st = _Device(torch, n, ch, stride).decode(blob, offs)
    finally:
        lib.sela_hip_debug_standard_first(-1)
    code = codec.decode_n_status_error(st)
    assert code == rc or (code == -4 and largest > stride), (label, mode, rc, st)
    if (offs[1:] >= offs[:-1]).all():  # (decreasing offsets: sela_hip_index_samples writes no sample offsets at all)
        assert np.array_equal(d_so, so), (label, mode)
    assert int(st[2]) == largest, (label, mode, st, largest)
    assert bool(st[0] & capi.FLAG_STRIDE) == (code == -4), (label, st)
    if code == -4:
        assert int(st[3]) == NONE and (d_pcm == SENTINEL).all(), (label, st)
    if route is not None:
        assert int(st[3]) == route, (label, st, route)
    if code == 0:
        total = int(so[n]) * ch
        assert int(st[0]) == 0 and int(st[1]) == 0, (label, st)
        assert np.array_equal(d_pcm[:total], pcm), (label, mode)
        assert (d_pcm[total:] == SENTINEL).all(), (label, "written past sample_offsets[n] * channels")
        assert int(st[3]) == (NONE if n == 0 else FAST if largest == 2048 and (so == np.arange(n + 1) * 2048).all() and stride >= 2048
                              and _all_2048(blob, offs, ch) else ANY), (label, st)
    return code, int(st[3])


def _all_2048(blob, offs, ch):
    """Every subframe says 2048, read as sela_hip_index_samples reads it, and the walk is whole."""
    return _walk_lengths(_bytes(blob), offs, ch) == {2048}


def _walk_lengths(fr, offs, ch):
    seen = set()
    for f in range(len(offs) - 1):
        fb = fr[int(offs[f]): int(offs[f + 1])].tobytes()
        p = 4
        for _ in range(ch):
            if p + 12 > len(fb):
                return set()
            cw = fb[p + 4] | (fb[p + 5] << 8)
            q = p + 7 + 4 * cw
            if q + 5 > len(fb):
                return set()
            rw = fb[q + 1] | (fb[q + 2] << 8)
            seen.add(fb[q + 3] | (fb[q + 4] << 8))
            p = q + 5 + 4 * rw
            if p > len(fb):
                return set()
    return seen


def _stream(blobs):
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)


# ---- 1. streams the encoders make ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(set(DECODE_LENGTHS) | set(ENCODE_LENGTHS)))
def test_encoder_streams_of_every_length(gpu, n):  # noqa: F811
    rng = np.random.default_rng(n)
    taken = 0
    for kinds in (("tone",), ("tone", "noise"), ("sparse", "tone", "dc"), tuple(["tone", "noise", "sparse"] * 3)):
        x = np.stack([_signal(rng, k, n, 15) for k in kinds])
        try:
            frames, offs = codec.encode_i32(np.stack([x, x[:, ::-1].copy()]))  # (two frames per call)
        except capi.SelaHipError:  # (a block not longer than its own order: the encoder refuses it)
            assert n <= 100
            continue
        code, route = _same(gpu, frames, offs, len(kinds), label=(n, len(kinds)))
        assert code == 0 and route == (FAST if n == 2048 else ANY), (n, len(kinds), route)
        taken += 1
    assert taken or n <= 100


def test_255_channels(gpu):  # noqa: F811
    rng = np.random.default_rng(255)
    for n in (2048, 300):
        x = np.stack([_signal(rng, ("tone", "noise", "sparse")[c % 3], n, 14) for c in range(255)])
        frames, offs = codec.encode_i32(x[None])
        code, route = _same(gpu, frames, offs, 255, label=("255", n))
        assert code == 0 and route == (FAST if n == 2048 else ANY)


@pytest.mark.parametrize("n", [1, 1000, 2048, 4097, 65535])
def test_round_trip_on_the_device(gpu, n):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(n + 7)
    frames_n = 3 if n < 65535 else 2
    pcm = np.stack([np.stack([_signal(rng, "tone", n, 15), _signal(rng, "noise", n, 12)], axis=1) for _ in range(frames_n)]).astype(np.int16)
    enc = codec.Encoder32(frames_n, 2, n)
    d_frames, d_offs, _ = enc.encode(torch.from_numpy(np.ascontiguousarray(pcm)).cuda())
    if n == 1:  # (the encoder refuses a block not longer than the order its analysis picks: one sample takes an order-0 frame by hand)
        with pytest.raises(capi.SelaHipError):
            enc.check()
        blobs = [_build_frame([(0, 0, 0, np.zeros(0, np.int32), pcm[f, :, 0].astype(np.int32)),
                               (1, 0, 1, np.zeros(0, np.int32), pcm[f, :, 1].astype(np.int32))]) for f in range(frames_n)]
        stream, offs = _stream(blobs)
        assert _same(gpu, stream, offs, 2, label="one sample") == (0, ANY)
        d_frames, d_offs = torch.from_numpy(stream).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    else:
        enc.check()
    dec = codec.DecoderN(frames_n, 2, max(n, 1))
    out, so = dec.decode(d_frames, d_offs, frames_n)
    dec.check()
    assert dec.route() == (FAST if n == 2048 else ANY)
    assert np.array_equal(so.cpu().numpy(), np.arange(frames_n + 1) * n)
    assert np.array_equal(out[: frames_n * n].cpu().numpy(), pcm.reshape(-1, 2))


def test_generic_cases_narrow_and_wide(gpu):  # noqa: F811
    for label, n, kind, wide in gc.all_cases():
        frames, offs = codec.encode_i32(gc.case_input(n, kind, wide)[None])
        assert _same(gpu, frames, offs, {"mono": 1, "three": 3}.get(kind, 2), label=label)[0] == 0


def test_ragged_frames(gpu):  # noqa: F811
    codes = set()
    blobs = []
    for label, chans in gc.ragged_cases():
        blob = codec.encode_ragged(chans)
        codes.add(_same(gpu, blob, _one(len(blob)), len(chans), label=label)[0])
        if len(chans) == 2:
            blobs.append(blob)
    stream, offs = _stream(blobs)
    codes.add(_same(gpu, stream, offs, 2, label="ragged stereo together")[0])
    assert -5 in codes  # (channels of different lengths: malformed for int16 output)


def test_a_late_odd_frame_and_the_bench_track(gpu):  # noqa: F811
    torch = gpu
    frames, offs = codec.encode_host(synth_frames(40, 2, 3))
    blobs = [frames[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(40)]
    odd = codec.encode_i32(np.stack([_signal(np.random.default_rng(1), "tone", 777, 15)] * 2)[None])[0].tobytes()
    stream, so = _stream(blobs[:35] + [odd] + blobs[35:])
    for mode in (-1, 2, 0):
        code, route = _same(gpu, stream, so, 2, stride=2048, mode=mode, label=("late odd", mode))
        assert code == 0 and route == ANY
    for mode in (-1, 2, 0):
        assert _same(gpu, frames, offs, 2, stride=2048, mode=mode, label=("all 2048", mode)) == (0, FAST)

    frames, offs = codec.encode_host(synth_frames(3875, 2, 0))
    f_d, o_d = torch.from_numpy(frames).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    ref = codec.Decoder(3875, 2)
    want = ref.decode(f_d, o_d, 3875)
    torch.cuda.synchronize()
    ref.check()
    dec = codec.DecoderN(3875, 2, 2048)
    pcm, so = dec.decode(f_d, o_d, 3875)
    dec.check()
    assert dec.route() == FAST
    assert np.array_equal(pcm.cpu().numpy(), want.reshape(-1, 2).cpu().numpy())
    pcm, so, fo, count = dec.decode_payload(f_d)
    dec.check()
    assert int(count.item()) == 3875 and dec.route() == FAST and np.array_equal(fo.cpu().numpy().view(np.uint64), offs)
    assert np.array_equal(pcm.cpu().numpy(), want.reshape(-1, 2).cpu().numpy())


def test_wide_samples_are_narrowed_as_the_host_narrows(gpu, generic_kats):  # noqa: F811
    from oracle_lib import oracle

    o = oracle()
    rng = np.random.default_rng(41)
    blobs = []
    for n, seed in ((2048, 1), (2048, 2), (1000, 4), (4096, 5)):
        subs, wraps = wc.stereo_wrap_subframes(o, n, seed)
        assert wraps > 0
        blobs.append(wc.frame_bytes(o, subs))
    stream, offs = _stream(blobs)
    for mode in (-1, 2, 0):
        assert _same(gpu, stream, offs, 2, mode=mode, label="wide stereo")[0] == 0
    assert _same(gpu, blobs[0] + blobs[1], _stream(blobs[:2])[1], 2, label="wide 2048") == (0, FAST)
    cases = wc.stage_cases(2048, rng, wc.FRAME_RESIDUES)
    clean = 0
    for i, order in enumerate(wc.ORDERS):
        blob = wc.frame_bytes(o, [(0, 0, 0, wc.fold_coefficients(order, rng), cases[i % len(cases)][1]),
                                  (1, 0, 1, wc.fold_coefficients(wc.ORDERS[-1 - i], rng), cases[(i + 3) % len(cases)][1])])
        clean += _same(gpu, blob, _one(len(blob)), 2, stride=2048, label=("wide order", order))[0] == 0
    assert clean >= 1
    for name in generic_kats["crafted_names"]:
        blob = generic_kats[f"crafted/{name}/bytes"]
        ch = int(generic_kats[f"crafted/{name}/channels"])
        stride = max(max(len(generic_kats[f"crafted/{name}/decoded{c}"]) for c in range(ch)), 1)
        for mode in (-1, 2, 0):
            _same(gpu, blob, _one(len(blob)), ch, stride=stride, mode=mode, label=name)


# ---- 2. hostile streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["short", "long", "2048"])
def test_hostile_streams(gpu, shape):  # noqa: F811
    rng = np.random.default_rng({"short": 17, "long": 18, "2048": 19}[shape])
    trials, n_lo, n_hi = {"short": (60, 1, 700), "long": (12, 3000, 30000), "2048": (40, 2048, 2049)}[shape]
    codes, routes = {}, {}
    for trial in range(trials):
        ch = int(rng.integers(1, 4))
        blobs = [_hostile_frame(rng, ch, n_lo, n_hi, shape == "long") for _ in range(2)]
        stream, offs = _stream(blobs)
        for mode in ((-1, 0) if trial % 2 else (-1,)):
            code, route = _same(gpu, stream, offs, ch, stride=max(n_hi, 2048), mode=mode, label=(shape, trial))
            codes[code] = codes.get(code, 0) + 1
            routes[route] = routes.get(route, 0) + 1
    assert codes.get(-5, 0) + codes.get(-6, 0) >= trials // 10, codes
    if shape == "2048":
        assert routes.get(FAST, 0) >= trials // 4, routes


def test_malformed_and_decreasing(gpu):  # noqa: F811
    rng = np.random.default_rng(9)
    a = codec.encode_i32(np.stack([_signal(rng, "tone", 500, 15)])[None])[0].tobytes()
    b = codec.encode_i32(np.stack([_signal(rng, "noise", 777, 12)])[None])[0].tobytes()
    stream, offs = _stream([a, b, a])
    offs2 = offs.copy()
    offs2[2] = offs2[1] - 4
    assert _same(gpu, stream, offs2, 1, stride=2048, label="decreasing") == (-5, NONE)
    c, c_offs = codec.encode_host(synth_frames(2, 1, 5))
    for stream, offs in ((stream, offs), (c, c_offs)):
        cut = offs.copy()
        cut[1] -= 8  # (the walk breaks in frame 0)
        code, route = _same(gpu, stream, cut, 1, stride=2048, label="broken")
        assert code == -5 and route == NONE
    assert _same(gpu, a[:4] + b"\0" * 40, _one(44), 1, stride=64, label="empty subframes") == (-5, NONE)
    # a frame at an offset that is not a multiple of 4: the any-length route takes it, the 2048-sample route refuses the stream
    stream = np.frombuffer(a + b"\x00" + b, np.uint8).copy()
    assert _same(gpu, stream, np.array([0, len(a) + 1, len(a) + 1 + len(b)], np.uint64), 1, label="odd offset") == (0, ANY)
    s2, o2 = codec.encode_host(synth_frames(2, 2, 6))
    f0, f1 = s2[: int(o2[1])].tobytes(), s2[int(o2[1]):].tobytes()
    stream = np.frombuffer(f0 + b"\x00" + f1, np.uint8).copy()
    assert _same(gpu, stream, np.array([0, len(f0) + 1, len(f0) + 1 + len(f1)], np.uint64), 2, stride=2048, label="odd offset, 2048") == (-5, NONE)


# ---- 3. the stride, the guards, the debug routes ------------------------------------------------------------------------------
def test_a_stride_too_small(gpu):  # noqa: F811
    lengths = (300, 5000, 2048, 777)
    blobs = [codec.encode_i32(np.stack([_signal(np.random.default_rng(n), "tone", n, 15)] * 2)[None])[0].tobytes() for n in lengths]
    stream, offs = _stream(blobs)
    for stride in (1, 299, 2048, 4999):
        _, _, st = _Device(gpu, 4, 2, stride).decode(stream, offs)
        assert int(st[2]) == 5000 and st[0] & capi.FLAG_STRIDE and int(st[3]) == NONE and codec.decode_n_status_error(st) == -4
    assert _same(gpu, stream, offs, 2, stride=5000) == (0, ANY)
    assert _same(gpu, stream, offs, 2, stride=7000) == (0, ANY)
    f2048, o2048 = codec.encode_host(synth_frames(3, 2, 1))
    for stride in (1, 2047):
        _, _, st = _Device(gpu, 3, 2, stride).decode(f2048, o2048)
        assert int(st[2]) == 2048 and st[0] & capi.FLAG_STRIDE and int(st[3]) == NONE and codec.decode_n_status_error(st) == -4
    assert _same(gpu, f2048, o2048, 2, stride=2048) == (0, FAST)
    assert _same(gpu, f2048, o2048, 2, stride=3000) == (0, FAST)
    # without d_sample_offsets: the same bytes
    d = _Device(gpu, 4, 2, 5000)
    with_o, so, _ = d.decode(stream, offs)
    d2 = _Device(gpu, 4, 2, 5000)
    without, so2, st = d2.decode(stream, offs, with_offsets=False)
    assert np.array_equal(with_o, without) and (so2 == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and codec.decode_n_status_error(st) == 0


def test_debug_routes_give_the_same_bytes(gpu):  # noqa: F811
    rng = np.random.default_rng(77)
    blobs = []
    for i in range(24):
        n = int(rng.integers(101, 9000)) if i % 5 else int(rng.choice([2048, 101, 4096, 8999]))
        x = np.stack([_signal(rng, ["tone", "noise", "sparse", "silence"][i % 4], n, 16), _signal(rng, "tone", n, 15)])
        blobs.append(codec.encode_i32(x[None])[0].tobytes())
    stream, offs = _stream(blobs)
    got = []
    for mode in (0, 2):
        capi.lib().sela_hip_debug_standard_first(mode)
        try:
            got.append(_Device(gpu, 24, 2, 9000).decode(stream, offs))
        finally:
            capi.lib().sela_hip_debug_standard_first(-1)
    assert np.array_equal(got[0][0], got[1][0]) and codec.decode_n_status_error(got[0][2]) == 0 and int(got[0][2][3]) == ANY
    assert _same(gpu, stream, offs, 2) == (0, ANY)


# ---- 4. the payload form ------------------------------------------------------------------------------------------------------
def _payload(torch, payload, max_frames, ch, stride, dec=None):
    dec = dec or codec.DecoderN(max_frames, ch, stride)
    buf = torch.zeros(max(len(payload), 4), dtype=torch.uint8, device="cuda")
    if len(payload):
        buf[: len(payload)].copy_(torch.from_numpy(np.frombuffer(bytes(payload), np.uint8).copy()))
    dec.pcm.fill_(SENTINEL)
    pcm, so, fo, count = dec.decode_payload(buf[: len(payload)] if len(payload) else buf[:0], max_frames)
    torch.cuda.synchronize()
    return dec, int(count.item()), pcm.cpu().numpy().reshape(-1), so.cpu().numpy().view(np.uint64), fo.cpu().numpy().view(np.uint64)


def _payload_same(torch, payload, max_frames, ch, stride, dec=None, label=""):
    dec, n, pcm, so, fo = _payload(torch, payload, max_frames, ch, stride, dec)
    want_offs = codec.index_frames(np.frombuffer(bytes(payload), np.uint8) if len(payload) else np.zeros(4, np.uint8), max_frames, ch)
    if not len(payload):
        want_offs = want_offs[:1]
    assert n == len(want_offs) - 1 and np.array_equal(fo[: n + 1], want_offs), label
    rc, hpcm, hso, largest = _host(payload if len(payload) else b"\0" * 4, want_offs, ch)
    st = dec.status.cpu().numpy().view(np.uint32)
    code = codec.decode_n_status_error(st)
    assert (code == rc or (code == -4 and largest > stride)) and int(st[2]) == largest, (label, rc, st)
    assert np.array_equal(so[: n + 1], hso), label
    if rc == 0 and code == 0:
        total = int(hso[n]) * ch
        assert np.array_equal(pcm[:total], hpcm) and (pcm[total:] == SENTINEL).all(), label
    else:
        assert (pcm[max_frames * stride * ch:] == SENTINEL).all(), label
    return code, n


def test_payload_of_the_odd_file(gpu):  # noqa: F811
    blob, pcm = gc.odd_file_bytes(lambda p: codec.encode_host(p[None])[0].tobytes())
    for cap in (8, 5, 12):
        code, n = _payload_same(gpu, blob[15:], cap, 2, 3000, label=cap)
        assert code == 0 and n == min(cap, 8)
    dec = codec.DecoderN(8, 2, 3000)
    out, so, _, count = dec.decode_payload(gpu.from_numpy(np.frombuffer(blob[15:], np.uint8).copy()).cuda())
    dec.check()
    assert dec.route() == ANY and int(count.item()) == 8 and int(so[8].item()) == len(pcm)
    assert np.array_equal(out[: len(pcm)].cpu().numpy(), pcm)


def test_payload_at_every_truncation_point(gpu):  # noqa: F811
    blobs = [codec.encode_i32(np.stack([_signal(np.random.default_rng(n), "tone", n, 16), _signal(np.random.default_rng(n + 1), "noise", n, 12)])[None])[0].tobytes()
             for n in (130, 300, 700)]
    payload = b"".join(blobs)
    dec = codec.DecoderN(4, 2, 2048)
    for length in range(0, len(payload) + 1, 3):
        _payload_same(gpu, payload[:length], 4, 2, 2048, dec, label=length)
    _payload_same(gpu, payload, 4, 2, 2048, dec, label="whole")


def test_payload_without_frames(gpu):  # noqa: F811
    for payload in (b"", b"\0" * 64, bytes.fromhex("00ff55aa") + b"\x07" * 60):
        dec, n, pcm, so, fo = _payload(gpu, payload, 4, 2, 128)
        st = dec.status.cpu().numpy().view(np.uint32)
        assert n == 0 and (st == 0).all() and int(so[0]) == 0, payload[:8]
        assert (pcm == SENTINEL).all()


def test_payload_of_more_than_a_tile(gpu):  # noqa: F811
    parts = []
    for i, n in enumerate((1000, 2048, 3000, 777) * 2):
        parts.append(codec.encode_host(synth_frames(550, 2, 20 + i)[:, : n] if n <= 2048 else np.tile(synth_frames(550, 2, 20 + i), (1, 2, 1))[:, :n])[0].tobytes())
    payload = b"".join(parts)
    assert _payload_same(gpu, payload, 4400, 2, 3000, label="4400") == (0, 4400)
    assert _payload_same(gpu, payload, 4500, 2, 3000, label="4500 cap") == (0, 4400)
    assert _payload_same(gpu, payload, 4400, 2, 2048, label="small stride") == (-4, 4400)
    track = codec.encode_host(synth_frames(4500, 2, 4))[0].tobytes()
    dec = codec.DecoderN(4500, 2, 2048)
    assert _payload_same(gpu, track, 4500, 2, 2048, dec, label="2048 x 4500") == (0, 4500)
    assert dec.route() == FAST


# ---- 5. graph capture ---------------------------------------------------------------------------------------------------------
def _mixed(n_frames, seed):
    rng = np.random.default_rng(seed)
    blobs = []
    for _ in range(n_frames):
        n = int(rng.integers(200, 3000))
        blobs.append(codec.encode_i32(np.stack([_signal(rng, "tone", n, 16), _signal(rng, "sparse", n, 14)])[None])[0].tobytes())
    return b"".join(blobs)


def test_payload_decode_in_a_graph(gpu):  # noqa: F811
    torch = gpu
    a, b = _mixed(30, 1), _mixed(21, 2)
    assert len(b) <= len(a)
    dec = codec.DecoderN(32, 2, 3000)
    buf = torch.from_numpy(np.frombuffer(a, np.uint8).copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.decode_payload(buf)  # (the workspace is allocated here, not under capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pcm, so, fo, count = dec.decode_payload(buf)
    buf.zero_()
    buf[: len(b)].copy_(torch.from_numpy(np.frombuffer(b, np.uint8).copy()))
    graph.replay()
    torch.cuda.synchronize()
    eager, n, want_pcm, want_so, want_fo = _payload(torch, b, 32, 2, 3000)
    assert int(count.item()) == n == 21
    assert np.array_equal(so[: n + 1].cpu().numpy().view(np.uint64), want_so[: n + 1])
    assert np.array_equal(fo[: n + 1].cpu().numpy().view(np.uint64), want_fo[: n + 1])
    total = int(want_so[n]) * 2
    assert np.array_equal(pcm.cpu().numpy().reshape(-1)[:total], want_pcm[:total])
    assert np.array_equal(dec.status.cpu().numpy(), eager.status.cpu().numpy()) and dec.route() == ANY


# ---- 6. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    blob = codec.encode_i32(np.stack([_signal(np.random.default_rng(0), "tone", 500, 16)] * 2)[None])[0].tobytes()
    n = len(blob)
    buf = torch.from_numpy(np.frombuffer(blob + b"\0" * 4, np.uint8).copy()).cuda()
    offs = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    ws_bytes = int(lib.sela_hip_decode_n_workspace_bytes(4, 2, 500))
    ix_bytes = int(lib.sela_hip_index_workspace_bytes(n, 4))
    ws = torch.empty(ws_bytes + ix_bytes, dtype=torch.uint8, device="cuda")
    out = torch.full((4 * 500 * 2,), SENTINEL, dtype=torch.int16, device="cuda")
    so = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    fo = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    nf = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def dev(frames=buf.data_ptr(), o=offs.data_ptr(), nfr=1, channels=2, stride=500, p=out.data_ptr(), st=status.data_ptr(), w=ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_decode_n_device(frames, o, nfr, channels, stride, p, so.data_ptr(), st, w, wb, stream)

    def pay(payload=buf.data_ptr(), channels=2, stride=500, p=out.data_ptr(), st=status.data_ptr(), o=fo.data_ptr(), k=nf.data_ptr(), w=ws.data_ptr(),
            wb=ws_bytes + ix_bytes):
        return lib.sela_hip_decode_payload_n_device(payload, n, 4, channels, stride, p, so.data_ptr(), o, k, st, w, wb, stream)

    for call, code in [(lambda: dev(frames=buf.data_ptr() + 1), -2), (lambda: dev(channels=0), -2), (lambda: dev(channels=256), -2),
                       (lambda: dev(stride=0), -2), (lambda: dev(p=None), -2), (lambda: dev(st=None), -2),
                       (lambda: dev(w=None), -2), (lambda: dev(o=None), -2), (lambda: dev(frames=None), -2),
                       (lambda: dev(wb=int(lib.sela_hip_decode_n_workspace_bytes(1, 2, 500)) - 1), -4),
                       (lambda: dev(nfr=0x40000000), -2),
                       (lambda: pay(payload=buf.data_ptr() + 2), -2), (lambda: pay(channels=0), -2), (lambda: pay(channels=256), -2),
                       (lambda: pay(stride=0), -2), (lambda: pay(p=None), -2), (lambda: pay(st=None), -2),
                       (lambda: pay(o=None), -2), (lambda: pay(k=None), -2), (lambda: pay(w=None), -2),
                       (lambda: pay(wb=ws_bytes + ix_bytes - 1), -4)]:
        assert call() == code
    torch.cuda.synchronize()  # nothing was enqueued: every output is as it was
    assert (out.cpu().numpy() == SENTINEL).all() and (so.cpu().numpy() == -1).all() and (fo.cpu().numpy() == -1).all()
    assert (status.cpu().numpy() == -1).all() and int(nf.item()) == -1
    # a workspace of the size asked for is enough, and no initialisation is needed
    ws.fill_(0xFF)
    assert dev(wb=int(lib.sela_hip_decode_n_workspace_bytes(1, 2, 500))) == 0
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert codec.decode_n_status_error(st) == 0 and int(st[2]) == 500 and int(st[3]) == ANY
    # no frames at all: a clean status, the one sample offset
    so.fill_(-1)
    assert dev(nfr=0) == 0
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and int(so[0].item()) == 0 and int(so[1].item()) == -1
