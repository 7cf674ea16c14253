"""sela_hip_decode_i32_device and sela_hip_decode_payload_i32_device: the 32-bit decode of any length on device pointers is the
host-pointer sela_hip_decode_i32 bit for bit -- samples up to each count, the counts, sela_hip_index_samples' sample offsets,
status[2] -- wherever the host call returns 0, and sela_hip_decode_status_error(device status) is the host call's code on every
input.  (The host calls are pinned to the oracle and the reference by test_gpu_decode_any_length.py, test_gpu_wide_samples.py and
the golden suites.)"""
import struct

import numpy as np
import pytest

import generic_cases as gc
import wide_cases as wc
from gpu_common import DECODE_LENGTHS, ENCODE_LENGTHS, _build_frame, _hostile_frame, _one, _rice_words, _signal, gpu  # noqa: F401
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

GUARD = 1024  # words behind the samples and the counts that no call may write
SENTINEL = 0x5EA15EA1


def _host(blob, offs, ch, stride):
    """sela_hip_decode_i32 and sela_hip_index_samples on host pointers -> (rc, samples, counts, sample offsets, largest)."""
    lib = capi.lib()
    fr = np.ascontiguousarray(np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else blob, np.uint8)
    fr = fr if len(fr) else np.zeros(4, np.uint8)
    o = np.ascontiguousarray(offs, np.uint64)
    n = len(o) - 1
    out = np.zeros((max(n, 1), ch, stride), np.int32)
    counts = np.zeros((max(n, 1), ch), np.uint32)
    rc = lib.sela_hip_decode_i32(fr.ctypes.data, o.ctypes.data, n, ch, out.ctypes.data, stride, counts.ctypes.data)
    so = np.zeros(n + 1, np.uint64)
    largest = lib.sela_hip_index_samples(fr.ctypes.data, o.ctypes.data, n, ch, so.ctypes.data)
    return rc, out[:n], counts[:n], so, int(largest)


class _Device:
    """Device buffers for one call of sela_hip_decode_i32_device, with guard words behind the samples and the counts."""

    def __init__(self, torch, n, ch, stride):
        self.torch, self.n, self.ch, self.stride = torch, n, ch, stride
        self.samples = torch.full((n * ch * stride + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.counts = torch.full((n * ch + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.sample_offsets = torch.full((n + 1 + GUARD,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(int(capi.lib().sela_hip_decode_i32_workspace_bytes(n, ch, stride)), dtype=torch.uint8, device="cuda")

    def decode(self, blob, offs):
        torch = self.torch
        data = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, np.uint8)
        frames = torch.zeros(max(len(data), 4), dtype=torch.uint8, device="cuda")
        if len(data):
            frames[: len(data)].copy_(torch.from_numpy(data.copy()))
        o = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).cuda()
        capi.check(capi.lib().sela_hip_decode_i32_device(
            frames.data_ptr(), o.data_ptr(), self.n, self.ch, self.stride, self.samples.data_ptr(), self.counts.data_ptr(),
            self.sample_offsets.data_ptr(), self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return self.results()

    def results(self):
        n, ch, stride = self.n, self.ch, self.stride
        s = self.samples.cpu().numpy()
        c = self.counts.cpu().numpy()
        so = self.sample_offsets.cpu().numpy()
        assert (s[n * ch * stride:] == SENTINEL).all() and (c[n * ch:] == SENTINEL).all(), "written past the outputs"
        assert (so[n + 1:] == -1).all(), "written past the sample offsets"
        st = self.status.cpu().numpy().view(np.uint32).copy()
        return s[: n * ch * stride].reshape(n, ch, stride), c[: n * ch].reshape(n, ch).view(np.uint32), so[: n + 1].view(np.uint64), st


def _same(torch, blob, offs, ch, stride=None, mode=-1, label=""):
    """Device call == host call on (blob, offs) under debug mode `mode` -> the host call's code."""
    lib = capi.lib()
    offs = np.ascontiguousarray(offs, np.uint64)
    n = len(offs) - 1
    if stride is None:
        fr = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else blob
        stride = max(codec.index_samples(fr if len(fr) else np.zeros(4, np.uint8), offs, ch)[1], 1)
    lib.sela_hip_debug_standard_first(mode)
    try:
        rc, out, counts, so, largest = _host(blob, offs, ch, stride)
        d_out, d_counts, d_so, st = _Device(torch, n, ch, stride).decode(blob, offs)
    finally:
        lib.sela_hip_debug_standard_first(-1)
    assert codec.decode_status_error(st) == rc, (label, mode, rc, st)
    if (offs[1:] >= offs[:-1]).all():  # (decreasing offsets: sela_hip_index_samples writes no sample offsets at all)
        assert np.array_equal(d_so, so), (label, mode)
    assert int(st[2]) == largest and int(st[3]) == 0, (label, mode, st, largest)
    assert bool(st[0] & capi.FLAG_STRIDE) == (rc == -4), (label, st)
    if rc == 0:
        assert int(st[0]) == 0 and int(st[1]) == 0, (label, st)
        assert np.array_equal(d_counts, counts), (label, mode)
        for f in range(n):
            for c in range(ch):
                k = int(counts[f, c])
                assert np.array_equal(d_out[f, c, :k], out[f, c, :k]), (label, mode, f, c)
    return rc


def _stream(blobs):
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)


# ---- 1. streams the encoders make ---------------------------------------------------------------------------------------------
def test_generic_cases_narrow_and_wide(gpu):  # noqa: F811
    for label, n, kind, wide in gc.all_cases():
        frames, offs = codec.encode_i32(gc.case_input(n, kind, wide)[None])
        assert _same(gpu, frames, offs, {"mono": 1, "three": 3}.get(kind, 2), label=label) == 0


@pytest.mark.parametrize("n", sorted(set(DECODE_LENGTHS) | set(ENCODE_LENGTHS)))
def test_encoder_streams_of_every_length(gpu, n):  # noqa: F811
    rng = np.random.default_rng(n)
    taken = 0
    for kinds, bits in ((("tone", "noise"), 16), (("sparse",), 16), (("tone", "silence", "dc"), 21)):
        x = np.stack([_signal(rng, k, n, bits) for k in kinds])
        try:
            frames, offs = codec.encode_i32(np.stack([x, x[:, ::-1].copy()]))  # (two frames per call)
        except capi.SelaHipError:  # (a block not longer than its own order: the encoder refuses it)
            assert n <= 100
            continue
        assert _same(gpu, frames, offs, len(kinds), label=(n, kinds)) == 0
        taken += 1
    assert taken or n <= 100


def test_ragged_frames(gpu):  # noqa: F811
    blobs = []
    for label, chans in gc.ragged_cases():
        blob = codec.encode_ragged(chans)
        assert _same(gpu, blob, _one(len(blob)), len(chans), label=label) == 0
        if len(chans) == 2:
            blobs.append(blob)
    stream, offs = _stream(blobs)  # (several in one call)
    assert _same(gpu, stream, offs, 2, label="ragged stereo together") == 0


def test_odd_file_and_a_long_rice_subframe(gpu):  # noqa: F811
    blob, _ = gc.odd_file_bytes(lambda pcm: codec.encode_host(pcm[None])[0].tobytes())
    payload = np.frombuffer(blob[15:], np.uint8).copy()
    offs = codec.index_frames(payload, 8, 2)
    assert len(offs) == 9
    assert _same(gpu, payload, offs, 2, label="odd file") == 0
    v, _, _ = gc.long_rice_stream()  # (its first 65535 values: the longest subframe the format carries, ~30 k Rice words)
    rng = np.random.default_rng(3)
    frame = _build_frame([(0, 0, 0, rng.integers(-4, 5, 2).astype(np.int32), v[:65535])])
    assert _same(gpu, frame, _one(len(frame)), 1, label="long rice") == 0


def test_wide_frames(gpu):  # noqa: F811
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
        assert _same(gpu, stream, offs, 2, mode=mode, label="wide stereo") == 0
    cases = wc.stage_cases(2048, rng, wc.FRAME_RESIDUES)
    clean = 0
    for i, order in enumerate(wc.ORDERS):
        blob = wc.frame_bytes(o, [(0, 0, 0, wc.fold_coefficients(order, rng), cases[i % len(cases)][1]),
                                  (1, 0, 1, wc.fold_coefficients(wc.ORDERS[-1 - i], rng), cases[(i + 3) % len(cases)][1])])
        for mode in (-1, 2, 0):
            clean += _same(gpu, blob, _one(len(blob)), 2, mode=mode, label=("wide order", order)) == 0
    assert clean >= len(wc.ORDERS)


def test_a_batch_that_mixes_lengths(gpu):  # noqa: F811
    rng = np.random.default_rng(77)
    blobs = []
    for i in range(60):
        n = int(rng.integers(101, 9000)) if i % 5 else int(rng.choice([2048, 101, 4096, 8999]))
        kind = ["tone", "noise", "sparse", "silence"][i % 4]
        x = np.stack([_signal(rng, kind, n, 16), _signal(rng, "tone", n, 15)])
        blobs.append(codec.encode_i32(x[None])[0].tobytes())
    stream, offs = _stream(blobs)
    for mode in (-1, 2, 0):
        assert _same(gpu, stream, offs, 2, mode=mode, label="mixed") == 0
    assert _same(gpu, stream, offs, 2, stride=9000, label="roomy stride") == 0


# ---- 2. the crafted KATs ------------------------------------------------------------------------------------------------------
def test_crafted_kats(gpu, generic_kats):  # noqa: F811
    for name in generic_kats["crafted_names"]:
        blob = generic_kats[f"crafted/{name}/bytes"]
        ch = int(generic_kats[f"crafted/{name}/channels"])
        want = [generic_kats[f"crafted/{name}/decoded{c}"] for c in range(ch)]
        stride = max(max(len(w) for w in want), 1)
        for mode in (-1, 2, 0):
            assert _same(gpu, blob, _one(len(blob)), ch, stride=stride, mode=mode, label=name) == 0
        d_out, d_counts, _, st = _Device(gpu, 1, ch, stride).decode(blob, _one(len(blob)))
        for c in range(ch):
            assert np.array_equal(d_out[0, c, : int(d_counts[0, c])], want[c]), (name, c)


# ---- 3. hostile streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["short", "long"])
def test_hostile_streams_under_every_route(gpu, shape):  # noqa: F811
    rng = np.random.default_rng(7 if shape == "short" else 8)
    trials, n_lo, n_hi = (80, 1, 700) if shape == "short" else (16, 3000, 30000)
    codes = {}
    for trial in range(trials):
        ch = int(rng.integers(1, 4))
        blob = _hostile_frame(rng, ch, n_lo, n_hi, shape == "long")
        for mode in (1, 2, 0):
            rc = _same(gpu, blob, _one(len(blob)), ch, mode=mode, label=(shape, trial))
            codes[rc] = codes.get(rc, 0) + 1
    assert codes.get(0, 0) >= trials // 5 and codes.get(-5, 0) + codes.get(-6, 0) >= trials // 10, codes


def _sub(c, typ, parent, order, q, ck, res, rk, n=None):
    cw = _rice_words(np.asarray(q, np.int32), ck) if order else np.zeros(0, np.uint32)
    rw = _rice_words(np.asarray(res, np.int32), rk)
    return (struct.pack("<BBBBHB", c, typ, parent, ck, len(cw), order) + cw.tobytes()
            + struct.pack("<BHH", rk, len(rw), len(res) if n is None else n) + rw.tobytes())


def test_crafted_hostile_shapes(gpu):  # noqa: F811
    """Orders above 100, coefficients outside the tables, a dry Rice stream, subframes not longer than their order, frames at odd
    offsets, decreasing offsets -- each alone and next to a good frame, under the three routes."""
    rng = np.random.default_rng(9)
    good = _sub(0, 0, 0, 2, [-40, 10], 4, rng.integers(-300, 301, 500), 8)
    frames = {
        "order 101": _sub(0, 0, 0, 101, rng.integers(-3, 4, 101), 3, rng.integers(-9, 9, 600), 4),
        "order 200": struct.pack("<BBBBHB", 0, 0, 0, 3, 0, 200) + struct.pack("<BHH", 4, 1, 5) + b"\0" * 4,
        "out of table": _sub(0, 0, 0, 3, [-40, 90, 3], 8, rng.integers(-9, 9, 600), 4),
        "dry": _sub(0, 0, 0, 2, [-40, 10], 4, np.full(400, 1000), 2, n=4000),
        "short": _sub(0, 0, 0, 20, rng.integers(-3, 4, 20), 3, rng.integers(-9, 9, 20), 4),
        "empty": _sub(0, 0, 0, 0, [], 0, np.zeros(0, np.int32), 0),
    }
    sync = bytes.fromhex("00ff55aa")
    for name, sub in frames.items():
        blob = sync + sub
        for mode in (1, 2, 0):
            assert _same(gpu, blob, _one(len(blob)), 1, stride=4096, mode=mode, label=name) != 0
            stream, offs = _stream([sync + good, blob, sync + good])
            assert _same(gpu, stream, offs, 1, stride=4096, mode=mode, label=name + " between good ones") != 0
    a, b = sync + good, sync + _sub(0, 0, 0, 1, [-50], 3, rng.integers(-99, 99, 777), 6)
    stream = np.frombuffer(a + b"\x00" + b, np.uint8).copy()
    for mode in (1, 2, 0):
        assert _same(gpu, stream, np.array([0, len(a) + 1, len(a) + 1 + len(b)], np.uint64), 1, mode=mode, label="odd offset") == 0
        stream2, offs2 = _stream([a, b, a])
        offs2[2] = offs2[1] - 4  # decreasing: EFORMAT from the host call, a malformed frame on the device
        assert _same(gpu, stream2, offs2, 1, stride=1000, mode=mode, label="decreasing") == -5


# ---- 4. the stride ------------------------------------------------------------------------------------------------------------
def test_a_stride_too_small(gpu):  # noqa: F811
    lengths = (300, 5000, 2048, 777)
    blobs = [codec.encode_i32(np.stack([_signal(np.random.default_rng(n), "tone", n, 16)] * 2)[None])[0].tobytes() for n in lengths]
    stream, offs = _stream(blobs)
    for stride in (1, 299, 2048, 4999):
        assert _same(gpu, stream, offs, 2, stride=stride, label=stride) == -4
        _, _, _, st = _Device(gpu, 4, 2, stride).decode(stream, offs)
        assert int(st[2]) == 5000 and st[0] & capi.FLAG_STRIDE
    assert _same(gpu, stream, offs, 2, stride=5000) == 0
    # a broken frame further on: the host walk gives 0, no ECAPACITY -- the decode finds the malformed frame
    broken = blobs[:3] + [blobs[3][:40]]
    stream, offs = _stream(broken)
    for stride in (299, 2048):
        assert _same(gpu, stream, offs, 2, stride=stride, label=("broken", stride)) == -5
        _, _, _, st = _Device(gpu, 4, 2, stride).decode(stream, offs)
        assert int(st[2]) == 0 and not st[0] & capi.FLAG_STRIDE


# ---- 5. the payload form ------------------------------------------------------------------------------------------------------
def _payload_decode(torch, payload, max_frames, ch, stride, dec=None):
    dec = dec or codec.Decoder32(max_frames, ch, stride)
    buf = torch.zeros(max(len(payload), 4), dtype=torch.uint8, device="cuda")
    if len(payload):
        buf[: len(payload)].copy_(torch.from_numpy(np.frombuffer(bytes(payload), np.uint8).copy()))
    dec.samples.fill_(SENTINEL)
    dec.counts.fill_(SENTINEL)
    samples, counts, so, fo, count = dec.decode_payload(buf[: len(payload)] if len(payload) else buf[:0], max_frames)
    torch.cuda.synchronize()
    n = int(count.item())
    return dec, n, samples.cpu().numpy(), counts.cpu().numpy().view(np.uint32), so.cpu().numpy().view(np.uint64), fo.cpu().numpy().view(np.uint64)


def _payload_same(torch, payload, max_frames, ch, stride, label=""):
    dec, n, samples, counts, so, fo = _payload_decode(torch, payload, max_frames, ch, stride)
    want_offs = codec.index_frames(np.frombuffer(bytes(payload), np.uint8) if len(payload) else np.zeros(4, np.uint8), max_frames, ch)
    if not len(payload):
        want_offs = want_offs[:1]
    assert n == len(want_offs) - 1 and np.array_equal(fo[: n + 1], want_offs), label
    rc, out, hc, hso, largest = _host(payload, want_offs, ch, stride)
    st = dec.status.cpu().numpy().view(np.uint32)
    assert codec.decode_status_error(st) == rc and int(st[2]) == largest, (label, rc, st)
    assert np.array_equal(so[: n + 1], hso), label
    assert (samples[n:] == SENTINEL).all() and (counts[n:] == SENTINEL).all(), (label, "frames beyond the count written")
    if rc == 0:
        assert np.array_equal(counts[:n], hc), label
        for f in range(n):
            for c in range(ch):
                k = int(hc[f, c])
                assert np.array_equal(samples[f, c, :k], out[f, c, :k]), (label, f, c)
    return rc, n


def test_payload_of_the_odd_file(gpu):  # noqa: F811
    blob, pcm = gc.odd_file_bytes(lambda p: codec.encode_host(p[None])[0].tobytes())
    for cap in (8, 5, 12):
        rc, n = _payload_same(gpu, blob[15:], cap, 2, 3000, label=cap)
        assert rc == 0 and n == min(cap, 8)
    dec = codec.Decoder32(8, 2, 3000)
    buf = gpu.from_numpy(np.frombuffer(blob[15:], np.uint8).copy()).cuda()
    samples, counts, so, _, count = dec.decode_payload(buf)
    dec.check()
    got = np.concatenate([samples[f, :, : int(counts[f, 0])].cpu().numpy().T for f in range(int(count.item()))])
    assert np.array_equal(got, pcm.astype(np.int32)) and int(so[8].item()) == len(pcm)


def test_payload_of_more_than_a_tile(gpu):  # noqa: F811
    """4400 stereo frames of 777 .. 3000 samples: the multi-launch index and the multi-workgroup sample scan."""
    parts = []
    for i, n in enumerate((1000, 2048, 3000, 777) * 2):
        parts.append(codec.encode_host(synth_frames(550, 2, 20 + i)[:, : n] if n <= 2048 else np.tile(synth_frames(550, 2, 20 + i), (1, 2, 1))[:, :n])[0].tobytes())
    payload = b"".join(parts)
    rc, n = _payload_same(gpu, payload, 4400, 2, 3000, label="4400")
    assert rc == 0 and n == 4400
    rc, n = _payload_same(gpu, payload, 4500, 2, 3000, label="4500 cap")
    assert rc == 0 and n == 4400
    rc, n = _payload_same(gpu, payload, 4400, 2, 2048, label="small stride")
    assert rc == -4 and n == 4400


def test_payload_at_every_truncation_point(gpu):  # noqa: F811
    blobs = [codec.encode_i32(np.stack([_signal(np.random.default_rng(n), "tone", n, 16), _signal(np.random.default_rng(n + 1), "noise", n, 12)])[None])[0].tobytes()
             for n in (130, 300, 700)]
    payload = b"".join(blobs)
    dec = codec.Decoder32(4, 2, 2048)
    for length in range(len(payload) + 1):
        cut = payload[:length]
        _, n, samples, counts, so, fo = _payload_decode(gpu, cut, 4, 2, 2048, dec)
        want = codec.index_frames(np.frombuffer(cut, np.uint8) if length else np.zeros(4, np.uint8), 4, 2)[: (None if length else 1)]
        assert n == len(want) - 1 and np.array_equal(fo[: n + 1], want), length
        rc, out, hc, hso, largest = _host(cut, want, 2, 2048)
        st = dec.status.cpu().numpy().view(np.uint32)
        assert codec.decode_status_error(st) == rc and int(st[2]) == largest and np.array_equal(so[: n + 1], hso), length
        assert (samples[n:] == SENTINEL).all() and (counts[n:] == SENTINEL).all(), length
        if rc == 0:
            assert np.array_equal(counts[:n], hc), length
            for f in range(n):
                for c in range(2):
                    assert np.array_equal(samples[f, c, : hc[f, c]], out[f, c, : hc[f, c]]), (length, f, c)


def test_payload_without_frames(gpu):  # noqa: F811
    for payload in (b"", b"\0" * 64, bytes.fromhex("00ff55aa") + b"\x07" * 60):
        dec, n, samples, counts, so, fo = _payload_decode(gpu, payload, 4, 2, 128)
        st = dec.status.cpu().numpy().view(np.uint32)
        assert n == 0 and (st == 0).all() and int(so[0]) == 0, payload[:8]
        assert (samples == SENTINEL).all() and (counts == SENTINEL).all()


# ---- 6. the 2048 x int16 shape ------------------------------------------------------------------------------------------------
def test_bench_sized_track(gpu):  # noqa: F811
    frames, offs = codec.encode_host(synth_frames(3875, 2, 0))
    pcm = codec.decode_host(frames, offs, 2)
    dec = codec.Decoder32(3875, 2, 2048)
    samples, counts, so = dec.decode(gpu.from_numpy(frames).cuda(), gpu.from_numpy(offs.view(np.int64)).cuda(), 3875)
    dec.check()
    assert (counts.cpu().numpy() == 2048).all() and np.array_equal(so.cpu().numpy(), np.arange(3876) * 2048)
    assert np.array_equal(samples.cpu().numpy().transpose(0, 2, 1), pcm.astype(np.int32))
    buf = gpu.from_numpy(frames).cuda()
    samples, counts, so, fo, count = dec.decode_payload(buf)
    dec.check()
    assert int(count.item()) == 3875 and np.array_equal(fo.cpu().numpy().view(np.uint64), offs)
    assert np.array_equal(samples.cpu().numpy().transpose(0, 2, 1), pcm.astype(np.int32))


# ---- 7. graph capture and concurrency -----------------------------------------------------------------------------------------
def _mixed(n_frames, seed):
    rng = np.random.default_rng(seed)
    blobs = []
    for i in range(n_frames):
        n = int(rng.integers(200, 3000))
        blobs.append(codec.encode_i32(np.stack([_signal(rng, "tone", n, 16), _signal(rng, "sparse", n, 14)])[None])[0].tobytes())
    return b"".join(blobs)


def test_payload_decode_in_a_graph_and_on_two_streams(gpu):  # noqa: F811
    torch = gpu
    a, b = _mixed(30, 1), _mixed(21, 2)
    assert len(b) <= len(a)
    dec = codec.Decoder32(32, 2, 3000)
    buf = torch.from_numpy(np.frombuffer(a, np.uint8).copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.decode_payload(buf)  # (the workspace is allocated here, not under capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        samples, counts, so, fo, count = dec.decode_payload(buf)
    buf.zero_()
    buf[: len(b)].copy_(torch.from_numpy(np.frombuffer(b, np.uint8).copy()))
    graph.replay()
    torch.cuda.synchronize()
    want = _payload_decode(torch, b, 32, 2, 3000)
    n = int(count.item())
    assert n == want[1] == 21
    assert np.array_equal(counts[:n].cpu().numpy().view(np.uint32), want[3][:n])
    assert np.array_equal(so[: n + 1].cpu().numpy().view(np.uint64), want[4][: n + 1])
    assert np.array_equal(fo[: n + 1].cpu().numpy().view(np.uint64), want[5][: n + 1])
    got = samples.cpu().numpy()
    for f in range(n):
        for c in range(2):
            k = int(want[3][f, c])
            assert np.array_equal(got[f, c, :k], want[2][f, c, :k]), (f, c)
    assert np.array_equal(dec.status.cpu().numpy(), want[0].status.cpu().numpy())

    decs = [codec.Decoder32(32, 2, 3000), codec.Decoder32(32, 2, 3000)]
    blobs = [a, b]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    payloads = [torch.from_numpy(np.frombuffer(x, np.uint8).copy()).cuda() for x in blobs]
    torch.cuda.synchronize()
    outs = []
    for d, s, p in zip(decs, streams, payloads):
        with torch.cuda.stream(s):
            outs.append(d.decode_payload(p))
    torch.cuda.synchronize()
    for (samples, counts, so, fo, count), blob in zip(outs, blobs):
        want_offs = codec.index_frames(np.frombuffer(blob, np.uint8), 32, 2)
        n = int(count.item())
        assert n == len(want_offs) - 1 and np.array_equal(fo[: n + 1].cpu().numpy().view(np.uint64), want_offs)
        rc, out, hc, hso, _ = _host(blob, want_offs, 2, 3000)
        assert rc == 0 and np.array_equal(counts[:n].cpu().numpy().view(np.uint32), hc) and np.array_equal(so[: n + 1].cpu().numpy().view(np.uint64), hso)
        got = samples.cpu().numpy()
        for f in range(n):
            for c in range(2):
                assert np.array_equal(got[f, c, : hc[f, c]], out[f, c, : hc[f, c]])


# ---- 8. argument errors and the workspace -------------------------------------------------------------------------------------
def test_argument_errors(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    blob = codec.encode_i32(np.stack([_signal(np.random.default_rng(0), "tone", 500, 16)] * 2)[None])[0].tobytes()
    n = len(blob)
    buf = torch.from_numpy(np.frombuffer(blob + b"\0" * 4, np.uint8).copy()).cuda()
    offs = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    ws_bytes = int(lib.sela_hip_decode_i32_workspace_bytes(4, 2, 500))
    ix_bytes = int(lib.sela_hip_index_workspace_bytes(n, 4))
    ws = torch.empty(ws_bytes + ix_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((4, 2, 500), dtype=torch.int32, device="cuda")
    cnt = torch.empty(8, dtype=torch.int32, device="cuda")
    so = torch.empty(5, dtype=torch.int64, device="cuda")
    fo = torch.empty(5, dtype=torch.int64, device="cuda")
    nf = torch.empty(1, dtype=torch.int32, device="cuda")
    status = torch.empty(4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def dev(frames=buf.data_ptr(), o=offs.data_ptr(), nfr=1, channels=2, stride=500, s=out.data_ptr(), c=cnt.data_ptr(), st=status.data_ptr(),
            w=ws.data_ptr(), wb=ws_bytes):
        return lib.sela_hip_decode_i32_device(frames, o, nfr, channels, stride, s, c, so.data_ptr(), st, w, wb, stream)

    def pay(payload=buf.data_ptr(), channels=2, stride=500, s=out.data_ptr(), c=cnt.data_ptr(), st=status.data_ptr(), o=fo.data_ptr(),
            k=nf.data_ptr(), w=ws.data_ptr(), wb=ws_bytes + ix_bytes):
        return lib.sela_hip_decode_payload_i32_device(payload, n, 4, channels, stride, s, c, so.data_ptr(), o, k, st, w, wb, stream)

    assert dev() == 0 and pay() == 0
    torch.cuda.synchronize()
    for call, code in [(lambda: dev(frames=buf.data_ptr() + 1), -2), (lambda: dev(channels=0), -2), (lambda: dev(channels=256), -2),
                       (lambda: dev(stride=0), -2), (lambda: dev(s=None), -2), (lambda: dev(c=None), -2), (lambda: dev(st=None), -2),
                       (lambda: dev(w=None), -2), (lambda: dev(o=None), -2), (lambda: dev(frames=None), -2),
                       (lambda: dev(wb=int(lib.sela_hip_decode_i32_workspace_bytes(1, 2, 500)) - 1), -4),
                       (lambda: dev(nfr=0x40000000), -2),
                       (lambda: pay(payload=buf.data_ptr() + 2), -2), (lambda: pay(channels=0), -2), (lambda: pay(channels=256), -2),
                       (lambda: pay(stride=0), -2), (lambda: pay(s=None), -2), (lambda: pay(c=None), -2), (lambda: pay(st=None), -2),
                       (lambda: pay(o=None), -2), (lambda: pay(k=None), -2), (lambda: pay(w=None), -2),
                       (lambda: pay(wb=ws_bytes + ix_bytes - 1), -4)]:
        assert call() == code
    # what one frame needs is less than what four do; a workspace of the size asked for is enough, and no initialisation is needed
    assert int(lib.sela_hip_decode_i32_workspace_bytes(1, 2, 500)) < ws_bytes
    ws.fill_(0xFF)
    status.fill_(-1)
    assert dev(wb=int(lib.sela_hip_decode_i32_workspace_bytes(1, 2, 500))) == 0
    torch.cuda.synchronize()
    assert codec.decode_status_error(status.cpu().numpy()) == 0 and int(status[2].item()) == 500 and int(status[3].item()) == 0
    # no frames at all: a clean status, the one sample offset
    so.fill_(-1)
    assert dev(nfr=0) == 0
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and int(so[0].item()) == 0 and int(so[1].item()) == -1
