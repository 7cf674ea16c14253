"""sela_hip_encode_i32_device and sela_hip_encode_n_device: the any-length / 32-bit encode on device pointers is the host-pointer
sela_hip_encode_i32 / sela_hip_encode bit for bit -- frame bytes and offsets -- wherever the host call returns 0, and
sela_hip_encode_status_error(device status) is the host call's code on every input.  (The host calls are pinned to the oracle and
the reference by test_gpu_encode_any_length.py, test_gpu_wide_samples.py and the golden suites.)  Every buffer the device call
writes starts poisoned: the status words, the workspace and the frames need no initialisation."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import generic_cases as gc
import wide_cases as wc
from gpu_common import ENCODE_LENGTHS, _signal, _wrap_taps, gpu  # noqa: F401
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes behind the frames (and entries behind the offsets) that no call may write
POISON = 0xA5
KINDS = ("silence", "dc", "noise", "tone", "sparse")


def _host(x, in16=False):
    """The host call on x (int32 [n_frames, ch, n], or int16 [n_frames, n, ch] with in16) -> (rc, frames bytes, offsets)."""
    lib = capi.lib()
    x = np.ascontiguousarray(x)
    nf = x.shape[0]
    ch, n = (x.shape[2], x.shape[1]) if in16 else (x.shape[1], x.shape[2])
    cap = max(int(lib.sela_hip_encode_bound_bytes_n(nf, ch, n)), 16)
    out = np.zeros(cap, np.uint8)
    offs = np.zeros(nf + 1, np.uint64)
    if in16:
        rc = lib.sela_hip_encode(x.ctypes.data, nf, ch, n, out.ctypes.data, cap, offs.ctypes.data)
    else:
        rc = lib.sela_hip_encode_i32(x.ctypes.data, nf, ch, n, out.ctypes.data, cap, offs.ctypes.data)
    return rc, (out[: int(offs[nf])].tobytes() if rc == 0 else None), offs


class _Device:
    """One call's buffers, poisoned: frames (cap + GUARD bytes of POISON), offsets (-1), status (-1), workspace (0xFF)."""

    def __init__(self, torch, nf, ch, n, cap):
        self.torch, self.nf, self.ch, self.n, self.cap = torch, nf, ch, n, cap
        lib = capi.lib()
        self.frames = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.offsets = torch.full((nf + 1 + GUARD // 8,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.full((int(lib.sela_hip_encode_i32_workspace_bytes(nf, ch, n)),), 0xFF, dtype=torch.uint8, device="cuda")

    def launch(self, d_x, in16=False):
        call = capi.lib().sela_hip_encode_n_device if in16 else capi.lib().sela_hip_encode_i32_device
        return call(d_x.data_ptr(), self.nf, self.ch, self.n, self.frames.data_ptr(), self.cap, self.offsets.data_ptr(), self.status.data_ptr(),
                    self.ws.data_ptr(), self.ws.numel(), self.torch.cuda.current_stream().cuda_stream)

    def encode(self, x, in16=False):
        torch = self.torch
        d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        capi.check(self.launch(d_x, in16))
        torch.cuda.synchronize()
        return self.results()

    def results(self):
        nf = self.nf
        fr = self.frames.cpu().numpy()
        o = self.offsets.cpu().numpy()
        assert (o[nf + 1:] == -1).all(), "written past the offsets"
        offs = o[: nf + 1].view(np.uint64).copy()
        assert (fr[self.cap:] == POISON).all(), "written at or past frames_cap"
        end = int(offs[nf])
        if end < len(fr):
            assert (fr[end:] == POISON).all(), "written past offsets[n_frames]"
        st = self.status.cpu().numpy().view(np.uint32).copy()
        assert int(st[2]) == 0 and int(st[3]) == 0, st
        return fr, offs, st


def _same(torch, x, in16=False, cap=None, label=""):
    """Device call == host call on x -> the host call's code."""
    rc, blob, offs = _host(x, in16)
    nf = x.shape[0]
    ch, n = (x.shape[2], x.shape[1]) if in16 else (x.shape[1], x.shape[2])
    if cap is None:
        cap = len(blob) if rc == 0 else int(capi.lib().sela_hip_encode_bound_bytes_n(nf, ch, n))
    fr, d_offs, st = _Device(torch, nf, ch, n, cap).encode(x, in16)
    assert codec.encode_status_error(st) == rc, (label, rc, st)
    if rc == 0:
        assert int(st[0]) & ~capi.FLAG_Q_RANGE == 0 and int(st[1]) == 0, (label, st)
        assert np.array_equal(d_offs, offs), label
        assert fr[: len(blob)].tobytes() == blob, (label, next(i for i in range(len(blob)) if fr[i] != blob[i]))
    return rc


def _frames(rng, nf, ch, n, kinds, bits):
    return np.stack([np.stack([_signal(rng, kinds[(f + c) % len(kinds)], n, bits[(f * ch + c) % len(bits)]) for c in range(ch)]) for f in range(nf)])


# ---- 1. parity over every length, width and channel count ---------------------------------------------------------------------
@pytest.mark.parametrize("n", ENCODE_LENGTHS)
def test_every_length_equals_the_host_call(gpu, n):  # noqa: F811
    rng = np.random.default_rng(1000 + n)
    nf = 3 if n <= 20000 else 1
    codes = {}
    for ch in (1, 2, 3):
        for bits in ((16,), (17,), (24,), (31,), (16, 24, 17)):
            x = _frames(rng, nf, ch, n, KINDS, bits)
            rc = _same(gpu, x, label=(n, ch, bits))
            codes[rc] = codes.get(rc, 0) + 1
        if ch == 2:  # near-copies: the difference candidate wins
            x = _frames(rng, nf, 1, n, ("tone", "noise"), (16,))
            x = np.concatenate([x, x - rng.integers(-2, 3, x.shape).astype(np.int32)], axis=1)
            rc = _same(gpu, x, label=(n, "diff"))
            codes[rc] = codes.get(rc, 0) + 1
        x = _frames(rng, nf, ch, n, ("silence", "dc"), (16, 24))  # (order 1: codes at every length, n = 2 included)
        rc = _same(gpu, x, label=(n, ch, "flat"))
        codes[rc] = codes.get(rc, 0) + 1
    assert codes.get(0, 0) >= 2, codes


def test_255_channels(gpu):  # noqa: F811
    rng = np.random.default_rng(255)
    for n in (64, 129, 300):
        x = _frames(rng, 2, 255, n, KINDS, (16, 17, 24))
        assert _same(gpu, x, label=("255", n)) in (0, -6)
        x = _frames(rng, 2, 255, n, ("tone", "silence", "dc"), (16,))
        assert _same(gpu, x, label=("255 tone", n)) in (0, -6)
        x = _frames(rng, 2, 255, n, ("silence", "dc"), (16, 24))
        assert _same(gpu, x, label=("255 flat", n)) == 0


# ---- 2. the int16 entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [101, 1000, 2047, 2048, 2049, 4096, 20000])
def test_int16_entry_equals_sela_hip_encode(gpu, n):  # noqa: F811
    rng = np.random.default_rng(n)
    for ch in (1, 2, 3):
        planar = _frames(rng, 4, ch, n, ("tone", "noise", "sparse", "dc"), (15,))
        pcm = np.ascontiguousarray(planar.transpose(0, 2, 1).astype(np.int16))
        assert _same(gpu, pcm, in16=True, label=(n, ch)) == 0
        # the int16 and the int32 entries: the same frames
        fr16, o16, _ = _Device(gpu, 4, ch, n, 1 << 22).encode(pcm, in16=True)
        fr32, o32, _ = _Device(gpu, 4, ch, n, 1 << 22).encode(planar.astype(np.int32))
        assert np.array_equal(o16, o32) and np.array_equal(fr16[: int(o16[4])], fr32[: int(o32[4])])
    if n == 2048:  # and the fast kernels' device call
        pcm = synth_frames(24, 2, 3)
        enc = codec.Encoder(24, 2)
        out = enc.encode(gpu.from_numpy(pcm).cuda())
        gpu.cuda.synchronize()
        fast, fast_offs = out.to_host()
        fr, offs, st = _Device(gpu, 24, 2, 2048, len(fast)).encode(pcm, in16=True)
        assert codec.encode_status_error(st) == 0 and np.array_equal(offs, fast_offs) and fr[: len(fast)].tobytes() == fast.tobytes()


# ---- 3. the reference's fixtures ------------------------------------------------------------------------------------------------
def test_reference_fixtures(gpu, generic_digests, generic_kats):  # noqa: F811
    for label, n, kind, wide in gc.all_cases():
        x = gc.case_input(n, kind, wide)
        fr, offs, st = _Device(gpu, 1, x.shape[0], n, 1 << 22).encode(x[None])
        assert codec.encode_status_error(st) == 0, label
        blob = fr[: int(offs[1])].tobytes()
        assert hashlib.sha256(blob).hexdigest() == generic_digests[label]["frame_sha256"], label
        assert int(offs[1]) == generic_digests[label]["frame_bytes"], label
        if f"{label}/bytes" in generic_kats:
            assert blob == generic_kats[f"{label}/bytes"].tobytes(), label


# ---- 4. what the host call refuses ----------------------------------------------------------------------------------------------
def test_error_codes_equal_the_host_calls(gpu):  # noqa: F811
    rng = np.random.default_rng(4)
    # a block not longer than its own order (at n = 2 some are, some are not: the code is the host call's either way)
    for _ in range(8):
        _same(gpu, rng.integers(-30000, 30000, (1, 1, 2)).astype(np.int32), label="n = 2")
    noise = np.random.default_rng(2).integers(-20000, 20000, (1, 1, 40)).astype(np.int32)
    assert _same(gpu, noise, label="order above 40") == -6
    # a residue of |r| >= 2^30: a dc of 2^30 (sample 0 is its own residue)
    dc = dict(wc.wide_signals(2048, 1))[f"dc {wc.P30}"]
    assert _same(gpu, dc[None, None], label="dc 2^30") == -6
    fr, offs, st = _Device(gpu, 1, 1, 2048, 1 << 20).encode(dc[None, None])
    assert st[0] & capi.FLAG_RICE_RANGE
    # a Rice stream beyond the u16 word count: the long stream's values, scaled to 29 bits, as a 65535-sample block
    v, _, _ = gc.long_rice_stream()
    big = (v[:65535].astype(np.int64) << 16).astype(np.int32)
    assert _same(gpu, big[None, None], label="words cap") == -6
    fr, offs, st = _Device(gpu, 1, 1, 65535, 1 << 20).encode(big[None, None])
    assert st[0] & capi.FLAG_WORDS_CAP
    # next to good frames, in one call
    good = _frames(rng, 1, 1, 2048, ("tone",), (16,))
    for bad in (dc[None, None], noise[:, :, :40]):
        n = bad.shape[2]
        x = np.concatenate([_frames(rng, 1, 1, n, ("tone",), (16,)), bad, _frames(rng, 1, 1, n, ("sparse",), (16,))])
        assert _same(gpu, x, label=("between", n)) == -6
    assert _same(gpu, good, label="good") == 0


# ---- 5. capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity(gpu):  # noqa: F811
    rng = np.random.default_rng(5)
    for ch, n in ((2, 1000), (3, 300), (1, 4097)):
        x = _frames(rng, 6, ch, n, ("tone", "noise", "sparse"), (16, 20))
        rc, blob, offs = _host(x)
        assert rc == 0
        total = int(offs[-1])
        mid = int(offs[3]) + (int(offs[4]) - int(offs[3])) // 2
        for cap in (total - 1, 0, mid, int(offs[2])):
            fr, d_offs, st = _Device(gpu, 6, ch, n, cap).encode(x)
            assert np.array_equal(d_offs, offs), cap  # (written in full)
            fits = int((offs[1:] <= cap).sum())
            assert int(st[1]) == 6 - fits and codec.encode_status_error(st) == -4, (cap, st)
            assert fr[: int(offs[fits])].tobytes() == blob[: int(offs[fits])], cap
            assert (fr[int(offs[fits]):] == POISON).all(), cap  # (the frames that do not fit: not a byte, the guard neither)
        fr, d_offs, st = _Device(gpu, 6, ch, n, total).encode(x)
        assert codec.encode_status_error(st) == 0 and fr[:total].tobytes() == blob


def test_encoder32_resizes_from_its_offsets(gpu):  # noqa: F811
    rng = np.random.default_rng(6)
    x = _frames(rng, 5, 2, 3000, ("noise",), (24,))
    rc, blob, offs = _host(x)
    assert rc == 0
    enc = codec.Encoder32(5, 2, 3000, capacity=1000)
    enc.encode(gpu.from_numpy(x).cuda())
    with pytest.raises(capi.SelaHipError) as err:
        enc.check()
    assert err.value.code == -4 and enc.needed_bytes() == len(blob)
    enc = codec.Encoder32(5, 2, 3000, capacity=enc.needed_bytes())
    enc.encode(gpu.from_numpy(x).cuda())
    frames, o = enc.to_host()
    assert frames.tobytes() == blob and np.array_equal(o, offs)
    y = _frames(rng, 5, 2, 3000, ("noise",), (20,))  # (the default capacity: an estimate that holds 20-bit noise)
    rc, blob, offs = _host(y)
    enc = codec.Encoder32(5, 2, 3000)
    enc.encode(gpu.from_numpy(y).cuda())
    assert rc == 0 and enc.to_host()[0].tobytes() == blob


# ---- 6. graphs, streams, an open job, the debug hook ----------------------------------------------------------------------------
def test_graph_replay_on_new_samples(gpu):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(7)
    a = _frames(rng, 8, 2, 1500, ("tone", "sparse"), (16, 24))
    b = _frames(rng, 8, 2, 1500, ("noise", "dc", "tone"), (17, 20))
    enc = codec.Encoder32(8, 2, 1500)
    d_x = torch.from_numpy(a).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.encode(d_x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enc.encode(d_x)
    d_x.copy_(torch.from_numpy(b))
    enc.frames.fill_(POISON)
    enc.status.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    rc, blob, offs = _host(b)
    assert rc == 0
    frames, o = enc.to_host()
    assert frames.tobytes() == blob and np.array_equal(o, offs)


def test_two_streams_at_once(gpu):  # noqa: F811
    torch = gpu
    rng = np.random.default_rng(8)
    xs = [_frames(rng, 40, 2, 2049, ("tone", "noise"), (16, 24)), _frames(rng, 30, 3, 777, ("sparse", "tone"), (17,))]
    encs = [codec.Encoder32(40, 2, 2049), codec.Encoder32(30, 3, 777)]
    d_xs = [torch.from_numpy(x).cuda() for x in xs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for e, s, d in zip(encs, streams, d_xs):
        with torch.cuda.stream(s):
            e.encode(d)
    torch.cuda.synchronize()
    for e, x in zip(encs, xs):
        rc, blob, offs = _host(x)
        frames, o = e.to_host()
        assert rc == 0 and frames.tobytes() == blob and np.array_equal(o, offs)


def test_an_open_decode_job_is_left_alone(gpu):  # noqa: F811
    lib = capi.lib()
    pcm = synth_frames(12, 2, 5)
    want_frames, want_offs = codec.encode_host(pcm)
    back = np.zeros(pcm.size, np.int16)
    job = C.c_void_p()
    ff = C.c_uint32(0)
    capi.check(lib.sela_hip_decode_begin(C.byref(job), 2, 12, back.ctypes.data))
    o = np.ascontiguousarray(want_offs[:6])
    capi.check(lib.sela_hip_decode_feed(job, want_frames.ctypes.data, o.ctypes.data, 5, C.byref(ff)))
    x = _frames(np.random.default_rng(9), 4, 2, 3000, ("tone", "noise"), (20,))
    rc, blob, offs = _host(x)
    fr, d_offs, st = _Device(gpu, 4, 2, 3000, len(blob)).encode(x)
    assert codec.encode_status_error(st) == 0 and fr[: len(blob)].tobytes() == blob
    o = np.ascontiguousarray(want_offs[5:] - want_offs[5])
    capi.check(lib.sela_hip_decode_feed(job, want_frames[int(want_offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12 and np.array_equal(back, pcm.reshape(-1))


def test_wrap_taps_hook(gpu):  # noqa: F811
    rng = np.random.default_rng(10)
    _wrap_taps(True)
    try:
        for ch, n, bits in ((2, 2048, (16,)), (1, 5000, (21, 24)), (3, 129, (16, 31))):
            x = _frames(rng, 3, ch, n, KINDS, bits)
            _same(gpu, x, label=("wrap", ch, n))
    finally:
        _wrap_taps(False)


# ---- 7. arguments ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_the_empty_call(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    x = torch.from_numpy(_frames(np.random.default_rng(11), 2, 2, 500, ("tone",), (16,))).cuda()
    x16 = torch.zeros((2, 500, 2), dtype=torch.int16, device="cuda")
    fr = torch.full((1 << 16,), POISON, dtype=torch.uint8, device="cuda")
    offs = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.sela_hip_encode_i32_workspace_bytes(2, 2, 500))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def enc(d=x.data_ptr(), nf=2, ch=2, n=500, f=fr.data_ptr(), o=offs.data_ptr(), s=st.data_ptr(), w=ws.data_ptr(), wb=ws_bytes, call=lib.sela_hip_encode_i32_device):
        return call(d, nf, ch, n, f, 1 << 16, o, s, w, wb, stream)

    assert enc() == 0
    torch.cuda.synchronize()
    assert codec.encode_status_error(st.cpu().numpy()) == 0
    for kw, code in [(dict(d=None), -2), (dict(f=None), -2), (dict(o=None), -2), (dict(s=None), -2), (dict(w=None), -2),
                     (dict(ch=0), -2), (dict(ch=256), -2), (dict(n=0), -2), (dict(n=65536), -2), (dict(nf=1 << 30, ch=2), -2),
                     (dict(nf=(1 << 31) // 255 + 1, ch=255), -2), (dict(f=fr.data_ptr() + 2), -2), (dict(d=x.data_ptr() + 2), -2),
                     (dict(d=x16.data_ptr() + 1, call=lib.sela_hip_encode_n_device), -2), (dict(wb=ws_bytes - 1), -4),
                     (dict(nf=3), -4)]:
        offs.fill_(-1)
        torch.cuda.synchronize()
        assert enc(**kw) == code, kw
        torch.cuda.synchronize()
        assert (offs.cpu().numpy() == -1).all(), kw  # (nothing enqueued)
    assert enc(d=x16.data_ptr() + 2, call=lib.sela_hip_encode_n_device) == 0  # (2-byte alignment is enough for int16)
    # the empty call: offsets[0] = 0 and zero status words
    st.fill_(-1)
    offs.fill_(-1)
    assert enc(nf=0, d=None, f=None) == 0
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and int(offs[0].item()) == 0 and int(offs[1].item()) == -1
    assert lib.sela_hip_encode_status_error(None) == -2


# ---- 8. random shapes ------------------------------------------------------------------------------------------------------------
def test_random_shapes(gpu):  # noqa: F811
    """Random calls -- 1 .. 6000 samples, 1 .. 6 channels, 1 .. 5 frames, widths 1 .. 31 bits, both entries -- against the host
    calls.  (A soak: SELA_ENCODE_DEVICE_TRIALS=2000 SELA_ENCODE_DEVICE_SEED=...)"""
    trials = int(os.environ.get("SELA_ENCODE_DEVICE_TRIALS", "120"))
    rng = np.random.default_rng(int(os.environ.get("SELA_ENCODE_DEVICE_SEED", "12")))
    landmarks = [1, 2, 3, 63, 64, 65, 100, 101, 102, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049]
    codes = {}
    for trial in range(trials):
        n = int(rng.choice(landmarks)) if trial % 3 == 0 else int(rng.integers(1, 6001))
        ch, nf = int(rng.integers(1, 7)), int(rng.integers(1, 6))
        bits = tuple(int(b) for b in rng.integers(1, 32, 2))
        x = _frames(rng, nf, ch, n, tuple(rng.permutation(KINDS)), bits)
        if ch == 2 and rng.random() < 0.4:
            x[:, 1] = x[:, 0] - rng.integers(-2, 3, (nf, n)).astype(np.int32)
        in16 = max(bits) <= 16 and rng.random() < 0.5
        if in16:
            x = np.ascontiguousarray(x.transpose(0, 2, 1).astype(np.int16))
        rc = _same(gpu, x, in16=in16, label=(trial, n, ch, nf, bits, in16))
        codes[rc] = codes.get(rc, 0) + 1
    assert codes.get(0, 0) >= trials // 2, codes
