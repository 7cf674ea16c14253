"""The paired encode calls on the GPU: sela_hip_encode_paired_i32_device, sela_hip_encode_paired_n_device,
sela_hip_encode_paired_i32 and sela_hip_encode_paired are the model of tests/paired_model.py byte for byte -- frames and offsets,
plain and lossless -- which tests/test_paired_model_cpu.py holds against the oracle and the reference's decoder.  Then the plan's
edges (255 channels, more than one tile of frames, no frame), the capacity, a captured call, and the stream through every decoder
of this library.  Every buffer a device call writes starts poisoned."""
import numpy as np
import pytest

import lossless_model
import paired_model as model
from gpu_common import _signal, gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from sela_amd.synth import synth_pcm

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes behind the frames (and entries behind the offsets) that no call may write
POISON = 0xA5
CASES = ["A6", "N300x6", "A5", "A3", "W4", "S6"]
MODES = [pytest.param(False, id="plain"), pytest.param(True, id="lossless")]


@pytest.fixture(scope="module")
def expected():
    """(case, lossless) -> (bytes uint8, offsets uint64) of the model, computed once."""
    o = oracle()
    return {(name, lossless): model.stream(o, frames, lossless) for name, frames in model.cases().items() for lossless in (False, True)}


class _Device:
    """One paired device call's buffers, poisoned: frames (cap + GUARD bytes of POISON), offsets (-1), status (-1), workspace (0xFF)."""

    def __init__(self, torch, nf, ch, n, cap, lossless=False):
        self.torch, self.nf, self.ch, self.n, self.cap = torch, nf, ch, n, cap
        self.options = capi.ENCODE_LOSSLESS if lossless else 0
        self.frames = torch.full((cap + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.offsets = torch.full((nf + 1 + GUARD // 8,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.full((int(capi.lib().sela_hip_encode_paired_workspace_bytes(nf, ch, n)),), 0xFF, dtype=torch.uint8, device="cuda")

    def launch(self, d_x):
        in16 = d_x is not None and d_x.dtype == self.torch.int16
        call = capi.lib().sela_hip_encode_paired_n_device if in16 else capi.lib().sela_hip_encode_paired_i32_device
        return call(d_x.data_ptr() if d_x is not None else 0, self.nf, self.ch, self.n, self.frames.data_ptr(), self.cap, self.offsets.data_ptr(),
                    self.status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), self.torch.cuda.current_stream().cuda_stream, self.options)

    def encode(self, x):
        d_x = self.torch.from_numpy(np.ascontiguousarray(x)).cuda()
        capi.check(self.launch(d_x))
        self.torch.cuda.synchronize()
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


def _device_equals(torch, x, want, lossless, label):
    """x: int32 [nf, ch, n] or int16 [nf, n, ch]; want: (bytes, offsets)."""
    blob, offs = want
    nf = x.shape[0]
    ch, n = (x.shape[2], x.shape[1]) if x.dtype == np.int16 else (x.shape[1], x.shape[2])
    fr, d_offs, st = _Device(torch, nf, ch, n, len(blob), lossless).encode(x)
    assert int(st[0]) & ~capi.FLAG_Q_RANGE == 0 and int(st[1]) == 0 and codec.encode_status_error(st) == 0, (label, st)
    assert np.array_equal(d_offs, offs), label
    assert np.array_equal(fr[: len(blob)], blob), (label, int(np.flatnonzero(fr[: len(blob)] != blob)[0]))


# ---- 1. byte identity through all four entry points ---------------------------------------------------------------------------
@pytest.mark.parametrize("lossless", MODES)
@pytest.mark.parametrize("case", CASES)
def test_every_entry_point_is_the_model(gpu, expected, case, lossless):  # noqa: F811
    frames = model.cases()[case]
    blob, offs = expected[case, lossless]
    inputs = [model.planar(frames)] + ([] if case in model.WIDE else [model.interleaved(frames)])
    for x in inputs:
        _device_equals(gpu, x, (blob, offs), lossless, (case, str(x.dtype), "device"))
        host = codec.encode_i32 if x.dtype == np.int32 else codec.encode_host
        got, got_offs = host(x, lossless=lossless, paired=True)
        assert np.array_equal(got_offs, offs) and np.array_equal(got, blob), (case, str(x.dtype), "host")


@pytest.mark.parametrize("case", ["A6", "N300x6"])
def test_int16_input_on_an_odd_word(gpu, expected, case):  # noqa: F811
    """An even channel count lets the kernel load a pair's two samples as one 32-bit word -- where the input is 4-byte aligned.
    2-byte alignment is all the call asks: the same samples one int16 further on give the same stream (paired, and the plain
    stereo frame, whose difference takes the same load)."""
    torch = gpu
    for x, want in ((model.interleaved(model.cases()[case]), expected[case, True]),
                    (model.interleaved(lossless_model.cases()["A"]), lossless_model.stream(oracle(), lossless_model.cases()["A"], True))):
        nf, n, ch = x.shape
        room = torch.zeros(x.size + 8, dtype=torch.int16, device="cuda")
        base = 1 if room.data_ptr() % 4 == 0 else 2  # (the first element whose address is 2 mod 4)
        d_x = room[base: base + x.size].view(nf, n, ch)
        d_x.copy_(torch.from_numpy(x))
        assert d_x.data_ptr() % 4 == 2 and d_x.is_contiguous()
        dev = _Device(torch, nf, ch, n, len(want[0]), True)
        capi.check(dev.launch(d_x))
        torch.cuda.synchronize()
        fr, offs, st = dev.results()
        assert codec.encode_status_error(st) == 0 and np.array_equal(offs, want[1]) and np.array_equal(fr[: len(want[0])], want[0]), (case, ch)


@pytest.mark.parametrize("lossless", MODES)
@pytest.mark.parametrize("case", ["M", "A", "N300"])
def test_one_and_two_channels_are_the_plain_device_call(gpu, case, lossless):  # noqa: F811
    torch = gpu
    frames = lossless_model.cases()[case]
    for x in (model.planar(frames), model.interleaved(frames)):
        nf = x.shape[0]
        ch, n = (x.shape[2], x.shape[1]) if x.dtype == np.int16 else (x.shape[1], x.shape[2])
        enc = codec.Encoder32(nf, ch, n, lossless=lossless)
        enc.encode(torch.from_numpy(x).cuda())
        plain, plain_offs = enc.to_host()
        _device_equals(torch, x, (plain, plain_offs), lossless, (case, str(x.dtype)))


# ---- 2. the plan's edges ---------------------------------------------------------------------------------------------------------
def test_255_channels(gpu):  # noqa: F811
    """127 pairs and a last channel alone, at the sample count of test_gpu_encode_i32_device's 255-channel frames that codes without
    a short block (300): every second pair is a near-copy, so that both outcomes of the decision occur."""
    rng = np.random.default_rng(255)
    n, kinds = 300, ("tone", "noise", "sparse", "dc", "silence")
    x = np.stack([np.stack([_signal(rng, kinds[(f + c // 2) % len(kinds)], n, 14) for c in range(255)]) for f in range(2)])
    x[:, 1:255:4] = x[:, 0:254:4] + rng.integers(-3, 4, x[:, 0:254:4].shape).astype(np.int32)
    assert np.abs(x).max() < 32768
    o = oracle()
    want = {}
    for lossless in (False, True):
        coded = [model.encode_frame(o, f, lossless) for f in x]
        odd = [t for _, types in coded for t in types[1::2]]
        assert 0 in odd and 1 in odd  # (the input bites)
        blobs = [b for b, _ in coded]
        want[lossless] = (np.frombuffer(b"".join(blobs), np.uint8), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64))
        _device_equals(gpu, x, want[lossless], lossless, ("255", lossless))
    _device_equals(gpu, np.ascontiguousarray(x.transpose(0, 2, 1).astype(np.int16)), want[True], True, "255 int16, lossless")


TILE_FRAMES, TILE_N = 4100, 101  # more than kPlanTile = 4096 frames; 101 samples: the shortest block no order (<= 100) makes short


def test_more_frames_than_a_tile_of_the_plan(gpu):  # noqa: F811
    """3 channels x 101 samples x 4100 frames of the synthetic track: the oracle codes every block of it (no SHORT_BLOCK, checked
    when the test was written: at 64 samples 16,276 of its 16,400 candidates are short, at 101 none can be)."""
    o = oracle()
    pcm = synth_pcm(TILE_FRAMES * TILE_N, 3, track=5).reshape(TILE_FRAMES, TILE_N, 3)
    planar = np.ascontiguousarray(pcm.transpose(0, 2, 1).astype(np.int32))
    blobs, stored = [], 0
    for f in range(TILE_FRAMES):  # the plain model straight from the oracle's frame encoder (tests/test_paired_model_cpu.py: the same bytes)
        pair = model.subframes(o.frame_encode_i32(planar[f, :2]))
        last = model.subframes(o.frame_encode_i32(planar[f, 2:]))
        stored += pair[1][1]
        blobs.append(model.SYNC + pair[0] + pair[1] + model._moved(last[0], 2))
    assert 0 < stored < TILE_FRAMES  # (both outcomes)
    want = (np.frombuffer(b"".join(blobs), np.uint8), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64))
    _device_equals(gpu, np.ascontiguousarray(pcm), want, False, "tile int16")
    _device_equals(gpu, planar, want, False, "tile int32")


@pytest.mark.parametrize("lossless", MODES)
def test_no_frame(gpu, lossless):  # noqa: F811
    torch = gpu
    for in16 in (False, True):
        dev = _Device(torch, 0, 6, 2048, 64, lossless)
        call = capi.lib().sela_hip_encode_paired_n_device if in16 else capi.lib().sela_hip_encode_paired_i32_device
        capi.check(call(0, 0, 6, 2048, 0, 0, dev.offsets.data_ptr(), dev.status.data_ptr(), dev.ws.data_ptr(), dev.ws.numel(), torch.cuda.current_stream().cuda_stream, dev.options))
        torch.cuda.synchronize()
        fr, offs, st = dev.results()
        assert list(offs) == [0] and list(st) == [0, 0, 0, 0] and (fr == POISON).all()
    blob, offs = codec.encode_i32(np.zeros((0, 6, 300), np.int32), lossless=lossless, paired=True)
    assert len(blob) == 0 and list(offs) == [0]


# ---- 3. capacity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lossless", MODES)
def test_capacity(gpu, expected, lossless):  # noqa: F811
    frames = model.cases()["A6"]
    blob, offs = expected["A6", lossless]
    x = model.interleaved(frames)
    nf, total = len(frames), int(offs[-1])
    k = 2
    inside = int(offs[k]) + (int(offs[k + 1]) - int(offs[k])) // 2
    for cap in (inside, total - 1, 0, int(offs[3])):
        fr, d_offs, st = _Device(gpu, nf, 6, 2048, cap, lossless).encode(x)
        assert np.array_equal(d_offs, offs), cap  # (written in full)
        fits = int((offs[1:] <= cap).sum())
        assert int(st[1]) == nf - fits and codec.encode_status_error(st) == -4, (cap, st)
        assert np.array_equal(fr[: int(offs[fits])], blob[: int(offs[fits])]), cap
        assert (fr[int(offs[fits]):] == POISON).all(), cap  # (the frames that do not fit: not a byte, the guard neither)
    enc = codec.Encoder32(nf, 6, 2048, capacity=inside, lossless=lossless, paired=True)
    enc.encode(gpu.from_numpy(x).cuda())
    with pytest.raises(capi.SelaHipError) as err:
        enc.check()
    assert err.value.code == -4 and enc.needed_bytes() == total


# ---- 4. a captured call -----------------------------------------------------------------------------------------------------------
def test_graph_replay_on_new_samples(gpu, expected):  # noqa: F811
    torch = gpu
    frames = model.cases()["S6"]
    a, b = model.interleaved(frames[:4]), model.interleaved(frames[4:8])
    enc = codec.Encoder32(4, 6, 2048, lossless=True, paired=True)
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
    blob, offs = expected["S6", True]
    lo, hi = int(offs[4]), int(offs[8])
    got, got_offs = enc.to_host()
    assert np.array_equal(got, blob[lo:hi]) and np.array_equal(got_offs, offs[4:9] - offs[4])


# ---- 5. the stream through this library's decoders ---------------------------------------------------------------------------------
def test_round_trip_on_the_device(gpu, expected):  # noqa: F811
    torch = gpu
    frames = model.cases()["S6"]
    nf = len(frames)
    pcm = model.interleaved(frames)  # [nf, 2048, 6]
    d_pcm = torch.from_numpy(pcm).cuda()
    enc = codec.Encoder32(nf, 6, 2048, lossless=True, paired=True)
    d_frames, d_offs, _ = enc.encode(d_pcm)
    enc.check()
    assert np.array_equal(enc.to_host()[0], expected["S6", True][0])
    d_offs = d_offs.contiguous()

    dec = codec.Decoder(nf, 6)  # sela_hip_decode_device
    out = dec.decode(d_frames, d_offs, nf)
    dec.check()
    assert torch.equal(out, d_pcm)

    dec_n = codec.DecoderN(nf, 6, 2048)  # sela_hip_decode_n_device
    out, so = dec_n.decode(d_frames, d_offs, nf)
    dec_n.check()
    assert int(so[nf].item()) == nf * 2048 and torch.equal(out[: nf * 2048].reshape(nf, 2048, 6), d_pcm)

    dec32 = codec.Decoder32(nf, 6, 2048)  # sela_hip_decode_i32_device
    samples, counts, _ = dec32.decode(d_frames, d_offs, nf)
    dec32.check()
    assert bool((counts == 2048).all()) and torch.equal(samples, d_pcm.permute(0, 2, 1).to(torch.int32))

    ver = codec.Verifier(nf, 6, 2048)  # sela_hip_verify_device
    diff, _ = ver.verify(d_frames, d_offs, nf, d_pcm)
    ver.check()
    assert ver.lossy_frames() == 0 and int(diff.sum().item()) == 0

    win = codec.WindowDecoder(1, 1000, 6)  # sela_hip_decode_windows_device: one crop across the boundary of frames 2 and 3
    start = 3 * 2048 - 400
    crop = win.decode(d_frames, d_offs, nf, torch.from_numpy(codec.WindowDecoder.pack([start], 0, nf)).cuda())
    win.check()
    assert int(win.flags[0].item()) == 0 and torch.equal(crop[0], d_pcm.reshape(nf * 2048, 6)[start: start + 1000])


def test_ten_channels_through_the_wide_decoder(gpu):  # noqa: F811
    torch = gpu
    frames = model.synth_frames()
    ten = [np.ascontiguousarray(np.concatenate([frames[f], frames[f + 1][:4]])) for f in (8, 10, 12, 16)]
    o = oracle()
    blob, offs = model.stream(o, ten, True)
    assert any(t for x in ten for t in model.encode_frame(o, x, True)[1])  # (a stored difference among them)
    pcm = model.interleaved(ten)
    d_pcm = torch.from_numpy(pcm).cuda()
    enc = codec.Encoder32(len(ten), 10, 2048, lossless=True, paired=True)
    d_frames, d_offs, _ = enc.encode(d_pcm)
    got, got_offs = enc.to_host()
    assert np.array_equal(got, blob) and np.array_equal(got_offs, offs)
    dec = codec.Decoder(len(ten), 10)
    out = dec.decode(d_frames, d_offs.contiguous(), len(ten))
    dec.check()
    assert torch.equal(out, d_pcm)
