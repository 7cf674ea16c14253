"""sela_hip_decode_whole_device, its payload form and sela_hip_decode_whole: a full decode of a whole-track stream,
frames 0 .. n - 2 on the 2048-sample decoder and the long last frame (1 .. 4095 samples) beside them.

Streams come from codec.encode_whole_host(..., lossless=True) of synthetic PCM, so the expected output is the PCM itself; every case
is also compared byte for byte with codec.DecoderN (sela_hip_decode_n_device) on the same stream.  Every device call is the raw
C ABI on fresh buffers full of sentinels: around the PCM, behind *d_n_samples and behind the status words."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from gpu_common import HOST, _build, _write_wav, gpu  # noqa: F401  (fixture and helpers)
from oracle_lib import oracle
from sela_amd import capi, codec
from sela_amd.synth import synth_frames, synth_pcm
from test_gpu_encode_whole import _second_subframe_type, _track

pytestmark = pytest.mark.gpu

B = 2048
FRONT, GUARD = 64, 63  # elements in front of the PCM (the stereo decoder stores 16 bytes at a time: the alignment stays) and behind
SENT16, SENT32, SENT64 = 0x5E1A, 0x5E1A5E1A, 0x5E1A5E1A5E1A5E1A
ECAPACITY, EFORMAT = -4, -5
BAD, DRY, STRIDE = capi.FLAG_BAD_FRAME, capi.FLAG_RICE_OVERRUN, 256
FRAMES_ARGS = ("d_frames", "d_frame_offsets", "n_frames", "channels", "d_pcm_out", "pcm_capacity", "d_n_samples", "d_status", "d_workspace", "workspace_bytes", "stream")
PAYLOAD_ARGS = ("d_frames", "payload_bytes", "n_frames", "channels", "d_pcm_out", "pcm_capacity", "d_n_samples", "d_frame_offsets", "d_n_frames", "d_status", "d_workspace",
                "workspace_bytes", "stream")
# two 2048-sample frames and a tail of 1, 777, 2047; one long frame alone (fast count 0); one short frame; no tail; nothing
SHAPES = [2 * B + 1, 2 * B + 777, 2 * B + 2047, 2049, 1500, 3 * B, 0]


@functools.lru_cache(maxsize=None)
def pcm_of(n, ch, k=0):
    """n samples per channel; up to three channels the corpus (for odd k the second channel follows the first, so that the
    difference wins), more from the synthetic track"""
    if ch <= 3:
        return _track(n, ch, k)
    if n == 0:
        return np.zeros((0, ch), np.int16)
    out = np.ascontiguousarray(synth_pcm(n, ch, 7 + k)).astype(np.int16)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stream_of(n, ch, k=0, lossless=True):
    frames, offs = codec.encode_whole_host(pcm_of(n, ch, k), lossless=lossless)
    frames.setflags(write=False), offs.setflags(write=False)
    return frames, offs


def blobs_of(frames, offs):
    return [frames[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(len(offs) - 1)]


def join(blobs):
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)


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


def to_device(torch, frames, offs):
    padded = np.zeros(max((len(frames) + 3) // 4 * 4, 4), np.uint8)
    padded[: len(frames)] = frames
    return torch.from_numpy(padded).cuda(), torch.from_numpy(np.ascontiguousarray(offs).view(np.int64).copy()).cuda()


def device_call(torch, frames, offs, ch, capacity, payload_max=None):
    """One raw call -> (pcm int16 [capacity, ch] as the call left it, *d_n_samples, status uint32 [4]); guards and inputs checked here.
    payload_max: the payload form with that max_frames; its offsets and count are compared with the stream's."""
    lib = capi.lib()
    n = len(offs) - 1
    d_frames, d_offs = to_device(torch, frames, offs)
    buf = torch.full(((FRONT + capacity + GUARD) * ch,), SENT16, dtype=torch.int16, device="cuda")
    d_n = torch.full((1 + GUARD,), SENT64, dtype=torch.int64, device="cuda")
    d_status = torch.full((4 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    max_frames = n if payload_max is None else payload_max
    need = int(lib.sela_hip_decode_whole_workspace_bytes(max_frames, ch))
    if payload_max is not None:
        need += int(lib.sela_hip_index_workspace_bytes(len(frames), max_frames))
        d_found_offs = torch.full((max_frames + 1 + GUARD,), SENT64, dtype=torch.int64, device="cuda")
        d_count = torch.full((1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    d_ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    frames_before, offs_before = d_frames.clone(), d_offs.clone()
    args = dict(d_frames=d_frames.data_ptr(), d_frame_offsets=d_offs.data_ptr(), n_frames=max_frames, channels=ch, d_pcm_out=buf.data_ptr() + FRONT * ch * 2, pcm_capacity=capacity,
                d_n_samples=d_n.data_ptr(), d_status=d_status.data_ptr(), d_workspace=d_ws.data_ptr(), workspace_bytes=need, stream=torch.cuda.current_stream().cuda_stream)
    if payload_max is None:
        rc = lib.sela_hip_decode_whole_device(*[args[k] for k in FRAMES_ARGS])
    else:
        args.update(payload_bytes=len(frames), d_frame_offsets=d_found_offs.data_ptr(), d_n_frames=d_count.data_ptr())
        rc = lib.sela_hip_decode_whole_payload_device(*[args[k] for k in PAYLOAD_ARGS])
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.sela_hip_last_error())
    assert torch.equal(d_frames, frames_before) and torch.equal(d_offs, offs_before), "an input was written"
    host = buf.cpu().numpy().reshape(-1, ch)
    assert (host[:FRONT] == np.int16(SENT16)).all() and (host[FRONT + capacity:] == np.int16(SENT16)).all(), "written around d_pcm_out"
    n_samples, status = d_n.cpu().numpy(), d_status.cpu().numpy().view(np.uint32)
    assert (n_samples[1:] == SENT64).all() and (status[4:] == SENT32).all(), "written behind d_n_samples or d_status"
    assert (d_ws[need:].cpu().numpy() == 0xA5).all(), "written behind the workspace"
    if payload_max is not None:
        found, count = d_found_offs.cpu().numpy(), d_count.cpu().numpy()
        assert int(count[0]) == n and np.array_equal(found[: n + 1].view(np.uint64), offs) and (found[max_frames + 1:] == SENT64).all() and (count[1:] == SENT32).all()
    return host[FRONT: FRONT + capacity].copy(), int(n_samples[0]), status[:4].copy()


def decoder_n(torch, frames, offs, ch):
    """codec.DecoderN on the stream -> (pcm int16 [S, ch], status uint32 [4])"""
    n = len(offs) - 1
    d_frames, d_offs = to_device(torch, frames, offs)
    dn = codec.DecoderN(max(n, 1), ch, 4095)
    pcm, so = dn.decode(d_frames, d_offs, n)
    torch.cuda.synchronize()
    return pcm.cpu().numpy()[: int(so.cpu().numpy()[n])].copy(), dn.status.cpu().numpy().view(np.uint32)


def host_code(frames, offs, ch):
    """sela_hip_decode's return code on the stream (room for whatever its headers say)"""
    n = len(offs) - 1
    pcm = np.zeros(((n + 1) * 65535, ch), np.int16)
    fr = np.ascontiguousarray(frames)
    return int(capi.lib().sela_hip_decode(fr.ctypes.data, np.ascontiguousarray(offs).ctypes.data, n, ch, pcm.ctypes.data))


def sentinel(a):
    return (a == np.int16(SENT16)).all()


# ---- well-formed streams --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch,k", [(1, 0), (2, 0), (2, 1), (3, 0), (8, 0)], ids=["mono", "stereo", "stereo_diff", "three", "eight"])
@pytest.mark.parametrize("n", SHAPES)
def test_a_lossless_whole_track_stream_comes_back(gpu, n, ch, k):  # noqa: F811
    frames, offs = stream_of(n, ch, k)
    pcm = pcm_of(n, ch, k)
    nf = len(offs) - 1
    tail = n % B != 0
    capacity = n + 5
    out, n_samples, status = device_call(gpu, frames, offs, ch, capacity)
    print("n", n, "channels", ch, "frames", nf, "n_samples", n_samples, "status", status)
    assert n_samples == n
    assert status.tolist() == [0, 0, 0, 3 if tail else (1 if n else 0)]
    assert np.array_equal(out[:n], pcm) and sentinel(out[n:])
    alone, st = decoder_n(gpu, frames, offs, ch)
    assert np.array_equal(alone, out[:n]) and int(st[0]) == 0 and (n == 0 or int(st[3]) == (2 if tail else 1))
    assert codec.decode_whole_status_error(status) == 0 == host_code(frames, offs, ch)
    if n and not tail:  # no tail: the 2048-sample decoder's bytes
        d_frames, d_offs = to_device(gpu, frames, offs)
        dec = codec.Decoder(nf, ch)
        plain = dec.decode(d_frames, d_offs, nf)
        gpu.cuda.synchronize()
        assert np.array_equal(plain.cpu().numpy().reshape(-1, ch), out[:n])
    if ch == 2 and k == 1 and n == 2 * B + 777:  # a difference-coded tail: the last frame's second subframe is of type 1
        assert _second_subframe_type(frames[int(offs[nf - 1]):].tobytes()) == 1
    # exactly its room, the payload form with more frames allowed than there are, and the Python class
    exact, n_exact, st_exact = device_call(gpu, frames, offs, ch, n)
    assert n_exact == n and np.array_equal(exact, pcm) and st_exact.tobytes() == status.tobytes()
    if n:
        pout, pn, pstatus = device_call(gpu, frames, offs, ch, capacity, payload_max=nf + 3)
        assert pn == n and pstatus.tobytes() == status.tobytes() and np.array_equal(pout, out)
    wd = codec.WholeDecoder(nf, ch)
    d_frames, d_offs = to_device(gpu, frames, offs)
    got, got_n = wd.decode(d_frames, d_offs, nf)
    gpu.cuda.synchronize()
    wd.check()
    assert int(got_n.item()) == n and np.array_equal(got.cpu().numpy()[:n], pcm) and wd.route() == int(status[3])
    if n:
        assert len(frames) % 4 == 0 and d_frames.numel() == len(frames)
        got, got_n, _, count = wd.decode_payload(d_frames, nf)
        gpu.cuda.synchronize()
        assert int(count.item()) == nf and int(got_n.item()) == n and np.array_equal(got.cpu().numpy()[:n], pcm)


def test_a_multichannel_paired_tail(gpu):  # noqa: F811
    """four channels: plain 2048-sample frames and a last frame from encode_paired at 2825 samples (two difference subframes)"""
    ch, n_last = 4, 2825
    front = np.ascontiguousarray(synth_pcm(2 * B, ch, 31).reshape(2, B, ch))
    rng = np.random.default_rng(521)
    base = synth_pcm(n_last, ch, 32).astype(np.int32)
    base[:, 1] = base[:, 0] - (rng.integers(-40, 40, n_last))
    base[:, 3] = base[:, 2] - (rng.integers(-40, 40, n_last))
    last = np.clip(base, -32768, 32767).astype(np.int16)
    f_frames, f_offs = codec.encode_host(front, lossless=True)
    l_frames, l_offs = codec.encode_host(last[None], lossless=True, paired=True)
    last_blob = l_frames.tobytes()
    types = []
    p = 4
    for _ in range(ch):
        types.append(last_blob[p + 1])
        cw = struct.unpack_from("<H", last_blob, p + 4)[0]
        rw = struct.unpack_from("<H", last_blob, p + 7 + 4 * cw + 1)[0]
        p += 12 + 4 * (cw + rw)
    assert types.count(1) >= 1, types
    frames, offs = join(blobs_of(f_frames, f_offs) + [last_blob])
    n = 2 * B + n_last
    out, n_samples, status = device_call(gpu, frames, offs, ch, n + 9)
    assert n_samples == n and status.tolist() == [0, 0, 0, 3]
    assert np.array_equal(out[: 2 * B], front.reshape(-1, ch)) and np.array_equal(out[2 * B: n], last) and sentinel(out[n:])
    alone, st = decoder_n(gpu, frames, offs, ch)
    assert np.array_equal(alone, out[:n]) and int(st[0]) == 0


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_a_plain_stream_gives_decoder_n_s_bytes_and_the_oracle_s(gpu, ch):  # noqa: F811
    n = 2 * B + 777
    frames, offs = stream_of(n, ch, 1, lossless=False)
    out, n_samples, status = device_call(gpu, frames, offs, ch, n)
    assert n_samples == n and status.tolist() == [0, 0, 0, 3]
    alone, st = decoder_n(gpu, frames, offs, ch)
    assert np.array_equal(alone, out) and int(st[0]) == 0
    o = oracle()
    blobs = blobs_of(frames, offs)
    for f, blob in enumerate(blobs[:-1]):
        want, used = o.frame_decode(blob, ch)
        assert used == len(blob) and np.array_equal(out[f * B: (f + 1) * B], want)
    assert len(blobs) == 2
    dec, used = o.frame_decode_i32(blobs[-1], ch, stride=B + 777)
    assert used == len(blobs[-1]) and np.array_equal(np.stack(dec, axis=1).astype(np.int16), out[B:])


# ---- trouble --------------------------------------------------------------------------------------------------------------------------
def front_of(torch, frames, offs, ch, n_front):
    """codec.Decoder on frames 0 .. n_front - 1 -> (pcm [n_front * 2048, ch], status uint32 [4])"""
    d_frames, d_offs = to_device(torch, frames, offs)
    dec = codec.Decoder(n_front, ch)
    pcm = dec.decode(d_frames, d_offs, n_front)
    torch.cuda.synchronize()
    return pcm.cpu().numpy().reshape(-1, ch).copy(), dec.status.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ["sync", "says_1000"])
def test_a_malformed_front_frame_costs_what_it_costs_the_decoder_and_the_tail_is_decoded(gpu, kind):  # noqa: F811
    n, ch = 4 * B + 777, 2  # three frames of 2048 samples and a last one of 2825
    frames, offs = stream_of(n, ch, 1)
    blobs = blobs_of(frames, offs)
    assert len(blobs) == 4
    if kind == "sync":
        bad = bytearray(blobs[1])
        bad[0] ^= 0xFF
        blobs[1] = bytes(bad)
    else:
        blobs[1] = patch_n(blobs[1], 1000)
    frames, offs = join(blobs)
    out, n_samples, status = device_call(gpu, frames, offs, ch, n + 3)
    want_front, want_status = front_of(gpu, frames, offs, ch, 3)
    print(kind, "status", status, "the decoder's on the front frames", want_status)
    assert n_samples == n and int(status[3]) == 3
    assert np.array_equal(out[: 3 * B], want_front) and status[:3].tobytes() == want_status[:3].tobytes()
    assert int(status[0]) & BAD and int(status[1]) == 1 and not want_front[B: 2 * B, 0].any()  # (the subframe that is refused: zeros)
    assert np.array_equal(out[3 * B: n], pcm_of(n, ch, 1)[3 * B:]) and sentinel(out[n:])
    assert codec.decode_whole_status_error(status) == EFORMAT == host_code(frames, offs, ch)
    hout, hn, rc = codec.decode_whole_host(frames, offs, ch, check=False)
    assert rc == EFORMAT and hn == n and np.array_equal(hout[3 * B: n], out[3 * B: n])


def test_a_last_frame_whose_rice_stream_runs_dry(gpu):  # noqa: F811
    """both subframes of the last frame say 100 samples more than their residue streams hold (the last word's padding is at most 31
    codewords): RICE_OVERRUN, the frame counted, and nothing of it written"""
    n, ch = 2 * B + 777, 2
    frames, offs = stream_of(n, ch, 0)
    blobs = blobs_of(frames, offs)
    blobs[-1] = patch_n(patch_n(blobs[-1], B + 877, sub=0), B + 877, sub=1)
    frames, offs = join(blobs)
    out, n_samples, status = device_call(gpu, frames, offs, ch, n + 200)
    print("status", status)
    assert n_samples == n + 100 and int(status[0]) == DRY and int(status[1]) == 1 and int(status[2]) == 0 and int(status[3]) == 3
    assert np.array_equal(out[:B], pcm_of(n, ch, 0)[:B]) and sentinel(out[B:])
    assert codec.decode_whole_status_error(status) == EFORMAT == host_code(frames, offs, ch)
    assert codec.decode_whole_host(frames, offs, ch, check=False)[2] == EFORMAT


def test_a_last_frame_that_says_4096_is_a_plain_frame(gpu):  # noqa: F811
    n, ch = 2 * B + 777, 2
    frames, offs = stream_of(n, ch, 0)
    blobs = blobs_of(frames, offs)
    blobs[-1] = patch_n(blobs[-1], 4096)
    frames, offs = join(blobs)
    out, n_samples, status = device_call(gpu, frames, offs, ch, 2 * B + 10)
    want, want_status = front_of(gpu, frames, offs, ch, 2)
    assert n_samples == 2 * B and int(status[3]) == 1 and int(status[0]) == BAD and int(status[1]) == 1
    assert np.array_equal(out[: 2 * B], want) and status[:3].tobytes() == want_status[:3].tobytes() and sentinel(out[2 * B:])
    assert not out[B: 2 * B].any()
    assert codec.decode_whole_status_error(status) == EFORMAT == host_code(frames, offs, ch)
    assert codec.decode_whole_host(frames, offs, ch, check=False)[2] == EFORMAT


@pytest.mark.parametrize("n", [2 * B + 777, 1500, 3 * B])
def test_a_stream_that_does_not_fit_is_not_decoded(gpu, n):  # noqa: F811
    """(sela_hip_decode takes no capacity, so there is no code of its to compare with: the host call's is SELA_HIP_ECAPACITY)"""
    ch = 2
    frames, offs = stream_of(n, ch, 0)
    for payload_max in (None, 7):
        out, n_samples, status = device_call(gpu, frames, offs, ch, n - 1, payload_max=payload_max)
        assert n_samples == n and status.tolist() == [STRIDE, 0, 0, 0] and sentinel(out)
    assert codec.decode_whole_status_error(status) == ECAPACITY
    hout, hn, rc = codec.decode_whole_host(frames, offs, ch, capacity=n - 1, check=False)
    assert rc == ECAPACITY and hn == n and not hout.any()


# ---- capture --------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_reads_the_stream_at_replay(gpu):  # noqa: F811
    """captured on a stream of two frames, the last of 2048 + 777 samples; replayed on another of two whose last has 2048 + 2047"""
    torch, ch = gpu, 2
    first, second = stream_of(2 * B + 777, ch, 1), stream_of(2 * B + 2047, ch, 0)
    size = max(len(first[0]), len(second[0])) + 8
    d_frames = torch.zeros(size, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(3, dtype=torch.int64, device="cuda")

    def load(stream):
        d_frames.zero_()
        d_frames[: len(stream[0])].copy_(torch.from_numpy(stream[0].copy()))
        d_offs.copy_(torch.from_numpy(stream[1].view(np.int64).copy()))

    load(first)
    wd = codec.WholeDecoder(2, ch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wd.decode(d_frames, d_offs, 2)  # one plain call: what the library asks the runtime once per kernel is asked here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, out_n = wd.decode(d_frames, d_offs, 2)
    for stream, n, k in ((first, 2 * B + 777, 1), (second, 2 * B + 2047, 0), (first, 2 * B + 777, 1)):
        load(stream)
        wd.pcm.fill_(SENT16), wd.n_samples.fill_(-1), wd.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_n, eager_status = device_call(gpu, stream[0], stream[1], ch, wd.capacity)
        replayed = out.cpu().numpy()
        assert int(out_n.item()) == n == eager_n and np.array_equal(wd.status.cpu().numpy().view(np.uint32), eager_status)
        assert np.array_equal(replayed, eager) and np.array_equal(replayed[:n], pcm_of(n, ch, k))


def test_an_encode_and_a_decode_fork_in_one_capture(gpu):  # noqa: F811
    """WholeEncoder.encode, then WholeDecoder.decode on the encoder's own buffers: two call families through the library's one
    side stream back to back -- eager on one stream, then both in one capture, replayed once on a second track.  Two frames, the
    last of 2048 + 777 samples: the smallest track with which both calls fork."""
    torch, ch, n = gpu, 2, 2 * B + 777
    tracks = [pcm_of(n, ch, 0), pcm_of(n, ch, 1)]
    for lossless in (True, False):
        enc, dec = codec.WholeEncoder(n, ch, lossless=lossless), codec.WholeDecoder(2, ch)
        d_x = torch.zeros((n, ch), dtype=torch.int16, device="cuda")

        def both():
            frames, offsets, _ = enc.encode(d_x)
            return dec.decode(frames, offsets, 2)

        def poison():
            enc.frames.fill_(0xA5), enc.offsets.fill_(-1), enc.status.fill_(-1)
            dec.pcm.fill_(SENT16), dec.n_samples.fill_(-1), dec.status.fill_(-1)

        def results(out, out_n):
            return out[:n].cpu().numpy().copy(), int(out_n.item()), enc.status.cpu().numpy().copy(), dec.status.cpu().numpy().copy()

        work, eager = torch.cuda.Stream(), []
        for x in tracks:  # form 1: both calls uncaptured on one stream
            d_x.copy_(torch.from_numpy(np.array(x, order="C")))
            poison()
            work.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(work):
                out, out_n = both()
            torch.cuda.current_stream().wait_stream(work)
            torch.cuda.synchronize()
            eager.append(results(out, out_n))
            assert eager[-1][1] == n, lossless
            assert not lossless or np.array_equal(eager[-1][0], x)
        d_x.copy_(torch.from_numpy(np.array(tracks[0], order="C")))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # form 2: both calls in one capture ...
            out, out_n = both()
        d_x.copy_(torch.from_numpy(np.array(tracks[1], order="C")))  # ... replayed once, on the second track
        poison()
        graph.replay()
        torch.cuda.synchronize()
        pcm, pcm_n, enc_status, dec_status = results(out, out_n)
        assert pcm_n == n and np.array_equal(enc_status, eager[1][2]) and np.array_equal(dec_status, eager[1][3]), lossless
        assert np.array_equal(pcm, tracks[1] if lossless else eager[1][0]), lossless


# ---- the host call --------------------------------------------------------------------------------------------------------------------
def host_equals_device(torch, n, ch, k):
    frames, offs = stream_of(n, ch, k)
    hout, hn, rc = codec.decode_whole_host(frames, offs, ch)
    assert rc == 0 and hn == n and np.array_equal(hout[:n], pcm_of(n, ch, k))
    out, dn, status = device_call(torch, frames, offs, ch, max(n, 1))
    assert dn == n and np.array_equal(out[:n], hout[:n]) and int(status[0]) == 0


@pytest.mark.parametrize("ch,k", [(1, 0), (2, 1), (3, 0), (8, 0)], ids=["mono", "stereo_diff", "three", "eight"])
def test_the_host_call_equals_the_device_call(gpu, ch, k):  # noqa: F811
    for n in SHAPES:
        host_equals_device(gpu, n, ch, k)


def test_the_host_call_leaves_an_open_streaming_job_alone(gpu):  # noqa: F811
    lib = capi.lib()
    job_pcm = synth_frames(12, 2, 5)
    job_frames, job_offs = codec.encode_host(job_pcm)
    back = np.zeros(job_pcm.size, np.int16)
    job = C.c_void_p()
    ff = C.c_uint32(0)
    capi.check(lib.sela_hip_decode_begin(C.byref(job), 2, 12, back.ctypes.data))
    o = np.ascontiguousarray(job_offs[:6])
    capi.check(lib.sela_hip_decode_feed(job, job_frames.ctypes.data, o.ctypes.data, 5, C.byref(ff)))
    for n in SHAPES:
        host_equals_device(gpu, n, 2, 1)
    o = np.ascontiguousarray(job_offs[5:] - job_offs[5])
    capi.check(lib.sela_hip_decode_feed(job, job_frames[int(job_offs[5]):].ctypes.data, o.ctypes.data, 7, C.byref(ff)))
    capi.check(lib.sela_hip_decode_end(job, C.byref(ff)))
    assert ff.value == 12 and np.array_equal(back, job_pcm.reshape(-1))


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def wav_data(path):
    data = open(path, "rb").read()
    at = data.index(b"data")
    size = struct.unpack_from("<I", data, at + 4)[0]
    assert struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and len(data) == at + 8 + size, (len(data), at, size)
    return size, data[at + 8:]


@pytest.mark.parametrize("ch", (1, 2, 3))
def test_the_cli_decodes_a_file_that_keeps_its_tail(gpu, tmp_path, ch):  # noqa: F811
    _build()
    cli = os.path.join(HOST, "sela_mi355x")
    n = 6 * B + 777
    pcm = pcm_of(n, ch, 5)
    wav, whole, back = (str(tmp_path / name) for name in ("in.wav", "whole.sela", "back.wav"))
    _write_wav(wav, pcm)
    run = lambda *args: subprocess.run([cli] + list(args), capture_output=True, text=True, timeout=120)  # noqa: E731
    done = run("-e", "--keep-tail", "--lossless", wav, whole)
    assert done.returncode == 0, done.stdout + done.stderr
    done = run("-d", whole, back)
    assert done.returncode == 0, done.stdout + done.stderr
    size, data = wav_data(back)
    assert size == n * ch * 2 and data == pcm.tobytes()
    # the player decodes through the streaming job alone and keeps refusing such a file
    assert run("-p", whole, str(tmp_path / "out.pcm")).returncode == 1


@pytest.mark.parametrize("ch, n", [(2, 6 * B + 777), (3, B + 5), (2, 1500), (2, 3 * B)])
def test_a_tailed_file_through_the_host_classes(gpu, tmp_path, ch, n):  # noqa: F811
    """sela::Decoder::process and decodeFile on streams, on a file of several frames, of one long frame, of less than one frame (no
    frame for the streaming job) and of whole frames only: each gives the WAV's samples."""
    _build()
    exe = str(tmp_path / "decode_whole_host")
    root = os.path.dirname(HOST)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I" + os.path.join(HOST, "include"), "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "c", "decode_whole_host.cpp"), os.path.join(HOST, "libsela_host.a"), "-L" + os.path.join(root, "sela_amd"), "-lsela_hip",
                           "-Wl,-rpath," + os.path.join(root, "sela_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    pcm = pcm_of(n, ch, 5)
    wav, whole = str(tmp_path / "in.wav"), str(tmp_path / "whole.sela")
    _write_wav(wav, pcm)
    done = subprocess.run([os.path.join(HOST, "sela_mi355x"), "-e", "--keep-tail", "--lossless", wav, whole], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    frames = len(codec.whole_frames(n))
    done = subprocess.run([exe, whole, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.splitlines() == ["process: %d samples" % (n * ch), "stream: %d frames" % frames], done.stdout
    for name in ("process.wav", "stream.wav"):
        size, data = wav_data(str(tmp_path / name))
        assert size == n * ch * 2 and data == pcm.tobytes(), name
