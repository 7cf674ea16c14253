"""GPU: a whole track with its tail -- sela_hip_encode_whole_device, sela_hip_encode_whole and the CLI's
-e --keep-tail.  The rule: frames 0 .. F - 2 of 2048 samples, byte for byte the plain call's, and a last frame of 2048 + t samples,
byte for byte frame::FrameEncoder's for a WavFrame of that length; below 2048 samples one frame.  Expected bytes are the oracle's
(oracle/sela_oracle.c, pinned against the unmodified reference): encode_frames on the 2048-sample frames, frame_encode on the last;
with SELA_HIP_ENCODE_LOSSLESS tests/lossless_model.py's."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import lossless_model
from gpu_common import HOST, _build, _write_wav, gpu  # noqa: F401  (fixture and helpers)
from oracle_lib import oracle, reference
from sela_amd import capi, codec
from sela_amd.synth import synth_pcm

pytestmark = pytest.mark.gpu

N = 2048
POISON = 0xA5
CHANNELS = (1, 2, 3)
# two fast-path frames and a tail of t; one long frame alone (no fast-path frame); whole frames only
SAMPLES = [2 * N + t for t in (1, 77, 100, 101, 2047)] + [N + 5, 3 * N]


@functools.lru_cache(maxsize=None)
def _corpus():
    import corpus

    return corpus.build(400, 20260927).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _track(n, ch, k=0):
    """n samples of the corpus from a place of k's; for odd k the second channel follows the first (the difference wins)."""
    start = (37 * k + 11 * ch) % 300 * N
    x = _corpus()[start: start + n].astype(np.int32)
    if k % 2:
        x[:, 1] = x[:, 0] - (x[:, 1] >> 7)
    out = np.clip(x[:, {1: [0], 2: [0, 1], 3: [0, 1, 0]}[ch]], -32768, 32767).astype(np.int16)
    if ch == 3:
        out[:, 2] = out[::-1, 2]
    out.setflags(write=False)
    return out


def _layout(n):
    """(frames of 2048 samples, samples of the last frame or 0) by the rule"""
    if n < N:
        return 0, n
    return (n // N - 1, N + n % N) if n % N else (n // N, 0)


def _join(blobs):
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    return b"".join(blobs), offs


@functools.lru_cache(maxsize=None)
def _expected(n, ch, k=0, lossless=False):
    """-> (bytes, offsets uint64 [frames + 1]) of the whole stream of _track(n, ch, k)"""
    o = oracle()
    pcm = _track(n, ch, k)
    whole, last = _layout(n)
    frames = [pcm[f * N: (f + 1) * N] for f in range(whole)] + ([pcm[whole * N:]] if last else [])
    if lossless:
        return _join([lossless_model.encode_frame(o, np.ascontiguousarray(x.T.astype(np.int32)), True) for x in frames])
    blobs = []
    if whole:
        blob, offs, _ = o.encode_frames(pcm[: whole * N].reshape(whole, N, ch))
        blobs = [blob[int(offs[f]): int(offs[f + 1])].tobytes() for f in range(whole)]
    if last:
        blobs.append(o.frame_encode(pcm[whole * N:]))
    return _join(blobs)


def _device(gpu, pcm, lossless=False, capacity=None, guard=0):  # noqa: F811
    """one call on a fresh encoder whose frames are poisoned -> (frames uint8 [capacity + guard], offsets uint64, status int64 [4])"""
    n, ch = pcm.shape
    enc = codec.WholeEncoder(n, ch, lossless=lossless, capacity=capacity)
    if guard:
        enc.frames = gpu.empty(enc.capacity + guard, dtype=gpu.uint8, device="cuda")
    enc.frames.fill_(POISON)
    enc.offsets.fill_(-1)
    enc.status.fill_(-1)
    enc.encode(gpu.from_numpy(np.array(pcm, order="C")).cuda() if n else gpu.empty((0, ch), dtype=gpu.int16, device="cuda"))
    gpu.cuda.synchronize()
    return enc.frames.cpu().numpy(), enc.offsets[: enc.n_frames + 1].cpu().numpy().view(np.uint64), enc.status.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _second_subframe_type(frame):
    cw = struct.unpack_from("<H", frame, 4 + 4)[0]
    rw = struct.unpack_from("<H", frame, 4 + 7 + 4 * cw + 1)[0]
    return frame[4 + 12 + 4 * (cw + rw) + 1]


# ---- 1. bytes against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("n", SAMPLES)
def test_bytes_equal_the_oracles(gpu, n, ch):  # noqa: F811
    k = SAMPLES.index(n)
    pcm = _track(n, ch, k)
    want, want_offs = _expected(n, ch, k)
    assert [(int(a), int(b)) for a, b in codec.whole_frames(n)] == [(f * N, N) for f in range(len(want_offs) - 2)] + [((len(want_offs) - 2) * N, n - (len(want_offs) - 2) * N)]
    frames, offs, st = _device(gpu, pcm)
    assert np.array_equal(offs, want_offs) and st.tolist() == [0, 0, 0, 0], (offs, want_offs, st)
    assert frames[: len(want)].tobytes() == want
    assert (frames[len(want):] == POISON).all()
    h_frames, h_offs = codec.encode_whole_host(pcm)
    assert h_frames.tobytes() == want and np.array_equal(h_offs, want_offs)
    whole, last = _layout(n)
    if last:  # the long frame comes back from the unmodified reference's frame decoder
        ref = reference() or oracle()
        dec, used = ref.frame_decode_i32(want[int(want_offs[whole]):], ch, stride=last)
        assert used == len(want) - int(want_offs[whole])
        back = np.stack(dec, axis=1)
        # (the plain stream is the reference's: a frame with a rounding tie comes back one off, DESIGN.md 2 -- none of these has one)
        assert back.shape == (last, ch) and np.array_equal(back, pcm[whole * N:].astype(np.int32))
    else:  # whole frames only: the plain device call's bytes and offsets
        enc = codec.Encoder(n // N, ch)
        out = enc.encode(gpu.from_numpy(np.array(pcm, order="C").reshape(n // N, N, ch)).cuda())
        gpu.cuda.synchronize()
        p_frames, p_offs = out.to_host()
        assert p_frames.tobytes() == want and np.array_equal(p_offs, want_offs)


def test_both_stereo_decisions_occur_in_the_long_frames():
    types = set()
    for n in SAMPLES:
        whole, last = _layout(n)
        if last:
            want, offs = _expected(n, 2, SAMPLES.index(n))
            types.add(_second_subframe_type(want[int(offs[whole]):]))
    assert types == {0, 1}


# ---- 2. below one frame ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [150, 2047])
def test_a_track_below_2048_samples_is_one_frame(gpu, n):  # noqa: F811
    for ch in (1, 2):
        pcm = _track(n, ch, 1)
        want = oracle().frame_encode(pcm)
        frames, offs, st = _device(gpu, pcm)
        assert offs.tolist() == [0, len(want)] and st.tolist() == [0, 0, 0, 0]
        assert frames[: len(want)].tobytes() == want
        h_frames, h_offs = codec.encode_whole_host(pcm)
        assert h_frames.tobytes() == want and h_offs.tolist() == [0, len(want)]


def test_a_short_noise_track_is_refused_as_the_plain_call_refuses_it(gpu):  # noqa: F811
    lib = capi.lib()
    pcm = np.ascontiguousarray(np.random.default_rng(2).integers(-20000, 20000, (20, 1)).astype(np.int16))
    out = np.zeros(1 << 16, np.uint8)
    offs = np.zeros(2, np.uint64)
    plain = lib.sela_hip_encode(pcm.ctypes.data, 1, 1, 20, out.ctypes.data, out.nbytes, offs.ctypes.data)
    assert plain == -6  # SELA_HIP_ERANGE: the block is no longer than the order its analysis picks
    assert lib.sela_hip_encode_whole(pcm.ctypes.data, 20, 1, out.ctypes.data, out.nbytes, offs.ctypes.data, 0) == plain
    _, _, st = _device(gpu, pcm)
    assert int(st[0]) & capi.FLAG_SHORT_BLOCK and codec.encode_status_error(st) == plain


def test_no_samples(gpu):  # noqa: F811
    frames, offs, st = _device(gpu, np.zeros((0, 2), np.int16))
    assert offs.tolist() == [0] and st.tolist() == [0, 0, 0, 0] and (frames == POISON).all()
    h_frames, h_offs = codec.encode_whole_host(np.zeros((0, 2), np.int16))
    assert len(h_frames) == 0 and h_offs.tolist() == [0]


# ---- 3. lossless ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("n", SAMPLES)
def test_lossless_streams_give_every_sample_back(gpu, n, ch):  # noqa: F811
    k = SAMPLES.index(n)
    pcm = _track(n, ch, k)
    want, want_offs = _expected(n, ch, k, True)
    enc = codec.WholeEncoder(n, ch, lossless=True)
    frames, offs, _ = enc.encode(gpu.from_numpy(np.array(pcm, order="C")).cuda())
    got, got_offs = enc.to_host()
    assert np.array_equal(got_offs, want_offs) and got.tobytes() == want
    h_frames, h_offs = codec.encode_whole_host(pcm, lossless=True)
    assert h_frames.tobytes() == want and np.array_equal(h_offs, want_offs)
    dec = codec.DecoderN(enc.n_frames, ch, 2 * N)
    back, sample_offs = dec.decode(frames, offs.contiguous(), enc.n_frames)
    gpu.cuda.synchronize()
    dec.check()
    assert sample_offs.cpu().numpy().tolist() == [f * N for f in range(enc.n_frames)] + [n]
    assert np.array_equal(back[:n].cpu().numpy(), pcm)


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", (2, 3))
def test_capacity(gpu, ch):  # noqa: F811
    n = 3 * N + 777
    pcm = _track(n, ch, 2)
    want, want_offs = _expected(n, ch, 2)
    for cap, fits in ((len(want) - 1, 2), (int(want_offs[1]) - 4, 0)):  # one byte short of the last frame's end; short of frame 0
        frames, offs, st = _device(gpu, pcm, capacity=cap, guard=4096)
        assert np.array_equal(offs, want_offs), cap  # (written in full)
        assert st.tolist() == [0, 3 - fits, 0, 0] and codec.encode_status_error(st) == -4, (cap, st)
        assert frames[: int(want_offs[fits])].tobytes() == want[: int(want_offs[fits])], cap
        assert (frames[int(want_offs[fits]):] == POISON).all(), cap  # (not a byte of a frame that does not fit; the guard neither)
    frames, offs, st = _device(gpu, pcm, capacity=len(want), guard=4096)
    assert st.tolist() == [0, 0, 0, 0] and frames[: len(want)].tobytes() == want and (frames[len(want):] == POISON).all()


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_replay_on_new_samples(gpu):  # noqa: F811
    torch = gpu
    n = 3 * N + 77
    a, b, c = _track(n, 2, 4), _track(n, 2, 7), _track(n, 2, 10)
    enc = codec.WholeEncoder(n, 2)
    d_x = torch.from_numpy(np.array(a, order="C")).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.encode(d_x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = enc.to_host()
    assert eager[0].tobytes() == _expected(n, 2, 4)[0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enc.encode(d_x)
    for x, k in ((b, 7), (c, 10)):
        d_x.copy_(torch.from_numpy(np.array(x, order="C")))
        enc.frames.fill_(POISON)
        enc.offsets.fill_(-1)
        enc.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert enc.status.cpu().numpy().tolist() == [0, 0, 0, 0]
        frames, offs = enc.to_host()
        want, want_offs = _expected(n, 2, k)
        assert frames.tobytes() == want and np.array_equal(offs, want_offs)
        e_frames, e_offs, e_st = _device(gpu, x)  # the eager call on the same samples
        assert e_frames[: len(want)].tobytes() == want and np.array_equal(e_offs, offs) and e_st.tolist() == [0, 0, 0, 0]


# ---- 6. scale, once: the team kernels' regime ---------------------------------------------------------------------------------------------
def test_a_whole_track_of_3875_frames_and_777_samples(gpu):  # noqa: F811
    torch = gpu
    frames_2048, tail = 3875, 777
    n = frames_2048 * N + tail
    pcm = synth_pcm(n, 2, 0)
    d_pcm = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
    enc = codec.WholeEncoder(n, 2)
    enc.frames.fill_(POISON)
    enc.encode(d_pcm)
    frames, offs = enc.to_host()
    assert len(offs) == frames_2048 + 1
    plain = codec.Encoder(frames_2048 - 1, 2)
    out = plain.encode(d_pcm[: (frames_2048 - 1) * N].reshape(frames_2048 - 1, N, 2))
    torch.cuda.synchronize()
    p_frames, p_offs = out.to_host()
    assert np.array_equal(offs[:frames_2048], p_offs) and frames[: len(p_frames)].tobytes() == p_frames.tobytes()
    last = oracle().frame_encode(pcm[(frames_2048 - 1) * N:])
    assert int(offs[-1]) == len(p_frames) + len(last) and frames[len(p_frames):].tobytes() == last
    enc.frames.fill_(POISON)  # again, on the same workspace
    enc.encode(d_pcm)
    again, again_offs = enc.to_host()
    assert np.array_equal(again_offs, offs) and again.tobytes() == frames.tobytes()


def test_a_thread_with_an_open_streaming_job_is_left_alone(gpu):  # noqa: F811
    from sela_amd.synth import synth_frames

    lib = capi.lib()
    job_pcm = synth_frames(12, 2, 5)
    want_frames, want_offs = codec.encode_host(job_pcm)
    out = np.zeros(int(lib.sela_hip_encode_bound_bytes(12, 2)), np.uint8)
    offs = np.zeros(13, np.uint64)
    job = C.c_void_p()
    capi.check(lib.sela_hip_encode_begin(C.byref(job), 2, 12, out.ctypes.data, out.nbytes, offs.ctypes.data))
    capi.check(lib.sela_hip_encode_feed(job, job_pcm.ctypes.data, 5, None, None))
    n = 2 * N + 101
    for lossless in (False, True):
        h_frames, h_offs = codec.encode_whole_host(_track(n, 2, 3), lossless=lossless)
        want, w_offs = _expected(n, 2, 3, lossless)
        assert h_frames.tobytes() == want and np.array_equal(h_offs, w_offs)
    capi.check(lib.sela_hip_encode_feed(job, job_pcm[5:].ctypes.data, 7, None, None))
    total = C.c_uint64(0)
    capi.check(lib.sela_hip_encode_end(job, None, C.byref(total)))
    assert np.array_equal(offs, want_offs) and out[: total.value].tobytes() == want_frames.tobytes()


# ---- 7. files ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", (2, 3))
def test_keep_tail_files(gpu, tmp_path, ch):  # noqa: F811
    _build()
    cli = os.path.join(HOST, "sela_mi355x")
    n = 2 * N * 3 + 777
    pcm = _track(n, ch, 5)
    wav, whole, cut, back = (str(tmp_path / name) for name in ("in.wav", "whole.sela", "cut.sela", "back.wav"))
    _write_wav(wav, pcm)
    run = lambda *args: subprocess.run([cli] + list(args), capture_output=True, text=True, timeout=120)  # noqa: E731
    done = run("-e", "--keep-tail", "--lossless", wav, whole)
    assert done.returncode == 0, done.stdout + done.stderr
    verdict = run("-v", wav, whole)
    assert verdict.returncode == 0 and "tail:" not in verdict.stdout, verdict.stdout + verdict.stderr
    assert run("-e", "--lossless", wav, cut).returncode == 0
    verdict = run("-v", wav, cut)
    assert verdict.returncode == 4 and "tail: 777 samples per channel" in verdict.stdout, verdict.stdout + verdict.stderr
    blob = open(whole, "rb").read()
    assert blob[:4] == b"SeLa" and struct.unpack_from("<I", blob, 11)[0] == 6 == len(codec.whole_frames(n))
    assert struct.unpack_from("<I", open(cut, "rb").read(), 11)[0] == 6
    api_frames, api_offs = codec.encode_whole_host(pcm, lossless=True)
    assert blob[15:] == api_frames.tobytes() and len(api_offs) == 7
    done = run("-d", whole, back)
    assert done.returncode == 0, done.stdout + done.stderr
    data = open(back, "rb").read()
    at = data.index(b"data")
    assert struct.unpack_from("<I", data, at + 4)[0] == pcm.nbytes and data[at + 8:] == pcm.tobytes()
    # -p decodes through the streaming job, which serves 2048-sample frames only: a tailed file is refused
    assert run("-p", whole, str(tmp_path / "out.pcm")).returncode == 1
    # the plain stream (no --lossless) keeps the tail as well: the reference's bytes for frames of those lengths
    plain = str(tmp_path / "plain.sela")
    assert run("-e", "--keep-tail", wav, plain).returncode == 0
    want, _ = _expected(n, ch, 5)
    assert open(plain, "rb").read()[15:] == want


@pytest.mark.parametrize("ch, n", [(2, 2 * N * 3 + 777), (3, N + 5), (2, 1500)])
def test_keep_tail_through_the_host_classes(gpu, tmp_path, ch, n):  # noqa: F811
    """The paths the CLI does not reach -- sela::Encoder::keepTail through process() and writeToFile, and encodeFile on streams --
    and the CLI's own, on a file of several frames, of one long frame, and of less than one frame (no frame for the streaming job):
    all three files are the 15-byte header with the rule's numFrames and sela_hip_encode_whole's bytes.  keepTail with
    pairChannels is refused by all three entries."""
    _build()
    exe = str(tmp_path / "keep_tail_host")
    root = os.path.dirname(HOST)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I" + os.path.join(HOST, "include"), "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "c", "keep_tail_host.cpp"), os.path.join(HOST, "libsela_host.a"), "-L" + os.path.join(root, "sela_amd"), "-lsela_hip",
                           "-Wl,-rpath," + os.path.join(root, "sela_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    pcm = _track(n, ch, 5)
    wav = str(tmp_path / "in.wav")
    _write_wav(wav, pcm)
    frames = len(codec.whole_frames(n))
    api_frames, api_offs = codec.encode_whole_host(pcm, lossless=True)
    assert len(api_offs) == frames + 1
    done = subprocess.run([exe, wav, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    lines = done.stdout.splitlines()
    assert lines[0] == "process: %d frames, header %d, %d bytes" % (frames, frames, len(api_frames)) and lines[1] == "stream: %d frames" % frames, lines
    assert lines[2:] == ["refused: Encoder: keepTail with pairChannels is not supported"] * 3, lines
    assert not os.path.exists(str(tmp_path / "never_path.sela"))
    cli = subprocess.run([os.path.join(HOST, "sela_mi355x"), "-e", "--keep-tail", "--lossless", wav, str(tmp_path / "cli.sela")], capture_output=True, text=True, timeout=120)
    assert cli.returncode == 0, cli.stdout + cli.stderr
    for name in ("process.sela", "stream.sela", "cli.sela"):
        blob = open(str(tmp_path / name), "rb").read()
        assert blob[:4] == b"SeLa" and struct.unpack_from("<I", blob, 11)[0] == frames, name
        assert blob[15:] == api_frames.tobytes(), name
