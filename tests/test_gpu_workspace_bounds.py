"""Every device-pointer call inside the workspace it asks for (sela_amd/csrc/sela_workspace.h): given exactly *_workspace_bytes
bytes at an address that is no multiple of 256 -- include/sela_hip.h promises that any alignment will do -- in the middle of a
poisoned buffer, a call returns the outputs and status words it returns with a roomy, 256-byte aligned workspace, and leaves the
4096 bytes in front of its workspace and the 4096 behind it as they were.  The shapes are the smallest that reach every piece."""
import numpy as np
import pytest

import topology_cases as tc
import wide_cases as wc
from gpu_common import gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 4096
ODD = 100  # the workspace starts at 4096 + 100 bytes into an allocation: no multiple of 256, nor of 8
FILL = 0x5A


def _both_ways(torch, obj, size, run, attr="workspace"):
    """run() makes the call through obj (which takes its workspace and that workspace's size from obj.<attr>) and returns the
    tensors the call wrote, the status words among them -> those of the run in the exact, misaligned, poisoned workspace."""
    roomy = torch.empty(size + 65536, dtype=torch.uint8, device="cuda")
    assert roomy.data_ptr() % 256 == 0
    setattr(obj, attr, roomy)
    want = [t.clone() for t in run()]
    torch.cuda.synchronize()
    buf = torch.full((GUARD + ODD + size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    ws = buf[GUARD + ODD: GUARD + ODD + size]
    assert ws.numel() == size and ws.data_ptr() % 256 != 0
    setattr(obj, attr, ws)
    got = [t.clone() for t in run()]
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), (i, g.shape, w.shape)
        assert not bool((g.contiguous().view(-1).view(torch.uint8) == FILL).all()), (i, "the call did not write this output")
    assert bool((buf[: GUARD + ODD] == POISON).all()), "the call wrote in front of its workspace"
    assert bool((buf[GUARD + ODD + size:] == POISON).all()), "the call wrote behind its workspace"
    return got


def _bytes_of(torch, *tensors):
    """Outputs hold neither the other run's values nor what the allocator left there."""
    for t in tensors:
        t.view(-1).view(torch.uint8).fill_(FILL)


def _cuda(torch, array):
    a = np.ascontiguousarray(array)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


@pytest.fixture(scope="module")
def stereo(gpu):  # noqa: F811
    """3 stereo frames of 2048 samples, coded: (pcm [3, 2048, 2], frames uint8, offsets int64), on the device."""
    pcm = gpu.from_numpy(np.ascontiguousarray(synth_frames(3, 2, 0))).cuda()
    enc = codec.Encoder(3, 2)
    out = enc.encode(pcm)
    gpu.cuda.synchronize()
    enc_frames, offsets = out.to_host()
    return pcm, _cuda(gpu, enc_frames), _cuda(gpu, offsets)


def test_encode_device(gpu, stereo):  # noqa: F811
    pcm = stereo[0]
    enc = codec.Encoder(3, 2)

    def run():
        _bytes_of(gpu, enc.frames, enc.offsets, enc.status)
        enc.encode(pcm)
        gpu.cuda.synchronize()
        return [enc.frames[: int(enc.offsets[3].item())], enc.offsets, enc.status]

    got = _both_ways(gpu, enc, int(capi.lib().sela_hip_encode_workspace_bytes(3, 2)), run)
    assert gpu.equal(got[0], stereo[1]) and got[2].tolist() == [0, 0, 0, 0]


def test_decode_device_and_decode_payload_device(gpu, stereo):  # noqa: F811
    pcm, frames, offsets = stereo
    lib = capi.lib()
    dec = codec.Decoder(3, 2)

    def run():
        _bytes_of(gpu, dec.pcm, dec.status)
        dec.decode(frames, offsets, 3)
        gpu.cuda.synchronize()
        return [dec.pcm, dec.status]

    got = _both_ways(gpu, dec, int(lib.sela_hip_decode_workspace_bytes(3, 2)), run)
    assert got[1].tolist() == [0, 0, 0, 0]
    decoded = got[0].clone()

    dec.decode_payload(frames)  # (makes the offsets and the count the call writes)

    def run_payload():
        _bytes_of(gpu, dec.pcm, dec.status, dec.payload_offsets, dec.payload_count)
        dec.decode_payload(frames)
        gpu.cuda.synchronize()
        return [dec.pcm, dec.status, dec.payload_offsets, dec.payload_count]

    size = int(lib.sela_hip_index_workspace_bytes(frames.numel(), 3)) + int(lib.sela_hip_decode_workspace_bytes(3, 2))
    got = _both_ways(gpu, dec, size, run_payload, attr="payload_workspace")
    assert gpu.equal(got[0], decoded) and got[3].tolist() == [3] and gpu.equal(got[2], offsets)


@pytest.mark.parametrize("whole", [False, True], ids=["windows", "windows_whole"])
@pytest.mark.parametrize("own_flags", [True, False], ids=["flags_given", "flags_in_the_workspace"])
def test_decode_windows_device(gpu, stereo, whole, own_flags):  # noqa: F811
    """One window of 2050 samples: over the three 2048-sample frames, and over a 5000-sample whole-track stream's second and last
    frame (2952 samples).  Without d_window_flags the call keeps the flag words in its workspace."""
    lib = capi.lib()
    if whole:
        track = gpu.from_numpy(np.ascontiguousarray(synth_frames(3, 2, 5).reshape(-1, 2)[:5000])).cuda()
        we = codec.WholeEncoder(5000, 2)
        we.encode(track)
        fr, offs = we.to_host()
        frames, offsets, n_frames, start = _cuda(gpu, fr), _cuda(gpu, offs), 2, 1500
    else:
        frames, offsets, n_frames, start = stereo[1], stereo[2], 3, 2047
    wd = codec.WindowDecoder(1, 2050, 2, whole=whole)
    windows = gpu.from_numpy(wd.pack([start], 0, n_frames)).cuda()
    stream = gpu.cuda.current_stream().cuda_stream

    def run():
        _bytes_of(gpu, wd.out, wd.status, wd.window_flags)
        capi.check(wd.call(frames.data_ptr(), offsets.data_ptr(), n_frames, 2, windows.data_ptr(), 1, 2050, wd.format, wd.out.data_ptr(),
                           wd.window_flags.data_ptr() if own_flags else None, wd.status.data_ptr(), wd.workspace.data_ptr(), wd.workspace.numel(), stream))
        gpu.cuda.synchronize()
        return [wd.out, wd.status] + ([wd.window_flags] if own_flags else [])

    sizing = lib.sela_hip_decode_windows_whole_workspace_bytes if whole else lib.sela_hip_decode_windows_workspace_bytes
    got = _both_ways(gpu, wd, int(sizing(1, 2050, 2)), run)
    assert got[0].shape == (1, 2050, 2) and got[1].tolist() == [0, 0, 0, 0]


def _any_length_stream(channels, n):
    """3 frames of n samples per channel, 16-bit material, coded by the host route -> (samples int32 [3, ch, n], frames, offsets)."""
    rng = np.random.default_rng(1000 * channels + n)
    t = np.arange(n)
    samples = np.stack([np.stack([np.round(9000 * np.sin(t * (0.01 + 0.003 * c) + f) + rng.normal(0, 40, n)).astype(np.int32) for c in range(channels)])
                        for f in range(3)])
    frames, offsets = codec.encode_i32(samples)
    return samples, frames, offsets


@pytest.mark.parametrize("n", [2049, 2048], ids=["any_length_route", "route_of_2048"])
@pytest.mark.parametrize("channels", [3, 9])
def test_decode_i32_decode_n_and_verify_device(gpu, channels, n):  # noqa: F811
    """3 frames at stride 2049.  9 channels: k_generic_combine's channel-major copy (the `all` piece) on the any-length route, and
    on the route of 2048 the decoder of more than eight channels, which verify lets decode into its workspace."""
    lib = capi.lib()
    stride = 2049
    _, fr, offs = _any_length_stream(channels, n)
    frames, offsets = _cuda(gpu, fr), _cuda(gpu, offs)

    d32 = codec.Decoder32(3, channels, stride)

    def run32():
        _bytes_of(gpu, d32.samples, d32.counts, d32.sample_offsets, d32.status)
        d32.decode(frames, offsets, 3)
        gpu.cuda.synchronize()
        return [d32.samples[:, :, :n], d32.counts, d32.sample_offsets, d32.status]

    got = _both_ways(gpu, d32, int(lib.sela_hip_decode_i32_workspace_bytes(3, channels, stride)), run32)
    assert got[1].tolist() == [[n] * channels] * 3 and got[3].tolist()[:2] == [0, 0]

    dn = codec.DecoderN(3, channels, stride)

    def run_n():
        _bytes_of(gpu, dn.pcm, dn.sample_offsets, dn.status)
        dn.decode(frames, offsets, 3)
        gpu.cuda.synchronize()
        return [dn.pcm[: 3 * n], dn.sample_offsets, dn.status]

    got = _both_ways(gpu, dn, int(lib.sela_hip_decode_n_workspace_bytes(3, channels, stride)), run_n)
    assert got[2].tolist()[:2] == [0, 0] and got[2].tolist()[3] == (1 if n == 2048 else 2)
    pcm = got[0].clone()
    pcm[n + 7, channels - 1] += 1  # a difference in frame 1

    ver = codec.Verifier(3, channels, stride)

    def run_verify():
        _bytes_of(gpu, ver.diff_counts, ver.first_diff, ver.sample_offsets, ver.status)
        ver.verify(frames, offsets, 3, pcm)
        gpu.cuda.synchronize()
        return [ver.diff_counts, ver.first_diff, ver.sample_offsets, ver.status]

    got = _both_ways(gpu, ver, int(lib.sela_hip_verify_workspace_bytes(3, channels, stride)), run_verify)
    assert got[0].tolist() == [0, 1, 0] and got[3].tolist()[2] == 1


def test_verify_i32_device_with_a_frame_for_the_fallback(gpu):  # noqa: F811
    """3 frames of 3 channels, the middle one a chain in stream order: no direct layout, so the whole call goes through the
    fallback's pieces (the samples by channel, the counts, the marks) -- and the hook that reads the control words finds them."""
    lib = capi.lib()
    o = oracle()
    good = [wc.frame_bytes(o, tc.subframes(layout, tc.ORDINARY, 40 + k)) for k, (_, layout) in enumerate(tc.ACCEPTED_LAYOUTS[3][:2])]
    chain = wc.frame_bytes(o, tc.subframes(tc.CHAIN_IN_STREAM_ORDER, tc.ORDINARY, 43))
    blobs = [good[0], chain, good[1]]
    frames = _cuda(gpu, np.frombuffer(b"".join(bytes(b) for b in blobs), np.uint8).copy())
    offsets = _cuda(gpu, np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64))
    d32 = codec.Decoder32(3, 3, tc.N)
    samples = d32.decode(frames, offsets, 3)[0].clone()
    gpu.cuda.synchronize()
    samples[1, 2, 5] += 1  # a difference in the fallback's frame
    ver = codec.Verifier32(3, 3, tc.N)

    def run():
        _bytes_of(gpu, ver.diff_counts, ver.first_diff, ver.sample_offsets, ver.status)
        ver.verify(frames, offsets, 3, samples)
        gpu.cuda.synchronize()
        assert ver.fallback_frames(3) == 1
        return [ver.diff_counts, ver.first_diff, ver.sample_offsets, ver.status]

    got = _both_ways(gpu, ver, int(lib.sela_hip_verify_i32_workspace_bytes(3, 3, tc.N)), run)
    assert got[0].tolist() == [0, 1, 0] and got[1].tolist()[1] == 2 * tc.N + 5 and got[3].tolist()[2] == 1


@pytest.mark.parametrize("channels,paired", [(3, False), (4, True)], ids=["encode_i32", "encode_paired"])
def test_encode_i32_device_and_paired(gpu, channels, paired):  # noqa: F811
    """One frame of 100 samples."""
    lib = capi.lib()
    rng = np.random.default_rng(channels)
    samples = np.stack([np.round(20000 * np.sin(np.arange(100) * 0.07 + c) + rng.normal(0, 30, 100)).astype(np.int32) for c in range(channels)])[None]
    want_frames, want_offsets = codec.encode_i32(samples, paired=paired)
    enc = codec.Encoder32(1, channels, 100, paired=paired)
    x = _cuda(gpu, samples)

    def run():
        _bytes_of(gpu, enc.frames, enc.offsets, enc.status)
        enc.encode(x)
        gpu.cuda.synchronize()
        return [enc.frames[: int(enc.offsets[1].item())], enc.offsets, enc.status]

    sizing = lib.sela_hip_encode_paired_workspace_bytes if paired else lib.sela_hip_encode_i32_workspace_bytes
    got = _both_ways(gpu, enc, int(sizing(1, channels, 100)), run)
    assert got[0].cpu().numpy().tobytes() == want_frames.tobytes() and got[1].tolist() == [0, int(want_offsets[1])]


def test_encode_whole_device(gpu):  # noqa: F811
    """A 5000-sample stereo track: one 2048-sample frame through the plain call's pieces, the last frame of 2952 samples through
    the any-length call's, coded into the workspace and spliced behind."""
    lib = capi.lib()
    track = np.ascontiguousarray(synth_frames(3, 2, 5).reshape(-1, 2)[:5000])
    want_frames, want_offsets = codec.encode_whole_host(track)
    enc = codec.WholeEncoder(5000, 2)
    x = gpu.from_numpy(track).cuda()

    def run():
        _bytes_of(gpu, enc.frames, enc.offsets, enc.status)
        enc.encode(x)
        gpu.cuda.synchronize()
        return [enc.frames[: int(enc.offsets[2].item())], enc.offsets, enc.status]

    got = _both_ways(gpu, enc, int(lib.sela_hip_encode_whole_workspace_bytes(5000, 2)), run)
    assert got[0].cpu().numpy().tobytes() == np.asarray(want_frames).tobytes() and got[2].tolist() == [0, 0, 0, 0]
    assert got[1].tolist() == [int(v) for v in want_offsets]
