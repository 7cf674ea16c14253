"""The step-up recursion with its reflection coefficients read from LDS (sela_device.h, step_up_lds): stages in groups of four,
the coefficient of a stage fetched four stages ahead, the group of stages 60 .. 63 changing from one register to two in its
middle.  Orders on both sides of every seam -- 1, 2, 3 (less than a group), 31 .. 33, 60 .. 66 (stage 62 is the first of the
second register), 99 and 100 -- in the decoders (the coefficients parked in a[] itself) and in the three encode kernels.

Decoder: stereo frames whose two subframes carry the order, quantised coefficients random within the tables, all -64 and all 63,
through k_decode_frames and the 32-bit decoder against the oracle's frame decoder; the predictor itself through the stage entry
against oracle.lpc_coeffs.  Encoder: blocks of those orders (the constructions of test_gpu_schur_phases.py) in launches of 1, 3
and 5 frames on k_encode_blocks and both k_encode_teams: order, coefficients and predictor of the trace instantiation and the
frame bytes of the product; five of them in lossless mode against the model of tests/lossless_model.py."""
import functools

import numpy as np
import pytest
from oracle_lib import oracle

import lossless_model as model
from gpu_common import _encode, gpu  # noqa: F401  (fixture and helper)
from synth_cases import COEF_OVERFLOW, ORDERS, decoder_frames  # (the decoder's frames: built once for every test of the synthesis)
from test_gpu_schur_phases import _echo, _noise

# encoder blocks: order -> (construction, argument, seed); the oracle's order of each is asserted below
ECHO_SEEDS = {1: 8, 2: 10, 3: 8, 31: 0, 32: 0, 33: 0, 60: 0, 61: 1, 62: 0, 63: 0, 64: 0, 65: 0, 66: 1}
NOISE_SEEDS = {99: 178, 100: 120}  # full-scale white noise
LAUNCHES = (1, 3, 5, 5, 1)         # frames per launch: the fifteen blocks in turn


@functools.lru_cache(maxsize=None)
def encoder_blocks():
    rows = [_echo(ECHO_SEEDS[o_], o_) if o_ in ECHO_SEEDS else _noise(NOISE_SEEDS[o_], 32767) for o_ in ORDERS]
    pcm = np.stack(rows)[:, :, None]
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def encoder_reference():
    """per block: (order, q, a[0 .. order]) of the oracle's analysis; and the oracle's frames of every launch"""
    o = oracle()
    pcm = encoder_blocks()
    per_block = []
    for b in pcm:
        order, q, _, a, _, _ = o.lpc_analyze(b[:, 0].astype(np.int32), with_trace=True)
        assert np.array_equal(a, o.lpc_coeffs(order, q))
        per_block.append((int(order), q, a))
    launches, at = [], 0
    for n in LAUNCHES:
        frames, offsets, _ = o.encode_frames(pcm[at: at + n], threads=2)
        launches.append((at, n, frames, offsets))
        at += n
    assert at == len(pcm)
    return per_block, launches


def test_the_cases_are_what_they_are_called():
    """(no kernel: the oracle alone)  The encoder blocks have the orders they were chosen for; the random coefficients stay
    inside what the reference defines at every order, the extreme ones leave it (2^35 x coefficient beyond int64) from order
    60 on, where only the 16-bit decoder, which keeps the reference's x86 result, still answers."""
    assert [r[0] for r in encoder_reference()[0]] == ORDERS
    for label, _, _, _, pcm, wide, flags in decoder_frames():
        assert flags in (0, COEF_OVERFLOW), (label, flags)
        if "random" in label:
            assert flags == 0, label
        assert all(np.array_equal(wide[c].astype(np.int16), pcm[:, c]) for c in range(2)), label
    assert any(f[6] for f in decoder_frames())


def _stream(frames):
    blobs = [f[3] for f in frames]
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_k_decode_frames_at_every_order(gpu, form):  # noqa: F811
    """Both recurrence forms of k_decode_frames (a launch of 45 frames would see the lonely-wave form alone)."""
    from sela_amd import capi, codec

    frames = decoder_frames()
    stream, offs = _stream(frames)
    dec = codec.Decoder(len(frames), 2)
    capi.lib().sela_hip_debug_decode_recurrence(form)
    try:
        pcm = dec.decode(gpu.from_numpy(stream).cuda(), gpu.from_numpy(offs.view(np.int64)).cuda(), len(frames))
        gpu.cuda.synchronize()
    finally:
        capi.lib().sela_hip_debug_decode_recurrence(-1)
    dec.check()
    got = pcm.cpu().numpy()
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], f[4]), f[0]


@pytest.mark.gpu
def test_the_32_bit_decoder_at_every_order(gpu):  # noqa: F811
    from sela_amd import capi, codec

    clean = [f for f in decoder_frames() if f[6] == 0]
    stream, offs = _stream(clean)
    got = codec.decode_i32(stream, offs, 2)
    for i, f in enumerate(clean):
        for c in range(2):
            assert np.array_equal(got[i][c], f[5][c]), (f[0], c)
            assert np.array_equal(got[i][c].astype(np.int16), f[4][:, c]), (f[0], c)
    # a predictor beyond int64 is outside what the reference defines: refused, as everywhere on this route
    refused = [f for f in decoder_frames() if f[6]]
    stream, offs = _stream(refused[:3])
    with pytest.raises(capi.SelaHipError):
        codec.decode_i32(stream, offs, 2)


@pytest.mark.gpu
def test_the_decoders_predictor_at_every_order(gpu):  # noqa: F811
    """a[0 .. order] itself, from the stage entry that runs the decoders' dequantisation and step-up."""
    from sela_amd import codec

    o = oracle()
    clean = [f for f in decoder_frames() if f[6] == 0]
    qs = [q for f in clean for q in (f[1], f[2])]
    order = np.array([len(q) for q in qs], np.int32)
    q = np.zeros((len(qs), 100), np.int32)
    for i, v in enumerate(qs):
        q[i, : len(v)] = v
    _, coefs = codec.lpc_decode(order, q, np.zeros((len(qs), 2048), np.int32), want_coefficients=True)
    for i, v in enumerate(qs):
        assert np.array_equal(coefs[i, : len(v) + 1], o.lpc_coeffs(len(v), v)), (len(v), i)


@pytest.fixture(params=[0, 8, 16], ids=["blocks", "teams_of_8", "teams_of_16"])
def kernel(request, gpu):  # noqa: F811
    from sela_amd import capi

    capi.lib().sela_hip_debug_encode_teams(request.param)
    yield request.param
    capi.lib().sela_hip_debug_encode_teams(-1)


@pytest.mark.gpu
def test_the_encoders_predictor_at_every_order(gpu, kernel):  # noqa: F811
    from sela_amd import capi

    pcm = encoder_blocks()
    per_block, launches = encoder_reference()
    for at, n, want_frames, want_offsets in launches:
        part = np.array(pcm[at: at + n])
        assert capi.lib().sela_hip_debug_encode_kernel(n, 1) == kernel
        frames, offsets, _, _ = _encode(gpu, part)
        assert np.array_equal(offsets, want_offsets) and np.array_equal(frames, want_frames), (kernel, at, n)
        frames, offsets, enc, _ = _encode(gpu, part, with_trace=True)
        assert np.array_equal(offsets, want_offsets) and np.array_equal(frames, want_frames), (kernel, at, n, "trace")
        traces = enc.traces(n)
        for i in range(n):
            order, q, a = per_block[at + i]
            assert traces[i].order == order, (kernel, at + i)
            assert np.array_equal(np.array(traces[i].q[:order], np.int32), q), (kernel, at + i)
            assert np.array_equal(np.array(traces[i].a[: order + 1], np.int64), a), (kernel, at + i)


@pytest.mark.gpu
def test_orders_across_the_second_register_in_lossless_mode(gpu):  # noqa: F811
    """Orders 62 .. 66 as one launch with SELA_HIP_ENCODE_LOSSLESS: the model's bytes."""
    from sela_amd import codec

    o = oracle()
    first = ORDERS.index(62)
    pcm = np.array(encoder_blocks()[first: first + 5])
    want_bytes, want_offs = model.stream(o, [np.ascontiguousarray(f.T.astype(np.int32)) for f in pcm], True)
    enc = codec.Encoder(len(pcm), 1, lossless=True)
    out = enc.encode(gpu.from_numpy(pcm).cuda())
    gpu.cuda.synchronize()
    frames, offs = out.to_host()
    assert np.array_equal(np.asarray(offs, np.uint64), want_offs)
    assert np.asarray(frames).tobytes() == want_bytes.tobytes()
