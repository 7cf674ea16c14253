"""GPU parity tests, by subject: 25- to 31-bit audio and residues near 2^29 / 2^30 through every decoder, the encoder and the LPC
stages on their own.  The decoders' folded synthesis (sela_decode_core.inc, synth_mac) keeps a residue only mod 2^29; these inputs
are where that shows if its range checks miss.  Every expected value is the oracle's (oracle/sela_oracle.c, pinned to the
unmodified reference on this range by tests/test_oracle_vs_reference.py); inputs come from tests/wide_cases.py."""
import ctypes as C

import numpy as np
import pytest

import wide_cases as wc
from gpu_common import _both_decoders, _build_frame, _decode, _one, _rice_words, _wrap_taps, gpu  # noqa: F401  (fixtures and helpers)
from oracle_lib import oracle

pytestmark = pytest.mark.gpu

ERANGE = -6


def _stream(frames):
    return np.frombuffer(b"".join(frames), np.uint8).copy(), np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)


def _check_i32(blob, offs, ch, want_frames, label):
    """decode_i32 with the standard kernel offered and with the any-length kernel alone, against the oracle's channels."""
    offered, alone, took = _both_decoders(blob, offs, ch)
    for f, want in enumerate(want_frames):
        for c in range(ch):
            assert np.array_equal(offered[f][c], want[c]), (label, f, c, "standard kernel offered")
            assert np.array_equal(alone[f][c], want[c]), (label, f, c, "any-length kernel alone")
    return took


def _check_16(gpu, frames, ch, label):  # noqa: F811
    """sela_hip_decode (host), Decoder.decode (sela_hip_decode_device) and Decoder.decode_payload against the oracle's int16
    frames."""
    from sela_amd import codec

    o = oracle()
    stream, offs = _stream(frames)
    want = np.stack([o.frame_decode(f, ch)[0] for f in frames])
    host = codec.decode_host(stream, offs, ch)
    assert host.shape == want.shape and np.array_equal(host, want), (label, "sela_hip_decode")
    dev = _decode(gpu, stream, offs, ch)
    for f in range(len(frames)):
        assert np.array_equal(dev[f], want[f]), (label, f, "sela_hip_decode_device")
    dec = codec.Decoder(len(frames), ch)
    pcm, _, count = dec.decode_payload(gpu.from_numpy(stream).cuda())
    gpu.cuda.synchronize()
    dec.check()
    assert int(count.cpu()[0]) == len(frames), label
    got = pcm.cpu().numpy()
    for f in range(len(frames)):
        assert np.array_equal(got[f], want[f]), (label, f, "decode_payload")


def _stage_batch(n, rng, o):
    """Blocks for the synthesis stage: every order below n, every wide residue at every placement, coefficients that start the
    synthesis folded."""
    orders, qs, res = [], [], []
    for order in wc.ORDERS:
        if order >= n:  # (the reference writes samples[1 .. order] whatever the length: refused, tested elsewhere)
            continue
        q = wc.fold_coefficients(order, rng)
        assert wc.fits_fold(o.lpc_coeffs(order, q)), order
        for _, r in wc.stage_cases(n, rng):
            orders.append(order)
            row = np.zeros(100, np.int32)
            row[:order] = q
            qs.append(row)
            res.append(r)
    return np.array(orders, np.int32), np.stack(qs), np.stack(res)


@pytest.mark.parametrize("n", [2048, 1, 63, 64, 65, 1000, 2049, 6000])
def test_the_synthesis_stage_on_wide_residues(gpu, n):  # noqa: F811
    """sela_hip_lpc_decode (2048) / sela_hip_lpc_decode_n (every n) on residues at k * 2^29 + d, +-(2^30 - 1), -2^30, +-2^28 +- 1
    and the range check's edges +-(2^23 - 1), +-2^23, at lane 0, lane 63 and in the second block of a ring of 128, for orders on
    both sides of every ring and group of the synthesis: the oracle's samples and Q35 predictors."""
    from sela_amd import codec

    o = oracle()
    rng = np.random.default_rng(900 + n)
    orders, q, res = _stage_batch(n, rng, o)
    runs = [("lpc_decode_n", codec.lpc_decode_n)] + ([("lpc_decode", codec.lpc_decode)] if n == 2048 else [])
    for label, call in runs:
        got, coefs = call(orders, q, res, want_coefficients=True)
        for b in range(len(orders)):
            order = int(orders[b])
            want = o.lpc_synth(order, q[b, :order], res[b])
            assert np.array_equal(got[b], want), (label, n, order, b, int(np.flatnonzero(got[b] != want)[0]))
            assert np.array_equal(coefs[b, : order + 1], o.lpc_coeffs(order, q[b, :order])), (label, n, order, b)


def _crafted_mono_frames(rng, o):
    frames = []
    for order in wc.ORDERS:
        q = wc.fold_coefficients(order, rng)
        for _, r in wc.stage_cases(2048, rng, wc.FRAME_RESIDUES):
            frames.append(_build_frame([(0, 0, 0, q, r)]))
    return frames


def test_crafted_wide_frames_through_every_decoder(gpu):  # noqa: F811
    """The stage's residues packed as mono frames (orders 0 .. 100, coefficients that start folded) through sela_hip_decode,
    Decoder.decode, Decoder.decode_payload and decode_i32 (k_decode_subframes32 offered and the any-length kernel alone)."""
    o = oracle()
    rng = np.random.default_rng(41)
    frames = _crafted_mono_frames(rng, o)
    _check_16(gpu, frames, 1, "mono")
    stream, offs = _stream(frames)
    took = _check_i32(stream, offs, 1, [o.frame_decode_i32(f, 1)[0] for f in frames], "mono")
    assert took > 0  # (the standard kernel decoded them)


def test_wide_residues_in_frames_of_more_than_eight_channels(gpu):  # noqa: F811
    """Nine and ten channels (k_decode_frames_wide), every channel a different wide residue vector and order."""
    o = oracle()
    rng = np.random.default_rng(42)
    cases = wc.stage_cases(2048, rng, wc.FRAME_RESIDUES)
    for ch in (9, 10):
        frames = []
        for f in range(4):
            subs = []
            for c in range(ch):
                order = wc.ORDERS[(f * ch + c) % len(wc.ORDERS)]
                subs.append((c, 0, c, wc.fold_coefficients(order, rng), cases[(f * ch + c) % len(cases)][1]))
            frames.append(_build_frame(subs))
        _check_16(gpu, frames, ch, f"{ch} channels")
        stream, offs = _stream(frames)
        _check_i32(stream, offs, ch, [o.frame_decode_i32(f, ch)[0] for f in frames], f"{ch} channels")


def test_a_difference_subframe_under_a_wide_parent(gpu):  # noqa: F811
    """Stereo frames whose channel 1 is parent - difference with the parent near +-2^30 (the sum wraps int32, as
    src/frame/frame_decoder.cpp:65 does it), and one with a wide parent and an ordinary difference."""
    o = oracle()
    frames = []
    for seed in (1, 2, 3):
        subs, wraps = wc.stereo_wrap_subframes(o, 2048, seed)
        assert wraps > 0
        frames.append(wc.frame_bytes(o, subs))
    rng = np.random.default_rng(43)
    r = rng.integers(-300, 301, 2048).astype(np.int32)
    r[[0, 63, 212, 1000]] = [wc.P29 + 5, -wc.P29 - 7, -wc.P30, wc.P30 - 1]
    frames.append(_build_frame([(0, 0, 0, wc.fold_coefficients(2, rng), r), (1, 1, 0, wc.fold_coefficients(48, rng), rng.integers(-40, 40, 2048))]))
    _check_16(gpu, frames, 2, "stereo")
    stream, offs = _stream(frames)
    _check_i32(stream, offs, 2, [o.frame_decode_i32(f, 2)[0] for f in frames], "stereo")
    for n, seed in ((1000, 4), (4096, 5)):  # (other lengths: the 32-bit decoders only)
        subs, wraps = wc.stereo_wrap_subframes(o, n, seed)
        assert wraps > 0
        blob = wc.frame_bytes(o, subs)
        _check_i32(np.frombuffer(blob, np.uint8).copy(), _one(len(blob)), 2, [o.frame_decode_i32(blob, 2)[0]], f"stereo {n}")


def _encode_i32(x):
    """sela_hip_encode_i32 on one frame x int32 [channels, n], with room for 65535 Rice words per subframe (the bound the library
    reports for 2048-sample frames covers samples of 17 bits, not wide ones)."""
    from sela_amd import capi

    ch, n = x.shape
    cap = 4 + ch * (12 + 4 * 128 + 4 * 65536 + 16 * n)
    frames = np.empty(cap, np.uint8)
    offs = np.zeros(2, np.uint64)
    p = np.ascontiguousarray(x, dtype=np.int32)
    capi.check(capi.lib().sela_hip_encode_i32(p.ctypes.data, 1, ch, n, frames.ctypes.data, cap, offs.ctypes.data))
    return frames[: int(offs[1])].copy(), offs


def _encode_and_check(x, label):
    """encode_i32 on one frame x int32 [channels, n]: SELA_HIP_ERANGE exactly where the format cannot carry it, else the oracle's
    bytes, decoded by both 32-bit decoders to the oracle's channels -> whether the frame was coded, and whether losslessly."""
    from sela_amd import capi

    o = oracle()
    if wc.encoder_refuses(o, x):
        with pytest.raises(capi.SelaHipError) as err:
            _encode_i32(x)
        assert err.value.code == ERANGE, label
        return False, False
    frames, offs = _encode_i32(x)
    want = o.frame_encode_i32(x)
    assert frames.tobytes() == want, label
    dec, used = o.frame_decode_i32(want, x.shape[0])
    assert used == len(want), label
    _check_i32(frames, offs, x.shape[0], [dec], label)
    return True, all(np.array_equal(dec[c], x[c]) for c in range(x.shape[0]))


def test_the_impulse_frame(gpu):  # noqa: F811
    """2048 zeros with s[700] = 2^29 + 5 and s[1500] = -1000: the encoder writes order 1 (q = 26) with a residue of 536870917 at
    700; every decoder gives the input back (the 16-bit ones its low 16 bits)."""
    s = wc.impulse_frame_signal()
    coded, lossless = _encode_and_check(s[None], "impulse")
    assert coded and lossless
    _check_16(gpu, [oracle().frame_encode_i32(s[None])], 1, "impulse")


@pytest.mark.parametrize("n", [2048, 1000, 4096])
def test_encoder_made_wide_audio_round_trips(gpu, n):  # noqa: F811
    """Impulses at +-2^29 +- d, DC at +-2^29 / +-(2^30 - x) / +-2^30 / +-(2^31 - 1), sparse clicks to full scale, tones of 24 to
    31 bits, noise, and stereo pairs whose difference wraps: through sela_hip_encode_i32 and back."""
    coded = lossless = refused = 0
    for name, s in wc.wide_signals(n, 3):
        c, l = _encode_and_check(s[None], (n, name))
        coded += c
        lossless += l
        refused += not c
    for name, x in wc.wrapping_stereo(n, 4):
        c, _ = _encode_and_check(x, (n, name))
        assert not c
    assert coded >= 12 and refused >= 5 and lossless >= coded - 2, (coded, refused, lossless)


def test_one_65535_sample_frame_and_a_ragged_frame_of_wide_audio(gpu):  # noqa: F811
    from sela_amd import codec

    o = oracle()
    sig = dict(wc.wide_signals(65535, 6))
    for name in ("impulses 536870915", "tone 25-bit", "sparse 30-bit", "noise 25-bit", "tone 31-bit"):
        _encode_and_check(sig[name][None], (65535, name))
    ch0, ch1 = dict(wc.wide_signals(3000, 7))["tone 26-bit"], dict(wc.wide_signals(2000, 8))["impulses -536870919"]
    for s in (ch0, ch1, (ch0[:2000].astype(np.int64) - ch1).astype(np.int32)):
        assert not wc.encoder_refuses(o, s[None])
    blob = codec.encode_ragged([ch0, ch1])
    assert blob == o.frame_encode_ragged([ch0, ch1])
    dec = o.frame_decode_i32(blob, 2)[0]
    _check_i32(np.frombuffer(blob, np.uint8).copy(), _one(len(blob)), 2, [dec], "ragged")


def test_the_encode_stage_on_wide_samples(gpu):  # noqa: F811
    """sela_hip_lpc_encode / _n on 24- to 31-bit blocks: order, coefficients and residues of the oracle's analysis, with the
    residue filter picked by the block's bound (FP64 taps where exact, 64-bit wrap-around taps elsewhere) and forced onto the
    wrap-around taps."""
    from sela_amd import codec

    o = oracle()
    for n in (2048, 1000, 4096):
        blocks = np.stack([s for _, s in wc.wide_signals(n, 9)] + [(np.round(3000 * np.sin(np.arange(n) * 0.05))).astype(np.int32)])
        wants = [o.lpc_analyze(b) for b in blocks]
        calls = [codec.lpc_encode_n] + ([codec.lpc_encode] if n == 2048 else [])
        for wrap in (False, True):
            for call in calls:
                _wrap_taps(wrap)
                try:
                    order, q, res = call(blocks)
                finally:
                    _wrap_taps(False)
                for i, (wo, wq, wr) in enumerate(wants):
                    assert order[i] == wo and np.array_equal(q[i, :wo], wq) and not q[i, wo:].any(), (n, i, wrap, call.__name__)
                    assert np.array_equal(res[i], wr), (n, i, wrap, call.__name__)


def test_the_zigzag_edge(gpu):  # noqa: F811
    """A residue of exactly -2^30 is the last one the reference's int32 zig-zag takes: encoding a block whose sample 0 (its own
    residue) is -2^30 gives the oracle's bytes, +2^30 is SELA_HIP_ERANGE.  Decoding takes both (the reference's Rice decoder has
    no such edge): the oracle's samples."""
    from sela_amd import capi

    o = oracle()
    rng = np.random.default_rng(44)
    s = np.round(2000 * np.sin(np.arange(2048) * 0.05)).astype(np.int32)
    s[0] = -wc.P30
    assert not wc.encoder_refuses(o, s[None])
    frames, _ = _encode_i32(s[None])
    assert frames.tobytes() == o.frame_encode_i32(s[None])
    s[0] = wc.P30
    with pytest.raises(capi.SelaHipError) as err:
        _encode_i32(s[None])
    assert err.value.code == ERANGE
    frames = []
    for v in (-wc.P30, wc.P30):
        for order in (0, 2):
            r = rng.integers(-100, 101, 2048).astype(np.int32)
            r[[0, 700]] = v
            frames.append(_build_frame([(0, 0, 0, wc.fold_coefficients(order, rng), r)], res_k=19))
    _check_16(gpu, frames, 1, "zig-zag edge")
    stream, offs = _stream(frames)
    _check_i32(stream, offs, 1, [o.frame_decode_i32(f, 1)[0] for f in frames], "zig-zag edge")


def test_seeded_fuzz_of_residues_at_multiples_of_2_29(gpu):  # noqa: F811
    """Frames of random shape -- 1 to 3 channels, 2048 samples or any length up to 5000, random orders, coefficients that start
    folded or anywhere in the tables, some difference subframes -- whose residue streams carry a few values at k * 2^29 + d
    (|value| <= 2^30) among small noise: the oracle's samples from both 32-bit decoders and, for 2048, the 16-bit ones."""
    o = oracle()
    rng = np.random.default_rng(2929)
    std, odd = [], []
    for trial in range(60):
        ch = int(rng.integers(1, 4))
        n = 2048 if trial % 2 == 0 else int(rng.integers(101, 5001))
        subs = []
        for c in range(ch):
            order = int(rng.integers(0, 101))
            q = wc.fold_coefficients(order, rng) if rng.random() < 0.6 else rng.integers(-64, 64, order).astype(np.int32)
            r = rng.integers(-(1 << int(rng.integers(1, 16))), 1 << int(rng.integers(1, 16)), n).astype(np.int32)
            pos = rng.integers(0, n, int(rng.integers(1, 5)))
            k = rng.integers(-2, 2, len(pos))
            r[pos] = np.clip(k * wc.P29 + rng.integers(-(1 << 22), 1 << 22, len(pos)), -wc.P30, wc.P30 - 1)
            roots = [sc for sc, st, _, _, _ in subs if st == 0]  # (a parent that is itself a difference: the 16-bit decoders refuse it)
            typ = 1 if (roots and rng.random() < 0.3) else 0
            subs.append((c, typ, int(rng.choice(roots)) if typ else c, q, r))
        blob = wc.frame_bytes(o, subs)
        fl = C.c_uint32(0)
        b = np.frombuffer(blob, np.uint8).copy()
        out = np.zeros((ch, n), np.int32)
        counts = np.zeros(ch, np.uint32)
        assert o._fdec32(b, ch, out, n, counts, C.byref(fl)) == len(blob)
        if fl.value & (8 | 2 | 32 | 1 | 128):  # (what the reference leaves undefined: the hostile fuzzers test the refusals)
            continue
        (std if n == 2048 else odd).append((ch, blob, [out[c, : int(counts[c])].copy() for c in range(ch)]))
    assert len(std) >= 20 and len(odd) >= 20, (len(std), len(odd))
    for ch, blob, want in std + odd:
        _check_i32(np.frombuffer(blob, np.uint8).copy(), _one(len(blob)), ch, [want], ("fuzz", ch, len(want[0])))
    for ch in (1, 2, 3):
        frames = [blob for c, blob, _ in std if c == ch]
        if frames:
            _check_16(gpu, frames, ch, ("fuzz", ch))
