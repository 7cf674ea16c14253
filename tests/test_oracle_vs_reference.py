"""Pin the CPU restatement to the REAL reference where it is available.

oracle/_ref/libsela_ref.so is the unmodified reference compiled by `make -C oracle ref`
(only possible where /root/reference exists; the prebuilt library travels to the GPU box).
Skipped when the library is absent -- tests/test_oracle_golden.py covers that case.
"""
import struct

import numpy as np
import pytest

from oracle_lib import oracle, reference
from sela_amd.synth import synth_frames

ref = reference()
pytestmark = pytest.mark.skipif(ref is None, reason="oracle/_ref/libsela_ref.so not built")


def _blocks(seed, count):
    rng = np.random.default_rng(seed)
    i = np.arange(2048)
    for c in range(count):
        kind = c % 6
        if kind == 0:  # coloured noise, random level
            x = np.cumsum(rng.integers(-300, 301, 2048)) // (1 + c % 7)
        elif kind == 1:  # white noise at a random level (k hovering near the 0.05 threshold)
            x = rng.integers(-(1 << (3 + c % 13)), 1 << (3 + c % 13), 2048)
        elif kind == 2:  # sinusoid mix computed in integers
            x = (20000 * np.sin(i * (0.01 + 0.002 * c)) + rng.integers(-50, 51, 2048)).astype(np.int64)
        elif kind == 3:  # 17-bit difference-like signal
            x = rng.integers(-65535, 65536, 2048)
        elif kind == 4:  # sparse
            x = np.where(rng.random(2048) < 0.01, rng.integers(-32768, 32768, 2048), 0)
        else:  # constant + tiny dither
            x = 1000 * (c % 30) + rng.integers(0, 2, 2048)
        yield np.clip(x, -65535, 65535).astype(np.int32)


def test_lpc_and_rice_stages_match():
    o = oracle()
    for s in _blocks(11, 120):
        order, q, r = o.lpc_analyze(s)
        order_r, q_r, r_r = ref.lpc_analyze(s)
        assert order == order_r and np.array_equal(q, q_r) and np.array_equal(r, r_r)
        assert np.array_equal(o.lpc_coeffs(order, q), ref.lpc_coeffs(order, q))
        assert np.array_equal(o.lpc_synth(order, q, r), ref.lpc_synth(order, q, r))
        for v in (q, r):
            k, w = o.rice_encode(v)
            k_r, w_r = ref.rice_encode(v)
            assert k == k_r and np.array_equal(w, w_r)
            assert np.array_equal(o.rice_decode(w, len(v), k), ref.rice_decode(w, len(v), k))


def test_synth_decoder_inputs_not_from_encoder():
    """Decoder-side functions on coefficient sets the encoder would not emit."""
    o = oracle()
    rng = np.random.default_rng(5)
    for _ in range(60):
        order = int(rng.integers(1, 101))
        q = rng.integers(-64, 64, order).astype(np.int32)
        q[2:] = rng.integers(-12, 12, max(order - 2, 0))
        r = rng.integers(-2000, 2000, 2048).astype(np.int32)
        assert np.array_equal(o.lpc_coeffs(order, q), ref.lpc_coeffs(order, q))
        assert np.array_equal(o.lpc_synth(order, q, r), ref.lpc_synth(order, q, r))


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_frames_match(channels):
    o = oracle()
    pcm = synth_frames(24, channels, 9 + channels)
    blob, offs, _ = o.encode_frames(pcm, threads=4)
    blob_r, offs_r, _ = ref.encode_frames(pcm, threads=4)
    assert np.array_equal(blob, blob_r) and np.array_equal(offs, offs_r)
    dec, _ = o.decode_frames(blob, offs, channels, threads=4)
    dec_r, _ = ref.decode_frames(blob_r, offs_r, channels, threads=4)
    assert np.array_equal(dec, dec_r) and np.array_equal(dec, pcm)


# ---- 25- to 31-bit samples and residues near 2^29 / 2^30 ---------------------------------------------------------------------
# The reference's integer arithmetic overflows on this range: int64 sums in lpc::ResidueGenerator / lpc::SampleGenerator, the
# int32 residue and sample, the int32 stereo difference, the int32 zig-zag.  All of that is undefined in C++; the judge here is
# what the committed recipe (oracle/Makefile: g++ -O2 on x86-64) builds, i.e. two's-complement wrap-around -- which is what the
# oracle states it does (oracle/sela_oracle.c, its header and the residue / stereo loops).  The GPU tests of the same range
# (tests/test_gpu_wide_samples.py) take every expected value from the oracle, so it is pinned here first.
import wide_cases as wc  # noqa: E402


def _same_frame_both_ways(o, planar):
    blob = o.frame_encode_i32(planar)
    assert blob == ref.frame_encode_i32(planar)
    ch = planar.shape[0]
    dec, used = o.frame_decode_i32(blob, ch)
    dec_r, used_r = ref.frame_decode_i32(blob, ch)
    assert used == used_r == len(blob)
    for c in range(ch):
        assert np.array_equal(dec[c], dec_r[c]), c
    return blob


@pytest.mark.parametrize("n", [2048, 1000])
def test_wide_signals_match(n):
    """Impulses at +-2^29 +- d, DC at +-2^29, +-(2^30 - x), -2^30, 2^30 and +-(2^31 - 1), sparse clicks up to full scale,
    tones of 24 to 31 bits, noise: the analysis, the predictor, the synthesis -- and, where the format can carry the block,
    the frame and its decode."""
    o = oracle()
    coded = refused = 0
    for name, s in wc.wide_signals(n, 3):
        order, q, r = o.lpc_analyze(s)
        order_r, q_r, r_r = ref.lpc_analyze(s)
        assert order == order_r and np.array_equal(q, q_r) and np.array_equal(r, r_r), name
        assert np.array_equal(o.lpc_coeffs(order, q), ref.lpc_coeffs(order, q)), name
        back = o.lpc_synth(order, q, r)
        assert np.array_equal(back, ref.lpc_synth(order, q, r)), name  # (not always s: the prediction keeps 29 bits, the encoder rounds half up and the decoder half down)
        if wc.encoder_refuses(o, s[None]):  # (the reference's Rice coder would run for ~2^64 bits)
            refused += 1
            continue
        _same_frame_both_ways(o, s[None])
        coded += 1
    assert coded >= 15 and refused >= 5, (coded, refused)


def test_the_impulse_frame_is_order_1_with_a_residue_of_2_29_plus_5():
    o = oracle()
    s = wc.impulse_frame_signal()
    for lib in (o, ref):
        order, q, r = lib.lpc_analyze(s)
        assert order == 1 and list(q) == [26] and r[700] == wc.P29 + 5
    _same_frame_both_ways(o, s[None])


def test_stereo_differences_that_wrap_match():
    """The int32 stereo difference beyond its range: on the encoder's side (frame_encoder.cpp:22-24) the analysis of the wrapped
    difference matches, and no such frame can be coded (wide_cases.wrapping_stereo says why); on the decoder's side
    (frame_decoder.cpp:65) crafted frames whose parent - difference wraps decode alike."""
    o = oracle()
    for name, x in wc.wrapping_stereo(2048, 4):
        d = x[0].astype(np.int64) - x[1]
        assert ((d > np.iinfo(np.int32).max) | (d < np.iinfo(np.int32).min)).any(), name
        for s in (x[0], x[1], d.astype(np.int32)):
            order, q, r = o.lpc_analyze(s)
            order_r, q_r, r_r = ref.lpc_analyze(s)
            assert order == order_r and np.array_equal(q, q_r) and np.array_equal(r, r_r), name
        assert wc.encoder_refuses(o, x), name
    for n, seed in ((2048, 1), (1000, 2), (4096, 3)):
        subs, wraps = wc.stereo_wrap_subframes(o, n, seed)
        assert wraps > 0
        blob = wc.frame_bytes(o, subs)
        dec, used = o.frame_decode_i32(blob, 2)
        dec_r, used_r = ref.frame_decode_i32(blob, 2)
        assert used == used_r == len(blob)
        assert all(np.array_equal(dec[c], dec_r[c]) for c in range(2)), n


def test_wide_residues_through_the_synthesis_and_the_rice_coder():
    """Residue vectors no encoder wrote -- k * 2^29 + d, +-(2^30 - 1), -2^30, +-2^28 +- 1, +-(2^23 - 1), +-2^23, at lane 0, lane
    63 and in the second block of a ring of 128 -- for orders 0, 1, 2, 47 .. 49, 60, 61, 64, 65 and 100, through the synthesis;
    and those the zig-zag takes through the Rice coder, both ways."""
    o = oracle()
    rng = np.random.default_rng(17)
    for order in wc.ORDERS:
        q = wc.fold_coefficients(order, rng)
        a = o.lpc_coeffs(order, q)
        assert np.array_equal(a, ref.lpc_coeffs(order, q)) and wc.fits_fold(a), order
        for name, r in wc.stage_cases(2048, rng):
            assert np.array_equal(o.lpc_synth(order, q, r), ref.lpc_synth(order, q, r)), (order, name)
    for v in wc.FRAME_RESIDUES:
        r = rng.integers(-300, 301, 500).astype(np.int32)
        r[::97] = v
        k, w = o.rice_encode(r)
        k_r, w_r = ref.rice_encode(r)
        assert k == k_r and np.array_equal(w, w_r), v
        assert np.array_equal(o.rice_decode(w, len(r), k), r) and np.array_equal(ref.rice_decode(w, len(r), k), r), v
