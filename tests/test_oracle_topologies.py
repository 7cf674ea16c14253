"""Every accepted layout of topology_cases.py through the REAL reference's frame::FrameDecoder and through the oracle: the same
int16 PCM, the same int32 channels, the same bytes consumed.  The GPU tests of these layouts (test_gpu_decode_topologies.py)
take every expected value from the oracle, so it is pinned here first.  Skipped where oracle/_ref/libsela_ref.so is absent,
as test_oracle_vs_reference.py is."""
import numpy as np
import pytest

import topology_cases as tc
import wide_cases as wc
from oracle_lib import oracle, reference

ref = reference()
needs_reference = pytest.mark.skipif(ref is None, reason="oracle/_ref/libsela_ref.so not built")


def _same_both_ways(o, blob, ch, label):
    pcm, used = o.frame_decode(blob, ch)
    pcm_r, used_r = ref.frame_decode(blob, ch)
    assert used == used_r == len(blob), label
    assert pcm.tobytes() == pcm_r.tobytes(), label
    dec, used = o.frame_decode_i32(blob, ch)
    dec_r, used_r = ref.frame_decode_i32(blob, ch)
    assert used == used_r == len(blob), label
    for c in range(ch):
        assert len(dec[c]) == len(dec_r[c]) == tc.N and dec[c].tobytes() == dec_r[c].tobytes(), (label, c)
    return pcm, dec


def test_the_modules_own_conditions_hold():
    """cases() asserts them while it builds: at +-12000 every subframe within the plan's 1072 words and a wrapped value in a
    dependent channel, the long subframes beyond the plan.  Here: every label once, every case 2048 samples, the counts."""
    cases = tc.cases()
    labels = [c[0] for c in cases]
    assert len(set(labels)) == len(labels)
    for label, ch, subs, _ in cases:
        assert len(subs) == ch and all(len(s[4]) == tc.N and 1 <= len(s[3]) <= 29 for s in subs), label
        assert all(-20 <= int(v) < 20 for s in subs for v in s[3]), label
    for ch in tc.accepted_channels():
        assert len(tc.accepted(ch)) <= 20
    for ch in tc.REFUSED_CHANNELS:
        cs, mask = tc.refused_stream(ch)[:2]
        assert len(cs) <= 20 and mask[0] and mask[-1] and not (~mask[1:] & ~mask[:-1]).any()  # (every refused frame between two accepted ones)
        assert int((~mask).sum()) == len(tc.refused(ch)) >= 7


@needs_reference
@pytest.mark.parametrize("ch", tc.accepted_channels())
def test_accepted_layouts_decode_as_the_reference_decodes_them(ch):
    o = oracle()
    cases = tc.accepted(ch)
    assert len(cases) >= 4
    for label, _, subs, _ in cases:
        pcm, dec = _same_both_ways(o, wc.frame_bytes(o, subs), ch, label)
        for c in range(ch):  # (the int16 PCM is the int32 result mod 2^16: src/file/wav_file.cpp:248-251)
            assert np.array_equal(pcm[:, c], dec[c].astype(np.uint32).astype(np.uint16).view(np.int16)), (label, c)
    # the streams the GPU tests decode are these frames, and their expectation the same PCM
    cs, stream, offs, pcm = tc.accepted_stream(ch)
    for f in range(len(cs)):
        blob = stream[int(offs[f]): int(offs[f + 1])].tobytes()
        assert np.array_equal(ref.frame_decode(blob, ch)[0], pcm[f]), cs[f][0]


@needs_reference
def test_a_parent_byte_on_an_independent_subframe_changes_nothing():
    o = oracle()
    label, ch, subs, _ = next(c for c in tc.accepted(2) if "parent bytes" in c[0] and f"+-{tc.ORDINARY}" in c[0])
    assert [s[2] for s in subs] == [7, 200]
    plain = [(c, t, c, q, r) for c, t, _, q, r in subs]
    a, _ = _same_both_ways(o, wc.frame_bytes(o, subs), ch, label)
    b, _ = _same_both_ways(o, wc.frame_bytes(o, plain), ch, label)
    assert np.array_equal(a, b)


@needs_reference
def test_a_chain_in_stream_order_is_defined_by_the_reference():
    """[(0, independent), (1 under 0), (2 under 1)]: the reference resolves its type-1 subframes in stream order, so channel 1 is
    final when channel 2 subtracts from it, and the oracle does the same.  The 32-bit decoders decode it; the int16 kernels of
    2048-sample frames refuse it by policy (test_gpu_decode_topologies.py keeps that refusal).  Against stream order the
    reference subtracts from a vector that is still empty: not run here."""
    o = oracle()
    for scale in (tc.ORDINARY, tc.WRAPPING):
        subs = tc.subframes(tc.CHAIN_IN_STREAM_ORDER, scale, 20261017 + scale)
        _, dec = _same_both_ways(o, wc.frame_bytes(o, subs), 3, ("chain", scale))
        raw = [o.lpc_synth(len(s[3]), s[3], s[4]) for s in subs]
        with np.errstate(over="ignore"):
            assert np.array_equal(dec[0], raw[0]) and np.array_equal(dec[1], raw[0] - raw[1]) and np.array_equal(dec[2], raw[0] - raw[1] - raw[2])
    # ... and with five channels, as topology_cases writes it among the refused frames
    label, ch, subs, _ = next(c for c in tc.refused(5) if "a chain in stream order" in c[0])
    _same_both_ways(o, wc.frame_bytes(o, subs), ch, label)
