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


def _same_both_ways(o, blob, ch, label, n=tc.N):
    pcm, used = o.frame_decode(blob, ch, n=n)
    pcm_r, used_r = ref.frame_decode(blob, ch, n=n)
    assert used == used_r == len(blob), label
    assert pcm.shape == (n, ch) and pcm.tobytes() == pcm_r.tobytes(), label
    dec, used = o.frame_decode_i32(blob, ch)
    dec_r, used_r = ref.frame_decode_i32(blob, ch)
    assert used == used_r == len(blob), label
    for c in range(ch):
        assert len(dec[c]) == len(dec_r[c]) == n and dec[c].tobytes() == dec_r[c].tobytes(), (label, c)
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
    # the long last frames: every label once, every subframe of the frame's own length, no layout an encoder writes; at +-12000
    # _tailed() asserts a wrapped value in a dependent channel while it builds
    labels = set()
    for ch, n_last, scale, chain in _TAILS:
        label, subs = tc.tail_subframes(ch, n_last, scale, chain)
        labels.add(label)
        layout = [s[:3] for s in subs]
        assert len(subs) == ch and all(len(s[4]) == n_last and 1 <= len(s[3]) <= 29 for s in subs), label
        assert sorted(s[0] for s in subs) == list(range(ch)) and tc.dependent_channels(subs), label
        assert layout != [(0, tc.IND, 0), (1, tc.DEP, 0)] + [(c, tc.IND, c) for c in range(2, ch)], label
        if chain:  # channel 2 under channel 1, itself a difference in front of it
            assert layout[:3] == tc.CHAIN_IN_STREAM_ORDER and all(s[1] == tc.IND for s in subs[3:]), label
        stream, offs, pcm = tc.tailed_stream(ch, n_last, scale, chain)
        assert len(offs) == 4 and int(offs[3]) == len(stream) and pcm.shape == (2 * tc.N + n_last, ch) and pcm.dtype == np.int16
        pcm32 = tc.tailed_stream_i32(ch, n_last, scale, chain)
        assert np.array_equal(pcm, pcm32.astype(np.uint32).astype(np.uint16).view(np.int16)), label
        if scale == tc.WRAPPING:
            assert (pcm32[2 * tc.N:] != pcm[2 * tc.N:]).any(), label
    assert len(labels) == len(_TAILS)


# (channels, samples of the last frame, residue scale, a chain as the last frame): what test_gpu_tail_topologies.py decodes
_TAILS = [(ch, n_last, scale, False) for ch in tc.TAIL_CHANNELS for n_last in tc.TAIL_LENGTHS for scale in (tc.ORDINARY, tc.WRAPPING)]
_TAILS += [(ch, 2825, scale, True) for ch in tc.TAIL_CHANNELS if ch >= 3 for scale in (tc.ORDINARY, tc.WRAPPING)]


@needs_reference
@pytest.mark.parametrize("ch", tc.TAIL_CHANNELS)
def test_long_last_frames_decode_as_the_reference_decodes_them(ch):
    """Every last frame of tailed_stream, the chains among them, through frame::FrameDecoder and the oracle: the same PCM at the
    frame's own length, the same int32 channels, the same bytes consumed; and the stream's PCM is those frames'."""
    o = oracle()
    mine = [t for t in _TAILS if t[0] == ch]
    assert len(mine) == (6 if ch == 2 else 8)
    for _, n_last, scale, chain in mine:
        label, subs = tc.tail_subframes(ch, n_last, scale, chain)
        blob = wc.frame_bytes(o, subs)
        pcm, dec = _same_both_ways(o, blob, ch, label, n=n_last)
        stream, offs, want = tc.tailed_stream(ch, n_last, scale, chain)
        assert stream[int(offs[2]):].tobytes() == blob, label
        assert np.array_equal(want[2 * tc.N:], pcm) and np.array_equal(tc.tailed_stream_i32(ch, n_last, scale, chain)[2 * tc.N:], np.stack(dec, axis=1)), label
        for f in range(2):
            front = stream[int(offs[f]): int(offs[f + 1])].tobytes()
            assert np.array_equal(ref.frame_decode(front, ch)[0], want[f * tc.N: (f + 1) * tc.N]), (label, f)
        if chain:  # resolved in stream order: channel 1 is final when channel 2 subtracts from it
            raw = [o.lpc_synth(len(s[3]), s[3], s[4]) for s in subs[:3]]
            with np.errstate(over="ignore"):
                assert np.array_equal(dec[1], raw[0] - raw[1]) and np.array_equal(dec[2], raw[0] - raw[1] - raw[2]), label


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
