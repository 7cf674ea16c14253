"""CPU-only: the model of the paired encode calls (tests/paired_model.py) against the pinned oracle and the
unmodified reference's decoder where it is built.

The GPU tests compare the kernels with this model byte for byte, so the model itself is held here: its lossless frames decode
to their input through the reference's decoder path, a paired frame is never longer than the plain one, one and two channels
are the plain frame, the inputs hold both outcomes of the decision, and the synthetic track gives the issue's byte counts."""
import numpy as np
import pytest

import lossless_model
import paired_model as model
from oracle_lib import oracle, reference

CASES = ["A6", "N300x6", "A5", "A3", "W4", "S6"]


@pytest.fixture(scope="module")
def coded():
    """case -> per frame (input, plain paired (bytes, types), lossless paired (bytes, types)), computed once."""
    o = oracle()
    return {name: [(x, model.encode_frame(o, x, False), model.encode_frame(o, x, True)) for x in frames] for name, frames in model.cases().items()}


def _same(back, x):
    return len(back) == len(x) and all(np.array_equal(b, c) for b, c in zip(back, x))


@pytest.mark.parametrize("case", CASES)
def test_lossless_paired_frames_decode_exactly(coded, case):
    o, ref = oracle(), reference()
    for i, (x, _, (blob, _)) in enumerate(coded[case]):
        dec = ref if ref is not None else o  # the unmodified reference's decoder where it is built
        back, used = dec.frame_decode_i32(blob, len(x))
        assert used == len(blob) and _same(back, x), (case, i)
        back, used = o.frame_decode_i32(blob, len(x))
        assert used == len(blob) and _same(back, x), (case, i, "oracle")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("lossless", [False, True])
def test_a_paired_frame_is_no_longer_than_the_plain_one(coded, case, lossless):
    o = oracle()
    for i, (x, plain, exact) in enumerate(coded[case]):
        blob, types = exact if lossless else plain
        assert len(blob) <= len(model.plain_frame(o, x, lossless)), (case, i)
        assert len(types) == len(x) and all(t == 0 for t in types[0::2]), (case, i)  # an even channel is always independent


def test_one_and_two_channels_are_the_plain_frame():
    o = oracle()
    for name in ("A", "M", "N300"):
        for i, x in enumerate(lossless_model.cases()[name]):
            assert model.encode_frame(o, x, False)[0] == o.frame_encode_i32(np.ascontiguousarray(x, np.int32)), (name, i)
            assert model.encode_frame(o, x, True)[0] == lossless_model.encode_frame(o, x, True), (name, i)


@pytest.mark.parametrize("case", model.MULTI_PAIR)
@pytest.mark.parametrize("lossless", [False, True])
def test_the_inputs_hold_both_outcomes(coded, case, lossless):
    """Guards the inputs (on the model, never on the library): a stored difference and a refused one in every multi-pair case."""
    odd = [t for _, plain, exact in coded[case] for t in (exact if lossless else plain)[1][1::2]]
    assert 1 in odd and 0 in odd, (case, odd)


def test_the_synthetic_track_s_byte_counts():
    """synth_pcm(20 * 2048, 6, track=3) in 20 frames: 365,556 bytes plain, 354,104 paired; 9 frames store no difference, 2 one, 9 all three."""
    o = oracle()
    frames = model.synth_frames()
    plain = sum(len(model.plain_frame(o, x, False)) for x in frames)
    paired = [model.encode_frame(o, x, False) for x in frames]
    assert (plain, sum(len(b) for b, _ in paired)) == (365556, 354104)
    stored = [sum(t) for _, t in paired]
    assert (stored.count(0), stored.count(1), stored.count(2), stored.count(3)) == (9, 2, 0, 9)
