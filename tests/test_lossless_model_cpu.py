"""CPU-only: the model of the lossless encode mode (tests/lossless_model.py) against the pinned oracle, the
unmodified reference's decoder where it is built, and the fixture tests/golden/lossless.json.

The GPU tests compare the kernels with this model byte for byte, so the model itself is pinned here: with lossless=False it IS
the reference's frame encoder (same bytes as the oracle's on every case), and with lossless=True its frames decode back to the
input exactly -- through the oracle's decoder and through the reference's own."""
import hashlib
import json
import os

import numpy as np
import pytest

import lossless_model as model
from oracle_lib import oracle, reference

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["A", "M", "T", "W", "N1000", "N300", "R"]


@pytest.fixture(scope="module")
def analysed():
    """case -> per frame (input, plain analysis, lossless analysis), computed once."""
    o = oracle()
    return {name: [(x, model.analyse_frame(o, x, False), model.analyse_frame(o, x, True)) for x in frames] for name, frames in model.cases().items()}


def _same(back, x):
    return len(back) == len(x) and all(np.array_equal(b, c) for b, c in zip(back, x))


@pytest.mark.parametrize("case", CASES)
def test_plain_model_is_the_reference_encoder(analysed, case):
    o = oracle()
    for i, (x, plain, _) in enumerate(analysed[case]):
        want = o.frame_encode_ragged(x) if isinstance(x, list) else o.frame_encode_i32(x)
        assert plain[0] == want, (case, i)


@pytest.mark.parametrize("case", CASES)
def test_lossless_frames_decode_exactly(analysed, case):
    o, ref = oracle(), reference()
    for i, (x, _, lossless) in enumerate(analysed[case]):
        back, used = o.frame_decode_i32(lossless[0], len(x))
        assert used == len(lossless[0]) and _same(back, x), (case, i)
        if ref is not None:  # the unmodified reference's decoder
            back, used = ref.frame_decode_i32(lossless[0], len(x))
            assert used == len(lossless[0]) and _same(back, x), (case, i, "reference")


@pytest.mark.parametrize("case", CASES)
def test_only_frames_with_a_tie_change_and_the_plain_ones_with_a_stored_tie_are_lossy(analysed, case):
    """The control: the inputs bite.  A frame without a tie in any candidate keeps its bytes; a plain frame with a tie in a
    stored candidate does not decode to its input; and the case holds both kinds."""
    o = oracle()
    kinds = set()
    for i, (x, plain, lossless) in enumerate(analysed[case]):
        _, ties, stored, _ = plain
        assert ties == lossless[1], (case, i)  # (the ties are a property of the input and the predictor)
        stored_tie = any(ties[c] for c in stored)
        if not any(ties):
            assert plain[0] == lossless[0], (case, i)
        if not stored_tie and stored == lossless[2]:
            assert plain[0] == lossless[0], (case, i)  # a tie in a discarded candidate only: nothing that is stored changes
        back, _ = o.frame_decode_i32(plain[0], len(x))
        assert _same(back, x) == (not stored_tie), (case, i)
        if stored_tie:
            assert plain[0] != lossless[0], (case, i)
        kinds.add("stored" if stored_tie else ("discarded" if any(ties) else "clean"))
    assert "stored" in kinds, case
    if case != "R":
        assert "clean" in kinds, case
    if case in ("A", "N1000", "N300"):
        assert "discarded" in kinds, case


def test_fixture_agrees_with_the_model(analysed):
    with open(os.path.join(HERE, "golden", "lossless.json")) as fh:
        gold = json.load(fh)
    assert gold["seed"] == model.SEED and gold["corpus_frames"] == model.CORPUS_FRAMES and sorted(gold["cases"]) == sorted(CASES)
    for case in CASES:
        rows = gold["cases"][case]
        assert len(rows) == len(analysed[case]), case
        for i, (row, (_, _, lossless)) in enumerate(zip(rows, analysed[case])):
            blob, ties, stored, _ = lossless
            assert (row["ties"], row["stored"], row["bytes"], row["sha256"]) == (ties, stored, len(blob), hashlib.sha256(blob).hexdigest()), (case, i)


def test_the_issue_s_tie_table():
    """corpus.build(3000, 20260927): the ties of case A's frames as (ch0, ch1, difference), and the four frames whose stored
    candidate holds one are those of verify_corpus.json among them."""
    o = oracle()
    ties = {f: model.analyse_frame(o, x, False)[1] for f, x in zip(model.A_FRAMES, model.cases()["A"])}
    assert ties == {400: [0, 0, 0], 401: [0, 1, 0], 402: [0, 0, 0], 580: [0, 0, 2], 1128: [1, 0, 0], 1158: [3, 0, 0], 1182: [1, 0, 0],
                    2395: [0, 0, 1], 2798: [0, 2, 0], 2799: [0, 0, 0]}
    with open(os.path.join(HERE, "golden", "verify_corpus.json")) as fh:
        gold = json.load(fh)
    lossy = {row["frame"] for row in gold["lossy"]}
    assert {f for f in model.A_FRAMES if f in lossy} == {401, 1128, 1158, 1182}
