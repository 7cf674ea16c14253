"""(no kernel: the oracle alone)  The cases of tests/synth_cases.py are what they are called: what the GPU matrix
(test_gpu_synth_matrix.py) believes about a case -- its flags, where it leaves the folded range, the form it starts in, whether
its frame is parsed just in time or parked in the workspace -- is shown here from the oracle and the frames' own headers."""
import numpy as np

import synth_cases as sc
import wide_cases as wc
from oracle_lib import oracle


def _every_frame():
    return sc.stereo_frames() + sc.length_frames() + tuple(f for ch in sc.WIDE_CHANNELS for f in sc.wide_frames(ch))


def test_the_oracles_flags():
    """0 everywhere, but exactly COEF_OVERFLOW where an extreme seam kind takes the predictor beyond int64."""
    flagged = 0
    for f in _every_frame():
        extreme = f.cases[0] is not None and f.cases[0].kind == "seam" and "random" not in f.label
        assert f.flags == 0 or (extreme and f.flags == sc.COEF_OVERFLOW), (f.label, f.flags)
        flagged += f.flags != 0
    assert flagged > 0
    assert all(f.flags == 0 for f in sc.hard_frames())
    assert {f.cases[0].order for f in sc.seam_frames() if "random" in f.label} == set(sc.ORDERS + sc.BOUNDARY_ORDERS)
    assert [f[0] for f in sc.decoder_frames()] == [f"order {o}, {k}" for o in sc.ORDERS for k in sc.KINDS]


def test_the_first_value_beyond_the_folded_range_lies_in_the_named_block():
    named = 0
    cases = list(sc.class_cases()) + list(sc.workspace_cases()) + [c for n in sc.LENGTHS for c in sc.length_cases(n)]
    for c in cases:
        at = sc.first_beyond(c.order, c.q, c.residues)
        if c.kind == "folded":
            assert at is None and c.block is None, c.label
        elif c.kind in ("residue", "leaves"):
            assert at is not None and at == c.at and at // 64 == c.block, (c.label, at)
            wide_residues = np.flatnonzero(np.abs(c.residues.astype(np.int64)) >= sc.P23)
            assert (len(wide_residues) == 1 and wide_residues[0] == at) if c.kind == "residue" else len(wide_residues) == 0, c.label
            named += 1
    assert named > 60
    # every class x (a) .. (d); (b) with each of the four values and in each of the four blocks, (c) in an odd and an even block
    for order in sc.CLASS_ORDERS:
        mine = [c for c in sc.class_cases() if c.order == order]
        assert [c.kind for c in mine] == ["folded"] + ["residue"] * 4 + ["leaves"] * 2 + ["exact"], order
        assert sorted(c.block for c in mine if c.kind == "residue") == sorted(sc.HAND_OVER_BLOCKS)
        assert sorted(int(c.residues[c.at]) for c in mine if c.kind == "residue") == sorted(sc.HAND_OVER_VALUES)
        assert [c.block for c in mine if c.kind == "leaves"] == [1, 2]
    # the run-time lengths: a departure in an odd and in an even block wherever the length has room for both
    for n in sc.LENGTHS:
        for order in sc.LENGTH_ORDERS:
            blocks = [c.block for c in sc.length_cases(n) if c.order == order and c.kind == "leaves"]
            assert blocks == (list(sc.leave_blocks(n)) if order < n else []), (n, order, blocks)
            assert all(len(c.residues) == n for c in sc.length_cases(n))
        assert n < 129 or [b % 2 for b in sc.leave_blocks(n)] == [1, 0], n


def test_the_form_a_case_starts_in():
    o = oracle()
    cases = list(sc.class_cases()) + list(sc.workspace_cases()) + [c for n in sc.LENGTHS for c in sc.length_cases(n)]
    for c in cases:
        assert wc.fits_fold(o.lpc_coeffs(c.order, c.q)) == (c.kind != "exact"), c.label
    assert sum(c.kind == "exact" for c in cases) == len(sc.CLASS_ORDERS)


def test_just_in_time_and_workspace_frames():
    """A just-in-time frame has no subframe beyond 1072 words; of a workspace frame every hard subframe is beyond them.  In the
    launch order every workspace frame has a just-in-time frame on either side."""
    for f in sc.stereo_frames() + tuple(f for ch in sc.WIDE_CHANNELS for f in sc.wide_frames(ch)):
        words = sc._subframe_words(f.blob, f.channels)
        if f.mode == "jit":
            assert max(words) <= sc.PLAN_WORDS, (f.label, words)
        else:
            assert all(w > sc.PLAN_WORDS for w, c in zip(words, f.cases) if c is not None), (f.label, words)
    modes = [f.mode for f in sc.stereo_frames()]
    parked = [i for i, m in enumerate(modes) if m == "workspace"]
    assert len(parked) == 5 + len(sc.workspace_cases()) and len(sc.workspace_cases()) == 3 * 6
    assert all(0 < i < len(modes) - 1 and modes[i - 1] == modes[i + 1] == "jit" for i in parked)
    for ch in sc.WIDE_CHANNELS:
        assert [f.mode for f in sc.wide_frames(ch)] == ["jit"] * 3 + ["workspace"]
        assert sum(c is None for c in sc.wide_frames(ch)[0].cases) == 2
    # the workspace cases are class cases under another Rice parameter: the same residues, the same samples
    by_label = {c.label: c for c in sc.class_cases()}
    for c in sc.workspace_cases():
        twin = by_label[c.label.rsplit(", k = ", 1)[0]]
        assert c.res_k == sc.WORKSPACE_K and twin.res_k is None and np.array_equal(c.residues, twin.residues) and np.array_equal(c.q, twin.q)


def test_the_int16_pcm_is_the_low_half_of_the_32_bit_samples():
    o = oracle()
    for f in _every_frame():
        assert f.pcm.shape == (f.n, f.channels) and all(len(w) == f.n for w in f.wide), f.label
        assert all(np.array_equal(f.wide[c].astype(np.int16), f.pcm[:, c]) for c in range(f.channels)), f.label
        for c, case in enumerate(f.cases):  # a channel that is no difference and has none under it is its subframe's synthesis
            if case is not None and f.channels <= 2:
                assert np.array_equal(f.wide[c], o.lpc_synth(case.order, case.q, case.residues)), (f.label, c)
    for ch in (1, 2):
        for s in sc.tail_streams(ch):
            n = len(s.case.residues)
            assert s.pcm.shape == ((2 * sc.N if n > sc.N else 0) + n, ch), s.label
            assert np.array_equal(s.pcm[-n:, 0], o.lpc_synth(s.case.order, s.case.q, s.case.residues).astype(np.int16)), s.label
        assert sorted({len(s.case.residues) for s in sc.tail_streams(ch)}) == [191] + sc.TAIL_LENGTHS
