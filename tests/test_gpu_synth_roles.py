"""GPU parity tests of the ring-of-128 synthesis (orders above 60; sela_decode_core.inc, synthesize<2, 16>), whose two
registers change roles behind every block of 64 samples while the loop runs ONE copy of the block's text: the smallest
shapes at which a role swap can go wrong -- odd and even counts of blocks, a last block partly masked, the hand-over from
the folded form to the exact one (a residue of 2^23 or more; samples that leave the folded range under small residues) in
an odd and in an even block, where the restore must put both registers back in the roles they have THERE.  Every expected
value is the oracle's, bit for bit; the threshold is the folded form's |r| < 2^23 / |s| < 2^23 of synth_mac."""
import numpy as np
import pytest

import wide_cases as wc
from gpu_common import _both_decoders, _build_frame, _decode, gpu  # noqa: F401  (fixture and helpers)
from oracle_lib import oracle
from synth_cases import _leaves_in_block, _q, _quiet  # (the builders: shared with tests/test_gpu_synth_matrix.py)

pytestmark = pytest.mark.gpu

P23 = 1 << 23
RING128 = [61, 62, 100]  # (112 is beyond the format: SELA_MAX_LPC_ORDER is 100)
LENGTHS = [64, 65, 128, 129, 191, 192, 2049]


def _stream(frames):
    return np.frombuffer(b"".join(frames), np.uint8).copy(), np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)


def _check_stage(orders, qs, res, with_2048):
    from sela_amd import codec

    o = oracle()
    orders = np.array(orders, np.int32)
    q = np.zeros((len(orders), 100), np.int32)
    for b, row in enumerate(qs):
        q[b, : len(row)] = row
    res = np.stack(res)
    for label, call in [("lpc_decode_n", codec.lpc_decode_n)] + ([("lpc_decode", codec.lpc_decode)] if with_2048 else []):
        got = call(orders, q, res)
        for b in range(len(orders)):
            want = o.lpc_synth(int(orders[b]), qs[b], res[b])
            assert np.array_equal(got[b], want), (label, res.shape[1], int(orders[b]), b, int(np.flatnonzero(got[b] != want)[0]))


def _check_frames(gpu, frames, ch, label, sixteen=True):  # noqa: F811
    """k_decode_frames (Decoder.decode) in both recurrence forms, and the 32-bit decoders (k_decode_subframes32 offered; the
    any-length kernel alone) on the same stream, against the oracle."""
    from sela_amd import capi

    o = oracle()
    stream, offs = _stream(frames)
    if sixteen:
        want = np.stack([o.frame_decode(f, ch)[0] for f in frames])
        for form in (0, 1):  # (launches of this size would see the lonely-wave form alone)
            capi.lib().sela_hip_debug_decode_recurrence(form)
            try:
                dev = _decode(gpu, stream, offs, ch)
            finally:
                capi.lib().sela_hip_debug_decode_recurrence(-1)
            for f in range(len(frames)):
                assert np.array_equal(dev[f], want[f]), (label, f, "k_decode_frames", form)
    want32 = [o.frame_decode_i32(f, ch)[0] for f in frames]
    offered, alone, took = _both_decoders(stream, offs, ch)
    assert took > 0, label  # (the standard kernel decoded them)
    for f in range(len(frames)):
        for c in range(ch):
            assert np.array_equal(offered[f][c], want32[f][c]), (label, f, c, "k_decode_subframes32")
            assert np.array_equal(alone[f][c], want32[f][c]), (label, f, c, "any-length kernel alone")


@pytest.mark.parametrize("n_frames", [1, 2, 3])
def test_stereo_frames_of_long_predictors(gpu, n_frames):  # noqa: F811
    """2048-sample stereo frames, one to three per launch, hand-built predictors of order 61, 62 and 100 on either channel: the
    whole subframe in the folded form (its samples stay below 2^23: asserted), 32 blocks, sixteen swaps of each direction."""
    o = oracle()
    rng = np.random.default_rng(6100 + n_frames)
    frames = []
    for f in range(n_frames):
        subs = []
        for c in range(2):
            order = RING128[(2 * f + c) % len(RING128)]
            subs.append((c, 0, c, _q(order, rng), _quiet(2048, rng)))
        frames.append(_build_frame(subs))
        for ch_samples in o.frame_decode_i32(frames[-1], 2)[0]:
            assert np.abs(ch_samples.astype(np.int64)).max() < P23
    _check_frames(gpu, frames, 2, ("stereo", n_frames))


@pytest.mark.parametrize("n", LENGTHS)
def test_run_time_lengths(gpu, n):  # noqa: F811
    """Odd and even counts of 64-sample blocks and a last block partly masked, orders 61 and 100: the stage on its own
    (sela_hip_lpc_decode_n) and mono and stereo frames of that length through k_decode_subframes32."""
    rng = np.random.default_rng(6200 + n)
    orders, qs, res = [], [], []
    for order in (61, 100):
        if order >= n:  # (a block not longer than its order: refused, tested elsewhere)
            continue
        for _ in range(2):
            orders.append(order)
            qs.append(_q(order, rng))
            res.append(_quiet(n, rng))
    _check_stage(orders, qs, res, False)
    frames = [_build_frame([(0, 0, 0, qs[b], res[b])]) for b in range(len(orders))]
    _check_frames(gpu, frames, 1, ("mono", n), sixteen=False)
    stereo = [_build_frame([(0, 0, 0, qs[0], res[0]), (1, 0, 1, qs[-1], res[-1])])]
    _check_frames(gpu, stereo, 2, ("stereo", n), sixteen=False)


@pytest.mark.parametrize("block", [0, 1, 2])
def test_hand_over_to_the_exact_form_in_mid_subframe(gpu, block):  # noqa: F811
    """One residue of 2^23 or more in block 0, block 1 (odd) and block 2 (even) -- the block starts in the exact form -- and
    samples that leave the folded range inside that block under residues below 2^23 -- the block is run folded, found out and
    run again from its restored sums: orders 61, 62 and 100, the stage and every frame decoder."""
    rng = np.random.default_rng(6300 + block)
    orders, qs, res = [], [], []
    for order in RING128:
        for v in (P23, -P23, (1 << 24) + 3, wc.P29 + 5):
            q, r = _q(order, rng), _quiet(2048, rng)
            r[64 * block + int(rng.integers(0, 64))] = v
            orders.append(order), qs.append(q), res.append(r)
        if block > 0:  # (samples cannot leave the range in block 0 before a residue does: the sums start empty)
            q = _q(order, rng)
            orders.append(order), qs.append(q), res.append(_leaves_in_block(order, q, block, 2048, rng))
    _check_stage(orders, qs, res, True)
    frames = [_build_frame([(0, 0, 0, qs[b], res[b]), (1, 0, 1, qs[-1 - b], res[-1 - b])]) for b in range(len(orders))]
    _check_frames(gpu, frames, 2, ("hand-over", block))


@pytest.mark.parametrize("block", [1, 2, 3])
def test_samples_leave_the_folded_range_at_run_time_lengths(gpu, block):  # noqa: F811
    """The restore in an odd and an even block of subframes that end on an odd block (n = 64 * 4 + 1) and an even one."""
    rng = np.random.default_rng(6400 + block)
    for n in (257, 320):
        orders, qs, res = [], [], []
        for order in (61, 100):
            q = _q(order, rng)
            orders.append(order), qs.append(q), res.append(_leaves_in_block(order, q, block, n, rng))
        _check_stage(orders, qs, res, False)
        _check_frames(gpu, [_build_frame([(0, 0, 0, qs[0], res[0]), (1, 0, 1, qs[1], res[1])])], 2, ("leaves", block, n), sixteen=False)


@pytest.mark.parametrize("order", [48, 60])
def test_ring_of_64_control(gpu, order):  # noqa: F811
    """The ring-of-64 forms once each (groups of 16 and of 4): one register, no roles -- quiet, a wide residue, samples that
    leave the range."""
    rng = np.random.default_rng(6500 + order)
    q = _q(order, rng)
    wide = _quiet(2048, rng)
    wide[64 + 17] = -P23
    res = [_quiet(2048, rng), wide, _leaves_in_block(order, q, 1, 2048, rng)]
    _check_stage([order] * 3, [q] * 3, res, True)
    _check_frames(gpu, [_build_frame([(0, 0, 0, q, res[0]), (1, 0, 1, q, res[1])]), _build_frame([(0, 0, 0, q, res[2]), (1, 0, 1, q, res[0])])], 2, ("ring of 64", order))
