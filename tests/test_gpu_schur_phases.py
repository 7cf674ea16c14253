"""The Schur recursion of k_encode_teams in phases: teams of 16 drop from 7 columns per lane to 6, 5, .. 1 at stages
5, 21, 37, 53, 69 and 85 and repack gen0 / gen1 inside the team in between; teams of 8 keep one phase (phased, they would change at
stages 5, 13, 21, .. 93: the boundary blocks below cover those stages too).  Every case runs on both (the `teams` fixture) and compares, against the CPU oracle, the bit patterns of all 100 reflection coefficients and the order from
the trace instantiation, and the frame bytes and offsets of the product instantiation.  (src/lpc/residue_generator.cpp:47-78.)"""
import functools

import numpy as np
import pytest
from oracle_lib import oracle

from gpu_common import _bits, _encode, _hard_blocks, gpu, teams  # noqa: F401  (fixtures and helpers)

PHASE_STAGES = tuple(range(5, 100, 8))  # the first stage of a phase: teams of 16 every other one (5, 21, .. 85), teams of 8 all twelve if they were phased
# white noise whose LAST reflection coefficients pass the order threshold (found with oracle().lpc_analyze, asserted below):
# seed -> the oracle's order
LATE_FULL_SCALE = {25: 99, 36: 98, 57: 98, 95: 97}
LATE_PLUS_MINUS_3 = {1003: 97, 1008: 97, 1014: 97, 1016: 97}
# x[n] = e[n] + 0.35 x[n - lag]: partial correlations end at `lag`.  (lag, seed) whose order IS the lag, within one of each stage
BOUNDARY = [(4, 8), (5, 1), (6, 8), (12, 1), (13, 8), (14, 0), (20, 0), (21, 1), (22, 1), (28, 0), (29, 0), (30, 1), (36, 0), (37, 0), (38, 0),
            (44, 0), (45, 0), (46, 0), (52, 1), (53, 0), (54, 0), (60, 0), (61, 1), (62, 0), (68, 0), (69, 0), (70, 0), (76, 0), (77, 0), (78, 0),
            (84, 0), (85, 0), (86, 0), (92, 0), (93, 0), (94, 0)]


def _noise(seed, amp):
    return np.random.default_rng(seed).integers(-amp, amp + 1, 2048).astype(np.int16)


def _echo(seed, lag, c=0.35, amp=6000):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, amp, 2048 + 512)
    for n in range(lag, len(x)):
        x[n] += c * x[n - lag]
    return np.clip(np.rint(x[512:]), -32768, 32767).astype(np.int16)


def _signals(pcm):
    """the blocks the encoder analyses, in its order: per frame the channels, and left - right behind a stereo pair"""
    ch = pcm.shape[2]
    for f in range(pcm.shape[0]):
        for c in range(ch):
            yield pcm[f, :, c].astype(np.int32)
        if ch == 2:
            yield pcm[f, :, 0].astype(np.int32) - pcm[f, :, 1]


def _check(gpu, pcm, who):
    o = oracle()
    ref_frames, ref_offsets, _ = o.encode_frames(pcm, threads=4)
    frames, offsets, _, _ = _encode(gpu, pcm)  # k_encode_teams<0, P>
    assert np.array_equal(offsets, ref_offsets) and np.array_equal(frames, ref_frames), who
    frames, offsets, enc, _ = _encode(gpu, pcm, with_trace=True)  # k_encode_teams<1, P>
    assert np.array_equal(offsets, ref_offsets) and np.array_equal(frames, ref_frames), who
    traces = enc.traces(pcm.shape[0])
    for i, s in enumerate(_signals(pcm)):
        order, _, _, _, tr, _ = o.lpc_analyze(s, with_trace=True)
        assert np.array_equal(_bits(list(traces[i].k)), _bits(list(tr.k))), (who, i)
        assert traces[i].order == order, (who, i)


@functools.lru_cache(maxsize=None)
def _late_blocks():
    rows = [_noise(s, 32767) for s in LATE_FULL_SCALE] + [_noise(s, 3) for s in LATE_PLUS_MINUS_3]
    return np.stack(rows)[:, :, None]


@functools.lru_cache(maxsize=None)
def _boundary_blocks():
    return np.stack([_echo(seed, lag) for lag, seed in BOUNDARY])[:, :, None]


def test_the_recorded_seeds_give_the_orders_they_were_chosen_for():
    """(no kernel: the oracle alone)  Eight noise blocks of order >= 97, and for every phase boundary blocks of order stage - 1,
    stage and stage + 1."""
    o = oracle()
    want = list(LATE_FULL_SCALE.values()) + list(LATE_PLUS_MINUS_3.values())
    got = [int(o.lpc_analyze(b[:, 0].astype(np.int32))[0]) for b in _late_blocks()]
    assert got == want and min(got) >= 97
    got = [int(o.lpc_analyze(b[:, 0].astype(np.int32))[0]) for b in _boundary_blocks()]
    assert got == [lag for lag, _ in BOUNDARY]
    assert {lag for lag, _ in BOUNDARY} == {s + d for s in PHASE_STAGES for d in (-1, 0, 1)}


@pytest.mark.gpu
def test_late_stages_bit_exact(gpu, teams):  # noqa: F811
    """Blocks whose order is 97 .. 100: the coefficients of the last phase (one column per lane, ever fewer lanes) decide
    their order and their bytes.  As mono frames, and the same blocks paired into stereo frames (their difference is a third)."""
    mono = _late_blocks()
    _check(gpu, mono, (teams, "mono"))
    _check(gpu, np.concatenate([mono[:4], mono[4:]], axis=2), (teams, "stereo"))


@pytest.mark.gpu
def test_orders_at_every_phase_boundary(gpu, teams):  # noqa: F811
    """The last coefficient above the threshold is computed in the last stage of a phase, the first stage of the next one, or the
    stage between: a column lost or misplaced by the repack changes it."""
    _check(gpu, _boundary_blocks(), teams)


@pytest.mark.gpu
def test_degenerate_blocks_cross_every_repack(gpu, teams):  # noqa: F811
    """_hard_blocks(): the all-zero block is NaN from stage 0 on, and its NaNs cross the repacks as the reference's do; constant
    and full-scale blocks, impulses, alternating extremes."""
    hard = _hard_blocks()
    _check(gpu, hard, (teams, "mono"))
    _check(gpu, np.concatenate([hard, hard[::-1]], axis=2), (teams, "stereo"))


def _alternating(n_frames, channels, loud_first):
    """silent frames and full-scale frames of alternating sign in turn: in a wave, every team's neighbour holds NaN columns or
    extreme ones.  (Stereo: right = -left - 1, so left - right is the widest signal there is.)"""
    pcm = np.zeros((n_frames, 2048, channels), np.int16)
    loud = np.where(np.arange(2048) % 2 == 0, 32767, -32768).astype(np.int16)
    for f in range(n_frames):
        if (f % 2 == 0) == bool(loud_first):
            for c in range(channels):
                pcm[f, :, c] = loud if c % 2 == 0 else ~loud
    return pcm


@pytest.mark.parametrize("n_frames,channels", [(1, 2), (4, 2), (5, 2), (8, 2), (9, 2), (9, 1)])
@pytest.mark.gpu
def test_nothing_leaks_from_a_neighbouring_team(gpu, teams, n_frames, channels):  # noqa: F811
    """A team's last column takes its neighbour from the next team's first lane.  1, 4 and 5 stereo frames are a wave with one
    block, a full wave and a full wave plus one block for teams of 16; 8 and 9 the same for teams of 8; 9 mono frames."""
    for loud_first in (0, 1):
        _check(gpu, _alternating(n_frames, channels, loud_first), (teams, n_frames, channels, loud_first))
