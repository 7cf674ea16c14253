"""The encoder's integer bookkeeping -- the residue filter's window and coefficient addresses (one base per group of 32 taps,
constant offsets), the PCM fetches (one address per block or chunk), the unpacking of a stereo signal (one branch per group of
words, not a select per sample), the 32-bit Rice sums, the range test behind the plain loop only (sela_encode.hip,
sela_encode_tail.inc) -- leaves every byte where it was: frame bytes and offsets of all three encode kernels,
in every form of the residue filter, against the CPU oracle's frame_encode, and every status word 0.

The inputs are chosen for what the new addressing must survive: predictor orders in each group of taps (<= 32, 33-64, 65-96,
97-100) and at the groups' edges (32 and 33 exactly), which the coverage test asserts of them with the oracle; batches that fill
waves of teams of 16 and leave shadow teams (9 stereo frames: two full waves per signal and one with three shadows), one frame,
mono and three channels (the fetches that stride by the channel count); silence (order 1), a full-scale square wave and
full-scale noise (loud blocks, long streams).
"""
import numpy as np
import pytest
from oracle_lib import oracle
from sela_amd.synth import synth_frames

from gpu_common import gpu  # noqa: F401  (fixture)


def _pool():
    """51 stereo frames: the first 24 of synthetic tracks 0 and 2, silence, a +-32767 square wave, full-scale noise."""
    rng = np.random.default_rng(20261017)
    square = np.where((np.arange(2048) // 32) % 2 == 0, 32767, -32767).astype(np.int16)
    extra = np.zeros((3, 2048, 2), np.int16)
    extra[1, :, 0], extra[1, :, 1] = square, -square  # (the difference signal swings +-65534)
    extra[2] = rng.integers(-32768, 32768, (2048, 2))
    return np.concatenate([synth_frames(24, 2, 0), synth_frames(24, 2, 2), extra])


def _batches():
    """[frames, 2048, channels] arrays: 9 stereo frames (five times), 5 stereo, 1 stereo, 5 mono, 3 frames of 3 channels."""
    pool = _pool()
    out = [pool[i: i + 9] for i in range(0, 45, 9)] + [pool[45:50], pool[50:51]]
    out.append(np.ascontiguousarray(pool[[3, 30, 48, 49, 50], :, :1]))  # mono: two tracks' frames, silence, square, noise
    three = np.stack([np.stack([pool[a, :, 0], pool[b, :, 1], pool[c, :, 0]], axis=1) for a, b, c in ((7, 31, 49), (48, 12, 40), (50, 2, 26))])
    out.append(np.ascontiguousarray(three))
    return out


def _signals(pcm):
    ch = pcm.shape[2]
    for f in range(pcm.shape[0]):
        if ch == 2:
            l, r = pcm[f, :, 0].astype(np.int32), pcm[f, :, 1].astype(np.int32)
            yield from (l, r, l - r)
        else:
            for c in range(ch):
                yield pcm[f, :, c].astype(np.int32)


@pytest.fixture(scope="module")
def cases():
    """(pcm, oracle frame bytes, oracle offsets) per batch, computed once."""
    o = oracle()
    out = []
    for pcm in _batches():
        frames = [o.frame_encode(pcm[f]) for f in range(pcm.shape[0])]
        offsets = np.cumsum([0] + [len(b) for b in frames]).astype(np.uint64)
        out.append((pcm, np.frombuffer(b"".join(frames), np.uint8), offsets))
    return out


def test_the_inputs_reach_every_group_of_taps():
    """A condition on the inputs (no GPU): the oracle's predictor orders over all the signals of all the batches."""
    o = oracle()
    orders = set()
    for pcm in _batches():
        orders |= {int(o.lpc_analyze(s)[0]) for s in _signals(pcm)}
    assert any(n <= 32 for n in orders) and any(33 <= n <= 64 for n in orders), sorted(orders)
    assert any(65 <= n <= 96 for n in orders) and any(97 <= n <= 100 for n in orders), sorted(orders)
    assert 32 in orders and 33 in orders and 1 in orders, sorted(orders)


@pytest.mark.gpu
@pytest.mark.parametrize("team_lanes,form", [(0, 0), (0, 2), (8, 0), (8, 2), (16, 0), (16, 2), (16, 1)],
                         ids=lambda v: str(v))
def test_frames_are_the_oracles_in_every_kernel_and_form(gpu, cases, team_lanes, form):  # noqa: F811
    """team_lanes 0 / 8 / 16: k_encode_blocks / k_encode_teams<0,8> / <0,16> (forced: batches this small never reach the team
    kernels by themselves); form 0: each block's own choice (one pass of FP64 taps on all but the loudest), 2: two passes wherever
    one would do, 1: the plain 64-bit loop, which this change leaves alone."""
    from sela_amd import capi, codec

    lib = capi.lib()
    lib.sela_hip_debug_encode_teams(team_lanes)
    lib.sela_hip_debug_force_plain_fir(form)
    try:
        for i, (pcm, want, want_offsets) in enumerate(cases):
            enc = codec.Encoder(pcm.shape[0], pcm.shape[2])
            out = enc.encode(gpu.from_numpy(pcm).cuda())
            gpu.cuda.synchronize()
            status = out.status.cpu().numpy()
            assert not status.any(), (i, status)
            offsets = out.offsets.cpu().numpy().view(np.uint64)
            assert np.array_equal(offsets, want_offsets), i
            assert np.array_equal(out.frames[: int(offsets[-1])].cpu().numpy(), want), i
    finally:
        lib.sela_hip_debug_force_plain_fir(0)
        lib.sela_hip_debug_encode_teams(-1)
