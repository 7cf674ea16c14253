"""Staging of the autocorrelation's ring: the teams of 16 stage a chunk of 64 samples at a place, from a
word set and with a mirror that are constants of the chunk's number mod 4, convert x = s / 32767 in two FP64 instructions
(tests/test_scale17_exact.py) and carry the window's LDS address as a byte offset mod 2048; the teams of 8 and k_encode_blocks
share the conversion.  Every case forces one of the three kernels and compares, against the CPU oracle, the frame bytes and
offsets of the product instantiation and, from the trace instantiation, every block's mean and ac[0..100] as 64-bit patterns
(src/lpc/residue_generator.cpp:12-44).

Frame counts (stereo): 1, 3, 4, 5 and 33 -- for teams of 16 a lone team, a partial last wave whose dead teams shadow frame 0, exactly
one wave, one wave plus one team, and several XCD columns.  A case whose material has more frames than the count runs it in
several launches of that many frames.
"""
import functools

import numpy as np
import pytest
from oracle_lib import oracle

from gpu_common import _bits, _encode, gpu  # noqa: F401  (fixture and helpers)
from test_gpu_schur_phases import _late_blocks, _signals

FRAME_COUNTS = (1, 3, 4, 5, 33)
IMPULSES = (0, 23, 24, 63, 64, 255, 256, 2047)  # the mirror's edge, the chunk's edge, the ring's wrap, the block's end


def _ramps(n):
    """Left: every 16-bit value once, in 32 frames.  Right: 32767 under the negative half and -32768 under the rest, so that
    left - right takes every value of [-65535, -32768] and of [32768, 65535]: between them the three signals of the 32 frames
    take every value in [-65535, 65535].  Frame 33: right walks down while left stands, and the difference crosses zero.
    Fewer frames than 33: that many of them, evenly spread from the first to the last (both extremes stay in)."""
    t = np.arange(65536)
    left = (t - 32768).astype(np.int16)
    right = np.where(t < 32768, 32767, -32768).astype(np.int16)
    pcm = np.stack([left, right], axis=1).reshape(32, 2048, 2)
    last = np.stack([np.full(2048, 5, np.int16), (1024 - np.arange(2048)).astype(np.int16)], axis=1)[None]
    pcm = np.concatenate([pcm, last])
    if n >= len(pcm):
        return pcm
    return pcm[np.unique(np.rint(np.linspace(0, len(pcm) - 1, n)).astype(int))] if n > 1 else pcm[:1]


def _long_predictors():
    """eight frames of blocks whose order is 97 .. 100 (tests/test_gpu_schur_phases.py: every one of the 101 lags and every wrap of
    the ring decides their bytes), each block once left and once right"""
    blocks = _late_blocks()[:, :, 0]
    return np.stack([np.stack([blocks[i], blocks[(i + 3) % len(blocks)]], axis=1) for i in range(len(blocks))])


def _impulses():
    """eight frames: one sample of each channel stands out of silence, left at IMPULSES[f] and right three places further on"""
    pcm = np.zeros((len(IMPULSES), 2048, 2), np.int16)
    for f, at in enumerate(IMPULSES):
        pcm[f, at, 0] = 32767 if f % 2 == 0 else -32768
        pcm[f, IMPULSES[(f + 3) % len(IMPULSES)], 1] = -32768 if f % 2 == 0 else 12345
    return pcm


@functools.lru_cache(maxsize=None)
def _launches(content, n):
    """the batches of n frames a case encodes, each with the oracle's bytes, offsets and per-block traces -- computed once and
    shared by the three kernels"""
    pool = {"ramps": lambda: _ramps(n), "long_predictors": _long_predictors, "impulses": _impulses}[content]()
    if content == "ramps":
        assert len(pool) == min(n, 33)
    starts = range(0, len(pool), n) if n < len(pool) else (0,)
    o = oracle()
    out = []
    for s in starts:
        pcm = np.ascontiguousarray(pool[(s + np.arange(n)) % len(pool)])
        frames, offsets, _ = o.encode_frames(pcm, threads=4)
        traces = [o.lpc_analyze(sig, with_trace=True)[4] for sig in _signals(pcm)]
        ref = [(_bits(tr.mean), _bits(list(tr.ac))) for tr in traces]
        for a in (frames, offsets):
            a.setflags(write=False)
        out.append((pcm, frames, offsets, ref))
    return tuple(out)


def test_the_ramps_take_every_value():
    """(no kernel)  33 frames: the channels and their difference between them take every value in [-65535, 65535]."""
    pcm = _ramps(33).astype(np.int32)
    seen = np.unique(np.concatenate([pcm[:, :, 0].ravel(), pcm[:, :, 1].ravel(), (pcm[:, :, 0] - pcm[:, :, 1]).ravel()]))
    assert np.array_equal(seen, np.arange(-65535, 65536))
    for n in FRAME_COUNTS:
        few = _ramps(n).astype(np.int32)
        assert len(few) == n and few[:, :, 0].min() == -32768 and (few[:, :, 0] - few[:, :, 1]).min() == -65535


@pytest.fixture(params=[16, 8, 0], ids=["teams_of_16", "teams_of_8", "k_encode_blocks"])
def kernel(request, gpu):  # noqa: F811
    from sela_amd import capi

    capi.lib().sela_hip_debug_encode_teams(request.param)
    yield request.param
    capi.lib().sela_hip_debug_encode_teams(-1)


@pytest.mark.parametrize("n_frames", FRAME_COUNTS)
@pytest.mark.parametrize("content", ["ramps", "long_predictors", "impulses"])
@pytest.mark.gpu
def test_staged_blocks_bit_exact(gpu, kernel, content, n_frames):  # noqa: F811
    from sela_amd import capi

    assert capi.lib().sela_hip_debug_encode_kernel(n_frames, 2) == kernel
    for at, (pcm, ref_frames, ref_offsets, ref) in enumerate(_launches(content, n_frames)):
        who = (kernel, content, n_frames, at)
        frames, offsets, _, _ = _encode(gpu, pcm)  # the product instantiation
        assert np.array_equal(offsets, ref_offsets) and np.array_equal(frames, ref_frames), who
        frames, offsets, enc, _ = _encode(gpu, pcm, with_trace=True)  # the trace instantiation
        assert np.array_equal(offsets, ref_offsets) and np.array_equal(frames, ref_frames), who
        traces = enc.traces(n_frames)
        assert len(traces) == len(ref) == 3 * n_frames
        for i, (mean, ac) in enumerate(ref):
            assert np.array_equal(_bits(traces[i].mean), mean), (who, i, "mean")
            assert np.array_equal(_bits(list(traces[i].ac)), ac), (who, i, "ac")
