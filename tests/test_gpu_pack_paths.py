"""The two copies of the residue pack (sela_encode_tail.inc): a block none of whose codewords is longer than a word -- decided
once per block from the largest of its zig-zagged residues, (max >> k) + 1 + k <= 32 -- is packed by a copy without the
per-codeword test; every other block by the copy that has it.  Frame bytes against the oracle's frame encoder, for 1 and 4 frames, on
k_encode_blocks and both k_encode_teams, for blocks at the corners of that decision:

  (a) silence with one sample of -16: order 1, k = 0, the longest codeword exactly 32 bits (ones + 1 = 32 in the short copy)
  (b) the same with +16: 33 bits, one codeword sends the whole block down the copy with the test
  (c) noise within +-6 with one spike, k = 2: the spike's amplitude searched (in steps of 1) for a longest codeword of 32 and of 33 bits
  (d) a block whose OR of the residues fails that test, (OR >> k) + 1 + k > 32, although none of its codewords is long (the
      kernel asks the maximum and takes the short copy; asking the OR, as rice_plan once offered, it would not)
  (e) a loud full-scale block, k >= 10

What each block is said to be is asserted on the oracle alone (no GPU) in the first test."""
import functools

import numpy as np
import pytest
from oracle_lib import oracle

from gpu_common import _encode, gpu  # noqa: F401  (fixture and helper)

N = 2048
SPIKE_SEED, SPIKE_AT = 1, 1000


def _zigzag(r):
    r = np.asarray(r, np.int64)
    return np.where(r < 0, -2 * r - 1, 2 * r).astype(np.uint64)


def facts(block):
    """(order, k, longest codeword in bits, whether the OR of the residues passes the test) by the oracle's analysis and parameter search"""
    o = oracle()
    order, _, r = o.lpc_analyze(np.asarray(block, np.int32))
    k, _ = o.rice_encode(r)
    u = _zigzag(r)
    longest = int((u >> np.uint64(k)).max()) + 1 + k
    passes = (int(np.bitwise_or.reduce(u)) >> k) + 1 + k <= 32
    return int(order), int(k), longest, passes


def _one_sample(v):
    x = np.zeros(N, np.int16)
    x[SPIKE_AT] = v
    return x


def _spiked(amp):
    x = np.random.default_rng(SPIKE_SEED).integers(-6, 7, N).astype(np.int16)
    x[SPIKE_AT] = amp
    return x


@functools.lru_cache(maxsize=None)
def blocks():
    """label -> int16[2048]; the spikes of (c) and (d) are found here, by the oracle."""
    out = {"a: -16 in silence": _one_sample(-16), "b: +16 in silence": _one_sample(16)}
    found = {}
    for amp in range(7, 400):
        x = _spiked(amp)
        _, k, longest, passes = facts(x)
        if k == 2 and longest in (32, 33) and f"c: {longest} bits" not in found:
            found[f"c: {longest} bits"] = x
        if longest <= 32 and not passes and "d" not in found:
            found["d"] = x
    assert "c: 32 bits" in found or "c: 33 bits" in found, "no spike gives a longest codeword of 32 or of 33 bits"
    assert "d" in found, "no spike fails the OR test with short codewords only"
    for label in sorted(found):
        out[label if label != "d" else "d: OR test fails, no long codeword"] = found[label]
    out["e: loud"] = np.random.default_rng(5).integers(-32768, 32768, N).astype(np.int16)
    for x in out.values():
        x.setflags(write=False)
    return out


def test_the_blocks_are_what_they_are_called():
    """(no kernel: the oracle alone)"""
    b = blocks()
    assert facts(b["a: -16 in silence"]) == (1, 0, 32, True)
    order, k, longest, passes = facts(b["b: +16 in silence"])
    assert (order, k, longest, passes) == (1, 0, 33, False)
    for bits in (32, 33):
        if f"c: {bits} bits" in b:
            _, k, longest, passes = facts(b[f"c: {bits} bits"])
            assert k == 2 and longest == bits and (passes is False or bits == 32)
    _, _, longest, passes = facts(b["d: OR test fails, no long codeword"])
    assert longest <= 32 and not passes
    _, k, longest, passes = facts(b["e: loud"])
    assert k >= 10 and passes


@functools.lru_cache(maxsize=None)
def _cases():
    """(label, pcm int16 [frames, 2048, channels], the oracle's bytes per frame): every block as one mono frame, and as four
    stereo frames with the other blocks for neighbours (left - right is a third block of each frame)."""
    o = oracle()
    b = blocks()
    labels = list(b)
    out = []
    for i, label in enumerate(labels):
        one = np.ascontiguousarray(b[label][None, :, None])
        four = np.zeros((4, N, 2), np.int16)
        for f in range(4):
            four[f, :, f % 2] = b[label]
            four[f, :, 1 - f % 2] = b[labels[(i + 1 + f) % len(labels)]]
        for pcm in (one, four):
            want = [o.frame_encode(pcm[f]) for f in range(len(pcm))]
            pcm.setflags(write=False)
            out.append((f"{label}, {len(pcm)} frame(s)", pcm, want))
    return tuple(out)


@pytest.fixture(params=[0, 8, 16], ids=["blocks", "teams_of_8", "teams_of_16"])
def kernel(request, gpu):  # noqa: F811
    from sela_amd import capi

    capi.lib().sela_hip_debug_encode_teams(request.param)
    yield request.param
    capi.lib().sela_hip_debug_encode_teams(-1)


@pytest.mark.gpu
def test_frame_bytes_on_either_copy_of_the_pack(gpu, kernel):  # noqa: F811
    from sela_amd import capi

    for label, pcm, want in _cases():
        assert capi.lib().sela_hip_debug_encode_kernel(pcm.shape[0], pcm.shape[2]) == kernel
        frames, offsets, _, _ = _encode(gpu, np.array(pcm))
        assert offsets.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist(), (kernel, label)
        assert frames.tobytes() == b"".join(want), (kernel, label)
