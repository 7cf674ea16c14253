"""The inputs the tests of whole 24- and 32-bit tracks share, and what the reference makes of them.  Not a test file.

Tracks are the synthetic music (sela_amd.synth) widened: shifted left and the low bits filled with noise -- 24-bit samples for a
3-byte container, 27-bit samples for a 4-byte one.  For odd k the second channel follows the first closely, so that the frame
encoder's stereo decision takes the difference.  Expected bytes are `reference() or oracle()`'s frame_encode_i32 per frame of the
layout sela_hip_whole_frames gives; with lossless=True tests/lossless_model.py's."""
import functools

import numpy as np

import lossless_model
from oracle_lib import oracle, reference
from sela_amd import codec
from sela_amd.synth import synth_pcm

N = 2048


def ref():
    return reference() or oracle()


def bits_of(b):
    return 24 if b == 3 else 27


@functools.lru_cache(maxsize=None)
def track(n, ch, b, k=0):
    """int32 [n, ch] interleaved, samples of bits_of(b) bits"""
    if n == 0:
        return np.zeros((0, ch), np.int32)
    shift = bits_of(b) - 16
    rng = np.random.default_rng(1000 * k + 10 * ch + b)
    x = synth_pcm(n + 64 * k, max(ch, 2), k % 5).astype(np.int32)[64 * k:, :ch]
    x = (x << shift) | rng.integers(0, 1 << shift, x.shape).astype(np.int32)
    if k % 2 and ch >= 2:
        x[:, 1] = np.clip(x[:, 0].astype(np.int64) - (x[:, 1] >> 9), -(1 << (bits_of(b) - 1)), (1 << (bits_of(b) - 1)) - 1).astype(np.int32)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def packed(x, b):
    """int32 [n, ch] -> the packed little-endian bytes, b per sample"""
    u = np.ascontiguousarray(x, np.int32).view(np.uint32)
    return np.ascontiguousarray(np.stack([(u >> np.uint32(8 * i)).astype(np.uint8) for i in range(b)], axis=-1).reshape(-1))


def frames_of(x):
    """the planar int32 [ch, length] frames of the whole-track layout of x [n, ch]"""
    return [np.ascontiguousarray(x[first: first + length].T) for first, length in codec.whole_frames(len(x))]


def join(blobs):
    return b"".join(blobs), np.cumsum([0] + [len(f) for f in blobs]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def expected(n, ch, b, k=0, lossless=False):
    """-> (bytes, offsets uint64 [frames + 1]) of the whole-track stream of track(n, ch, b, k); every frame is one the reference
    encodes (an empty frame would be its refusal)."""
    r = ref()
    blobs = [lossless_model.encode_frame(oracle(), f, True) if lossless else r.frame_encode_i32(f) for f in frames_of(track(n, ch, b, k))]
    assert all(len(f) > 4 for f in blobs), (n, ch, b, k)
    return join(blobs)


def decoded(blob, offs, ch):
    """the reference's frame_decode_i32 per frame, concatenated -> int32 [samples, ch]"""
    r = ref()
    out = []
    for f in range(len(offs) - 1):
        chans, used = r.frame_decode_i32(blob[int(offs[f]): int(offs[f + 1])], ch, stride=4096)
        assert used == int(offs[f + 1]) - int(offs[f])
        out.append(np.stack(chans, axis=1))
    return np.concatenate(out) if out else np.zeros((0, ch), np.int32)


def second_subframe_type(frame):
    import struct

    cw = struct.unpack_from("<H", frame, 4 + 4)[0]
    rw = struct.unpack_from("<H", frame, 4 + 7 + 4 * cw + 1)[0]
    return frame[4 + 12 + 4 * (cw + rw) + 1]
