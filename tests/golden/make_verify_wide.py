#!/usr/bin/env python3
"""Generate verify_wide.json FROM THE REAL REFERENCE: which frames of the verification corpus, widened to 24 bits, the
reference's own decoder returns differently from the samples its encoder was given, how many values, and the first of them
(index c * 2048 + i, channel by channel: the planar layout of data::WavFrame).

Runs only where oracle/_ref/libsela_ref.so exists (`make -C oracle ref` compiles the unmodified reference).  The fixture is
pure data; tests/test_verify32_cpu.py holds the restatement oracle against it, tests/test_gpu_verify_i32_device.py the GPU.

    python tests/golden/make_verify_wide.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import corpus  # noqa: E402
from oracle_lib import reference  # noqa: E402

SEED, NOISE_SEED, FRAMES, BITS = 20260927, 20261017, 1500, 24


def wide_frames(frames=FRAMES, seed=SEED, noise_seed=NOISE_SEED, bits=BITS):
    """int32 [frames, 2, 2048]: the corpus' 16-bit frames shifted up to `bits` bits with noise in the new low bits."""
    pcm = corpus.build(frames, seed)
    rng = np.random.default_rng(noise_seed)
    shift = bits - 16
    out = np.empty((frames, 2, 2048), np.int32)
    for f in range(frames):
        x = (pcm[f].T.astype(np.int64) << shift) + rng.integers(-(1 << (shift - 1)), 1 << (shift - 1), (2, 2048))
        out[f] = np.clip(x, -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(np.int32)
    return out


def lossy_frames(codec, samples):
    """Encode and decode every frame with `codec` (the reference or the oracle) -> [{frame, count, first}] of those that differ."""
    out = []
    for f, x in enumerate(samples):
        back, _ = codec.frame_decode_i32(codec.frame_encode_i32(x), x.shape[0], stride=x.shape[1])
        assert [len(b) for b in back] == [x.shape[1]] * x.shape[0]
        diff = (np.stack(back) != x).ravel()
        if diff.any():
            out.append({"frame": int(f), "count": int(diff.sum()), "first": int(diff.argmax())})
    return out


def main():
    ref = reference()
    assert ref is not None, "oracle/_ref/libsela_ref.so is missing: make -C oracle ref"
    out = {"seed": SEED, "noise_seed": NOISE_SEED, "frames": FRAMES, "bits": BITS, "channels": 2, "samples_per_frame": 2048,
           "lossy": lossy_frames(ref, wide_frames())}
    with open(os.path.join(HERE, "verify_wide.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(out["lossy"])


if __name__ == "__main__":
    main()
