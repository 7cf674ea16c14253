#!/usr/bin/env python3
"""Generate verify_corpus.json FROM THE REAL REFERENCE: which frames of the verification corpus the reference's own decoder
returns differently from the PCM its encoder was given, how many values, and the first of them.

Runs only where oracle/_ref/libsela_ref.so exists (`make -C oracle ref` compiles the unmodified reference).  The fixture is
pure data; tests/test_verify_cpu.py holds the restatement oracle against it, tests/test_gpu_verify_device.py the GPU against
that oracle.

    python tests/golden/make_verify_corpus.py
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

SEED, FRAMES = 20260927, 3000


def lossy_frames(codec, pcm, threads=8):
    """Encode and decode with `codec` (the reference or the oracle) -> [{frame, count, first}] of the frames that differ."""
    frames, offs, _ = codec.encode_frames(pcm, threads=threads)
    back, _ = codec.decode_frames(frames, offs, pcm.shape[2], threads=threads)
    diff = (back != pcm).reshape(len(pcm), -1)
    return [{"frame": int(f), "count": int(diff[f].sum()), "first": int(diff[f].argmax())} for f in np.flatnonzero(diff.any(1))]


def main():
    ref = reference()
    assert ref is not None, "oracle/_ref/libsela_ref.so is missing: make -C oracle ref"
    pcm = corpus.build(FRAMES, SEED)
    out = {"seed": SEED, "frames": FRAMES, "channels": 2, "samples_per_frame": 2048, "lossy": lossy_frames(ref, pcm)}
    with open(os.path.join(HERE, "verify_corpus.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(out["lossy"])


if __name__ == "__main__":
    main()
