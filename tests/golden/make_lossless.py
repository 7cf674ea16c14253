#!/usr/bin/env python3
"""Generate lossless.json: per case and frame of tests/lossless_model.py the samples at which the encoder's and the decoder's
predictions differ (per candidate: the channels, then the difference of an exactly-stereo frame), which candidates the frame
stores, and the SHA-256 of the frame the lossless mode writes.

A frame is written only after THE REAL REFERENCE's decoder has turned the model's lossless frame back into the input exactly, so
the script runs only where oracle/_ref/libsela_ref.so exists (`make -C oracle ref` compiles the unmodified reference).  The
fixture is pure data; tests/test_lossless_model_cpu.py holds the model against it, tests/test_gpu_encode_lossless.py the GPU
against the model.

    python tests/golden/make_lossless.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lossless_model as model  # noqa: E402
from oracle_lib import oracle, reference  # noqa: E402


def main():
    ref = reference()
    assert ref is not None, "oracle/_ref/libsela_ref.so is missing: make -C oracle ref"
    o = oracle()
    out = {"seed": model.SEED, "corpus_frames": model.CORPUS_FRAMES, "cases": {}}
    for name, frames in model.cases().items():
        rows = []
        for x in frames:
            blob, ties, stored, _ = model.analyse_frame(o, x, True)
            back, used = ref.frame_decode_i32(blob, len(x))
            assert used == len(blob) and len(back) == len(x) and all(np.array_equal(b, c) for b, c in zip(back, x)), (name, len(rows))
            rows.append({"ties": ties, "stored": stored, "bytes": len(blob), "sha256": hashlib.sha256(blob).hexdigest()})
        out["cases"][name] = rows
    with open(os.path.join(HERE, "lossless.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print({k: [r["ties"] for r in v] for k, v in out["cases"].items()})


if __name__ == "__main__":
    main()
