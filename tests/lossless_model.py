"""The lossless encode mode restated on the CPU, and the inputs its tests share.  Not a test file.

frame::FrameEncoder with one change: a block's residues are taken against the DECODER's prediction
    dec_pred[i] = -(int32)((2^34 - sum_{j=1..min(i,order)} a[j] s[i-j]) >> 35)        (src/lpc/sample_generator.cpp:25-28)
instead of the encoder's (int32)((2^34 + sum) >> 35) (src/lpc/residue_generator.cpp:113-117).  Everything else is the pinned
oracle's: the analysis (order, q[], a[]) from lpc_analyze(..., with_trace=True), the Rice coder, and the frame's bytes from
wide_cases.frame_bytes; the stereo decision is the strict `<` of src/frame/frame_encoder.cpp:64-72.  With lossless=False the
model is the reference's encoder, which tests/test_lossless_model_cpu.py holds against the oracle byte for byte."""
import functools

import numpy as np

import wide_cases

Q_SHIFT = 35
SEED, CORPUS_FRAMES = 20260927, 3000
A_FRAMES = [400, 401, 402, 580, 1128, 1158, 1182, 2395, 2798, 2799]
W_FRAMES = [186, 187, 642, 906, 939]
N1000_FRAMES = [1127, 1128, 1129, 1488]
N300_FRAMES = [19, 20, 21, 1200]


def predictions(a, s):
    """(encoder's, decoder's) prediction of every sample of s (int32[n]) under the Q35 predictor a[0 .. order], both in the
    reference's own 64-bit wrap-around arithmetic, as int32."""
    s64 = np.asarray(s, np.int32).astype(np.int64)
    a = np.asarray(a, np.int64)
    total = np.zeros(len(s64), np.int64)
    with np.errstate(over="ignore"):
        for j in range(1, len(a)):
            if j < len(s64):
                total[j:] += a[j] * s64[:-j]
        half = np.int64(1) << (Q_SHIFT - 1)
        enc = ((half + total) >> Q_SHIFT).astype(np.int32)
        dec = (np.int32(0) - ((half - total) >> Q_SHIFT).astype(np.int32)).astype(np.int32)
    return enc, dec


def code_signal(o, s, lossless):
    """One block -> (q int32[order], residues int32[n], ties): ties = the samples at which the two predictions differ."""
    s = np.ascontiguousarray(s, np.int32)
    order, q, _, a, _, _ = o.lpc_analyze(s, with_trace=True)
    enc, dec = predictions(a, s)
    with np.errstate(over="ignore"):
        r = (s - (dec if lossless else enc)).astype(np.int32)
    return q, r, int((enc != dec).sum())


def _words(o, q, r):
    return len(o.rice_encode(q)[1]) + len(o.rice_encode(r)[1])


def analyse_frame(o, planar, lossless):
    """planar: int32 [channels, n], or a list of int32 arrays of different lengths (a ragged frame)
    -> (bytes, ties per candidate [ch0, ch1, ... (, difference)], index of every STORED candidate, word counts per candidate)."""
    chans = [np.ascontiguousarray(c, np.int32).ravel() for c in planar]
    signals = list(chans)
    if len(chans) == 2:
        n1 = len(chans[1])
        with np.errstate(over="ignore"):
            signals.append((chans[0][:n1] - chans[1]).astype(np.int32))
    coded = [code_signal(o, s, lossless) for s in signals]
    words = [_words(o, q, r) for q, r, _ in coded]
    subframes, stored = [], []
    for c in range(len(chans)):
        if len(chans) == 2 and c == 1 and words[2] < words[1]:  # strictly fewer words: the difference
            subframes.append((1, 1, 0, coded[2][0], coded[2][1]))
            stored.append(2)
        else:
            subframes.append((c, 0, c, coded[c][0], coded[c][1]))
            stored.append(c)
    return wide_cases.frame_bytes(o, subframes), [t for _, _, t in coded], stored, words


def encode_frame(o, planar_int32, lossless):
    """-> the frame's bytes."""
    return analyse_frame(o, planar_int32, lossless)[0]


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus():
    import corpus

    return corpus.build(CORPUS_FRAMES, SEED)


@functools.lru_cache(maxsize=None)
def _wide():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_verify_wide import wide_frames

    return wide_frames()


@functools.lru_cache(maxsize=None)
def cases():
    """name -> list of frames, each int32 [channels, n] -- or, in R, a list of two arrays of different lengths."""
    pcm = _corpus()
    planar = lambda frames, n=2048: [np.ascontiguousarray(pcm[f, :n].T.astype(np.int32)) for f in frames]
    a = planar(A_FRAMES)
    return {
        "A": a,
        "M": [np.ascontiguousarray(x[:1]) for x in a],
        "T": [np.ascontiguousarray(np.stack([x[0], x[1], x[0]])) for x in a],
        "W": [np.ascontiguousarray(_wide()[f]) for f in W_FRAMES],
        "N1000": planar(N1000_FRAMES, 1000),
        "N300": planar(N300_FRAMES, 300),
        "R": [[np.ascontiguousarray(pcm[1128, :1000, 0].astype(np.int32)), np.ascontiguousarray(pcm[1128, :300, 1].astype(np.int32))]],
    }


def interleaved(frames):
    """A case's frames as the int16 PCM the 16-bit calls take: [n_frames, n, channels]."""
    return np.ascontiguousarray(np.stack([np.asarray(x).T for x in frames]).astype(np.int16))


def stream(o, frames, lossless):
    """(bytes uint8[...], offsets uint64[n_frames + 1]) of the frames back to back."""
    blobs = [encode_frame(o, x, lossless) for x in frames]
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), offs
