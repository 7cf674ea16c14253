"""The paired encode calls restated on the CPU, and the inputs their tests share.  Not a test file.

A paired frame of C channels is, byte for byte, the sync word followed by the two subframes of the stereo frame of
(ch[2p], ch[2p + 1]) for every pair p = 0 .. C / 2 - 1, then the mono subframe of an odd last channel -- each with its
channel byte (byte 0) and its parent byte (byte 2) moved up by the pair's first channel.  The stereo and mono frames are
lossless_model.encode_frame's: the reference's frame encoder (tests/test_lossless_model_cpu.py holds that), or the lossless
mode's."""
import functools

import numpy as np

import lossless_model

SYNC = bytes([0x00, 0xFF, 0x55, 0xAA])
SYNTH_FRAMES, SYNTH_CHANNELS, SYNTH_TRACK = 20, 6, 3  # the issue's known answer: 365,556 bytes plain, 354,104 paired
# lossless_model.W_FRAMES all refuse their difference: each is stacked with a frame of the same wide corpus that stores it
W_PARTNERS = [1, 2, 6, 9, 11]


def subframes(blob):
    """A frame's bytes -> its subframes' bytes, in order (the header of include/sela_format.h: channel, type, parent, coef_k,
    coef_words u16, order | words | res_k, res_words u16, n u16 | words)."""
    assert blob[:4] == SYNC
    out, p = [], 4
    while p < len(blob):
        cw = blob[p + 4] | (blob[p + 5] << 8)
        h = p + 7 + 4 * cw
        rw = blob[h + 1] | (blob[h + 2] << 8)
        end = h + 5 + 4 * rw
        out.append(blob[p:end])
        p = end
    assert p == len(blob)
    return out


def _moved(sub, first):
    b = bytearray(sub)
    b[0] += first
    b[2] += first
    return bytes(b)


def encode_frame(o, planar, lossless):
    """planar: int32 [channels, n] -> (the paired frame's bytes, the type byte of every subframe)."""
    x = np.ascontiguousarray(planar, np.int32)
    out, types = [SYNC], []
    for c0 in range(0, len(x), 2):
        subs = subframes(lossless_model.encode_frame(o, np.ascontiguousarray(x[c0:c0 + 2]), lossless))
        assert len(subs) == len(x[c0:c0 + 2])
        for s in subs:
            out.append(_moved(s, c0))
            types.append(s[1])
    return b"".join(out), types


def plain_frame(o, planar, lossless):
    """The plain call's frame: lossless_model.encode_frame (every channel alone unless the frame is exactly stereo)."""
    return lossless_model.encode_frame(o, np.ascontiguousarray(planar, np.int32), lossless)


def stream(o, frames, lossless):
    """(bytes uint8[...], offsets uint64[n_frames + 1]) of the paired frames back to back."""
    blobs = [encode_frame(o, x, lossless)[0] for x in frames]
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), offs


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synth_frames():
    """synth_pcm(20 * 2048, 6, track=3) cut into 20 frames, int32 [6, 2048] each."""
    from sela_amd import synth

    pcm = synth.synth_pcm(SYNTH_FRAMES * 2048, SYNTH_CHANNELS, track=SYNTH_TRACK).reshape(SYNTH_FRAMES, 2048, SYNTH_CHANNELS)
    return [np.ascontiguousarray(pcm[f].T.astype(np.int32)) for f in range(SYNTH_FRAMES)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> list of frames, int32 [channels, n]: multichannel frames stacked from the stereo corpus frames
    lossless_model.cases() names (so its tie frames are in them), and frames 8..19 of the synthetic 6-channel track."""
    base = lossless_model.cases()
    a, n300, w = base["A"], base["N300"], base["W"]
    stack = lambda parts: np.ascontiguousarray(np.concatenate(parts))
    return {
        "A6": [stack([a[i], a[(i + 3) % 10], a[(i + 6) % 10]]) for i in range(5)],
        "N300x6": [stack([n300[i], n300[(i + 1) % 4], n300[(i + 2) % 4]]) for i in range(4)],
        "A5": [stack([a[i], a[i + 1], a[i + 2][:1]]) for i in (0, 3, 6)],
        "A3": [stack([a[i], a[i + 1][:1]]) for i in (1, 4, 7)],
        "W4": [stack([w[i], np.ascontiguousarray(lossless_model._wide()[j])]) for i, j in enumerate(W_PARTNERS)],
        "S6": synth_frames()[8:],
    }


MULTI_PAIR = ["A6", "N300x6", "A5", "W4", "S6"]  # the cases with more than one pair per frame
WIDE = ["W4"]  # samples beyond 16 bits: the int32 calls only


def planar(frames):
    """A case's frames as the int32 calls take them: [n_frames, channels, n]."""
    return np.ascontiguousarray(np.stack(frames).astype(np.int32))


def interleaved(frames):
    """A case's frames as the int16 calls take them: [n_frames, n, channels]."""
    return lossless_model.interleaved(frames)
