"""Subframe layouts, shared by the oracle-versus-reference test (test_oracle_topologies.py) and the GPU tests of every kernel
that restates the reference's second pass.  Frames of 2048 samples: k_decode_frames, k_decode_frames_wide, k_verify_frames and
k_verify_compare (test_gpu_decode_topologies.py); k_level_frames, k_digest_frames, k_envelope_frames, k_window_frames and the
cold routes behind the wide kernel (test_gpu_fused_topologies.py); k_window32_decode / k_window32_store
(test_gpu_tail_topologies.py); the first layouts per channel count also the 32-bit verify, levels, envelope and digest tests.
Long last frames of whole-track streams (tailed_stream): the consumers of tail_store_list -- k_tailwin_store, k_whole_store,
k_tail32_store (test_gpu_tail_topologies.py).  Not a test file, and no GPU module is imported here.

frame::FrameDecoder::process (src/frame/frame_decoder.cpp:11-72) decodes the independent subframes first, wherever they stand in
the stream and whatever channel they name, then turns every type-1 subframe into allSamples[parent] - difference.  The
reference's encoder writes one dependent layout only (stereo, channel order, 1 under 0: src/frame/frame_encoder.cpp:18,67);
the cases here are the others: subframes out of channel order, a difference in front of its parent, a parent with the higher
channel number, two differences under one parent, a parent byte on a type-0 subframe -- each at a residue scale of +-300 and
at +-12000, where parent - difference leaves int16 while every subframe still fits the parser's on-chip plan -- and the
layouts this project refuses (BAD_FRAME).

A case is (label, channels, subframes, accepted); subframes are (channel, type, parent, q, residues) tuples in stream order
for wide_cases.frame_bytes."""
import functools
import struct
import zlib

import numpy as np

import wide_cases as wc

N = 2048
PLAN_WORDS = 1072          # kStreamCap: the aligned words of a subframe the segment-parallel parse takes
ORDINARY, WRAPPING, LONG = 300, 12000, 120000
IND, DEP = 0, 1

# ---- layouts: (channel, type, parent) in stream order -------------------------------------------------------------------------
ACCEPTED_LAYOUTS = {
    2: [
        ("independent", [(0, IND, 0), (1, IND, 1)]),
        ("1 under 0", [(0, IND, 0), (1, DEP, 0)]),
        ("0 under 1", [(0, DEP, 1), (1, IND, 1)]),
        ("independent, swapped", [(1, IND, 1), (0, IND, 0)]),
        ("1 under 0, the difference first", [(1, DEP, 0), (0, IND, 0)]),
        ("0 under 1, swapped", [(1, IND, 1), (0, DEP, 1)]),
        ("parent bytes 7 and 200 on type 0", [(0, IND, 7), (1, IND, 200)]),
    ],
    3: [
        # out of channel order; the parent has the higher channel number
        ("2, 0 under 2, 1", [(2, IND, 2), (0, DEP, 2), (1, IND, 1)]),
        # two differences under one parent that stands behind both in the stream
        ("1 and 0 under 2, the parent last", [(1, DEP, 2), (0, DEP, 2), (2, IND, 2)]),
        ("2 and 1 under 0", [(0, IND, 0), (2, DEP, 0), (1, DEP, 0)]),
    ],
    5: [
        ("3, 0 under 3, 4 under 2, 2, 1 under 2", [(3, IND, 3), (0, DEP, 3), (4, DEP, 2), (2, IND, 2), (1, DEP, 2)]),
        ("reversed, 4 and 3 under 0, 2 under 1", [(4, DEP, 0), (3, DEP, 0), (2, DEP, 1), (1, IND, 1), (0, IND, 0)]),
        ("channel order, 0 under 4, 3 under 2, 1 alone", [(0, DEP, 4), (1, IND, 1), (2, IND, 2), (3, DEP, 2), (4, IND, 200)]),
    ],
    8: [
        ("7, 0 and 1 under 7, 6, 2 under 6, 5 under 3, 3, 4 under 3",
         [(7, IND, 7), (0, DEP, 7), (1, DEP, 7), (6, IND, 6), (2, DEP, 6), (5, DEP, 3), (3, IND, 3), (4, DEP, 3)]),
        ("channel order, parents 4, 2 and 6, 1 alone",
         [(0, DEP, 4), (1, IND, 1), (2, IND, 2), (3, DEP, 2), (4, IND, 4), (5, DEP, 6), (6, IND, 6), (7, DEP, 6)]),
        ("reversed, every odd channel under the even one below", [(c, DEP if c & 1 else IND, c - 1 if c & 1 else c) for c in range(7, -1, -1)]),
    ],
    # more than eight channels: stream position p is decoded by wave p % 8 in round p / 8
    9: [
        # 7 (round 0) under 0 (round 1, behind it); 1 under 8 (above it, in front of it); 3 under 2
        ("8, 1 under 8, 2, 3 under 2, 4, 5, 6, 7 under 0, 0",
         [(8, IND, 8), (1, DEP, 8), (2, IND, 2), (3, DEP, 2), (4, IND, 4), (5, IND, 5), (6, IND, 6), (7, DEP, 0), (0, IND, 0)]),
        # 8 (round 1) under 0 (round 0, before it); 0's other dependant 5; 2 under 6 (above it, behind it)
        ("channel order, 8 and 5 under 0, 2 under 6",
         [(0, IND, 0), (1, IND, 1), (2, DEP, 6), (3, IND, 3), (4, IND, 4), (5, DEP, 0), (6, IND, 6), (7, IND, 7), (8, DEP, 0)]),
    ],
    12: [
        # 1 (round 0) under 10 (round 1, above, behind); 9 under 10 too; 8 (round 1) under 0 (round 0, below, before);
        # 5 under 4 (same round, below); 2 under 11 (round 0 under round 1, above)
        ("3, 0, 1 under 10, 2 under 11, 4, 5 under 4, 6, 7, 11, 9 under 10, 10, 8 under 0",
         [(3, IND, 3), (0, IND, 0), (1, DEP, 10), (2, DEP, 11), (4, IND, 4), (5, DEP, 4), (6, IND, 6), (7, IND, 7), (11, IND, 11), (9, DEP, 10),
          (10, IND, 10), (8, DEP, 0)]),
        # reversed: 11 (round 0) under 0 (round 1, the last subframe); 7 and 6 under 0 too; 3 under 4; 1 under 9 (round 1 under round 0)
        ("reversed, 11, 7 and 6 under 0, 3 under 4, 1 under 9",
         [(11, DEP, 0), (10, IND, 10), (9, IND, 9), (8, IND, 8), (7, DEP, 0), (6, DEP, 0), (5, IND, 5), (4, IND, 4), (3, DEP, 4), (2, IND, 2),
          (1, DEP, 9), (0, IND, 0)]),
    ],
}

# one subframe beyond the plan (position in the stream -> scale); the stereo case has a dependent channel
SERIAL_LAYOUTS = {
    2: [("a long parent, 1 under 0", [(0, IND, 0), (1, DEP, 0)], {0: LONG}),
        ("a long difference in front of its parent", [(1, DEP, 0), (0, IND, 0)], {0: LONG})],
    5: [("3, a long 0 under 3, 4 under 2, 2, 1 under 2", [(3, IND, 3), (0, DEP, 3), (4, DEP, 2), (2, IND, 2), (1, DEP, 2)], {1: LONG})],
    12: [("reversed, a long 0 with three dependants", ACCEPTED_LAYOUTS[12][1][1], {11: LONG})],
}

TYPE_2 = 2


def refused_layouts(ch):
    """(label, layout): what k_decode_frames, k_decode_frames_wide and k_verify_frames answer with BAD_FRAME.  The first
    channels keep the layout's point; the rest are independent, in channel order."""
    rest = [(c, IND, c) for c in range(2, ch)]
    out = [
        ("channel 0 twice, channel 1 never", [(0, IND, 0), (0, IND, 0)] + rest),
        ("1 under itself", [(0, IND, 0), (1, DEP, 1)] + rest),
        ("0 under 1 under 0", [(0, DEP, 1), (1, DEP, 0)] + rest),
        ("0 under 1 under 0, swapped", [(1, DEP, 0), (0, DEP, 1)] + rest),
        ("a parent that is no channel", [(0, IND, 0), (1, DEP, ch)] + rest),
        ("parent 255", [(1, DEP, 255), (0, IND, 0)] + rest),
        ("type 2", [(0, IND, 0), (1, TYPE_2, 0)] + rest),
    ]
    if ch >= 3:
        last = ch - 1
        # defined by the reference (test_oracle_topologies.py pins it) and decoded by the 32-bit decoders; the int16 kernels
        # of 2048-sample frames refuse it by policy
        out.append(("a chain in stream order", [(0, IND, 0), (1, DEP, 0)] + rest[:-1] + [(last, DEP, 1)]))
        # the reference subtracts from a vector that is still empty
        out.append(("a chain against stream order", [(last, DEP, 1), (0, IND, 0), (1, DEP, 0)] + rest[:-1]))
    return out


REFUSED_CHANNELS = (2, 5, 12)
CHAIN_IN_STREAM_ORDER = [(0, IND, 0), (1, DEP, 0), (2, DEP, 1)]

# a seed that missed one of the assertions below is replaced here (label -> another seed), never the assertion
_RESEED = {}


def _seed(label):
    return _RESEED.get(label, zlib.crc32(label.encode()))


def subframes(layout, scale, seed, scales=None, n=N):
    """(channel, type, parent, q, residues) tuples of a layout: q 1 to 29 values in [-20, 20), n residues in [-scale, scale)."""
    rng = np.random.default_rng(seed)
    out = []
    for pos, (channel, typ, parent) in enumerate(layout):
        q = rng.integers(-20, 20, size=int(rng.integers(1, 30))).astype(np.int32)
        s = (scales or {}).get(pos, scale)
        out.append((channel, typ, parent, q, rng.integers(-s, s, size=n).astype(np.int32)))
    return out


def subframe_words(blob, ch):
    """aligned words (coefficient words + 2 + residue words) of every subframe of one frame, in stream order"""
    out, p = [], 4
    for _ in range(ch):
        cw = struct.unpack_from("<H", blob, p + 4)[0]
        rw = struct.unpack_from("<H", blob, p + 7 + 4 * cw + 1)[0]
        out.append(cw + 2 + rw)
        p += 12 + 4 * (cw + rw)
    assert p == len(blob)
    return out


def dependent_channels(subs):
    return sorted({s[0] for s in subs if s[1] == DEP})


def parent_channels(subs):
    return sorted({s[2] for s in subs if s[1] == DEP})


def unrelated_channels(subs):
    """channels that neither are nor have a dependant"""
    taken = set(dependent_channels(subs)) | set(parent_channels(subs))
    return sorted({s[0] for s in subs} - taken)


def _wrapped(o, blob, subs, ch):
    """per dependent channel: the values of the reference's int32 result outside int16"""
    dec, used = o.frame_decode_i32(blob, ch)
    assert used == len(blob)
    return {c: (dec[c] < -32768) | (dec[c] > 32767) for c in dependent_channels(subs)}


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, the module's own conditions asserted by the oracle alone -> tuple of (label, channels, subframes, accepted)."""
    from oracle_lib import oracle

    o = oracle()
    out = []
    both_halves = 0
    for ch, layouts in ACCEPTED_LAYOUTS.items():
        for name, layout in layouts:
            for scale in (ORDINARY, WRAPPING):
                label = f"{ch}ch {name} +-{scale}"
                subs = subframes(layout, scale, _seed(label))
                if scale == WRAPPING:
                    blob = wc.frame_bytes(o, subs)
                    words = subframe_words(blob, ch)
                    assert max(words) <= PLAN_WORDS, (label, words)
                    if dependent_channels(subs):
                        wrapped = _wrapped(o, blob, subs, ch)
                        assert any(w.any() for w in wrapped.values()), label
                        if ch == 2:  # both 16-bit halves of one packed word (samples 2 i and 2 i + 1) wrap
                            both_halves += int(any((w[0::2] & w[1::2]).any() for w in wrapped.values()))
                out.append((label, ch, subs, True))
    assert both_halves >= 3, both_halves
    for ch, layouts in SERIAL_LAYOUTS.items():
        for name, layout, scales in layouts:
            label = f"{ch}ch {name}"
            subs = subframes(layout, ORDINARY, _seed(label), scales)
            words = subframe_words(wc.frame_bytes(o, subs), ch)
            for pos in range(ch):
                assert (words[pos] > PLAN_WORDS) == (pos in scales), (label, words)
            out.append((label, ch, subs, True))
    for ch in REFUSED_CHANNELS:
        for name, layout in refused_layouts(ch):
            label = f"{ch}ch refused: {name}"
            out.append((label, ch, subframes(layout, ORDINARY, _seed(label)), False))
    return tuple(out)


def accepted(ch):
    return [c for c in cases() if c[1] == ch and c[3]]


def refused(ch):
    return [c for c in cases() if c[1] == ch and not c[3]]


def accepted_channels():
    return sorted(ACCEPTED_LAYOUTS)


@functools.lru_cache(maxsize=None)
def accepted_stream(ch):
    """All accepted cases of one channel count as one stream -> (cases, blobs, stream uint8, offsets uint64, oracle PCM int16
    [frames, 2048, ch]).  The PCM is the oracle's (pinned to the reference by test_oracle_topologies.py); treat it as read-only."""
    from oracle_lib import oracle

    o = oracle()
    cs = accepted(ch)
    blobs = [wc.frame_bytes(o, c[2]) for c in cs]
    return (cs,) + _stream(o, blobs, ch)


@functools.lru_cache(maxsize=None)
def refused_stream(ch):
    """Every refused case of one channel count between two accepted ones -> (cases, accepted mask bool [frames], stream, offsets,
    oracle PCM); the PCM of a refused frame is whatever the oracle makes of it and stands for nothing."""
    from oracle_lib import oracle

    o = oracle()
    bad = refused(ch)
    good = [c for c in accepted(ch) if f"+-{ORDINARY}" in c[0]]
    cs = [good[0]]
    for i, c in enumerate(bad):
        cs += [c, good[(i + 1) % len(good)]]
    blobs = [wc.frame_bytes(o, c[2]) for c in cs]
    mask = np.array([c[3] for c in cs], bool)
    return (cs, mask) + _stream(o, blobs, ch)


def _stream(o, blobs, ch):
    stream = np.frombuffer(b"".join(blobs), np.uint8).copy()
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    pcm = np.stack([o.frame_decode(b, ch)[0] for b in blobs])
    for a in (stream, offs, pcm):
        a.setflags(write=False)
    return stream, offs, pcm


# ---- whole-track streams: two frames of 2048 samples and a long last frame ----------------------------------------------------
TAIL_CHANNELS = (2, 3, 5, 8)
TAIL_LENGTHS = (2049, 2825, 4095)   # both ends of a last frame's range (2049 .. 4095) and one inside
# the last frame's layout: none is channel order with 1 under 0, which is all an encoder writes
TAIL_LAYOUTS = {
    2: ("1 under 0, the difference first", [(1, DEP, 0), (0, IND, 0)]),
    3: ACCEPTED_LAYOUTS[3][1],
    5: ACCEPTED_LAYOUTS[5][0],
    8: ACCEPTED_LAYOUTS[8][0],
}


def chain_layout(ch):
    """CHAIN_IN_STREAM_ORDER and independent subframes in channel order behind it"""
    return CHAIN_IN_STREAM_ORDER + [(c, IND, c) for c in range(3, ch)]


def tail_subframes(ch, n_last, scale=ORDINARY, chain=False):
    """-> (label, subframes) of the last frame of tailed_stream(ch, n_last, scale, chain)"""
    name, layout = ("a chain in stream order", chain_layout(ch)) if chain else TAIL_LAYOUTS[ch]
    label = f"{ch}ch last frame of {n_last}: {name} +-{scale}"
    return label, subframes(layout, scale, _seed(label), n=n_last)


@functools.lru_cache(maxsize=None)
def _tailed(ch, n_last, scale, chain):
    from oracle_lib import oracle

    o = oracle()
    assert ch in TAIL_CHANNELS and N < n_last < 2 * N and (ch >= 3 or not chain)
    front = [c for c in accepted(ch) if f"+-{ORDINARY}" in c[0]][:2]
    label, subs = tail_subframes(ch, n_last, scale, chain)
    last = wc.frame_bytes(o, subs)
    blobs = [wc.frame_bytes(o, c[2]) for c in front] + [last]
    dec, used = o.frame_decode_i32(last, ch)
    assert used == len(last) and all(len(d) == n_last for d in dec), label
    if scale == WRAPPING:
        assert any(((dec[c] < -32768) | (dec[c] > 32767)).any() for c in dependent_channels(subs)), label
    stream = np.frombuffer(b"".join(blobs), np.uint8).copy()
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    parts, wide = [], []
    for b, n in zip(blobs, (N, N, n_last)):
        pcm, used = o.frame_decode(b, ch, n=n)
        assert used == len(b), label
        parts.append(pcm)
        wide.append(np.stack(o.frame_decode_i32(b, ch)[0], axis=1))
    pcm, pcm32 = np.concatenate(parts), np.concatenate(wide)
    assert pcm.shape == pcm32.shape == (2 * N + n_last, ch)
    for a in (stream, offs, pcm, pcm32):
        a.setflags(write=False)
    return stream, offs, pcm, pcm32


def tailed_stream(ch, n_last, scale=ORDINARY, chain=False):
    """The first two +-300 frames of accepted(ch), then one last frame of n_last samples in TAIL_LAYOUTS[ch] (chain: in
    chain_layout(ch)) -> (stream uint8, offsets uint64 [4], oracle PCM int16 [4096 + n_last, ch]).  At +-12000 a dependent channel
    of the last frame leaves int16 (asserted from the oracle's int32 decode, as cases() does).  Cached and read-only."""
    return _tailed(ch, n_last, scale, chain)[:3]


def tailed_stream_i32(ch, n_last, scale=ORDINARY, chain=False):
    """The oracle's int32 samples of the same stream, int32 [4096 + n_last, ch]: parent - difference kept, not wrapped."""
    return _tailed(ch, n_last, scale, chain)[3]
