"""What tests/test_salvage_unaligned_cpu.py and tests/test_gpu_salvage_unaligned.py share: a model of the any-byte salvage rule
(include/sela_hip.h, "salvage at any byte") written from its definition, and the damages that move frames off the word grid.
Not a test module.  Frames, streams and the word-position damages: tests/salvage_cases.py."""
import bisect

import numpy as np

from salvage_cases import SYNC_BYTES, Stream, crafted_frame, frame_end, plant_fake


# ---- the model ---------------------------------------------------------------------------------------------------------------
def candidates(buf, channels):
    """{byte offset b: end(b)} of every candidate of the payload."""
    buf = bytes(buf)
    ends = {}
    at = buf.find(SYNC_BYTES)
    while at >= 0:
        e = frame_end(buf, at, channels)  # (salvage_cases.frame_end reads at any byte offset)
        if e:
            ends[at] = e
        at = buf.find(SYNC_BYTES, at + 1)
    return ends


def model(buf, channels, max_frames):
    """The rule, from the list of all candidates: -> (records as (offset, skipped_before, bytes) tuples, totals list of 4)."""
    buf = bytes(buf)
    B = len(buf)
    ends = candidates(buf, channels) if 1 <= channels <= 255 else {}
    confirmed = sorted(b for b, e in ends.items() if B - e < 4 or e in ends)
    records, p = [], 0
    while len(records) < max_frames:
        if p in ends:
            q = p
        else:
            k = bisect.bisect_left(confirmed, p)
            if k == len(confirmed):
                break
            q = confirmed[k]
        records.append((q, q - p, ends[q] - q))
        p = ends[q]
    totals = [len(records), sum(1 for r in records if r[1]), sum(r[2] for r in records), records[-1][0] + records[-1][2] if records else 0]
    return records, totals


# ---- streams and damages -----------------------------------------------------------------------------------------------------
def rice_stream(channels, n=12, words=(3, 1, 5, 2)):
    """n crafted frames of 4 + 12 channels bytes plus a few Rice words each (lengths differ from frame to frame)."""
    return Stream([crafted_frame(channels, rice_words=words[f % len(words)], tag=f) for f in range(n)], channels)


def garbage(n, seed=0):
    """n bytes none of which is a byte of the sync word: no window that touches them holds it."""
    return bytes(np.random.default_rng(1000 + 16 * n + seed).integers(1, 0x50, n, dtype=np.uint8))


def insert(payload, at, extra):
    """The payload (uint8 array) with bytes `extra` put in front of byte `at`."""
    return np.concatenate([payload[:at], np.frombuffer(extra, np.uint8), payload[at:]]).astype(np.uint8)


def delete(payload, at, n):
    return np.concatenate([payload[:at], payload[at + n:]]).astype(np.uint8)


def concatenated(a, b, channels):
    """Stream a's payload, then a whole second FILE: its 15-byte header ('SeLa', rate, bits, channels, frames) and b's payload."""
    header = b"SeLa" + (44100).to_bytes(4, "little") + (16).to_bytes(2, "little") + bytes([channels]) + (len(b.offs) - 1).to_bytes(4, "little")
    assert len(header) == 15 and SYNC_BYTES not in header
    return np.concatenate([a.payload(), np.frombuffer(header, np.uint8), b.payload()])


def fake_at_odd_phase(stream, f, confirmed, shift=1):
    """`shift` bytes of garbage in front of frame f, frames f and f + 1 without their sync words, and a fake 4 bytes into frame f
    that ends on frame f + 2 (confirmed) or 4 bytes into frame f + 1 (a place that holds no sync word).  -> (payload, the fake's
    offset): the fake and everything behind it sit `shift` bytes off the word grid."""
    s = stream.copy()
    s.buf[s.offs[f]] ^= 0xFF
    s.buf[s.offs[f + 1]] ^= 0xFF
    at = s.offs[f] + 4
    plant_fake(s.buf, at, s.channels, s.offs[f + 2] if confirmed else max(s.offs[f + 1] + 4, at + 4 + 12 * s.channels))
    return insert(s.payload(), s.offs[f], garbage(shift)), at + shift
