"""What tests/test_salvage_cpu.py and tests/test_gpu_salvage.py share: a model of the salvage rule (include/sela_hip.h, "salvage")
written from its definition with the byte reader, crafted frames, and the damage cases.  Not a test module."""
import bisect
import itertools
import struct

import numpy as np

SYNC = 0xAA55FF00
SYNC_BYTES = struct.pack("<I", SYNC)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def _subframe_end(buf, B, p):
    """sela_subframe_read_bytes: the byte behind the subframe whose header starts at p, or 0 when it runs past B."""
    if p + 12 > B:
        return 0
    cw = buf[p + 4] | (buf[p + 5] << 8)
    q = p + 7 + 4 * cw
    if q + 5 > B:
        return 0
    rw = buf[q + 1] | (buf[q + 2] << 8)
    nxt = q + 5 + 4 * rw
    return nxt if nxt <= B else 0


def frame_end(buf, off, channels):
    """end(w) for w = off / 4, or 0 when off is no candidate."""
    B = len(buf)
    if off + 4 > B or bytes(buf[off:off + 4]) != SYNC_BYTES:
        return 0
    p = off + 4
    for _ in range(channels):
        p = _subframe_end(buf, B, p)
        if not p:
            return 0
    return p


def model(buf, channels, max_frames):
    """The rule, from the list of all candidates: -> (records as (offset, skipped_before, bytes) tuples, totals list of 4)."""
    buf = bytes(buf)
    B = len(buf)
    W = B // 4
    words = np.frombuffer(buf, "<u4", count=W)
    ends = {}
    for w in np.flatnonzero(words == SYNC):
        e = frame_end(buf, 4 * int(w), channels)
        if e:
            ends[int(w)] = e
    confirmed = sorted(w for w, e in ends.items() if e == 4 * W or e // 4 in ends)
    records, p = [], 0
    while len(records) < max_frames:
        if p % 4 == 0 and p // 4 in ends:
            q = p // 4
        else:
            k = bisect.bisect_left(confirmed, (p + 3) // 4)
            if k == len(confirmed):
                break
            q = confirmed[k]
        records.append((4 * q, 4 * q - p, ends[q] - 4 * q))
        p = ends[q]
    totals = [len(records), sum(1 for r in records if r[1]), sum(r[2] for r in records), records[-1][0] + records[-1][2] if records else 0]
    return records, totals


def as_tuples(records):
    """SALVAGED_DTYPE records -> the model's tuples (reserved must be 0)."""
    assert not np.any(records["reserved"])
    return [(int(r["offset"]), int(r["skipped_before"]), int(r["bytes"])) for r in records]


# ---- crafted frames ----------------------------------------------------------------------------------------------------------
def crafted_frame(channels, rice_words=0, tag=0, fill=0x5A):
    """A frame of `channels` subframes without coefficient words, the first with `rice_words` words of Rice data (bytes `fill`,
    never the sync word): 4 + 12 channels + 4 rice_words bytes.  cw = rw = 0 and 4 + 12 channels bytes by default."""
    out = bytearray(SYNC_BYTES)
    for c in range(channels):
        rw = rice_words if c == 0 else 0
        out += bytes([c & 0xFF, 0, 0, 3]) + struct.pack("<H", 0) + bytes([0]) + bytes([5]) + struct.pack("<HH", rw, (tag + c) & 0xFFFF)
        out += bytes([fill]) * (4 * rw)
    return bytes(out)


def plant_fake(buf, at, channels, end):
    """A sync word and `channels` headers at byte `at` whose frame would end at byte `end` (the last subframe takes the words)."""
    rw = end - at - 4 - 12 * channels
    assert rw >= 0 and rw % 4 == 0 and rw // 4 <= 65535 and end <= len(buf)
    head = bytearray(SYNC_BYTES)
    for c in range(channels):
        head += bytes([c & 0xFF, 0, 0, 0, 0, 0, 0, 0]) + struct.pack("<HH", rw // 4 if c == channels - 1 else 0, 7)
    buf[at:at + len(head)] = head


class Stream:
    """Frames back to back: the bytes, where each frame starts (and the end), the channel count."""

    def __init__(self, frames, channels):
        self.buf = bytearray(b"".join(frames))
        self.offs = list(itertools.accumulate([0] + [len(f) for f in frames]))
        self.channels = channels
        self.cut = None     # truncation, applied after the in-place damage
        self.prefix = b""   # garbage in front, applied last

    def copy(self):
        s = Stream([], self.channels)
        s.buf, s.offs, s.cut, s.prefix = bytearray(self.buf), list(self.offs), self.cut, self.prefix
        return s

    def rice(self, f):
        """(first byte, words) of frame f's first subframe's Rice data."""
        p = self.offs[f] + 4
        cw = self.buf[p + 4] | (self.buf[p + 5] << 8)
        q = p + 7 + 4 * cw
        return q + 5, self.buf[q + 1] | (self.buf[q + 2] << 8)

    def payload(self):
        body = self.buf if self.cut is None else self.buf[:self.cut]
        return np.frombuffer(self.prefix + bytes(body), np.uint8).copy()


# ---- damage: name -> function(Stream), for a stream of 12 frames ------------------------------------------------------------
def _flip(f):
    def op(s):
        s.buf[s.offs[f]] ^= 0xFF
    return op


def _zero_rice(f):
    def op(s):
        at, rw = s.rice(f)
        s.buf[at + 4:at + 4 * min(rw, 12) - 4] = bytes(max(4 * min(rw, 12) - 8, 0))
    return op


def _zero_header(f):
    def op(s):
        lo = max(s.offs[f] - 8, 0)
        s.buf[lo:s.offs[f] + 16] = bytes(s.offs[f] + 16 - lo)
    return op


def _cut_header(f, phase):
    def op(s):
        at = s.offs[f] + 8  # inside frame f's first header
        s.cut = at + (phase - at) % 4
    return op


def _cut_rice(f, phase):
    def op(s):
        at, rw = s.rice(f)
        at += 4 * (rw // 2)
        s.cut = at + (phase - at) % 4
    return op


def _prefix(words):
    def op(s):
        rng = np.random.default_rng(words)
        s.prefix = (rng.integers(0, 0xAA000000, words, dtype=np.uint32)).astype("<u4").tobytes()  # (never the sync word)
    return op


def _fake(f, confirmed):
    """Frames f and f + 1 lose their sync words; a fake starts one word into the gap and ends on frame f + 2 (confirmed: it is
    taken) or one word past the start of frame f + 1 (a place that holds no sync word: it is skipped)."""
    def op(s):
        s.buf[s.offs[f]] ^= 0xFF
        s.buf[s.offs[f + 1]] ^= 0xFF
        at = s.offs[f] + 4
        end = s.offs[f + 2] if confirmed else max(s.offs[f + 1] + 4, at + 4 + 12 * s.channels)
        plant_fake(s.buf, at, s.channels, end)
    return op


def damage_cases(has_rice):
    """The single damages; `has_rice`: the frames carry Rice data (the crafted minimal ones do not)."""
    ops = {
        "sync_first": _flip(0), "sync_middle": _flip(5), "sync_last": _flip(11),
        "zero_header": _zero_header(7),
        "adjacent_headers": lambda s: (_flip(2)(s), _flip(3)(s)),
        "intact_between_damaged": lambda s: (_flip(5)(s), _flip(7)(s)),
        "fake_unconfirmed": _fake(8, False), "fake_confirmed": _fake(8, True),
        "garbage_prefix": _prefix(3),
    }
    for phase in range(4):
        ops["cut_header_%d" % phase] = _cut_header(9, phase)
    if has_rice:
        ops["zero_rice"] = _zero_rice(4)
        for phase in range(4):
            ops["cut_rice_%d" % phase] = _cut_rice(9, phase)
    return ops


def damaged(stream, ops, names):
    s = stream.copy()
    for n in names:
        ops[n](s)
    return s


def singles_and_pairs(ops):
    names = sorted(ops)
    return [(n,) for n in names] + [p for p in itertools.combinations(names, 2)
                                    if not (p[0].startswith("cut_") and p[1].startswith("cut_"))]  # (one truncation a payload)
