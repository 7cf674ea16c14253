"""No GPU: sela_hip_salvage_frames_unaligned, the host walk that defines the salvage at any byte (include/sela_hip.h, DESIGN.md
5.33), against a model of the rule written from its definition (tests/salvage_unaligned_cases.py): the word salvage's damage
cases, and the damages that move frames off the word grid -- inserted and deleted bytes, concatenated files -- each beside what
the word salvage makes of the same bytes; the walk alone under ASan + UBSan in a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import salvage_unaligned_cases as ua
from salvage_cases import SYNC_BYTES, as_tuples, damage_cases, damaged, singles_and_pairs
from sela_amd import capi, codec
from test_salvage_cpu import golden_stream, minimal_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sela_hip_salvage_frames_unaligned", "sela_hip_salvage_unaligned_workspace_bytes", "sela_hip_salvage_frames_unaligned_device",
         "sela_hip_salvage_payload_unaligned_device"]


def packed(payload, records):
    return np.concatenate([payload[int(r["offset"]):int(r["offset"]) + int(r["bytes"])] for r in records]) if len(records) else np.zeros(0, np.uint8)


def check_consequences(payload, channels, max_frames, records, totals):
    """What follows from the rule (include/sela_hip.h, "salvage at any byte"), on one result of the walk."""
    n = len(records)
    assert [int(t) for t in totals] == [n, int(np.count_nonzero(records["skipped_before"])), int(records["bytes"].sum()),
                                        int(records["offset"][-1]) + int(records["bytes"][-1]) if n else 0]
    assert int(totals[3]) <= len(payload) and not np.any(records["bytes"] % 4)
    # 1. where the index finds its frames, the salvage finds the same ones without a gap
    offs = codec.index_frames(payload, max_frames, channels) if len(payload) else np.zeros(1, np.uint64)
    found = len(offs) - 1
    assert n >= found and records["offset"][:found].tolist() == offs[:-1].tolist() and not np.any(records["skipped_before"][:found])
    assert (records["offset"][:found] + records["bytes"][:found]).tolist() == offs[1:].tolist()
    # 2. offsets strictly increase, frames never overlap, and the gaps are what lies between them
    ends = records["offset"] + records["bytes"]
    before = np.concatenate([[0], ends[:-1]]).astype(np.uint64)
    assert np.all(records["bytes"] > 0) and np.all(records["offset"] >= before) and (records["offset"] - before).tolist() == records["skipped_before"].tolist()
    # 3. the taken frames back to back: the index reads them to the last byte, and BOTH salvages take them whole with no gap
    body = packed(payload, records)
    if n:
        again = codec.index_frames(body, n + 1, channels)
        assert again.tolist() == np.concatenate([[0], np.cumsum(records["bytes"], dtype=np.uint64)]).tolist()
    for unaligned in (False, True):
        rec2, tot2 = codec.salvage_frames(body, channels, n + 1, unaligned=unaligned)
        assert rec2["bytes"].tolist() == records["bytes"].tolist() and not np.any(rec2["skipped_before"]) and int(tot2[3]) == len(body)


def walk_and_check(payload, channels, max_frames=64):
    records, totals = codec.salvage_frames(payload, channels, max_frames, unaligned=True)
    want, want_totals = ua.model(payload.tobytes(), channels, max_frames)
    assert as_tuples(records) == want and [int(t) for t in totals] == want_totals
    check_consequences(payload, channels, max_frames, records, totals)
    return records, totals


def test_the_calls_are_declared_and_exported():
    import __graft_entry__ as entry

    assert all(n in capi.EXPORTS for n in NAMES)
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES)
    assert "sela_salvage_unaligned.hip" in entry.HIP_SOURCES


def test_an_intact_stream_is_the_index_and_the_word_salvage(kats):
    for s in [golden_stream(kats)] + [ua.rice_stream(c) for c in (1, 2, 3, 255)]:
        for cap in (0, 1, 11, 12, 13, 1000):
            records, totals = walk_and_check(s.payload(), s.channels, cap)
            word, word_totals = codec.salvage_frames(s.payload(), s.channels, cap)
            assert as_tuples(records) == as_tuples(word) and totals.tolist() == word_totals.tolist()
            assert records["offset"].tolist() == s.offs[:min(cap, 12)] and int(totals[1]) == 0
        records, totals = codec.salvage_frames(s.payload(), s.channels, unaligned=True)  # the default cap: what the bytes could hold
        assert len(records) == 12 and int(totals[3]) == len(s.buf)


STREAMS = ["golden", "minimal1", "minimal2", "minimal3", "rice2"]


def _stream(name, kats):
    return golden_stream(kats) if name == "golden" else ua.rice_stream(2) if name == "rice2" else minimal_stream(int(name[7:]))


@pytest.mark.parametrize("name", STREAMS)
def test_every_word_damage_singly_and_in_pairs_is_the_model(name, kats):
    base = _stream(name, kats)
    ops = damage_cases(has_rice=name in ("golden", "rice2"))
    for case in singles_and_pairs(ops):
        s = damaged(base, ops, case)
        try:
            walk_and_check(s.payload(), s.channels)
        except AssertionError as e:
            raise AssertionError("%s %s: %s" % (name, case, e)) from e


@pytest.mark.parametrize("channels", [2, 1, 3])
@pytest.mark.parametrize("extra", [1, 2, 3, 5, 15])
def test_inserted_garbage_loses_nothing_here_and_everything_behind_it_there(channels, extra):
    """THE assertion of the feature: sync-free garbage between frames f - 1 and f.  Every frame is taken with one gap of that
    length; sela_hip_salvage_frames on the same bytes stops at f."""
    s = ua.rice_stream(channels)
    for f in (1, 5, 11):
        payload = ua.insert(s.payload(), s.offs[f], ua.garbage(extra, f))
        records, totals = walk_and_check(payload, channels)
        assert records["offset"].tolist() == s.offs[:f] + [o + extra for o in s.offs[f:12]]
        assert records["skipped_before"].tolist() == [0] * f + [extra] + [0] * (11 - f) and totals.tolist() == [12, 1, len(s.buf), len(payload)]
        word, word_totals = codec.salvage_frames(payload, channels, 64)
        assert word["offset"].tolist() == s.offs[:f] and int(word_totals[0]) == f, "the word salvage loses everything behind the insertion"
        assert packed(payload, records).tobytes() == bytes(s.buf)


def test_two_insertions_of_different_phases():
    s = ua.rice_stream(2)
    for a, b in ((1, 2), (3, 3), (2, 5), (1, 3)):  # (1 + 3: the frames behind both are back on the word grid)
        payload = ua.insert(ua.insert(s.payload(), s.offs[8], ua.garbage(b, 1)), s.offs[3], ua.garbage(a))
        records, totals = walk_and_check(payload, 2)
        assert records["offset"].tolist() == s.offs[:3] + [o + a for o in s.offs[3:8]] + [o + a + b for o in s.offs[8:12]]
        assert totals.tolist() == [12, 2, len(s.buf), len(payload)] and int(records["skipped_before"][3]) == a and int(records["skipped_before"][8]) == b
        assert len(codec.salvage_frames(payload, 2, 64)[0]) == (3 if (a + b) % 4 else 3 + 4)


def test_a_garbage_prefix_of_any_length():
    s = ua.rice_stream(2)
    for n in (1, 2, 3):
        payload = ua.insert(s.payload(), 0, ua.garbage(n))
        records, totals = walk_and_check(payload, 2)
        assert records["offset"].tolist() == [o + n for o in s.offs[:12]] and int(records["skipped_before"][0]) == n and int(totals[1]) == 1
        assert len(codec.salvage_frames(payload, 2, 64)[0]) == 0


def test_two_files_concatenated():
    """`cat a.sela b.sela`: the second file's 15-byte header puts its frames at phase 3."""
    a, b = ua.rice_stream(2, 12), ua.rice_stream(2, 7, words=(2, 4))
    payload = ua.concatenated(a, b, 2)
    records, totals = walk_and_check(payload, 2)
    assert records["offset"].tolist() == a.offs[:12] + [len(a.buf) + 15 + o for o in b.offs[:7]]
    assert totals.tolist() == [19, 1, len(a.buf) + len(b.buf), len(payload)] and int(records["skipped_before"][12]) == 15
    assert len(codec.salvage_frames(payload, 2, 64)[0]) == 12


def test_bytes_deleted_inside_a_frame_the_stated_limit():
    """Limit, as the header states it: a trusted frame whose length field is wrong sends the walk astray.  Frame 4 loses 1 .. 3
    bytes of its LAST subframe's Rice data (mono: the only one); its headers still fit, so it is taken at its full announced
    length, with the head of frame 5 in it, and frame 5 is lost.  Where the bytes go missing in front of a later subframe's header
    (stereo: the first subframe's Rice data), frame 4 is no candidate any more: it alone is lost."""
    s = ua.rice_stream(1)
    for n in (1, 2, 3):
        payload = ua.delete(s.payload(), s.rice(4)[0] + 1, n)
        records, totals = walk_and_check(payload, 1)
        assert records["offset"].tolist() == s.offs[:5] + [o - n for o in s.offs[6:12]], "frame 5 is lost"
        assert int(records["bytes"][4]) == s.offs[5] - s.offs[4] and int(records["skipped_before"][5]) == s.offs[6] - s.offs[5] - n
        assert packed(payload, records)[s.offs[5] - n:s.offs[5]].tobytes() == SYNC_BYTES[:n], "frame 4 holds the head of frame 5"
        assert len(codec.salvage_frames(payload, 1, 64)[0]) == 5
    s = ua.rice_stream(2)
    for n in (1, 2, 3):
        payload = ua.delete(s.payload(), s.rice(4)[0] + 1, n)
        records, totals = walk_and_check(payload, 2)
        assert records["offset"].tolist() == s.offs[:4] + [o - n for o in s.offs[5:12]] and int(records["skipped_before"][4]) == s.offs[5] - s.offs[4] - n
        assert len(codec.salvage_frames(payload, 2, 64)[0]) == 4


def test_a_fake_sync_word_at_an_odd_phase():
    s = ua.rice_stream(2)
    for shift in (1, 2, 3):
        payload, at = ua.fake_at_odd_phase(s, 8, True, shift)
        records, _ = walk_and_check(payload, 2)
        assert records["offset"].tolist() == s.offs[:8] + [at] + [o + shift for o in s.offs[10:12]], "a fake that ends on a candidate is taken: the rule"
        assert at % 4 == shift and int(records["skipped_before"][8]) == 4 + shift
        payload, at = ua.fake_at_odd_phase(s, 8, False, shift)
        records, _ = walk_and_check(payload, 2)
        assert records["offset"].tolist() == s.offs[:8] + [o + shift for o in s.offs[10:12]], "a fake whose end is no candidate is skipped"


def test_truncation_at_every_phase():
    """B - end < 4 confirms: frame 9, behind a damaged frame 8 and `shift` bytes off the grid, ends 0 .. 3 bytes before the
    payload does and is taken; with 4 bytes or more behind it nothing confirms it."""
    s = ua.rice_stream(2)
    for shift in range(4):
        whole = ua.insert(s.payload(), s.offs[2], ua.garbage(shift)) if shift else s.payload()
        whole[s.offs[8] + shift] ^= 0xFF
        for tail in range(8):
            payload = np.concatenate([whole[:s.offs[10] + shift], np.frombuffer(ua.garbage(tail), np.uint8)]).astype(np.uint8)
            records, totals = walk_and_check(payload, 2)
            want = s.offs[:2] + [o + shift for o in s.offs[2:8]] + ([s.offs[9] + shift] if tail < 4 else [])
            assert records["offset"].tolist() == want and len(payload) - int(totals[3]) == (tail if tail < 4 else len(payload) - s.offs[8] - shift)


def test_payloads_without_a_frame():
    for n in range(20):
        for fill in (b"", SYNC_BYTES):
            body = (fill * 5)[:n] if fill else bytes(n)
            records, totals = walk_and_check(np.frombuffer(body, np.uint8).copy(), 1, 8)
            assert len(records) == 0 and totals.tolist() == [0, 0, 0, 0]
    for back in range(1, 8):  # a lone sync word (or as much of it as fits) at each of the last 7 byte positions
        for n in (16, 17, 18, 19, 40):
            body = bytearray(n)
            body[n - back:] = SYNC_BYTES[:back]
            records, _ = walk_and_check(np.frombuffer(bytes(body[:n]), np.uint8).copy(), 1, 8)
            assert len(records) == 0
    # null outputs are allowed, channel counts the format cannot say find nothing
    frame = np.frombuffer(b"\x11" + ua.crafted_frame(1), np.uint8).copy()
    lib = capi.lib()
    assert lib.sela_hip_salvage_frames_unaligned(frame.ctypes.data, frame.nbytes, 4, 1, None, None) == 1
    assert lib.sela_hip_salvage_frames_unaligned(frame.ctypes.data, frame.nbytes, 4, 0, None, None) == 0
    assert lib.sela_hip_salvage_frames_unaligned(frame.ctypes.data, frame.nbytes, 4, 256, None, None) == 0


def test_the_workspace_formula_and_the_refusals_need_no_gpu():
    """include/sela_hip.h: 9 up(4 W) + 2 up(4 (K + 1)) + 3 up(4 F) + 5 * 256 + 256 -- one entry per WORD, no more than the word
    salvage's; a payload of 2^32 bytes or more is refused before anything touches a device."""
    lib = capi.lib()

    def up(b):
        return (b + 255) // 256 * 256

    for n_bytes, cap in ((0, 0), (3, 5), (4, 1), (17, 1), (35003, 12), (81920, 4096), (81923, 4097), (4096 * 4 + 5, 7), (22_800_001, 3875), ((1 << 32) - 1, 1 << 28)):
        W = n_bytes // 4
        K, F = (W + 4095) // 4096, min(cap, W)
        want = 9 * up(4 * W) + 2 * up(4 * (K + 1)) + 3 * up(4 * F) + 5 * 256 + 256
        assert int(lib.sela_hip_salvage_unaligned_workspace_bytes(n_bytes, cap)) == want, (n_bytes, cap)
        assert want == codec.salvage_workspace_bytes(n_bytes, cap) == codec.salvage_workspace_bytes(n_bytes, cap, unaligned=True)
    fake, einval = 1 << 20, -2  # (pointers nobody follows: the checks come first)
    assert capi.ERRORS[einval] == "EINVAL"
    for n_bytes in (1 << 32, (1 << 32) + 4, 1 << 34):
        assert lib.sela_hip_salvage_frames_unaligned_device(fake, n_bytes, 8, 2, fake, fake, fake, 1 << 62, None) == einval
        assert b"4 GiB" in lib.sela_hip_last_error()
        assert lib.sela_hip_salvage_payload_unaligned_device(fake, n_bytes, 8, 2, fake + (1 << 40), 64, fake, None, fake, fake, 1 << 62, None) == einval
    # the other refusals, in the word calls' order and with their codes
    assert lib.sela_hip_salvage_frames_unaligned_device(fake, 64, 8, 0, fake, fake, fake, 1 << 30, None) == einval
    assert lib.sela_hip_salvage_frames_unaligned_device(fake, 64, 8, 2, fake, None, fake, 1 << 30, None) == einval
    assert lib.sela_hip_salvage_frames_unaligned_device(fake + 2, 64, 8, 2, fake, fake, fake, 1 << 30, None) == einval
    assert lib.sela_hip_salvage_payload_unaligned_device(fake, 64, 8, 2, fake + 4096 + 1, 64, fake, None, fake, fake, 1 << 30, None) == einval
    assert lib.sela_hip_salvage_payload_unaligned_device(fake, 64, 8, 2, fake + 32, 64, fake, None, fake, fake, 1 << 30, None) == einval
    assert b"overlap" in lib.sela_hip_last_error()
    assert lib.sela_hip_salvage_frames_unaligned_device(fake, 64, 8, 2, fake, fake, fake, codec.salvage_workspace_bytes(64, 8, True) - 1, None) == -4


def test_the_walk_stand_alone_under_asan_and_ubsan(tmp_path):
    """tests/c/salvage_walk_unaligned.cpp: sela_amd/csrc/sela_salvage_walk_unaligned.h alone under -fsanitize=address,undefined,
    run directly -- every truncation of streams with inserted bytes in a heap buffer of exactly that many bytes, at each of
    the four alignments, so that a read past the end traps."""
    from test_pcm_cpu import _compile

    exe = _compile(tmp_path, "salvage_walk_unaligned", [os.path.join(ROOT, "tests", "c", "salvage_walk_unaligned.cpp")],
                   ["-I" + os.path.join(ROOT, "sela_amd", "csrc"), "-I" + os.path.join(ROOT, "include")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "salvage_walk_unaligned: 0 failures" in out.stdout and "runtime error" not in out.stderr \
        and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr
