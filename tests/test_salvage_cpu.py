"""No GPU: sela_hip_salvage_frames, the host walk that defines the salvage of a damaged payload (include/sela_hip.h, DESIGN.md
5.30), against a model of the rule written from its definition (tests/salvage_cases.py), on golden and crafted streams under
every damage case singly and in pairs, with the three consequences the header states checked on every one; the walk alone
under ASan + UBSan in a stand-alone program on exactly-sized heap buffers."""
import os
import subprocess

import numpy as np
import pytest

from salvage_cases import Stream, as_tuples, crafted_frame, damage_cases, damaged, frame_end, model, singles_and_pairs
from sela_amd import capi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sela_hip_salvage_frames", "sela_hip_salvage_workspace_bytes", "sela_hip_salvage_frames_device", "sela_hip_salvage_payload_device"]


def golden_stream(kats):
    blobs = [kats["frame/stereo_same_sine/bytes"].tobytes(), kats["frame/stereo_synth_diff/bytes"].tobytes(), kats["frame/stereo_silence/bytes"].tobytes()]
    return Stream(blobs * 4, 2)


def minimal_stream(channels):
    return Stream([crafted_frame(channels, tag=f) for f in range(12)], channels)


def check_consequences(payload, channels, max_frames, records, totals):
    """What follows from the rule (include/sela_hip.h), on one result of the walk."""
    n = len(records)
    assert [int(t) for t in totals] == [n, int(np.count_nonzero(records["skipped_before"])), int(records["bytes"].sum()),
                                        int(records["offset"][-1]) + int(records["bytes"][-1]) if n else 0]
    assert int(totals[3]) <= len(payload)
    # 1. where the index finds its frames, the salvage finds the same ones without a gap
    offs = codec.index_frames(payload, max_frames, channels) if len(payload) else np.zeros(1, np.uint64)
    found = len(offs) - 1
    assert n >= found and records["offset"][:found].tolist() == offs[:-1].tolist() and not np.any(records["skipped_before"][:found])
    assert (records["offset"][:found] + records["bytes"][:found]).tolist() == offs[1:].tolist()
    # 2. offsets strictly increase, frames never overlap, and the gaps are what lies between them
    ends = records["offset"] + records["bytes"]
    before = np.concatenate([[0], ends[:-1]]).astype(np.uint64)
    assert np.all(records["bytes"] > 0) and np.all(records["offset"] >= before) and (records["offset"] - before).tolist() == records["skipped_before"].tolist()
    # 3. the taken frames back to back are a payload the index reads to its end, and salvaging it again changes nothing
    packed = np.concatenate([payload[int(r["offset"]):int(r["offset"]) + int(r["bytes"])] for r in records]) if n else np.zeros(0, np.uint8)
    if n:
        again = codec.index_frames(packed, n + 1, channels)
        assert again.tolist() == np.concatenate([[0], np.cumsum(records["bytes"], dtype=np.uint64)]).tolist()
    rec2, tot2 = codec.salvage_frames(packed, channels, n + 1)
    assert rec2["bytes"].tolist() == records["bytes"].tolist() and not np.any(rec2["skipped_before"]) and int(tot2[3]) == len(packed)


def walk_and_check(payload, channels, max_frames):
    records, totals = codec.salvage_frames(payload, channels, max_frames)
    want, want_totals = model(payload.tobytes(), channels, max_frames)
    assert as_tuples(records) == want and [int(t) for t in totals] == want_totals
    check_consequences(payload, channels, max_frames, records, totals)
    return records, totals


def test_the_calls_are_declared_and_exported():
    assert all(n in capi.EXPORTS for n in NAMES)
    lib = capi.lib()
    assert all(hasattr(lib, n) for n in NAMES)
    assert codec.SALVAGED_DTYPE.itemsize == 24


def test_an_intact_stream_is_the_index(kats):
    for s in [golden_stream(kats)] + [minimal_stream(c) for c in (1, 2, 3, 255)]:
        for cap in (0, 1, 11, 12, 13, 1000):
            records, totals = walk_and_check(s.payload(), s.channels, cap)
            assert records["offset"].tolist() == s.offs[:min(cap, 12)] and int(totals[1]) == 0
        records, totals = codec.salvage_frames(s.payload(), s.channels)  # the default cap: what the bytes could hold
        assert len(records) == 12 and int(totals[3]) == len(s.buf)


STREAMS = ["golden", "minimal1", "minimal2", "minimal3", "minimal255"]


def _stream(name, kats):
    return golden_stream(kats) if name == "golden" else minimal_stream(int(name[7:]))


@pytest.mark.parametrize("name", STREAMS)
def test_every_damage_singly_and_in_pairs_is_the_model(name, kats):
    base = _stream(name, kats)
    ops = damage_cases(has_rice=name == "golden")
    for case in singles_and_pairs(ops):
        s = damaged(base, ops, case)
        try:
            walk_and_check(s.payload(), s.channels, 64)
        except AssertionError as e:
            raise AssertionError("%s %s: %s" % (name, case, e)) from e


@pytest.mark.parametrize("name", STREAMS)
def test_what_each_damage_does(name, kats):
    """The single cases, each with what the rule says of it -- the limits included: they are the rule, not wishes."""
    base = _stream(name, kats)
    ops = damage_cases(has_rice=name == "golden")
    offs, ch = base.offs, base.channels

    def taken(case, cap=64):
        s = damaged(base, ops, (case,))
        records, totals = walk_and_check(s.payload(), ch, cap)
        return records["offset"].tolist(), records, totals, s

    got, records, totals, _ = taken("sync_first")
    assert got == offs[1:12] and int(records["skipped_before"][0]) == offs[1] and int(totals[1]) == 1
    got, records, totals, _ = taken("sync_middle")
    assert got == offs[:5] + offs[6:12] and records["skipped_before"].tolist() == [0] * 5 + [offs[6] - offs[5]] + [0] * 5
    got, records, totals, s = taken("sync_last")
    assert got == offs[:11] and int(totals[3]) == offs[11] and len(s.buf) - int(totals[3]) == offs[12] - offs[11]  # (the lost frame: trailing bytes)
    got, _, _, _ = taken("zero_header")
    assert got == offs[:7] + offs[8:12]  # (frame 6 loses its last 8 bytes' contents, not its shape: trusted, taken)
    got, _, _, _ = taken("adjacent_headers")
    assert got == offs[:2] + offs[4:12]
    got, _, _, _ = taken("intact_between_damaged")
    assert got == offs[:5] + offs[8:12], "frame 6 is intact, but neither trusted nor confirmed: missed"
    got, _, _, _ = taken("fake_unconfirmed")
    assert got == offs[:8] + offs[10:12], "a fake whose end is no candidate is skipped"
    got, records, _, _ = taken("fake_confirmed")
    assert got == offs[:8] + [offs[8] + 4] + offs[10:12], "a fake that ends on a candidate is taken: the rule, as documented"
    assert int(records["skipped_before"][8]) == 4 and int(records["bytes"][8]) == offs[10] - offs[8] - 4
    got, records, _, _ = taken("garbage_prefix")
    assert got == [12 + o for o in offs[:12]] and int(records["skipped_before"][0]) == 12
    for phase in range(4):
        got, _, totals, s = taken("cut_header_%d" % phase)
        assert got == offs[:9] and len(s.payload()) % 4 == phase and len(s.payload()) - int(totals[3]) == s.cut - offs[9]
    if name == "golden":
        got, _, totals, _ = taken("zero_rice")
        assert got == offs[:12] and int(totals[1]) == 0, "damage inside Rice data leaves a candidate: taken, no gap"
        for phase in range(4):
            got, _, _, s = taken("cut_rice_%d" % phase)
            assert got == offs[:9] and len(s.payload()) % 4 == phase
    # max_frames inside a clean run, right at the gap, behind it, and 0
    for cap, want in ((0, []), (3, offs[:3]), (5, offs[:5]), (6, offs[:5] + offs[6:7]), (11, offs[:5] + offs[6:12])):
        got, _, totals, _ = taken("sync_middle", cap)
        assert got == want and int(totals[0]) == len(want)


def test_payloads_without_a_frame():
    for n in range(4):
        for ch in (1, 2, 255):
            records, totals = walk_and_check(np.frombuffer(b"\x00\xff\x55\xaa"[:n], np.uint8).copy(), ch, 8)
            assert len(records) == 0 and totals.tolist() == [0, 0, 0, 0]
    lone = np.frombuffer(bytes(8) + bytes.fromhex("00ff55aa"), np.uint8).copy()  # a sync word as the last word: no header fits
    assert frame_end(lone.tobytes(), 8, 1) == 0
    records, totals = walk_and_check(lone, 1, 8)
    assert len(records) == 0
    # null outputs are allowed, channel counts the format cannot say find nothing
    frame = np.frombuffer(crafted_frame(1), np.uint8).copy()
    lib = capi.lib()
    assert lib.sela_hip_salvage_frames(frame.ctypes.data, frame.nbytes, 4, 1, None, None) == 1
    assert lib.sela_hip_salvage_frames(frame.ctypes.data, frame.nbytes, 4, 0, None, None) == 0
    assert lib.sela_hip_salvage_frames(frame.ctypes.data, frame.nbytes, 4, 256, None, None) == 0


def test_any_alignment_of_the_payload(kats):
    s = damaged(golden_stream(kats), damage_cases(True), ("sync_middle", "cut_rice_1"))
    body = s.payload()
    want = as_tuples(codec.salvage_frames(body, 2, 64)[0])
    lib = capi.lib()
    for shift in range(1, 4):
        room = np.zeros(len(body) + 8, np.uint8)
        view = room[shift:shift + len(body)]
        view[:] = body
        records, totals = np.zeros(64, codec.SALVAGED_DTYPE), np.zeros(4, np.uint64)
        found = lib.sela_hip_salvage_frames(view.ctypes.data, len(body), 64, 2, records.ctypes.data, totals.ctypes.data)
        assert view.ctypes.data % 4 == (room.ctypes.data + shift) % 4 and as_tuples(records[:found]) == want


def test_the_workspace_formula_needs_no_gpu():
    """include/sela_hip.h: 9 up(4 W) + 2 up(4 (K + 1)) + 3 up(4 F) + 5 * 256 + 256, and the pieces that make it."""
    lib = capi.lib()

    def up(b):
        return (b + 255) // 256 * 256

    for n_bytes, cap in ((0, 0), (3, 5), (4, 1), (35000, 12), (35000, 3), (81920, 4096), (81921, 4097), (4096 * 4, 1 << 20), (4096 * 4 + 4, 7), (22_800_000, 3875),
                         ((1 << 34) - 4, 1 << 31)):
        W = n_bytes // 4
        K, F = (W + 4095) // 4096, min(cap, W)
        want = 9 * up(4 * W) + 2 * up(4 * (K + 1)) + 3 * up(4 * F) + 5 * 256 + 256
        assert int(lib.sela_hip_salvage_workspace_bytes(n_bytes, cap)) == want, (n_bytes, cap)
        pieces = capi.workspace_pieces("salvage", n_bytes, cap)
        assert len(pieces) == 19 and pieces[:8] == capi.workspace_pieces("index", n_bytes), "the index's own pieces open the workspace"
        end = 0
        for offset, nbytes in pieces:
            assert offset % 256 == 0 and offset >= end
            end = offset + nbytes
        assert end + 255 <= want


def test_the_walk_stand_alone_under_asan_and_ubsan(tmp_path):
    """tests/c/salvage_walk.cpp: sela_amd/csrc/sela_salvage_walk.h alone under -fsanitize=address,undefined, run directly --
    every truncation of crafted streams in a heap buffer of exactly that many bytes, at every alignment, so that a read past
    the end traps."""
    from test_pcm_cpu import _compile

    exe = _compile(tmp_path, "salvage_walk", [os.path.join(ROOT, "tests", "c", "salvage_walk.cpp")],
                   ["-I" + os.path.join(ROOT, "sela_amd", "csrc"), "-I" + os.path.join(ROOT, "include")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "salvage_walk: 0 failures" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, \
        out.stdout + out.stderr
