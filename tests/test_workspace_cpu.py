"""No GPU: the workspaces of the device-pointer calls (sela_amd/csrc/sela_workspace.h).  Every public sizing function returns what
tests/golden/workspace_sizes.json recorded before the calls were given one description each; the pieces that description cuts
-- listed by sela_hip_debug_workspace_pieces from the function the launch runs -- lie inside that size at any alignment of the
caller's pointer; the carver itself under ASan + UBSan in a stand-alone program."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from sela_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_workspace_sizes import GRID, SIZE_MAX, function_of, measure  # noqa: E402

CALL_OF = {  # the sizing function's key in the fixture -> (the hook's call, the fixture's arguments -> the hook's a, b, c)
    "sela_hip_encode_workspace_bytes": ("encode", lambda f, c: (f, c, 0)),
    "encode_device_dependent": ("encode", lambda f, c: (f, c, 0)),
    "sela_hip_decode_workspace_bytes": ("decode", lambda f, c: (f, c, 0)),
    "sela_hip_index_workspace_bytes": ("index", lambda p, m: (p, 0, 0)),
    "sela_hip_decode_i32_workspace_bytes": ("decode_i32", lambda f, c, s: (f, c, s)),
    "sela_hip_decode_n_workspace_bytes": ("decode_n", lambda f, c, s: (f, c, s)),
    "sela_hip_verify_workspace_bytes": ("verify", lambda f, c, s: (f, c, s)),
    "sela_hip_verify_i32_workspace_bytes": ("verify_i32", lambda f, c, s: (f, c, s)),
    "sela_hip_encode_i32_workspace_bytes": ("encode_i32", lambda f, c, s: (f, c, s)),
    "sela_hip_encode_paired_workspace_bytes": ("encode_paired", lambda f, c, s: (f, c, s)),
    "sela_hip_decode_windows_workspace_bytes": ("windows", lambda w, s, c: (w, s, c)),
    "sela_hip_decode_windows_whole_workspace_bytes": ("windows_whole", lambda w, s, c: (w, s, c)),
    "sela_hip_encode_whole_workspace_bytes": ("encode_whole", lambda n, c: (n, c, 0)),
}


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")) as fh:
        rows = json.load(fh)
    assert {k: [tuple(r[:-1]) for r in v] for k, v in rows.items()} == {k: [tuple(a) for a in v] for k, v in GRID.items()}, "the fixture is not the grid's"
    return {k: {tuple(r[:-1]): r[-1] for r in v} for k, v in rows.items()}


def device_visible():
    return capi.lib().sela_hip_device_count() > 0


@pytest.mark.parametrize("key", [k for k in GRID if k != "encode_device_dependent"])
def test_every_public_size_is_the_recorded_one(recorded, key):
    lib = capi.lib()
    differ = [(args, measure(lib, key, args), want) for args, want in recorded[key].items() if measure(lib, key, args) != want]
    assert not differ, differ[:10]
    assert any(v == SIZE_MAX for v in recorded[key].values()) == (key not in (
        "sela_hip_encode_workspace_bytes", "sela_hip_decode_workspace_bytes", "sela_hip_index_workspace_bytes", "sela_hip_decode_windows_workspace_bytes",
        "sela_hip_decode_windows_whole_workspace_bytes")), "the refusals are in the fixture"


def test_the_encode_size_from_2048_frames_on_where_no_device_is_visible(recorded):
    """From 2048 frames on sela_hip_encode_workspace_bytes asks the current device for its CU count (encode_split_frames: room
    for a launch cut in two where the library would give it to teams of 16), so the fixture holds what it says without one."""
    if device_visible():
        pytest.skip("recorded without a device: with one, the size goes by its CU count")
    lib = capi.lib()
    key = "encode_device_dependent"
    differ = [(args, measure(lib, key, args), want) for args, want in recorded[key].items() if measure(lib, key, args) != want]
    assert not differ, differ[:10]


def ordered(pieces, what):
    """Every offset a multiple of 256, the pieces ascending without overlap -> where the last one ends."""
    assert pieces, what
    end = 0
    for offset, nbytes in pieces:
        assert offset % 256 == 0 and offset >= end, (what, pieces)
        end = offset + nbytes
    return end


def fits(pieces, size, what):
    """ordered(), and the last piece's end inside the size at the worst misalignment of the caller's pointer (255 bytes).  A
    condition: no tolerance."""
    end = ordered(pieces, what)
    assert end + 255 <= size, (what, end, size)


def shifted(inner, part, what):
    """`part` of a stacked workspace is the inner call's own pieces, shifted by one constant."""
    assert len(part) == len(inner) and [b for _, b in part] == [b for _, b in inner], (what, inner, part)
    assert len({o - i for (o, _), (i, _) in zip(part, inner)}) <= 1, (what, inner, part)


@pytest.mark.parametrize("key", list(GRID))
def test_the_carve_fits_the_public_size(key):
    lib = capi.lib()
    call, to_abc = CALL_OF[key]
    for args in GRID[key]:
        size = measure(lib, key, args)  # (held to the fixture above)
        pieces = capi.workspace_pieces(call, *to_abc(*args))
        if size == SIZE_MAX:
            assert pieces is None, (key, args)
            continue
        fits(pieces, size, (key, args))
        if call == "verify":
            shifted(capi.workspace_pieces("decode_n", *args), pieces[:-2], (key, args))
        elif call == "verify_i32":
            shifted(capi.workspace_pieces("decode_i32", *args), pieces[:-5], (key, args))
        elif call == "windows_whole":
            shifted(capi.workspace_pieces("windows", *args), pieces[:-4], (key, args))
        elif call == "encode_whole":
            n, ch = args
            frames = n // 2048 if n >= 2048 else (1 if n else 0)
            main = capi.workspace_pieces("encode", frames, ch)
            last = capi.workspace_pieces("encode_i32", 1, ch, max(min(n, 4095), 1))
            assert len(pieces) == len(main) + len(last) + 2
            shifted(main, pieces[:len(main)], (key, args))
            shifted(last, pieces[len(main):-2], (key, args))
            assert pieces[len(main)][0] >= pieces[len(main) - 1][0] + pieces[len(main) - 1][1]  # (the second range starts behind the first)


def test_the_pieces_are_the_ones_each_call_is_documented_to_have():
    """How many pieces a call has, and the sizes of a small shape's by hand."""
    P = capi.workspace_pieces
    assert [len(P(c, 3, 2, 2049)) for c in ("decode_i32", "decode_n", "verify", "verify_i32", "encode_i32", "encode_paired")] == [4, 6, 8, 9, 7, 7]
    assert [len(P("encode", 3, 2)), len(P("decode", 3, 2)), len(P("index", 4096)), len(P("windows", 1, 2050, 2)), len(P("windows_whole", 1, 2050, 2))] == [9, 1, 8, 2, 6]
    assert [b for _, b in P("decode_n", 3, 9, 2049)] == [3 * 9 * 2049 * 4, 3 * 9 * 8, 32, 16, 4 * 8, 3 * 9 * 2049 * 4]  # (SampleTile: 16 bytes)
    assert [b for _, b in P("decode_n", 3, 8, 2049)][-1] == 0  # up to 8 channels: no channel-major copy
    assert [b for _, b in P("verify_i32", 0, 3, 100)] == [0, 0, 16, 16, 0, 0, 4, 8, 8]  # no frames: the pieces that are never empty
    assert P("windows", 1, 2050, 2) == [(0, 3 * 2 * 2048 * 4), (3 * 2 * 2048 * 4, 4)]  # (a window of 2050 samples touches up to three frames)
    assert P("encode_split", 100, 2, 0) is None and P("encode_split", 100, 2, 100) is None  # (no first half, no second half)
    assert capi.lib().sela_hip_debug_workspace_pieces(99, 1, 1, 1, None, 0) == -1


@pytest.mark.parametrize("frames", [4096, 4097, 16384])
@pytest.mark.parametrize("channels", [1, 2, 3, 8, 9, 255])
def test_a_launch_cut_in_two_fits_the_size_the_callers_are_told(frames, channels):
    """sela_hip_debug_encode_split: the second half's workspace lies behind the first's, both are launch_encode's own, and where
    the library would cut the launch (teams of 16) the public size holds both at any share."""
    lib = capi.lib()
    size = int(lib.sela_hip_encode_workspace_bytes(frames, channels))
    for first in (32, (frames // 2) // 32 * 32, (frames - 32) // 32 * 32):
        pieces = capi.workspace_pieces("encode_split", frames, channels, first)
        a, b = capi.workspace_pieces("encode", first, channels), capi.workspace_pieces("encode", frames - first, channels)
        shifted(a, pieces[:len(a)], (frames, channels, first))
        shifted(b, pieces[len(a):], (frames, channels, first))
        if lib.sela_hip_debug_encode_kernel(frames, channels) == 16:
            fits(pieces, size, (frames, channels, first))
        else:  # (never cut, so the size promises no room for two halves: their places only)
            ordered(pieces, (frames, channels, first))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_carver_under_asan_and_ubsan(tmp_path):
    """tests/c/workspace_carve.cpp: mixed-type pieces and a nested range out of malloc'ed buffers of exactly bytes() at each of the
    256 misalignments of the base, every byte written; the measuring and the placing pass agree; counts of 0."""
    exe = tmp_path / "workspace_carve"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "sela_amd", "csrc"), os.path.join(ROOT, "tests", "c", "workspace_carve.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])


def test_no_stray_alignment_arithmetic_in_the_library():
    """A lint, not a proof: outside sela_workspace.h nothing in sela_amd/csrc rounds up with a mask by hand -- `+ 255) & ~`,
    `+ (N - 1)) & ~` or the header's own constant spelled out -- so that a new workspace is led to the carver.  What holds the
    pieces inside their sizes is test_the_carve_fits_the_public_size and tests/test_gpu_workspace_bounds.py."""
    import re

    by_hand = re.compile(r"\+\s*\(?\s*(255|0x[fF]{2}|\w+\s*-\s*1)\s*\)+\s*&\s*~")
    csrc = os.path.join(ROOT, "sela_amd", "csrc")
    found = [(name, m.group(0)) for name in sorted(os.listdir(csrc)) if name != "sela_workspace.h"
             for m in by_hand.finditer(open(os.path.join(csrc, name)).read())]
    assert found == [], found
    assert by_hand.search(open(os.path.join(csrc, "sela_workspace.h")).read()), "the pattern no longer finds the one place that rounds"
