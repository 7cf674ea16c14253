"""No GPU: what the full decode of a whole-track stream decides before a device is asked for.  The sizing function
against the header's formula and against the carve; every argument error of sela_hip_decode_whole_device, its payload form and
sela_hip_decode_whole with its code, on made-up addresses (every row ends in a refusal, so nothing is dereferenced and nothing is
launched); the order of sela_hip_decode_whole_status_error; the plan under ASan + UBSan in a stand-alone program; the two new
kernels' registers and scratch."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sela_amd import capi, codec
from test_isa_handoffs import _kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENODEV, EINVAL, ECAPACITY, EFORMAT, ERANGE = -1, -2, -4, -5, -6
Q_RANGE, COEF_OVERFLOW, RICE_OVERRUN, BAD_FRAME, INTERNAL, SHORT_BLOCK, STRIDE = 1, 2, 8, 32, 64, 128, 256


def A(k):
    """a made-up device address, 4096-aligned"""
    return 0x7F0000000000 + 0x100000 * k


def workspace_bytes(max_frames, channels):
    return int(capi.lib().sela_hip_decode_whole_workspace_bytes(max_frames, channels))


FRAMES_ARGS = [("d_frames", A(1)), ("d_frame_offsets", A(2)), ("n_frames", 5), ("channels", 2), ("d_pcm_out", A(3)), ("pcm_capacity", 5 * 2048 + 2047),
               ("d_n_samples", A(4)), ("d_status", A(5)), ("d_workspace", A(6)), ("workspace_bytes", None), ("stream", 0)]
PAYLOAD_BYTES = 4096
PAYLOAD_ARGS = [("d_payload", A(1)), ("payload_bytes", PAYLOAD_BYTES), ("max_frames", 5), ("channels", 2), ("d_pcm_out", A(3)), ("pcm_capacity", 5 * 2048 + 2047),
                ("d_n_samples", A(4)), ("d_frame_offsets", A(2)), ("d_n_frames", A(7)), ("d_status", A(5)), ("d_workspace", A(6)), ("workspace_bytes", None),
                ("stream", 0)]


def frames_call(short=1, **changes):
    """short = 1: a call that passes every other check ends at the capacity (nothing is ever launched here)"""
    a = dict(FRAMES_ARGS)
    assert not set(changes) - set(a)
    a.update(changes)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(workspace_bytes(a["n_frames"], a["channels"]) - short, 0)
    lib = capi.lib()
    rc = lib.sela_hip_decode_whole_device(*[a[k] for k, _ in FRAMES_ARGS])
    return rc, lib.sela_hip_last_error().decode()


def payload_call(short=1, **changes):
    a = dict(PAYLOAD_ARGS)
    assert not set(changes) - set(a)
    a.update(changes)
    lib = capi.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(int(lib.sela_hip_index_workspace_bytes(a["payload_bytes"], a["max_frames"])) + workspace_bytes(a["max_frames"], a["channels"]) - short, 0)
    rc = lib.sela_hip_decode_whole_payload_device(*[a[k] for k, _ in PAYLOAD_ARGS])
    return rc, lib.sela_hip_last_error().decode()


def test_the_sizing_function_is_the_header_s_formula_and_holds_the_carve():
    """sela_hip_decode_workspace_bytes, per channel a record (16) and 4096 decoded 32-bit samples, and 1024 for the plan's record,
    the count and the alignment of the pieces; the pieces the launch really takes end inside it."""
    lib = capi.lib()
    for max_frames, channels in ((0, 1), (1, 1), (3, 2), (5, 3), (64, 8), (3876, 2), (100000, 8)):
        want = int(lib.sela_hip_decode_workspace_bytes(max_frames, channels)) + channels * (16 + 4 * 4096) + 1024
        assert workspace_bytes(max_frames, channels) == want, (max_frames, channels)
        pieces = capi.workspace_pieces("decode_whole", max_frames, channels)
        assert pieces and len(pieces) >= 5
        starts = [o for o, _ in pieces]
        assert all(o % 256 == 0 for o in starts) and starts == sorted(starts)
        assert all(o0 + b0 <= o1 for (o0, b0), (o1, _) in zip(pieces, pieces[1:]))  # disjoint
        assert pieces[-1][0] + pieces[-1][1] + 256 <= want  # (256: the caller's pointer may have any alignment)
        assert [b for _, b in pieces[-4:]] == [32, 4, 16 * channels, 4 * 4096 * channels]


def test_a_smaller_workspace_is_a_capacity_error():
    rc, text = frames_call(short=1)
    assert rc == ECAPACITY and "sela_hip_decode_whole_workspace_bytes()" in text
    assert frames_call(workspace_bytes=int(capi.lib().sela_hip_decode_workspace_bytes(5, 2)))[0] == ECAPACITY
    rc, text = payload_call(short=1)
    assert rc == ECAPACITY and "sela_hip_index_workspace_bytes() + sela_hip_decode_whole_workspace_bytes()" in text
    # the frames form's workspace does not hold the index's
    assert payload_call(workspace_bytes=workspace_bytes(5, 2))[0] == ECAPACITY


REFUSALS = [
    ({"channels": 0}, "channels must be in 1..8"),
    ({"channels": 9}, "channels must be in 1..8"),
    ({"d_status": 0}, "null device pointer"),
    ({"d_n_samples": 0}, "null device pointer"),
    ({"d_workspace": 0}, "null device pointer"),
    ({"d_pcm_out": 0}, "null device pointer"),
    ({"d_frame_offsets": 0}, "null device pointer"),
    ({"d_pcm_out": A(3) + 1}, "d_pcm_out must be 2-byte aligned"),
    ({"d_n_samples": A(4) + 4}, "d_n_samples 8-byte aligned"),
    ({"d_status": A(5) + 2}, "d_status 4-byte aligned"),
]
FRAMES_REFUSALS = REFUSALS + [({"d_frames": 0}, "null device pointer"), ({"d_frames": A(1) + 2}, "d_frames must be 4-byte aligned")]
# (the payload form asks the index's checks first: its text for no channels)
PAYLOAD_REFUSALS = [({"channels": 0}, "channels must be in 1..255")] + REFUSALS[1:] + [({"d_payload": 0}, "null device pointer"), ({"d_payload": A(1) + 2}, "d_payload must be 4-byte aligned"),
                               ({"d_n_frames": 0}, "null device pointer")]
ids = lambda rows: [",".join(f"{k}={v}" for k, v in c.items()) for c, _ in rows]  # noqa: E731


@pytest.mark.parametrize("changes,text", FRAMES_REFUSALS, ids=ids(FRAMES_REFUSALS))
def test_the_frames_form_refuses_before_it_asks_for_a_device(changes, text):
    rc, said = frames_call(short=0, **changes)  # (the whole workspace: the refusal is not the capacity's)
    assert rc == EINVAL and text in said, (rc, said)


@pytest.mark.parametrize("changes,text", PAYLOAD_REFUSALS, ids=ids(PAYLOAD_REFUSALS))
def test_the_payload_form_refuses_before_it_asks_for_a_device(changes, text):
    rc, said = payload_call(short=0, **changes)
    assert rc == EINVAL and text in said, (rc, said)


def test_every_alignment_the_elements_allow_is_taken():
    assert frames_call(d_pcm_out=A(3) + 2)[0] == ECAPACITY
    assert frames_call(d_status=A(5) + 4, d_n_samples=A(4) + 8)[0] == ECAPACITY
    # no frames: no frames pointer and no PCM is asked for
    assert frames_call(n_frames=0, d_frames=0, d_pcm_out=0)[0] == ECAPACITY


def test_the_host_call_refuses_before_it_asks_for_a_device():
    lib = capi.lib()
    n = np.full(1, 77, np.uint64)
    for args in ((A(1), A(2), 3, 0, A(3), 10000, n.ctypes.data), (A(1), A(2), 3, 9, A(3), 10000, n.ctypes.data), (0, A(2), 3, 2, A(3), 10000, n.ctypes.data),
                 (A(1), 0, 3, 2, A(3), 10000, n.ctypes.data), (A(1), A(2), 3, 2, 0, 10000, n.ctypes.data), (A(1), A(2), 3, 2, A(3), 10000, 0)):
        assert lib.sela_hip_decode_whole(*args) == EINVAL, args
    # no frames: done without a device, and no samples
    assert lib.sela_hip_decode_whole(0, 0, 0, 2, 0, 0, n.ctypes.data) == 0 and int(n[0]) == 0
    # decreasing offsets, and a stream that does not fit: refused on the host's bytes
    frames = np.zeros(64, np.uint8)
    offs = np.array([0, 32, 16], np.uint64)
    pcm = np.zeros((8192, 2), np.int16)
    assert lib.sela_hip_decode_whole(frames.ctypes.data, offs.ctypes.data, 2, 2, pcm.ctypes.data, 8192, n.ctypes.data) == EFORMAT
    offs = np.array([0, 32, 64], np.uint64)
    assert lib.sela_hip_decode_whole(frames.ctypes.data, offs.ctypes.data, 2, 2, pcm.ctypes.data, 4095, n.ctypes.data) == ECAPACITY
    assert int(n[0]) == 4096 and not pcm.any()


STATUS_ORDER = [
    ([STRIDE | BAD_FRAME | RICE_OVERRUN | Q_RANGE | COEF_OVERFLOW | INTERNAL, 3, 0, 0], ECAPACITY),
    ([STRIDE, 0, 0, 0], ECAPACITY),
    ([BAD_FRAME | Q_RANGE | COEF_OVERFLOW | INTERNAL, 1, 0, 3], EFORMAT),
    ([BAD_FRAME, 2, 0, 1], EFORMAT),
    ([COEF_OVERFLOW, 1, 0, 3], ERANGE),  # (the count includes a last frame declined for its coefficients: the flags decide)
    ([RICE_OVERRUN | COEF_OVERFLOW | INTERNAL, 0, 0, 3], EFORMAT),
    ([COEF_OVERFLOW | INTERNAL, 0, 0, 3], ERANGE),
    ([Q_RANGE | INTERNAL, 0, 0, 1], ERANGE),
    ([INTERNAL, 0, 0, 3], ENODEV),
    ([0, 0, 0, 3], 0),
    ([0, 0, 0, 1], 0),
    ([0, 0, 0, 0], 0),
]


@pytest.mark.parametrize("status,code", STATUS_ORDER, ids=[f"{s[0]:#x}-{s[1]}-{s[3]}" for s, _ in STATUS_ORDER])
def test_the_status_words_map_in_the_header_s_order(status, code):
    assert codec.decode_whole_status_error(status) == code
    assert capi.lib().sela_hip_decode_whole_status_error(0) == EINVAL


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_plan_under_asan_and_ubsan(tmp_path):
    """plan_decode_whole (sela_decode_whole_plan.h), driven by tests/c/decode_whole_plan.cpp on streams of real header bytes: no
    frames, one frame of 1500 samples, a last frame that says 2048, 2049, 4095, 4096 and 0, one too short to hold a subframe header,
    each with room, with exactly its samples' room and with one sample less."""
    exe = tmp_path / "decode_whole_plan"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "sela_amd", "csrc"), os.path.join(ROOT, "tests", "c", "decode_whole_plan.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])


def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    res = _kernel_resources()
    for part in ("k_whole_plan", "k_whole_store"):
        names = [n for n in res if part in n]
        assert len(names) == 1, (part, names)
        r = res[names[0]]
        print(part, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (part, r)
    # the last frame's decode is the window calls' kernel: one copy of it, and no other copy of the synthesis for this call
    assert len([n for n in res if "k_tailwin_decode" in n]) == 1
