"""No GPU: what the window calls for 24- and 32-bit streams decide before a device is asked for.  The header, the
binding and the library agree on the new names; every argument error of sela_hip_decode_windows_i32_device and
sela_hip_decode_windows_i32 with its code, in sela_hip_decode_windows_device's order (the pointers are made-up addresses: every row
ends in a refusal, so nothing is dereferenced and nothing is launched); the workspace formula of the header against the function
and against the carve; the packed 3-byte store's byte arithmetic under ASan + UBSan in a stand-alone program."""
import os
import re
import shutil
import subprocess

import pytest

from sela_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
I16, F32, I32, PCM24, PCM32 = 0, 1, 2, 3, 4
NEW = ["sela_hip_decode_windows_i32", "sela_hip_decode_windows_i32_device", "sela_hip_decode_windows_i32_workspace_bytes"]


def A(k):
    """a made-up device address, 4096-aligned"""
    return 0x7F0000000000 + 0x100000 * k


def cover(window_samples):
    return (window_samples + 2046) // 2048 + 1


def formula(n_windows, window_samples, channels):
    """include/sela_hip.h: workspace = n_windows * cover * channels * (16 + 4 * 2048) + 4 * n_windows + 1024"""
    return n_windows * cover(window_samples) * channels * (16 + 4 * 2048) + 4 * n_windows + 1024


def workspace_bytes(n_windows, window_samples, channels):
    return int(capi.lib().sela_hip_decode_windows_i32_workspace_bytes(n_windows, window_samples, channels))


DEVICE_ARGS = [("d_frames", A(1)), ("d_frame_offsets", A(2)), ("n_frames_total", 5), ("channels", 2), ("d_windows", A(3)), ("n_windows", 4),
               ("window_samples", 777), ("format", I32), ("sample_bits", 24), ("d_out", A(4)), ("d_window_flags", A(5)), ("d_status", A(6)), ("d_workspace", A(7)),
               ("workspace_bytes", None), ("stream", 0)]
HOST_ARGS = [("frames", A(1)), ("frame_offsets", A(2)), ("n_frames_total", 5), ("channels", 2), ("windows", A(3)), ("n_windows", 4), ("window_samples", 777),
             ("format", I32), ("sample_bits", 24), ("out", A(4)), ("window_flags", A(5))]


def device_call(short=0, **changes):
    a = dict(DEVICE_ARGS)
    assert not set(changes) - set(a)
    a.update(changes)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(workspace_bytes(a["n_windows"], a["window_samples"], a["channels"]) - short, 0)
    lib = capi.lib()
    rc = lib.sela_hip_decode_windows_i32_device(*[a[k] for k, _ in DEVICE_ARGS])
    return rc, lib.sela_hip_last_error().decode()


def host_call(**changes):
    a = dict(HOST_ARGS)
    assert not set(changes) - set(a)
    a.update(changes)
    lib = capi.lib()
    rc = lib.sela_hip_decode_windows_i32(*[a[k] for k, _ in HOST_ARGS])
    return rc, lib.sela_hip_last_error().decode()


def test_header_binding_and_library_agree_on_the_new_names():
    text = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sela_hip_[a-z0-9_]+)\s*\(", text))
    lib = capi.lib()
    for name in NEW:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    for name, value in (("I32_PLANAR", 2), ("PCM24_INTERLEAVED", 3), ("PCM32_INTERLEAVED", 4)):
        assert re.search(r"#define\s+SELA_HIP_WINDOW_%s\s+%du\b" % (name, value), text), name
        assert getattr(capi, "WINDOW_" + name) == value
    assert "windows_i32" in capi.WORKSPACE_CALLS


def test_the_header_s_formula_is_the_function_and_holds_the_carve():
    """Per (window, cover slot, channel) a 16-byte record and 2048 int32, a flag word per window, alignment slack -- and the pieces
    the launch carves (sela_hip_debug_workspace_pieces) lie ascending, on multiples of 256, inside that size with the base's
    alignment to spare."""
    assert "n_windows * cover * channels * (16 + 4 * 2048) + 4 * n_windows + 1024" in open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    for n_windows in (0, 1, 3, 1000):
        for window_samples in (1, 2047, 2048, 2049, 1 << 24):
            for channels in range(1, 9):
                shape = (n_windows, window_samples, channels)
                size = workspace_bytes(*shape)
                assert size == formula(*shape), shape
                pieces = capi.workspace_pieces("windows_i32", *shape)
                slots = n_windows * cover(window_samples) * channels
                assert [b for _, b in pieces] == [16 * slots, 8192 * slots, 4 * n_windows], shape
                end = 0
                for at, nbytes in pieces:
                    assert at % 256 == 0 and at >= end, (shape, pieces)
                    end = at + nbytes
                assert end + 255 <= size, (shape, end, size)  # (the caller's pointer may be 255 bytes short of a multiple of 256)


DEVICE_REFUSALS = [
    (dict(channels=0), EINVAL, "channels"), (dict(channels=9), EINVAL, "channels must be in 1..8"), (dict(channels=255), EINVAL, "channels"),
    (dict(window_samples=0), EINVAL, "window_samples"), (dict(window_samples=(1 << 24) + 1), EINVAL, "window_samples"),
    (dict(format=I16), EINVAL, "format"), (dict(format=5), EINVAL, "format"), (dict(format=0xFFFFFFFF), EINVAL, "format"),
    (dict(format=F32, sample_bits=0), EINVAL, "sample_bits"), (dict(format=F32, sample_bits=33), EINVAL, "sample_bits"),
    (dict(n_windows=1 << 29, window_samples=2, channels=2), EINVAL, "2^31"), (dict(n_windows=0x7FFFFFFF, window_samples=3, channels=1), EINVAL, "2^31"),
    (dict(n_windows=1 << 27, window_samples=2048, channels=8), EINVAL, "2^31"),
    (dict(n_windows=1 << 24, window_samples=1, channels=1), EINVAL, "2^24"), (dict(n_windows=(1 << 26) + 5, window_samples=1, channels=2), EINVAL, "2^24"),
    (dict(d_status=0), EINVAL, "null"), (dict(d_windows=0), EINVAL, "null"), (dict(d_out=0), EINVAL, "null"), (dict(d_workspace=0), EINVAL, "null"),
    (dict(d_frames=0), EINVAL, "null"), (dict(d_frame_offsets=0), EINVAL, "null"),
    (dict(d_frames=A(1) + 2), EINVAL, "d_frames must be 4-byte aligned"), (dict(d_windows=A(3) + 4), EINVAL, "d_windows must be 8-byte aligned"),
    (dict(d_out=A(4) + 1), EINVAL, "d_out"), (dict(d_out=A(4) + 2), EINVAL, "d_out"), (dict(d_out=A(4) + 2, format=PCM24), EINVAL, "d_out"),
    (dict(d_out=A(4) + 3, format=PCM32), EINVAL, "d_out"), (dict(d_out=A(4) + 2, format=F32), EINVAL, "d_out"),
    (dict(d_window_flags=A(5) + 2), EINVAL, "d_window_flags"), (dict(d_status=A(6) + 2), EINVAL, "d_status"),
    (dict(short=1), ECAPACITY, "workspace smaller than sela_hip_decode_windows_i32_workspace_bytes()"), (dict(workspace_bytes=0), ECAPACITY, "workspace"),
]


@pytest.mark.parametrize("changes,code,text", DEVICE_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _, _ in DEVICE_REFUSALS])
def test_device_call_refuses_before_it_asks_for_a_device(changes, code, text):
    rc, said = device_call(**changes)
    assert rc == code and text in said, (rc, said)


# every row breaks two things: the one that sela_hip_decode_windows_device checks first is the one reported
ORDER = [
    (dict(channels=9, window_samples=0), "channels"), (dict(window_samples=0, format=I16), "window_samples"), (dict(format=I16, n_windows=1 << 30), "format"),
    (dict(format=F32, sample_bits=0, n_windows=1 << 30), "sample_bits"), (dict(n_windows=1 << 30, d_status=0), "2^31"), (dict(n_windows=1 << 24, window_samples=1, d_status=0), "2^24"), (dict(d_status=0, d_out=A(4) + 2), "null"),
    (dict(d_out=A(4) + 2, d_frames=0), "d_out"), (dict(d_frames=0, short=1), "null"), (dict(d_frames=A(1) + 2, short=1), "d_frames must be 4-byte aligned"),
]


@pytest.mark.parametrize("changes,text", ORDER, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in ORDER])
def test_device_call_checks_in_the_int16_call_s_order(changes, text):
    rc, said = device_call(**changes)
    assert rc == EINVAL and text in said, (rc, said)


def test_device_call_takes_what_its_formats_allow():
    """Every format of the four, sample_bits of any value where it is ignored and 1 and 32 with F32, no flag array, the most windows
    a call takes: the refusal that follows is the next one in line (only refused calls are made here: one with the full workspace
    would be launched on the made-up addresses wherever there is a device)."""
    for format in (F32, I32, PCM24, PCM32):
        assert device_call(format=format, short=1)[0] == ECAPACITY, format
    for format in (I32, PCM24, PCM32):
        assert device_call(format=format, sample_bits=0, short=1)[0] == ECAPACITY and device_call(format=format, sample_bits=77, short=1)[0] == ECAPACITY
    assert device_call(format=F32, sample_bits=1, short=1)[0] == ECAPACITY and device_call(format=F32, sample_bits=32, short=1)[0] == ECAPACITY
    assert device_call(d_window_flags=0, short=1)[0] == ECAPACITY
    assert device_call(n_windows=(1 << 24) - 1, window_samples=1, channels=8, workspace_bytes=1 << 20)[0] == ECAPACITY


HOST_REFUSALS = [
    (dict(channels=0), "channels"), (dict(channels=9), "channels"), (dict(window_samples=0), "window_samples"), (dict(window_samples=(1 << 24) + 1), "window_samples"),
    (dict(format=I16), "format"), (dict(format=5), "format"), (dict(format=F32, sample_bits=0), "sample_bits"), (dict(format=F32, sample_bits=33), "sample_bits"),
    (dict(n_windows=1 << 29, window_samples=2, channels=2), "2^31"), (dict(n_windows=1 << 24, window_samples=1, windows=0), "2^24"), (dict(windows=0), "null"), (dict(out=0), "null"), (dict(frames=0), "null"),
    (dict(frame_offsets=0), "null"), (dict(channels=9, format=I16), "channels"), (dict(format=I16, windows=0), "format"),
]


@pytest.mark.parametrize("changes,text", HOST_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in HOST_REFUSALS])
def test_host_call_refuses_before_it_asks_for_a_device(changes, text):
    rc, said = host_call(**changes)
    assert rc == EINVAL and text in said, (rc, said)


def test_host_call_of_no_windows_is_done_without_a_device():
    assert host_call(n_windows=0, windows=0, out=0)[0] == 0
    assert host_call(channels=9)[0] == EINVAL and int(capi.lib().sela_hip_debug_windows_staged_bytes()) == 0  # refused: nothing staged


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_pcm24_edges_under_asan_and_ubsan(tmp_path):
    """sela_pcm24_edges.h, the byte arithmetic k_window32_store stores packed 3-byte samples by, driven by tests/c/pcm24_edges.cpp:
    every byte phase, every share length of 0 .. 40 bytes for 1, 2, 3, 5 and 8 channels, rounds of several sizes -- dwords plus edge
    bytes cover the share exactly once, and nothing outside it."""
    exe = tmp_path / "pcm24_edges"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "sela_amd", "csrc"), os.path.join(ROOT, "tests", "c", "pcm24_edges.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "pcm24_edges ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
