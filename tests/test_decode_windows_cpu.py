"""No GPU: what the window calls decide before a device is asked for.  The sizing function and `cover`; every
argument error of sela_hip_decode_windows_device and sela_hip_decode_windows with its code (the pointers are made-up addresses:
every row ends in a refusal, so nothing is dereferenced and nothing is launched); the host call's plan -- which frames are staged,
the descriptors on the compacted table -- under ASan + UBSan in a stand-alone program; the CLI's misuse of --start / --count."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from sela_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
I16, F32 = 0, 1


def A(k):
    """a made-up device address, 4096-aligned"""
    return 0x7F0000000000 + 0x100000 * k


def cover(window_samples):
    return (window_samples + 2046) // 2048 + 1


def workspace_bytes(n_windows, window_samples, channels):
    return int(capi.lib().sela_hip_decode_windows_workspace_bytes(n_windows, window_samples, channels))


DEVICE_ARGS = [("d_frames", A(1)), ("d_frame_offsets", A(2)), ("n_frames_total", 5), ("channels", 2), ("d_windows", A(3)), ("n_windows", 4),
               ("window_samples", 777), ("format", I16), ("d_out", A(4)), ("d_window_flags", A(5)), ("d_status", A(6)), ("d_workspace", A(7)),
               ("workspace_bytes", None), ("stream", 0)]
HOST_ARGS = [("frames", A(1)), ("frame_offsets", A(2)), ("n_frames_total", 5), ("channels", 2), ("windows", A(3)), ("n_windows", 4), ("window_samples", 777),
             ("format", I16), ("out", A(4)), ("window_flags", A(5))]


def device_call(short=0, **changes):
    a = dict(DEVICE_ARGS)
    assert not set(changes) - set(a)
    a.update(changes)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(workspace_bytes(a["n_windows"], a["window_samples"], a["channels"]) - short, 0)
    lib = capi.lib()
    rc = lib.sela_hip_decode_windows_device(*[a[k] for k, _ in DEVICE_ARGS])
    return rc, lib.sela_hip_last_error().decode()


def host_call(**changes):
    a = dict(HOST_ARGS)
    assert not set(changes) - set(a)
    a.update(changes)
    lib = capi.lib()
    rc = lib.sela_hip_decode_windows(*[a[k] for k, _ in HOST_ARGS])
    return rc, lib.sela_hip_last_error().decode()


def test_cover_and_the_sizing_function():
    """cover = (window_samples + 2046) / 2048 + 1, the most frames a window touches; the workspace holds one block of residues per
    (workgroup, channel), a flag word per window, and the alignment."""
    assert [cover(n) for n in (1, 2, 2049, 2050)] == [1, 2, 2, 3]
    assert [cover(n) for n in (2048, 3 * 2048, 16000, 1 << 24)] == [2, 4, 9, 8193]
    for n_windows, window_samples, channels in ((1, 1, 1), (4, 777, 2), (64, 2050, 3), (256, 16000, 2), (3, 1 << 24, 8), (0, 5, 2)):
        want = n_windows * cover(window_samples) * channels * 2048 * 4 + n_windows * 4 + 256
        assert workspace_bytes(n_windows, window_samples, channels) == want, (n_windows, window_samples, channels)
    # ... which is what the capacity check goes by: `cover` enters the call through it alone.  (Only refused calls are made here:
    # one with the full workspace would be launched on the made-up addresses wherever there is a device.)
    for window_samples, frames in ((1, 1), (2, 2), (2049, 2), (2050, 3)):
        assert workspace_bytes(4, window_samples, 2) == 4 * frames * 2 * 2048 * 4 + 4 * 4 + 256
        rc, text = device_call(window_samples=window_samples, short=1)
        assert rc == ECAPACITY and "sela_hip_decode_windows_workspace_bytes()" in text


DEVICE_REFUSALS = [
    (dict(channels=0), EINVAL, "channels"), (dict(channels=9), EINVAL, "sela_hip_decode_device"), (dict(channels=255), EINVAL, "channels"),
    (dict(window_samples=0), EINVAL, "window_samples"), (dict(window_samples=(1 << 24) + 1), EINVAL, "window_samples"),
    (dict(format=2), EINVAL, "format"), (dict(format=0xFFFFFFFF), EINVAL, "format"),
    (dict(n_windows=1 << 30, window_samples=2), EINVAL, "2^31"), (dict(n_windows=0x7FFFFFFF, window_samples=3), EINVAL, "2^31"),
    (dict(d_status=0), EINVAL, "null"), (dict(d_windows=0), EINVAL, "null"), (dict(d_out=0), EINVAL, "null"), (dict(d_workspace=0), EINVAL, "null"),
    (dict(d_frames=0), EINVAL, "null"), (dict(d_frame_offsets=0), EINVAL, "null"),
    (dict(d_frames=A(1) + 2), EINVAL, "d_frames must be 4-byte aligned"), (dict(d_windows=A(3) + 4), EINVAL, "d_windows must be 8-byte aligned"),
    (dict(d_out=A(4) + 1), EINVAL, "d_out"), (dict(d_out=A(4) + 2, format=F32), EINVAL, "d_out"),
    (dict(d_window_flags=A(5) + 2), EINVAL, "d_window_flags"), (dict(d_status=A(6) + 2), EINVAL, "d_status"),
    (dict(short=1), ECAPACITY, "workspace smaller than sela_hip_decode_windows_workspace_bytes()"), (dict(workspace_bytes=0), ECAPACITY, "workspace"),
]


@pytest.mark.parametrize("changes,code,text", DEVICE_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _, _ in DEVICE_REFUSALS])
def test_device_call_refuses_before_it_asks_for_a_device(changes, code, text):
    rc, said = device_call(**changes)
    assert rc == code and text in said, (rc, said)


def test_device_call_takes_every_alignment_its_elements_allow():
    """d_out of int16 at any even address, of float at any multiple of four: the refusal that follows is the next one in line."""
    assert device_call(d_out=A(4) + 2, short=1)[0] == ECAPACITY
    assert device_call(d_out=A(4) + 4, format=F32, short=1)[0] == ECAPACITY
    assert device_call(d_window_flags=0, short=1)[0] == ECAPACITY  # (NULL: no per-window flags)


HOST_REFUSALS = [
    (dict(channels=0), "channels"), (dict(channels=9), "channels"), (dict(window_samples=0), "window_samples"), (dict(window_samples=(1 << 24) + 1), "window_samples"),
    (dict(format=2), "format"), (dict(n_windows=1 << 30, window_samples=2), "2^31"), (dict(windows=0), "null"), (dict(out=0), "null"), (dict(frames=0), "null"),
    (dict(frame_offsets=0), "null"),
]


@pytest.mark.parametrize("changes,text", HOST_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in HOST_REFUSALS])
def test_host_call_refuses_before_it_asks_for_a_device(changes, text):
    rc, said = host_call(**changes)
    assert rc == EINVAL and text in said, (rc, said)


def test_host_call_of_no_windows_is_done_without_a_device():
    assert host_call(n_windows=0, windows=0, out=0)[0] == 0


def test_the_debug_hooks_answer_without_a_device():
    lib = capi.lib()
    staged = []
    fresh = threading.Thread(target=lambda: staged.append(int(lib.sela_hip_debug_windows_staged_bytes())))  # (the count is the thread's)
    fresh.start()
    fresh.join()
    assert staged == [0]
    assert host_call(channels=9)[0] == EINVAL and int(lib.sela_hip_debug_windows_staged_bytes()) == 0  # refused: nothing staged
    assert int(lib.sela_hip_debug_window_lds_bytes(2)) > 0 and int(lib.sela_hip_debug_window_lds_bytes(9)) == 0


def test_pack_is_the_struct_s_layout():
    from sela_amd.codec import WindowDecoder

    packed = WindowDecoder.pack([0, 2047, 2 ** 64 - 1], [0, 2, 0xFFFFFFFF], 3)
    assert packed.dtype == np.int64 and packed.shape == (3, 2)
    raw = np.frombuffer(packed.tobytes(), dtype=np.dtype([("start", "<u8"), ("first_frame", "<u4"), ("n_frames", "<u4")]))
    assert raw["start"].tolist() == [0, 2047, 2 ** 64 - 1] and raw["first_frame"].tolist() == [0, 2, 0xFFFFFFFF] and raw["n_frames"].tolist() == [3, 3, 3]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_host_call_s_plan_under_asan_and_ubsan(tmp_path):
    """sela_window_plan.h, the plain C++ the host call compacts its table with, driven by tests/c/window_compact.cpp: over seeded
    random batches and the edges, every output position names the same frame and sample through the remapped descriptors on the
    compacted table as through the caller's on the whole one, and nothing is staged that no window touches."""
    exe = tmp_path / "window_compact"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "sela_amd", "csrc"), os.path.join(ROOT, "tests", "c", "window_compact.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])


def test_cli_refuses_start_and_count_where_they_do_not_belong(tmp_path):
    """--start S --count N is -d's alone, both, numeric, in front of the paths: anything else gets the usage text and exit code 2,
    and nothing is written."""
    from test_host_cpp import HOST, _build, _write_wav

    _build()
    cli = os.path.join(HOST, "sela_mi355x")
    wav = tmp_path / "in.wav"
    _write_wav(wav, np.zeros((2048, 2), np.int16))
    x = tmp_path / "x.wav"
    for args in (("-d", "--start", "0", wav, x), ("-d", "--count", "5", wav, x), ("-d", "--count", "5", "--start", "0", wav, x),
                 ("-d", "--start", "abc", "--count", "5", wav, x), ("-d", "--start", "0", "--count", "-5", wav, x), ("-d", "--start", "0", "--count", "5x", wav, x),
                 ("-d", "--start", "", "--count", "5", wav, x), ("-d", wav, x, "--start", "0", "--count", "5"), ("-d", "--start", "0", "--count", "5", wav),
                 ("-d", "--start", "0", "--count", "5", wav, x, x), ("-e", "--start", "0", "--count", "5", wav, tmp_path / "x.sela"),
                 ("-v", "--start", "0", "--count", "5", wav, wav), ("-D", tmp_path, "--start", "0", wav), ("-p", "--count", "5", wav),
                 ("-d", "--start", "0", "--count", "5", "--lossless", x), ("-d", "--start", "0", "--count", "99999999999999999999", wav, x)):
        r = subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-d [--start S --count N]" in r.stdout, (args, r.stdout, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["in.wav"]
