"""No GPU: what the calls for whole 24- and 32-bit tracks decide before a device is asked for.  The header, the binding
and the library agree on the new names; both sizing functions equal the header's formulas over a grid and hold the carve the
launches run; every refusal of the device and host entries comes with its code and text (the pointers are made-up addresses: every
row ends in a refusal, so nothing is dereferenced and nothing is launched); the bound is monotone and never below the int16 one;
the CLI refuses --whole where it does not belong; the shipped code object holds the new store kernel once, without spill or
scratch; and the store's packed 3-byte plan under ASan + UBSan in a stand-alone program."""
import os
import re
import shutil
import subprocess

import pytest

from sela_amd import capi
from test_host_cpp import HOST, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
N = 2048
I16, F32, I32, PCM24, PCM32 = 0, 1, 2, 3, 4
NEW = ["sela_hip_encode_whole_pcm_bound_bytes", "sela_hip_encode_whole_pcm_workspace_bytes", "sela_hip_encode_whole_pcm_device", "sela_hip_encode_whole_pcm",
       "sela_hip_decode_windows_i32_whole_workspace_bytes", "sela_hip_decode_windows_i32_whole_device", "sela_hip_decode_windows_i32_whole"]


def A(k):
    """a made-up device address, 4096-aligned"""
    return 0x7F0000000000 + 0x100000 * k


def up(b):
    return (b + 255) // 256 * 256


def test_header_binding_and_library_agree_on_the_new_names():
    text = open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sela_hip_[a-z0-9_]+)\s*\(", text))
    lib = capi.lib()
    for name in NEW:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert "windows_i32_whole" in capi.WORKSPACE_CALLS and "encode_whole_pcm" in capi.WORKSPACE_CALLS
    import __graft_entry__ as entry

    assert "sela_window32_whole.hip" in entry.HIP_SOURCES


# ---- the sizes ------------------------------------------------------------------------------------------------------------------------
def whole_frames(n):
    return n // N if n >= N else (1 if n else 0)


def test_the_window_workspace_is_the_header_s_formula_and_holds_the_carve():
    lib = capi.lib()
    assert "+ n_windows * (48 + channels * (16 + 4 * 4096)) + 1024" in open(os.path.join(ROOT, "include", "sela_hip.h")).read()
    for n_windows in (0, 1, 3, 1000):
        for window_samples in (1, 2047, 2048, 2049, 1 << 24):
            for channels in range(1, 9):
                shape = (n_windows, window_samples, channels)
                size = int(lib.sela_hip_decode_windows_i32_whole_workspace_bytes(*shape))
                assert size == int(lib.sela_hip_decode_windows_i32_workspace_bytes(*shape)) + n_windows * (48 + channels * (16 + 4 * 4096)) + 1024, shape
                pieces = capi.workspace_pieces("windows_i32_whole", *shape)
                plain = capi.workspace_pieces("windows_i32", *shape)
                assert pieces[: len(plain)] == plain, shape  # (launch_window32 carves the same base: its pieces lie where it looks for them)
                assert [b for _, b in pieces[len(plain):]] == [16 * n_windows, 32 * n_windows, 16 * n_windows * channels, 4 * 4096 * n_windows * channels], shape
                end = 0
                for at, nbytes in pieces:
                    assert at % 256 == 0 and at >= end, (shape, pieces)
                    end = at + nbytes
                assert end + 255 <= size, (shape, end, size)  # (the caller's pointer may be 255 bytes short of a multiple of 256)


def test_the_encode_workspace_is_the_header_s_formula_and_holds_the_carve():
    lib = capi.lib()
    for n in (0, 1, 300, 2047, 2048, 2049, 4095, 4096, 4097, 3 * N + 777, 100 * N + 5, 3875 * N + 777):
        for channels in (1, 2, 3, 8, 255):
            frames, last = whole_frames(n), min(max(n, 1), 4095)
            size = int(lib.sela_hip_encode_whole_pcm_workspace_bytes(n, channels))
            main, tail = int(lib.sela_hip_encode_i32_workspace_bytes(frames, channels, N)), int(lib.sela_hip_encode_i32_workspace_bytes(1, channels, last))
            want = up(4 * frames * N * channels) + main + up(4 * last * channels) + tail + up(int(lib.sela_hip_encode_pcm_bound_bytes(1, channels, last, 4))) + 256 + 256
            assert size == want, (n, channels, size, want)
            pieces = capi.workspace_pieces("encode_whole_pcm", n, channels, 0)
            a, b = capi.workspace_pieces("encode_i32", frames, channels, N), capi.workspace_pieces("encode_i32", 1, channels, last)
            assert len(pieces) == 1 + len(a) + 1 + len(b) + 2
            assert pieces[0][1] == 4 * frames * N * channels and pieces[1 + len(a)][1] == 4 * last * channels and pieces[-1][1] == 32
            for inner, part in ((a, pieces[1: 1 + len(a)]), (b, pieces[2 + len(a): -2])):  # the two calls' own pieces, shifted by one constant each
                assert [x for _, x in part] == [x for _, x in inner] and len({o - i for (o, _), (i, _) in zip(part, inner)}) <= 1
            end = 0
            for at, nbytes in pieces:
                assert at % 256 == 0 and at >= end, (n, channels, pieces)
                end = at + nbytes
            assert end + 255 <= size
    assert int(lib.sela_hip_encode_whole_pcm_workspace_bytes(N, 0)) == SIZE_MAX and int(lib.sela_hip_encode_whole_pcm_workspace_bytes(N, 256)) == SIZE_MAX
    assert int(lib.sela_hip_encode_whole_pcm_workspace_bytes((1 << 31) * N, 1)) == SIZE_MAX
    assert capi.workspace_pieces("encode_whole_pcm", N, 0, 0) is None


def test_the_bound_is_the_header_s_monotone_and_never_below_the_int16_one():
    lib = capi.lib()
    bound = lambda n, ch, b: int(lib.sela_hip_encode_whole_pcm_bound_bytes(n, ch, b))  # noqa: E731
    per = lambda ch, n, b: int(lib.sela_hip_encode_pcm_bound_bytes(1, ch, n, b))  # noqa: E731
    for b in (3, 4):
        for ch in (1, 2, 3, 8, 255):
            before = 0
            for n in (1, 2, 300, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 100 * N + 5, 3875 * N + 777):
                frames = whole_frames(n)
                got = bound(n, ch, b)
                assert got == (frames - 1) * per(ch, N, b) + per(ch, n - (frames - 1) * N, b), (n, ch, b)
                assert got >= int(lib.sela_hip_encode_whole_bound_bytes(n, ch)), (n, ch, b)
                assert got >= before, (n, ch, b)
                before = got
            assert ch == 255 or bound(3 * N + 5, ch + 1, b) > bound(3 * N + 5, ch, b)
    assert bound(0, 2, 3) == 0 and bound(N, 0, 3) == 0 and bound(N, 256, 3) == 0 and bound(N, 2, 2) == 0 and bound(N, 2, 5) == 0
    assert bound(1 << 62, 2, 3) == SIZE_MAX


# ---- the encode entries' refusals -------------------------------------------------------------------------------------------------------
T_BYTES = "bytes_per_sample must be 3 or 4 (16-bit samples: sela_hip_encode_whole_device and sela_hip_encode_whole)"
T_CHANNELS = "channels must be in 1..255"
T_SIGNALS = "frames * signals per frame must stay below 2^31"
T_OPTIONS = "options: a bit this library does not know (SELA_HIP_ENCODE_LOSSLESS is the only one)"
T_NULL = "null pointer"
T_ALIGN = "d_pcm and d_frames must be 4-byte aligned"
T_WORKSPACE = "workspace smaller than sela_hip_encode_whole_pcm_workspace_bytes()"

ENC_DEVICE = [("d_pcm", A(1)), ("bytes_per_sample", 3), ("n_samples", 2 * N + 77), ("channels", 2), ("options", 0), ("d_frames", A(2)), ("frames_cap", 1 << 20),
              ("d_frame_offsets", A(3)), ("d_status", A(4)), ("d_workspace", A(5)), ("workspace_bytes", None), ("stream", 0)]
ENC_HOST = [("pcm", A(1)), ("bytes_per_sample", 3), ("n_samples", 2 * N + 77), ("channels", 2), ("options", 0), ("frames_out", A(2)), ("frames_cap", 1 << 20),
            ("frame_offsets_out", A(3))]


def _enc_device(short=0, **changes):
    a = dict(ENC_DEVICE)
    assert not set(changes) - set(a)
    a.update(changes)
    lib = capi.lib()
    if a["workspace_bytes"] is None:
        need = int(lib.sela_hip_encode_whole_pcm_workspace_bytes(a["n_samples"], a["channels"]))
        a["workspace_bytes"] = max(need - short, 0) if need != SIZE_MAX else 0
    return lib.sela_hip_encode_whole_pcm_device(*[a[k] for k, _ in ENC_DEVICE]), lib.sela_hip_last_error().decode()


ENC_DEVICE_ROWS = [
    (EINVAL, T_BYTES, dict(bytes_per_sample=2)), (EINVAL, T_BYTES, dict(bytes_per_sample=5, channels=0)),  # order: the container first
    (EINVAL, T_CHANNELS, dict(channels=0)), (EINVAL, T_CHANNELS, dict(channels=256, options=2)),
    (EINVAL, T_SIGNALS, dict(n_samples=(1 << 31) * N, channels=1)), (EINVAL, T_SIGNALS, dict(n_samples=((1 << 31) // 2 + 1) * N, channels=2, options=2)),
    (EINVAL, T_OPTIONS, dict(options=2)), (EINVAL, T_OPTIONS, dict(options=capi.ENCODE_LOSSLESS | 0x80000000, d_pcm=0)),
    (EINVAL, T_NULL, dict(d_pcm=0)), (EINVAL, T_NULL, dict(d_frames=0)), (EINVAL, T_NULL, dict(d_frame_offsets=0)), (EINVAL, T_NULL, dict(d_frame_offsets=0, n_samples=0)),
    (EINVAL, T_NULL, dict(d_status=0)), (EINVAL, T_NULL, dict(d_workspace=0)),
    (EINVAL, T_ALIGN, dict(d_pcm=A(1) + 2)), (EINVAL, T_ALIGN, dict(d_frames=A(2) + 2, short=1)),  # order: the alignment before the capacity
    (ECAPACITY, T_WORKSPACE, dict(short=1)), (ECAPACITY, T_WORKSPACE, dict(short=1, options=capi.ENCODE_LOSSLESS, bytes_per_sample=4)),
    (ECAPACITY, T_WORKSPACE, dict(short=1, n_samples=0, d_pcm=0, d_frames=0)),  # (no samples: the two may be null)
    (ECAPACITY, T_WORKSPACE, dict(short=1, n_samples=100)), (ECAPACITY, T_WORKSPACE, dict(short=1, n_samples=3 * N)), (ECAPACITY, T_WORKSPACE, dict(workspace_bytes=0)),
]


@pytest.mark.parametrize("code, text, changes", ENC_DEVICE_ROWS, ids=[str(i) for i in range(len(ENC_DEVICE_ROWS))])
def test_encode_device_refusal(code, text, changes):
    assert _enc_device(**changes) == (code, text)


ENC_HOST_ROWS = [
    (EINVAL, T_BYTES, dict(bytes_per_sample=2)), (EINVAL, T_BYTES, dict(bytes_per_sample=0, channels=0)), (EINVAL, T_CHANNELS, dict(channels=0)),
    (EINVAL, T_CHANNELS, dict(channels=256)), (EINVAL, T_SIGNALS, dict(n_samples=(1 << 31) * N, channels=1)), (EINVAL, T_OPTIONS, dict(options=2)),
    (EINVAL, T_OPTIONS, dict(options=8, pcm=0)), (EINVAL, T_NULL, dict(pcm=0)), (EINVAL, T_NULL, dict(frames_out=0)), (EINVAL, T_NULL, dict(frame_offsets_out=0)),
    (EINVAL, T_NULL, dict(frame_offsets_out=0, n_samples=0)),
]


@pytest.mark.parametrize("code, text, changes", ENC_HOST_ROWS, ids=[str(i) for i in range(len(ENC_HOST_ROWS))])
def test_encode_host_refusal(code, text, changes):
    a = dict(ENC_HOST)
    a.update(changes)
    lib = capi.lib()
    assert (lib.sela_hip_encode_whole_pcm(*[a[name] for name, _ in ENC_HOST]), lib.sela_hip_last_error().decode()) == (code, text)


# ---- the window entries' refusals: sela_hip_decode_windows_i32*'s, in its order --------------------------------------------------------------
WIN_DEVICE = [("d_frames", A(1)), ("d_frame_offsets", A(2)), ("n_frames_total", 5), ("channels", 2), ("d_windows", A(3)), ("n_windows", 4), ("window_samples", 777),
              ("format", I32), ("sample_bits", 24), ("d_out", A(4)), ("d_window_flags", A(5)), ("d_status", A(6)), ("d_workspace", A(7)), ("workspace_bytes", None),
              ("stream", 0)]
WIN_HOST = [("frames", A(1)), ("frame_offsets", A(2)), ("n_frames_total", 5), ("channels", 2), ("windows", A(3)), ("n_windows", 4), ("window_samples", 777),
            ("format", I32), ("sample_bits", 24), ("out", A(4)), ("window_flags", A(5))]


def _win_device(whole, short=0, **changes):
    a = dict(WIN_DEVICE)
    assert not set(changes) - set(a)
    a.update(changes)
    lib = capi.lib()
    sizing = lib.sela_hip_decode_windows_i32_whole_workspace_bytes if whole else lib.sela_hip_decode_windows_i32_workspace_bytes
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(int(sizing(a["n_windows"], a["window_samples"], a["channels"])) - short, 0)
    call = lib.sela_hip_decode_windows_i32_whole_device if whole else lib.sela_hip_decode_windows_i32_device
    return call(*[a[k] for k, _ in WIN_DEVICE]), lib.sela_hip_last_error().decode()


WIN_DEVICE_ROWS = [
    dict(channels=0), dict(channels=9), dict(channels=9, window_samples=0), dict(window_samples=0), dict(window_samples=(1 << 24) + 1, format=I16), dict(format=I16),
    dict(format=5, n_windows=1 << 30), dict(format=F32, sample_bits=0), dict(format=F32, sample_bits=33, n_windows=1 << 30), dict(n_windows=1 << 29, window_samples=2, channels=2),
    dict(n_windows=1 << 30, d_status=0), dict(n_windows=1 << 24, window_samples=1, channels=1, d_status=0), dict(d_status=0), dict(d_status=0, d_out=A(4) + 2), dict(d_windows=0),
    dict(d_out=0), dict(d_workspace=0), dict(d_frames=0), dict(d_frame_offsets=0), dict(d_frames=A(1) + 2, short=1), dict(d_windows=A(3) + 4), dict(d_out=A(4) + 2, format=PCM24),
    dict(d_out=A(4) + 2, d_frames=0), dict(d_window_flags=A(5) + 2), dict(d_status=A(6) + 2), dict(d_frames=0, short=1),
]


@pytest.mark.parametrize("changes", WIN_DEVICE_ROWS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in WIN_DEVICE_ROWS])
def test_window_device_call_refuses_as_the_plain_call_does(changes):
    """the same code and the same text, row by row: the same checks in the same order"""
    plain, whole = _win_device(False, **changes), _win_device(True, **changes)
    assert whole == plain and plain[0] == EINVAL, (plain, whole)


def test_window_device_call_wants_its_own_workspace():
    assert _win_device(True, short=1) == (ECAPACITY, "workspace smaller than sela_hip_decode_windows_i32_whole_workspace_bytes()")
    lib = capi.lib()
    plain = int(lib.sela_hip_decode_windows_i32_workspace_bytes(4, 777, 2))
    assert _win_device(True, workspace_bytes=plain)[0] == ECAPACITY and _win_device(True, workspace_bytes=0)[0] == ECAPACITY
    for fmt in (F32, I32, PCM24, PCM32):  # every format is taken: the refusal that follows is the next one in line
        assert _win_device(True, format=fmt, short=1)[0] == ECAPACITY, fmt
    assert _win_device(True, d_window_flags=0, short=1)[0] == ECAPACITY


WIN_HOST_ROWS = [dict(channels=0), dict(channels=9, format=I16), dict(window_samples=0), dict(window_samples=(1 << 24) + 1), dict(format=I16, windows=0), dict(format=5),
                 dict(format=F32, sample_bits=0), dict(format=F32, sample_bits=33), dict(n_windows=1 << 29, window_samples=2, channels=2),
                 dict(n_windows=1 << 24, window_samples=1, windows=0), dict(windows=0), dict(out=0), dict(frames=0), dict(frame_offsets=0)]


@pytest.mark.parametrize("changes", WIN_HOST_ROWS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in WIN_HOST_ROWS])
def test_window_host_call_refuses_as_the_plain_call_does(changes):
    a = dict(WIN_HOST)
    a.update(changes)
    lib = capi.lib()
    got = []
    for call in (lib.sela_hip_decode_windows_i32, lib.sela_hip_decode_windows_i32_whole):
        got.append((call(*[a[k] for k, _ in WIN_HOST]), lib.sela_hip_last_error().decode()))
        assert int(lib.sela_hip_debug_windows_staged_bytes()) == 0  # refused: nothing staged
    assert got[0] == got[1] and got[0][0] == EINVAL, got


def test_window_host_call_of_no_windows_is_done_without_a_device():
    a = dict(WIN_HOST, n_windows=0, windows=0, out=0)
    assert capi.lib().sela_hip_decode_windows_i32_whole(*[a[k] for k, _ in WIN_HOST]) == 0


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [
    ["-e", "--whole", "--pair-channels", "in.wav", "out.sela"],
    ["-e", "--pair-channels", "--whole", "in.wav", "out.sela"],
    ["-e", "--whole", "--pair-channels", "--lossless", "in.wav", "out.sela"],
    ["-e", "--lossless", "--whole", "in.wav", "out.sela"],
    ["-e", "--whole", "--keep-tail", "in.wav", "out.sela"],
    ["-e", "--keep-tail", "--whole", "in.wav", "out.sela"],
    ["-e", "--whole", "--whole", "in.wav", "out.sela"],
    ["-e", "in.wav", "out.sela", "--whole"],
    ["-e", "--whole", "in.wav"],
    ["-E", "out_dir", "--whole", "a.wav", "b.wav"],
    ["-E", "--whole", "out_dir", "a.wav"],
    ["-d", "--whole", "in.sela", "out.wav"],
    ["-d", "--whole", "--start", "0", "--count", "5", "in.sela", "out.wav"],
    ["-v", "--whole", "in.wav", "in.sela"],
])
def test_cli_refuses_whole_where_it_does_not_belong(tmp_path, args):
    _build()
    out = subprocess.run([os.path.join(HOST, "sela_mi355x")] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert out.returncode == 2 and "Usage:" in out.stdout, out.stdout + out.stderr
    assert not os.listdir(str(tmp_path))  # (refused before anything is opened or written)


def test_cli_usage_names_whole(tmp_path):
    _build()
    out = subprocess.run([os.path.join(HOST, "sela_mi355x")], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert out.returncode == 2 and "-e --whole [--lossless] path/to/input.wav path/to/output.sela" in out.stdout


# ---- the store kernel ---------------------------------------------------------------------------------------------------------------------
def test_the_store_kernel_is_there_once_and_spills_nothing():
    """From the shipped code object's notes: one k_tail32_store, no VGPR or SGPR spill, no scratch, LDS within the table it declares
    (the lead and 256 x 8 values, the list of writes, the carry and the wide count); the kernels it runs beside are as many as before."""
    from test_isa_handoffs import _kernel_resources

    res = _kernel_resources()
    names = [n for n in res if "k_tail32_store" in n]
    assert len(names) == 1, names
    r = res[names[0]]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert 4 * (1 + 256 * 8) <= r["lds"] <= 4 * (1 + 256 * 8) + 4 * (5 * 8 + 2) + 8 + 16, r
    for part, count in (("k_tailwin", 3), ("k_window32_", 3), ("k_pcm_unpack", 2), ("k_splice_tail", 1)):
        assert len([n for n in res if part in n]) == count, part


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_store_s_packed_plan_under_asan_and_ubsan(tmp_path):
    """tests/c/tail32_store_plan.cpp: the shares of the long last frame through the host plan for tailed tables, and k_tail32_store's
    rounds of pcm24_span over them at every byte phase, share length and channel count 1 .. 8 -- every byte of a share once, none
    outside.  A stand-alone program with its own main, run as its own process."""
    exe = tmp_path / "tail32_store_plan"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "sela_amd", "csrc"), os.path.join(ROOT, "tests", "c", "tail32_store_plan.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
