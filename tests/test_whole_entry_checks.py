"""CPU-only: a whole track with its tail as far as it needs no device -- the layout rule, the sizing functions, every
refusal the two entries give for their arguments -- its code and the whole text of sela_hip_last_error() (the pointers are made-up
addresses, so a row that got past its refusal would fault: that nothing is enqueued is not observed here) --, the CLI's usage errors, the Python names, and the splice kernel's resources from the
shipped code object."""
import os
import subprocess

import pytest

from sela_amd import capi, codec
from test_host_cpp import HOST, _build

EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
N = 2048


def A(k):
    """a made-up device address, 4096-aligned"""
    return 0x7F0000000000 + 0x100000 * k


def _rule(n):
    """the table of the issue, restated: [(first_sample, length)]"""
    if n == 0:
        return []
    if n < N:
        return [(0, n)]
    frames = n // N
    return [(f * N, N) for f in range(frames - 1)] + [((frames - 1) * N, N + n % N)]


@pytest.mark.parametrize("n", [0, 1, 100, 2047, 2048, 2049, 4095, 4096, 6143])
def test_layout(n):
    assert codec.whole_frames(n) == _rule(n)
    assert int(capi.lib().sela_hip_whole_frames(n)) == len(_rule(n))
    assert sum(length for _, length in codec.whole_frames(n)) == n


def test_layout_beyond_32_bits():
    import ctypes as C

    lib = capi.lib()
    n = (1 << 32) + 5
    frames = n // N
    assert int(lib.sela_hip_whole_frames(n)) == frames == 2097152
    first, length = C.c_uint64(), C.c_uint32()
    for f, want in ((0, (0, N)), (frames - 2, ((frames - 2) * N, N)), (frames - 1, ((frames - 1) * N, N + 5))):
        assert lib.sela_hip_whole_frame(n, f, C.byref(first), C.byref(length)) == 0
        assert (first.value, length.value) == want
    assert lib.sela_hip_whole_frame(n, frames, C.byref(first), C.byref(length)) == EINVAL
    assert lib.sela_hip_whole_frame(0, 0, C.byref(first), C.byref(length)) == EINVAL
    assert lib.sela_hip_whole_frame(n, 0, None, C.byref(length)) == EINVAL


def test_exports_and_python_names():
    lib = capi.lib()
    for name in ("sela_hip_whole_frames", "sela_hip_whole_frame", "sela_hip_encode_whole_bound_bytes", "sela_hip_encode_whole_workspace_bytes",
                 "sela_hip_encode_whole_device", "sela_hip_encode_whole"):
        assert name in capi.EXPORTS and hasattr(lib, name), name
    header = open(os.path.join(os.path.dirname(HOST), "include", "sela_hip.h")).read()
    for name in capi.EXPORTS[-6:]:
        assert name + "(" in header, name
    assert callable(codec.WholeEncoder) and callable(codec.encode_whole_host) and callable(codec.whole_frames)
    for method in ("encode", "check", "to_host"):
        assert callable(getattr(codec.WholeEncoder, method))


def test_bound_bytes():
    lib = capi.lib()
    bound = lambda n, ch: int(lib.sela_hip_encode_whole_bound_bytes(n, ch))  # noqa: E731
    for ch in (1, 2, 3, 255):
        per = int(lib.sela_hip_encode_bound_bytes(1, ch))
        assert bound(0, ch) == 0
        assert bound(3 * N, ch) == 3 * per == int(lib.sela_hip_encode_bound_bytes(3, ch))  # whole frames only: the plain call's bound
        assert bound(3 * N + 777, ch) == 2 * per + int(lib.sela_hip_encode_bound_bytes_n(1, ch, N + 777))
        assert bound(150, ch) == int(lib.sela_hip_encode_bound_bytes_n(1, ch, 150))
        assert bound(N + 5, ch) == int(lib.sela_hip_encode_bound_bytes_n(1, ch, N + 5))


def test_workspace_bytes():
    """It says nothing about the data or the device, holds the pieces the header names, grows with the samples, and is SIZE_MAX
    for what the call refuses."""
    lib = capi.lib()
    ws = lambda n, ch: int(lib.sela_hip_encode_whole_workspace_bytes(n, ch))  # noqa: E731
    for ch in (1, 2, 3, 8):
        sizes = [ws(n, ch) for n in (0, 1, 100, 2047, 2048, 2049, 4095, 4096, 6143, 3875 * N, 3875 * N + 777, 3876 * N)]
        assert sizes == sorted(sizes), (ch, sizes)
        n = 3875 * N + 777
        assert ws(n, ch) >= int(lib.sela_hip_encode_i32_workspace_bytes(1, ch, 4095)) + int(lib.sela_hip_encode_bound_bytes_n(1, ch, 4095)) + 512
    assert ws(5000, 0) == SIZE_MAX and ws(5000, 256) == SIZE_MAX
    assert ws((1 << 31) * N, 1) == SIZE_MAX and ws(((1 << 31) // 3 + 1) * N, 2) == SIZE_MAX


# ---- the refusals of the two entries ---------------------------------------------------------------------------------------------------
DEVICE = [("d_pcm", A(1)), ("n_samples", 3 * N + 777), ("channels", 2), ("d_frames", A(2)), ("frames_cap", 1 << 20), ("d_frame_offsets", A(3)),
          ("d_status", A(4)), ("d_workspace", A(5)), ("workspace_bytes", None), ("stream", 0), ("options", 0)]
HOST_CALL = [("pcm", A(1)), ("n_samples", 3 * N + 777), ("channels", 2), ("frames_out", A(2)), ("frames_cap", 1 << 20), ("frame_offsets_out", A(3)),
             ("options", 0)]

T_OPTIONS = "options: a bit this library does not know (SELA_HIP_ENCODE_LOSSLESS is the only one)"
T_CHANNELS = "channels must be in 1..255"
T_SIGNALS = "frames * signals per frame must stay below 2^31"
T_NULL = "null pointer"
T_ALIGN = "d_pcm and d_frames must be 4-byte aligned"
T_WORKSPACE = "workspace smaller than sela_hip_encode_whole_workspace_bytes()"


def _device(**changes):
    short = changes.pop("short", 0)
    a = dict(DEVICE)
    assert not set(changes) - set(a)
    a.update(changes)
    lib = capi.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(int(lib.sela_hip_encode_whole_workspace_bytes(a["n_samples"], a["channels"])) - short, 0) & SIZE_MAX
    rc = lib.sela_hip_encode_whole_device(*[a[name] for name, _ in DEVICE])
    return rc, lib.sela_hip_last_error().decode()


DEVICE_ROWS = [
    (EINVAL, T_OPTIONS, dict(options=2)),
    (EINVAL, T_OPTIONS, dict(options=capi.ENCODE_LOSSLESS | 0x80000000)),
    (EINVAL, T_OPTIONS, dict(options=4, channels=0)),  # order: the options first
    (EINVAL, T_CHANNELS, dict(channels=0)),
    (EINVAL, T_CHANNELS, dict(channels=256, options=capi.ENCODE_LOSSLESS)),
    (EINVAL, T_SIGNALS, dict(n_samples=(1 << 31) * N, channels=1)),
    (EINVAL, T_SIGNALS, dict(n_samples=((1 << 31) // 3 + 1) * N, channels=2)),
    (EINVAL, T_NULL, dict(d_pcm=0)),
    (EINVAL, T_NULL, dict(d_frames=0)),
    (EINVAL, T_NULL, dict(d_frame_offsets=0)),
    (EINVAL, T_NULL, dict(d_frame_offsets=0, n_samples=0)),
    (EINVAL, T_NULL, dict(d_status=0)),
    (EINVAL, T_NULL, dict(d_workspace=0)),
    (EINVAL, T_ALIGN, dict(d_pcm=A(1) + 2)),
    (EINVAL, T_ALIGN, dict(d_frames=A(2) + 2, short=1)),  # order: the alignment before the capacity
    (ECAPACITY, T_WORKSPACE, dict(short=1)),
    (ECAPACITY, T_WORKSPACE, dict(short=1, options=capi.ENCODE_LOSSLESS)),
    (ECAPACITY, T_WORKSPACE, dict(short=1, n_samples=0, d_pcm=0, d_frames=0)),  # (no samples: the two may be null)
    (ECAPACITY, T_WORKSPACE, dict(short=1, n_samples=100)),
    (ECAPACITY, T_WORKSPACE, dict(short=1, n_samples=3 * N)),
    (ECAPACITY, T_WORKSPACE, dict(workspace_bytes=0)),
]


@pytest.mark.parametrize("code, text, changes", DEVICE_ROWS, ids=[str(i) for i in range(len(DEVICE_ROWS))])
def test_device_refusal(code, text, changes):
    assert _device(**changes) == (code, text)


@pytest.mark.parametrize("code, text, changes", [
    (EINVAL, T_OPTIONS, dict(options=2)),
    (EINVAL, T_OPTIONS, dict(options=8, channels=0)),
    (EINVAL, T_CHANNELS, dict(channels=0)),
    (EINVAL, T_CHANNELS, dict(channels=256)),
    (EINVAL, T_SIGNALS, dict(n_samples=(1 << 31) * N, channels=1)),
    (EINVAL, T_NULL, dict(pcm=0)),
    (EINVAL, T_NULL, dict(frames_out=0)),
    (EINVAL, T_NULL, dict(frame_offsets_out=0)),
    (EINVAL, T_NULL, dict(frame_offsets_out=0, n_samples=0)),
], ids=[str(i) for i in range(9)])
def test_host_refusal(code, text, changes):
    a = dict(HOST_CALL)
    a.update(changes)
    lib = capi.lib()
    assert (lib.sela_hip_encode_whole(*[a[name] for name, _ in HOST_CALL]), lib.sela_hip_last_error().decode()) == (code, text)


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [
    ["-e", "--keep-tail", "--pair-channels", "in.wav", "out.sela"],
    ["-e", "--pair-channels", "--keep-tail", "in.wav", "out.sela"],
    ["-e", "--keep-tail", "--pair-channels", "--lossless", "in.wav", "out.sela"],
    ["-e", "--lossless", "--keep-tail", "in.wav", "out.sela"],
    ["-e", "in.wav", "out.sela", "--keep-tail"],
    ["-e", "--keep-tail", "in.wav"],
    ["-E", "out_dir", "--keep-tail", "a.wav", "b.wav"],
    ["-E", "--keep-tail", "out_dir", "a.wav"],
    ["-d", "--keep-tail", "in.sela", "out.wav"],
    ["-v", "--keep-tail", "in.wav", "in.sela"],
])
def test_cli_refuses_keep_tail_where_it_does_not_belong(tmp_path, args):
    _build()
    out = subprocess.run([os.path.join(HOST, "sela_mi355x")] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert out.returncode == 2 and "Usage:" in out.stdout, out.stdout + out.stderr
    assert not os.listdir(str(tmp_path))  # (refused before anything is opened or written)


def test_cli_usage_names_keep_tail(tmp_path):
    _build()
    out = subprocess.run([os.path.join(HOST, "sela_mi355x")], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert out.returncode == 2 and "-e --keep-tail [--lossless] path/to/input.wav path/to/output.sela" in out.stdout


# ---- the splice kernel ------------------------------------------------------------------------------------------------------------------
def test_the_splice_kernel_spills_nothing():
    """From the shipped code object: one k_splice_tail, no spill, no scratch, no LDS."""
    from test_isa_handoffs import _kernel_resources

    res = _kernel_resources()
    names = [n for n in res if "k_splice_tail" in n]
    assert len(names) == 1, names
    r = res[names[0]]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, r
