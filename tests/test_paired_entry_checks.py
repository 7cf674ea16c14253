"""CPU-only: every refusal the two paired device entries give before they launch anything -- its code and
the whole text of sela_hip_last_error() -- and, where two conditions hold at once, which of them is reported.  The pointers
are made-up addresses: every row ends in a refusal, so nothing is dereferenced and nothing is launched, with a GPU or without.
Also the two sizing functions: the signals per frame, and the one-channel workspace, which is the plain call's."""
import pytest

from sela_amd import capi

EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
FRAMES, CHANNELS, SAMPLES = 3, 6, 300


def A(k):
    """a made-up device address, 4096-aligned"""
    return 0x7F0000000000 + 0x100000 * k


def _entry(first):
    return [(first, A(1)), ("n_frames", FRAMES), ("channels", CHANNELS), ("samples_per_channel", SAMPLES), ("d_frames", A(2)), ("frames_cap", 1 << 20),
            ("d_frame_offsets", A(3)), ("d_status", A(4)), ("d_workspace", A(5)), ("workspace_bytes", None), ("stream", 0), ("options", 0)]


ENTRIES = {"encode_paired_i32_device": _entry("d_samples"), "encode_paired_n_device": _entry("d_pcm")}


def _call(entry, **changes):
    """The entry with its passing arguments and `changes`; workspace_bytes: what the arguments need, less changes["short"]."""
    short = changes.pop("short", 0)
    a = dict(ENTRIES[entry])
    unknown = set(changes) - set(a)
    assert not unknown, (entry, unknown)
    a.update(changes)
    lib = capi.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = int(lib.sela_hip_encode_paired_workspace_bytes(a["n_frames"], a["channels"], a["samples_per_channel"])) - short
    rc = getattr(lib, "sela_hip_" + entry)(*[a[name] for name, _ in ENTRIES[entry]])
    return rc, lib.sela_hip_last_error().decode()


T_OPTIONS = "options: a paired call takes 0 or SELA_HIP_ENCODE_LOSSLESS"
T_CHANNELS = "channels must be in 1..255"
T_SAMPLES = "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)"
T_SIGNALS = "n_frames * signals per frame must stay below 2^31"
T_NULL = "null device pointer"
T_ALIGN = "d_frames must be 4-byte aligned, the samples aligned to their type"
T_WORKSPACE = "workspace smaller than sela_hip_encode_paired_workspace_bytes()"

ROWS = []


def row(entry, code, text, **changes):
    name = "%s-%s" % (entry, "-".join("%s=%s" % (k, "%#x" % v if v > 9 else v) for k, v in changes.items()))
    assert name not in {r.id for r in ROWS}
    ROWS.append(pytest.param(entry, changes, code, text, id=name))


for e in ENTRIES:
    sample_ptr = "d_pcm" if "_n_" in e else "d_samples"
    for opt in (2, 4, capi.ENCODE_LOSSLESS | 2, capi.ENCODE_LOSSLESS | 0x80000000, 0xFFFFFFFF):
        row(e, EINVAL, T_OPTIONS, options=opt)
    row(e, EINVAL, T_OPTIONS, options=2, channels=0)  # order: the options before the call's other checks
    row(e, EINVAL, T_OPTIONS, options=2, samples_per_channel=0, d_status=0, short=1)
    for lossless in (0, capi.ENCODE_LOSSLESS):  # both accepted values: the call's own checks, in the plain device call's order
        row(e, EINVAL, T_CHANNELS, options=lossless, channels=0)
        row(e, EINVAL, T_CHANNELS, options=lossless, channels=256)
        row(e, EINVAL, T_SAMPLES, options=lossless, samples_per_channel=0)
        row(e, EINVAL, T_SAMPLES, options=lossless, samples_per_channel=65536)
        row(e, ECAPACITY, T_WORKSPACE, options=lossless, short=1)
    # the 2^31 limit counts the PAIRED signals: 9 per 6-channel frame, 3 per stereo frame, 4 per 3-channel frame, 1 for mono
    row(e, EINVAL, T_SIGNALS, n_frames=(1 << 31) // 9 + 1)
    row(e, ECAPACITY, T_WORKSPACE, n_frames=(1 << 31) // 9, workspace_bytes=1 << 20)  # (the largest call below the limit: only its workspace is short)
    row(e, EINVAL, T_SIGNALS, n_frames=1 << 29, channels=3)
    row(e, EINVAL, T_SIGNALS, n_frames=1 << 30, channels=2, workspace_bytes=SIZE_MAX)
    row(e, EINVAL, T_SIGNALS, n_frames=1 << 31, channels=1)
    for p in ("d_frame_offsets", "d_status", "d_workspace", "d_frames", sample_ptr):
        row(e, EINVAL, T_NULL, **{p: 0})
    row(e, EINVAL, T_ALIGN, d_frames=A(2) + 2)
    row(e, EINVAL, T_ALIGN, **{sample_ptr: A(1) + (1 if "_n_" in e else 2)})
    row(e, EINVAL, T_CHANNELS, channels=0, samples_per_channel=0)  # order: the channels, the length ...
    row(e, EINVAL, T_SAMPLES, samples_per_channel=0, n_frames=1 << 30)  # ... the 2^31 limit ...
    row(e, EINVAL, T_SIGNALS, n_frames=1 << 30, d_status=0)  # ... the pointers ...
    row(e, EINVAL, T_NULL, d_status=0, d_frames=A(2) + 2, short=1)  # ... their alignment, and the capacity last
    row(e, EINVAL, T_ALIGN, d_frames=A(2) + 2, short=1)


@pytest.mark.parametrize("entry, changes, code, text", ROWS)
def test_refusal(entry, changes, code, text):
    assert _call(entry, **changes) == (code, text)


def test_an_int16_input_may_sit_on_an_odd_word():
    """2-byte alignment is all the int16 entry asks, as sela_hip_encode_n_device: with one byte short of workspace the call gets
    as far as the capacity."""
    assert _call("encode_paired_n_device", d_pcm=A(1) + 2, short=1) == (ECAPACITY, T_WORKSPACE)


def test_signals_per_frame():
    lib = capi.lib()
    assert [int(lib.sela_hip_paired_signals_per_frame(c)) for c in (1, 2, 3, 6, 255)] == [1, 3, 4, 9, 382]


@pytest.mark.parametrize("n_frames, n", [(0, 2048), (1, 1), (3, 300), (7, 2048), (4097, 65535)])
def test_workspace_of_one_and_two_channels_is_the_plain_one(n_frames, n):
    lib = capi.lib()
    for channels in (1, 2):
        assert int(lib.sela_hip_encode_paired_workspace_bytes(n_frames, channels, n)) == int(lib.sela_hip_encode_i32_workspace_bytes(n_frames, channels, n))
    # ... and grows with the pairs' signals beyond: 9 against 6
    assert int(lib.sela_hip_encode_paired_workspace_bytes(n_frames, 6, n)) >= int(lib.sela_hip_encode_i32_workspace_bytes(n_frames, 6, n))
    if n_frames:
        assert int(lib.sela_hip_encode_paired_workspace_bytes(n_frames, 6, n)) > int(lib.sela_hip_encode_i32_workspace_bytes(n_frames, 6, n))


def test_workspace_size_refuses_what_the_calls_refuse():
    lib = capi.lib()
    for args in ((1, 0, 300), (1, 256, 300), (1, 6, 0), (1, 6, 65536), ((1 << 31) // 9 + 1, 6, 300)):
        assert int(lib.sela_hip_encode_paired_workspace_bytes(*args)) == SIZE_MAX, args


def test_the_paired_kernels_keep_the_plain_kernels_budgets():
    """From the shipped code object: the pairs are kernels and instantiations of their own (the plain calls keep theirs), held to what
    the plain ones are held to -- every k_generic_analyse, the four paired ones among its eight, 102 VGPRs, at most 16 spilled, LDS
    for five waves per SIMD; both k_paired_plan no VGPR spill and no scratch, as k_generic_plan."""
    from test_isa_handoffs import _kernel_resources

    res = _kernel_resources()
    analyse = [n for n in res if "k_generic_analyse" in n]
    assert len(analyse) == 8
    for n in analyse:
        assert res[n]["vgpr"] <= 102 and res[n]["vgpr_spill"] <= 16 and res[n]["lds"] <= 160 * 1024 // 20, (n, res[n])
    plans = [n for n in res if "k_paired_plan" in n]
    assert len(plans) == 2  # (the host route's and the device call's)
    for n in plans:
        assert res[n]["vgpr_spill"] == 0 and res[n]["scratch"] == 0, (n, res[n])
