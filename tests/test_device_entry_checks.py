"""CPU-only: every refusal the device-pointer entries give before they launch anything -- its code and the whole text of
sela_hip_last_error() -- and, where two conditions hold at once, which of them is reported.  The pointers are made-up
addresses: every row ends in a refusal, so nothing is dereferenced and nothing is launched, with a GPU or without."""
import pytest

from sela_amd import capi

EINVAL, ECAPACITY = -2, -4
SIZE_MAX = (1 << 64) - 1
FRAMES, CHANNELS, STRIDE, PAYLOAD, SAMPLES = 3, 2, 2048, 4096, 300


def A(k):
    """a made-up device address, 4096-aligned"""
    return 0x7F0000000000 + 0x100000 * k


# ---- the entries: their parameters in the C order, each with a value that passes every check -------------------------------
_FRAMES_HEAD = [("d_frames", A(1)), ("d_frame_offsets", A(2)), ("n_frames", FRAMES), ("channels", CHANNELS)]
_PAYLOAD_HEAD = [("d_payload", A(1)), ("payload_bytes", PAYLOAD), ("n_frames", FRAMES), ("channels", CHANNELS)]
_INDEX_OUT = [("d_frame_offsets", A(2)), ("d_n_frames", A(3))]
_TAIL = [("d_status", A(4)), ("d_workspace", A(5)), ("workspace_bytes", None), ("stream", 0)]
_STRIDE = [("stride", STRIDE)]
_I32_OUT = [("d_samples_out", A(6)), ("d_counts_out", A(7)), ("d_sample_offsets", A(8))]
_N_OUT = [("d_pcm_out", A(6)), ("d_sample_offsets", A(8))]
_VERIFY = [("d_pcm", A(6)), ("d_diff_counts", A(9)), ("d_first_diff", A(10)), ("d_sample_offsets", A(8))]
_VERIFY32 = [("d_samples", A(6)), ("d_lengths", A(7)), ("d_diff_counts", A(9)), ("d_first_diff", A(10)), ("d_sample_offsets", A(8))]
_ENC_TAIL = [("d_frames", A(2)), ("frames_cap", 1 << 20), ("d_frame_offsets", A(3))] + _TAIL[:3]

ENTRIES = {
    "decode_device": _FRAMES_HEAD + [("d_pcm_out", A(6))] + _TAIL,
    "decode_payload_device": _PAYLOAD_HEAD + [("d_pcm_out", A(6))] + _INDEX_OUT + _TAIL,
    "decode_i32_device": _FRAMES_HEAD + _STRIDE + _I32_OUT + _TAIL,
    "decode_payload_i32_device": _PAYLOAD_HEAD + _STRIDE + _I32_OUT + _INDEX_OUT + _TAIL,
    "decode_n_device": _FRAMES_HEAD + _STRIDE + _N_OUT + _TAIL,
    "decode_payload_n_device": _PAYLOAD_HEAD + _STRIDE + _N_OUT + _INDEX_OUT + _TAIL,
    "verify_device": _FRAMES_HEAD + _STRIDE + _VERIFY + _TAIL,
    "verify_payload_device": _PAYLOAD_HEAD + _STRIDE + _VERIFY + _INDEX_OUT + _TAIL,
    "verify_i32_device": _FRAMES_HEAD + _STRIDE + _VERIFY32 + _TAIL,
    "verify_payload_i32_device": _PAYLOAD_HEAD + _STRIDE + _VERIFY32 + _INDEX_OUT + _TAIL,
    "index_frames_device": _PAYLOAD_HEAD + _INDEX_OUT + _TAIL[1:],
    "encode_device": [("d_pcm", A(1)), ("n_frames", FRAMES), ("channels", CHANNELS)] + _ENC_TAIL + [("d_trace", 0), ("stream", 0)],
    "encode_i32_device": [("d_samples", A(1)), ("n_frames", FRAMES), ("channels", CHANNELS), ("samples_per_channel", SAMPLES)] + _ENC_TAIL + [("stream", 0)],
    "encode_n_device": [("d_pcm", A(1)), ("n_frames", FRAMES), ("channels", CHANNELS), ("samples_per_channel", SAMPLES)] + _ENC_TAIL + [("stream", 0)],
}
for _name in ("encode_device", "encode_i32_device", "encode_n_device"):
    ENTRIES[_name + "_opt"] = ENTRIES[_name] + [("options", capi.ENCODE_LOSSLESS)]

_OWN_WORKSPACE = {"decode": "decode", "decode_i32": "decode_i32", "decode_n": "decode_n", "verify": "verify", "verify_i32": "verify_i32"}


def _kind(entry):
    """decode_payload_i32_device -> ("decode_i32", payload form?)"""
    core = entry[:-len("_device")]
    return core.replace("_payload", ""), "_payload" in core


def _workspace_need(entry, a):
    lib = capi.lib()
    if entry == "index_frames_device":
        return int(lib.sela_hip_index_workspace_bytes(a["payload_bytes"], a["n_frames"]))
    if entry.startswith("encode_device"):
        return int(lib.sela_hip_encode_workspace_bytes(a["n_frames"], a["channels"]))
    if entry.startswith("encode_"):
        return int(lib.sela_hip_encode_i32_workspace_bytes(a["n_frames"], a["channels"], a["samples_per_channel"]))
    kind, payload = _kind(entry)
    fn = getattr(lib, "sela_hip_%s_workspace_bytes" % _OWN_WORKSPACE[kind])
    own = int(fn(a["n_frames"], a["channels"]) if kind == "decode" else fn(a["n_frames"], a["channels"], a["stride"]))
    if own == SIZE_MAX or not payload:
        return own
    return own + int(lib.sela_hip_index_workspace_bytes(a["payload_bytes"], a["n_frames"]))


def _call(entry, **changes):
    """The entry with its passing arguments and `changes`; workspace_bytes: what the arguments need, plus changes["short"]."""
    short = changes.pop("short", 0)
    a = dict(ENTRIES[entry])
    unknown = set(changes) - set(a)
    assert not unknown, (entry, unknown)
    a.update(changes)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = _workspace_need(entry, a) - short
    lib = capi.lib()
    rc = getattr(lib, "sela_hip_" + entry)(*[a[name] for name, _ in ENTRIES[entry]])
    return rc, lib.sela_hip_last_error().decode()


# ---- the texts ----------------------------------------------------------------------------------------------------------------
T_CHANNELS = "channels must be in 1..255"
T_STRIDE = "stride must not be 0"
T_SUBS = "n_frames * channels must stay below 2^31"
T_SIGNALS = "n_frames * signals per frame must stay below 2^31"
T_NULL = "null device pointer"
T_FRAMES_ALIGN = "d_frames must be 4-byte aligned"
T_PAYLOAD_ALIGN = "d_payload must be 4-byte aligned"
T_PAYLOAD_SIZE = "payloads of 16 GiB and more are not indexed on the device (32-bit word indices)"
T_VERIFY_ALIGN = "d_pcm must be 2-byte aligned, d_diff_counts and d_first_diff 4-byte aligned"
T_VERIFY32_ALIGN = "d_samples, d_lengths, d_diff_counts and d_first_diff must be 4-byte aligned"
T_ENCODE_ALIGN = "d_pcm and d_frames must be 4-byte aligned"
T_ENCODE32_ALIGN = "d_frames must be 4-byte aligned, the samples aligned to their type"
T_SAMPLES = "samples_per_channel must be 1 .. 65535 (the subframe's field is 16 bits wide)"
T_OPTIONS = "options: a bit this library does not know (SELA_HIP_ENCODE_LOSSLESS is the only one)"
T_LOSSLESS_TRACE = "SELA_HIP_ENCODE_LOSSLESS with d_trace: the trace is the reference's arithmetic"
T_WORKSPACE = {
    "index_frames_device": "workspace smaller than sela_hip_index_workspace_bytes()",
    "encode_device": "workspace smaller than sela_hip_encode_workspace_bytes()",
    "encode_i32_device": "workspace smaller than sela_hip_encode_i32_workspace_bytes()",
    "encode_n_device": "workspace smaller than sela_hip_encode_i32_workspace_bytes()",
}
for _entry in ENTRIES:
    if _entry.endswith("_opt"):
        T_WORKSPACE[_entry] = T_WORKSPACE[_entry[:-4]]
    elif _entry not in T_WORKSPACE:
        _k, _p = _kind(_entry)
        T_WORKSPACE[_entry] = "workspace smaller than " + ("sela_hip_index_workspace_bytes() + " if _p else "") + "sela_hip_%s_workspace_bytes()" % _k

DECODERS = [e for e in ENTRIES if e.startswith(("decode", "verify"))]
PAYLOAD = [e for e in DECODERS if "_payload" in e]
STRIDED = [e for e in DECODERS if "stride" in dict(ENTRIES[e])]
ENCODERS = [e for e in ENTRIES if e.startswith("encode")]
ENCODERS_N = [e for e in ENCODERS if "samples_per_channel" in dict(ENTRIES[e])]

ROWS = []


def row(entry, code, text, **changes):
    name = "%s-%s" % (entry, "-".join("%s=%s" % (k, "%#x" % v if v > 9 else v) for k, v in changes.items()))
    if name not in {r.id for r in ROWS}:
        ROWS.append(pytest.param(entry, changes, code, text, id=name))


for e in ENTRIES:
    row(e, EINVAL, T_CHANNELS, channels=0)
    row(e, EINVAL, T_CHANNELS, channels=256)
    row(e, ECAPACITY, T_WORKSPACE[e], short=1)
for e in STRIDED:
    row(e, EINVAL, T_STRIDE, stride=0)
    row(e, EINVAL, T_SUBS, n_frames=1 << 30, channels=2)
    # n_frames * channels * stride from 2^60: no size is computed, and no capacity is enough.  (sela_hip_decode_i32_device alone
    # compares with the size it got, so the largest capacity that it refuses is one below.)
    row(e, ECAPACITY, T_WORKSPACE[e], n_frames=1 << 30, channels=1, stride=0xFFFFFFFF,
        workspace_bytes=SIZE_MAX - 1 if e == "decode_i32_device" else SIZE_MAX)
for e in ENCODERS_N:
    row(e, EINVAL, T_SAMPLES, samples_per_channel=0)
    row(e, EINVAL, T_SAMPLES, samples_per_channel=65536)
    row(e, EINVAL, T_SIGNALS, n_frames=1 << 30, channels=2)  # (three signals per stereo frame)
    row(e, EINVAL, T_SIGNALS, n_frames=1 << 30, channels=2, workspace_bytes=SIZE_MAX)
    for p in ("d_frame_offsets", "d_status", "d_workspace", "d_frames", "d_pcm" if "_n_" in e else "d_samples"):
        row(e, EINVAL, T_NULL, **{p: 0})
    row(e, EINVAL, T_ENCODE32_ALIGN, d_frames=A(2) + 2)
    row(e, EINVAL, T_ENCODE32_ALIGN, **({"d_pcm": A(1) + 1} if "_n_" in e else {"d_samples": A(1) + 2}))
    row(e, EINVAL, T_SAMPLES, samples_per_channel=0, d_status=0)  # order: the shape before the pointers
    row(e, EINVAL, T_NULL, d_status=0, d_frames=A(2) + 2, short=1)  # ... the pointers before their alignment and the capacity
for e in ("encode_device", "encode_device_opt"):
    for p in ("d_frame_offsets", "d_status", "d_pcm", "d_frames", "d_workspace"):
        row(e, EINVAL, T_NULL, **{p: 0})
    row(e, EINVAL, T_ENCODE_ALIGN, d_pcm=A(1) + 2)
    row(e, EINVAL, T_ENCODE_ALIGN, d_frames=A(2) + 1)
    row(e, EINVAL, T_NULL, d_status=0, d_pcm=A(1) + 2, short=1)
for e in ENCODERS:
    if e.endswith("_opt"):
        row(e, EINVAL, T_OPTIONS, options=2)
        row(e, EINVAL, T_OPTIONS, options=capi.ENCODE_LOSSLESS | 0x80000000)
        row(e, EINVAL, T_OPTIONS, options=2, channels=0)     # order: the options before the call's own checks
        row(e, EINVAL, T_CHANNELS, options=0, channels=0)    # (no options: the plain call)
row("encode_device_opt", EINVAL, T_LOSSLESS_TRACE, d_trace=A(11))
row("encode_device_opt", EINVAL, T_LOSSLESS_TRACE, d_trace=A(11), channels=0)  # order: before the call's own checks
row("encode_device_opt", EINVAL, T_OPTIONS, d_trace=A(11), options=3)
row("encode_device_opt", EINVAL, T_CHANNELS, d_trace=A(11), options=0, channels=0)

# the index's own checks: alone, and first in every payload call
for e in PAYLOAD + ["index_frames_device"]:
    for p in ("d_frame_offsets", "d_n_frames", "d_workspace", "d_payload"):
        row(e, EINVAL, T_NULL, **{p: 0})
    row(e, EINVAL, T_PAYLOAD_ALIGN, d_payload=A(1) + 2)
    row(e, EINVAL, T_PAYLOAD_SIZE, payload_bytes=4 * 0xFFFFFFFF)
    row(e, EINVAL, T_NULL, d_n_frames=0, d_payload=A(1) + 1, payload_bytes=4 * 0xFFFFFFFF, short=1)
for e in PAYLOAD:  # order: the index's checks before the call's
    row(e, EINVAL, T_PAYLOAD_ALIGN, d_payload=A(1) + 2, d_status=0)
    row(e, EINVAL, T_PAYLOAD_SIZE, payload_bytes=4 * 0xFFFFFFFF, d_status=0, short=1)
    if e in STRIDED:
        row(e, EINVAL, T_PAYLOAD_ALIGN, d_payload=A(1) + 2, stride=0)
        row(e, EINVAL, T_NULL, d_n_frames=0, n_frames=1 << 30)
        row(e, EINVAL, T_STRIDE, stride=0, d_status=0, short=1)  # ... then the call's, in their order
        row(e, EINVAL, T_SUBS, n_frames=1 << 30, d_status=0)

# the frames calls: the call's own checks, then d_frames and its offsets, then the capacity
for e in DECODERS:
    if e in PAYLOAD:
        continue
    row(e, EINVAL, T_NULL, d_frames=0)
    row(e, EINVAL, T_NULL, d_frame_offsets=0)
    row(e, EINVAL, T_FRAMES_ALIGN, d_frames=A(1) + 2)
    row(e, EINVAL, T_FRAMES_ALIGN, d_frames=A(1) + 1, short=1)
    if e in STRIDED:
        row(e, EINVAL, T_STRIDE, stride=0, d_frames=0)
        row(e, EINVAL, T_SUBS, n_frames=1 << 30, d_frames=A(1) + 2)
        row(e, EINVAL, T_NULL, d_status=0, d_frames=A(1) + 2)

# every other pointer of the decoders and verifiers, and the alignment of the compare's arrays
_POINTERS = {
    "decode": ["d_status", "d_pcm_out", "d_workspace"],
    "decode_i32": ["d_status", "d_workspace", "d_samples_out", "d_counts_out"],
    "decode_n": ["d_status", "d_workspace", "d_pcm_out"],
    "verify": ["d_status", "d_workspace", "d_pcm", "d_diff_counts", "d_first_diff"],
    "verify_i32": ["d_status", "d_workspace", "d_samples", "d_diff_counts", "d_first_diff"],
}
for e in DECODERS:
    kind, payload = _kind(e)
    for p in _POINTERS[kind]:
        row(e, EINVAL, T_NULL, **{p: 0})
    if kind == "verify":
        row(e, EINVAL, T_VERIFY_ALIGN, d_pcm=A(6) + 1)
        row(e, EINVAL, T_VERIFY_ALIGN, d_diff_counts=A(9) + 2)
        row(e, EINVAL, T_VERIFY_ALIGN, d_first_diff=A(10) + 2)
        row(e, EINVAL, T_NULL, d_first_diff=0, d_pcm=A(6) + 1)  # order: the pointers before their alignment
        row(e, EINVAL, T_VERIFY_ALIGN, d_pcm=A(6) + 1, short=1)
        if not payload:
            row(e, EINVAL, T_VERIFY_ALIGN, d_pcm=A(6) + 1, d_frames=0)  # ... and that before d_frames
    if kind == "verify_i32":
        for p, base in (("d_samples", A(6)), ("d_lengths", A(7)), ("d_diff_counts", A(9)), ("d_first_diff", A(10))):
            row(e, EINVAL, T_VERIFY32_ALIGN, **{p: base + 2})
        row(e, EINVAL, T_NULL, d_samples=0, d_lengths=A(7) + 2)
        row(e, EINVAL, T_VERIFY32_ALIGN, d_lengths=A(7) + 2, short=1)
        if not payload:
            row(e, EINVAL, T_VERIFY32_ALIGN, d_lengths=A(7) + 2, d_frames=0)


@pytest.mark.parametrize("entry, changes, code, text", ROWS)
def test_refusal(entry, changes, code, text):
    assert _call(entry, **changes) == (code, text)


def test_the_table_covers_every_entry_and_the_passing_arguments_need_a_workspace():
    assert len(ENTRIES) == 17 and {r.values[0] for r in ROWS} == set(ENTRIES)
    for e in ENTRIES:
        need = _workspace_need(e, dict(ENTRIES[e]))
        assert 0 < need < SIZE_MAX, e  # (so that "one byte short" is a capacity that exists)
