"""CPU-only: the host side of sela_hip_decode_i32_device -- sela_hip_decode_status_error maps status words to the code
sela_hip_decode_i32 returns, in that call's order of checks; the workspace formula needs no GPU; the sample-index kernels of the
shipped code object spill nothing."""
import numpy as np
import pytest

from sela_amd import capi, codec

OK, ENODEV, EINVAL, ECAPACITY, EFORMAT, ERANGE = 0, -1, -2, -4, -5, -6
Q, COEF, OVERRUN, BAD, INTERNAL, SHORT, STRIDE = (capi.FLAG_Q_RANGE, capi.FLAG_COEF_OVERFLOW, capi.FLAG_RICE_OVERRUN, capi.FLAG_BAD_FRAME,
                                                 capi.FLAG_INTERNAL, capi.FLAG_SHORT_BLOCK, capi.FLAG_STRIDE)


@pytest.mark.parametrize("status, code", [
    ([0, 0, 0, 0], OK),
    ([0, 0, 2048, 0], OK),                     # [2] is the stream's largest length, not an error
    ([0, 0, 65535, 0], OK),
    ([STRIDE, 0, 4096, 0], ECAPACITY),
    ([STRIDE | BAD, 3, 4096, 0], ECAPACITY),   # the host call refuses the stride before it decodes anything
    ([STRIDE | COEF | Q | SHORT | OVERRUN, 0, 9, 0], ECAPACITY),
    ([BAD, 1, 0, 0], EFORMAT),                 # a malformed frame (decreasing offsets are one on the device)
    ([0, 1, 0, 0], EFORMAT),
    ([OVERRUN, 0, 700, 0], EFORMAT),
    ([BAD | COEF | Q | SHORT, 2, 0, 0], EFORMAT),
    ([OVERRUN | COEF, 0, 700, 0], EFORMAT),
    ([COEF, 0, 700, 0], ERANGE),
    ([Q, 0, 700, 0], ERANGE),
    ([SHORT, 0, 3, 0], ERANGE),
    ([Q | SHORT | INTERNAL, 0, 3, 0], ERANGE),
    ([INTERNAL, 0, 2048, 0], ENODEV),
    ([capi.FLAG_RICE_RANGE | capi.FLAG_WORDS_CAP, 0, 2048, 0], OK),  # (encoder flags: no decoder sets them)
])
def test_status_words_give_the_host_calls_code(status, code):
    assert codec.decode_status_error(np.array(status, np.uint32)) == code
    assert codec.decode_status_error(np.array(status, np.int64)) == code  # (the int32 tensor's bit patterns are taken as uint32)


T_STRIDE = "stride is smaller than the largest samplesPerChannel of the stream (status[2])"
T_BAD = ("malformed frame (decreasing offsets, sync word, sizes, an order above 100, a Rice parameter above 31, a channel or parent that does not exist, "
         "or channels of different lengths)")
T_OVERRUN = "a Rice stream ended before all its values were read"
T_COEF = "decode: a predictor coefficient left the int64 range"
T_Q = "decode: a quantised reflection coefficient outside [-64, 63] (the reference indexes past its tables, src/lpc/linear_predictor.cpp:23-26)"
T_SHORT = ("decode: a subframe without samples or not longer than its predictor order (the reference writes past its vector, "
           "src/lpc/sample_generator.cpp:14-22)")
T_INTERNAL = "decode: a bounded wait inside a kernel ran out"


@pytest.mark.parametrize("status, code, text", [
    ([STRIDE | BAD, 3, 4096, 0], ECAPACITY, T_STRIDE),
    ([BAD | COEF | Q | SHORT, 2, 0, 0], EFORMAT, T_BAD),
    ([0, 1, 0, 0], EFORMAT, T_BAD),
    ([OVERRUN | COEF, 0, 700, 0], EFORMAT, T_OVERRUN),
    ([COEF | Q, 0, 700, 0], ERANGE, T_COEF),
    ([Q | SHORT | INTERNAL, 0, 3, 0], ERANGE, T_Q),
    ([SHORT | INTERNAL, 0, 3, 0], ERANGE, T_SHORT),
    ([INTERNAL, 0, 2048, 0], ENODEV, T_INTERNAL),
])
def test_status_words_give_the_host_calls_text(status, code, text):
    assert codec.decode_status_error(np.array(status, np.uint32)) == code
    assert capi.lib().sela_hip_last_error().decode() == text


def test_status_error_of_a_null_pointer():
    assert capi.lib().sela_hip_decode_status_error(None) == EINVAL


def test_every_single_flag_in_order_of_precedence():
    order = [(STRIDE, ECAPACITY), (BAD, EFORMAT), (OVERRUN, EFORMAT), (COEF, ERANGE), (Q, ERANGE), (SHORT, ERANGE), (INTERNAL, ENODEV)]
    for i, (flag, code) in enumerate(order):
        later = 0
        for f, _ in order[i + 1:]:
            later |= f
        assert codec.decode_status_error([flag | later, 0, 0, 0]) == code, hex(flag)


def test_workspace_bytes_without_a_gpu():
    lib = capi.lib()
    ws = lib.sela_hip_decode_i32_workspace_bytes
    for frames, ch, stride in [(0, 1, 1), (1, 1, 1), (1, 2, 2048), (3875, 2, 2048), (4097, 3, 777), (550_000, 2, 2048), (7, 255, 65535)]:
        got = int(ws(frames, ch, stride))
        subs = frames * ch
        tiles = max(1, (frames + 4095) // 4096)
        # decoded subframes (int32) + one 8-byte record per subframe + counters + one 16-byte record per 4096 frames, each
        # 256-aligned, and the base's alignment
        up = lambda b: (b + 255) // 256 * 256  # noqa: E731
        assert got == up(subs * stride * 4) + up(subs * 8) + up(16) + up(tiles * 16) + 256, (frames, ch, stride)
    assert int(ws(4, 2, 4096)) >= int(ws(4, 2, 2048)) >= int(ws(3, 2, 2048))
    assert int(ws(0xFFFFFFFF, 255, 0xFFFFFFFF)) == (1 << 64) - 1  # (beyond what any device holds: SIZE_MAX, never a wrapped size)


def test_the_sample_index_kernels_spill_nothing():
    """The new kernels of the device-pointer 32-bit decode, from the shipped code object: no spill, no scratch; and the fast
    kernel of any length keeps its budget with the device-side frame count (72 VGPRs, no spill, 5.8 KB of LDS)."""
    from test_isa_handoffs import _kernel_resources

    res = _kernel_resources()
    for part in ("k_index_samples", "k_sample_tiles", "k_sample_spread"):
        names = [n for n in res if part in n]
        assert names, part
        for n in names:
            r = res[n]
            assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
    assert len([n for n in res if "k_index_samples" in n]) == 2  # (one tile and many)
    for n in [n for n in res if "k_decode_subframes32" in n]:
        r = res[n]
        assert r["vgpr"] <= 72 and r["vgpr_spill"] == 0 and r["lds"] <= 160 * 1024 // 28, (n, r)
