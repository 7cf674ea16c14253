"""CPU-only: the host side of sela_hip_encode_i32_device / sela_hip_encode_n_device -- sela_hip_encode_status_error maps status
words to the code the host call returns, in that call's order of checks; the workspace formula needs no GPU and follows the
layout; the frame writer of the shipped code object spills nothing and keeps to 5 KB of LDS."""
import numpy as np
import pytest

from sela_amd import capi, codec

OK, EINVAL, ECAPACITY, ERANGE = 0, -2, -4, -6
Q, COEF, RICE, WORDS, SHORT = capi.FLAG_Q_RANGE, capi.FLAG_COEF_OVERFLOW, capi.FLAG_RICE_RANGE, capi.FLAG_WORDS_CAP, capi.FLAG_SHORT_BLOCK


@pytest.mark.parametrize("status, code", [
    ([0, 0, 0, 0], OK),
    ([Q, 0, 0, 0], OK),                        # (the host call codes such a frame: the encoder's verdict leaves Q_RANGE alone)
    ([SHORT, 0, 0, 0], ERANGE),
    ([RICE, 0, 0, 0], ERANGE),
    ([COEF, 0, 0, 0], ERANGE),
    ([WORDS, 0, 0, 0], ERANGE),
    ([Q | WORDS, 0, 0, 0], ERANGE),
    ([0, 1, 0, 0], ECAPACITY),
    ([Q, 3875, 0, 0], ECAPACITY),
    ([SHORT, 5, 0, 0], ERANGE),                # the flags before the capacity, as the host call checks them
    ([RICE | COEF, 0xFFFFFFFF, 0, 0], ERANGE),
    ([capi.FLAG_RICE_OVERRUN | capi.FLAG_BAD_FRAME | capi.FLAG_STRIDE, 0, 0, 0], OK),  # (decoder flags: no encoder sets them)
])
def test_status_words_give_the_host_calls_code(status, code):
    assert codec.encode_status_error(np.array(status, np.uint32)) == code
    assert codec.encode_status_error(np.array(status, np.int64)) == code  # (the int32 tensor's bit patterns are taken as uint32)


@pytest.mark.parametrize("status, code, text", [
    ([SHORT | RICE, 5, 0, 0], ERANGE,
     "encode: a block is not longer than its predictor order (the reference reads past its vector there, src/lpc/residue_generator.cpp:104-110)"),
    ([RICE | COEF, 0xFFFFFFFF, 0, 0], ERANGE, "encode: a residue is beyond the reference's int32 zig-zag (|value| >= 2^30)"),
    ([COEF | WORDS, 0, 0, 0], ERANGE, "encode: a predictor coefficient left the int64 range"),
    ([Q | WORDS, 0, 0, 0], ERANGE, "encode: a Rice stream needs more words than a subframe's 16-bit count can say"),
    ([Q, 3875, 0, 0], ECAPACITY, "d_frames too small: status[1] frames were not written (d_frame_offsets[n_frames] bytes are needed)"),
])
def test_status_words_give_the_host_calls_text(status, code, text):
    assert codec.encode_status_error(np.array(status, np.uint32)) == code
    assert capi.lib().sela_hip_last_error().decode() == text


def test_status_error_of_a_null_pointer():
    assert capi.lib().sela_hip_encode_status_error(None) == EINVAL


def test_every_single_flag_in_order_of_precedence():
    order = [SHORT, RICE, COEF, WORDS]
    for i, flag in enumerate(order):
        later = 0
        for f in order[i + 1:]:
            later |= f
        assert codec.encode_status_error([flag | later | Q, 7, 0, 0]) == ERANGE, hex(flag)
    assert codec.encode_status_error([Q, 7, 0, 0]) == ECAPACITY


def _layout(frames, ch, n):
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    blocks, subs = frames * (3 if ch == 2 else ch), frames * ch
    # signals, residues (int32 each), q (100 int32), one 28-byte record, word bases (u64, one more), choices (u32), the plan's
    # total (u64): each 256-aligned, and the base's alignment
    return 2 * up(blocks * n * 4) + up(blocks * 400) + up(blocks * 28) + up((subs + 1) * 8) + up(subs * 4) + up(8) + 256


def test_workspace_bytes_without_a_gpu():
    ws = capi.lib().sela_hip_encode_i32_workspace_bytes
    for frames, ch, n in [(0, 1, 1), (1, 1, 1), (1, 2, 2048), (3875, 2, 2048), (4097, 3, 777), (7, 255, 65535), (60, 2, 65535)]:
        assert int(ws(frames, ch, n)) == _layout(frames, ch, n), (frames, ch, n)
    base = int(ws(10, 2, 1000))
    assert int(ws(11, 2, 1000)) > base and int(ws(10, 4, 1000)) > base and int(ws(10, 2, 1001)) > base
    assert int(ws(10, 3, 1000)) >= base  # (a stereo frame analyses three signals, as a three-channel one does)
    assert int(ws(10, 4, 1000)) > int(ws(10, 3, 1000)) > int(ws(10, 1, 1000))
    # what the call refuses has no size
    for frames, ch, n in [(1, 0, 100), (1, 256, 100), (1, 2, 0), (1, 2, 65536), (1 << 30, 2, 1), ((1 << 31) // 255 + 1, 255, 1)]:
        assert int(ws(frames, ch, n)) == (1 << 64) - 1, (frames, ch, n)
    assert int(ws((1 << 31) // 255, 255, 1)) == _layout((1 << 31) // 255, 255, 1)


def test_the_frame_writer_keeps_its_budget():
    """k_generic_write, from the shipped code object: no spill, no scratch, at most 5 KB of LDS (eight waves per SIMD, like
    k_generic_pack); and the plan of the device call spills nothing either."""
    from test_isa_handoffs import _kernel_resources

    res = _kernel_resources()
    names = [n for n in res if "k_generic_write" in n]
    assert len(names) == 1
    r = res[names[0]]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 5 * 1024, r
    plans = [n for n in res if "k_generic_plan" in n]
    assert len(plans) == 2  # (the host route's and the device call's)
    for n in plans:
        assert res[n]["vgpr_spill"] == 0 and res[n]["scratch"] == 0, (n, res[n])
