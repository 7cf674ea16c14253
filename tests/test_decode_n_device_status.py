"""CPU-only: the host side of sela_hip_decode_n_device -- sela_hip_decode_n_status_error maps status words to the code
sela_hip_decode returns, by the route the device took (the streaming job's mapping behind the 2048-sample decoder,
generic_decode's order behind the any-length kernels, EFORMAT where the walk refuses the stream); the workspace formula needs no
GPU; the new kernels of the shipped code object spill nothing."""
import numpy as np
import pytest

from sela_amd import capi, codec

OK, ENODEV, EINVAL, ECAPACITY, EFORMAT, ERANGE = 0, -1, -2, -4, -5, -6
Q, COEF, OVERRUN, BAD, INTERNAL, SHORT, STRIDE = (capi.FLAG_Q_RANGE, capi.FLAG_COEF_OVERFLOW, capi.FLAG_RICE_OVERRUN, capi.FLAG_BAD_FRAME,
                                                 capi.FLAG_INTERNAL, capi.FLAG_SHORT_BLOCK, capi.FLAG_STRIDE)
NONE, FAST, ANY = 0, 1, 2  # status[3]: the route

# each route's flags in its order of precedence, each with the code it gives
ORDER = {
    FAST: [(STRIDE, ECAPACITY), (BAD, EFORMAT), (OVERRUN, EFORMAT), (COEF, ERANGE), (Q, ERANGE)],  # job_end; SHORT / INTERNAL: not looked at
    ANY: [(STRIDE, ECAPACITY), (BAD, EFORMAT), (OVERRUN, EFORMAT), (COEF, ERANGE), (Q, ERANGE), (SHORT, ERANGE), (INTERNAL, ENODEV)],
    NONE: [(STRIDE, ECAPACITY), (BAD, EFORMAT)],
}


@pytest.mark.parametrize("status, code", [
    ([0, 0, 0, NONE], OK),                      # no frames
    ([0, 0, 2048, FAST], OK),
    ([0, 0, 65535, ANY], OK),
    ([STRIDE, 0, 2048, NONE], ECAPACITY),       # a 2048 stream and stride < 2048
    ([STRIDE, 0, 4096, NONE], ECAPACITY),
    ([BAD, 0, 0, NONE], EFORMAT),               # the walk breaks, offsets decrease, or the largest length is 0
    ([BAD, 0, 700, NONE], EFORMAT),
    ([BAD, 1, 2048, FAST], EFORMAT),
    ([0, 1, 2048, FAST], EFORMAT),
    ([OVERRUN | COEF | Q, 0, 2048, FAST], EFORMAT),
    ([COEF | Q, 0, 2048, FAST], ERANGE),
    ([Q, 0, 2048, FAST], ERANGE),
    ([SHORT, 0, 2048, FAST], OK),                # (what the job's verdict does not look at)
    ([INTERNAL, 0, 2048, FAST], OK),
    ([BAD | SHORT, 2, 700, ANY], EFORMAT),
    ([0, 1, 700, ANY], EFORMAT),
    ([SHORT | INTERNAL, 0, 3, ANY], ERANGE),
    ([INTERNAL, 0, 700, ANY], ENODEV),
    ([capi.FLAG_RICE_RANGE | capi.FLAG_WORDS_CAP, 0, 2048, FAST], OK),  # (encoder flags: no decoder sets them)
    ([capi.FLAG_RICE_RANGE | capi.FLAG_WORDS_CAP, 0, 700, ANY], OK),
])
def test_status_words_give_the_host_calls_code(status, code):
    assert codec.decode_n_status_error(np.array(status, np.uint32)) == code
    assert codec.decode_n_status_error(np.array(status, np.int64)) == code  # (the int32 tensor's bit patterns are taken as uint32)


@pytest.mark.parametrize("route", [NONE, FAST, ANY])
def test_every_single_flag_in_order_of_precedence(route):
    order = ORDER[route]
    for i, (flag, code) in enumerate(order):
        later = 0
        for f, _ in order[i + 1:]:
            later |= f
        assert codec.decode_n_status_error([flag, 0, 0, route]) == code, (route, hex(flag))
        assert codec.decode_n_status_error([flag | later, 0, 0, route]) == code, (route, hex(flag))


def test_the_any_length_route_maps_as_the_i32_call():
    rng = np.random.default_rng(5)
    for _ in range(300):
        st = [int(rng.integers(0, 512)), int(rng.integers(0, 2)), int(rng.integers(0, 70000)), ANY]
        assert codec.decode_n_status_error(st) == codec.decode_status_error(st[:3] + [0]), st


T_STRIDE = "stride is smaller than the largest samplesPerChannel of the stream (status[2])"
T_BAD = {
    NONE: "malformed frame stream (the header walk breaks, frame offsets decrease, or no subframe says a length)",
    FAST: "malformed frame stream (bad sync word or subframe header)",
    ANY: ("malformed frame (decreasing offsets, sync word, sizes, an order above 100, a Rice parameter above 31, a channel or parent that does not exist, "
          "or channels of different lengths)"),
}
T_OVERRUN = "a Rice stream ended before all its values were read"
T_COEF = "decode: a predictor coefficient left the int64 range"
T_Q = "decode: a quantised reflection coefficient outside [-64, 63] (the reference indexes past its tables, src/lpc/linear_predictor.cpp:23-26)"
T_SHORT = ("decode: a subframe without samples or not longer than its predictor order (the reference writes past its vector, "
           "src/lpc/sample_generator.cpp:14-22)")
T_INTERNAL = "decode: a bounded wait inside a kernel ran out"


@pytest.mark.parametrize("status, code, text", [
    ([STRIDE | BAD, 0, 4096, NONE], ECAPACITY, T_STRIDE),
    ([STRIDE | BAD, 0, 4096, FAST], ECAPACITY, T_STRIDE),
    ([STRIDE | BAD, 0, 4096, ANY], ECAPACITY, T_STRIDE),
    ([BAD, 0, 700, NONE], EFORMAT, T_BAD[NONE]),
    ([0, 1, 2048, FAST], EFORMAT, T_BAD[FAST]),
    ([BAD | SHORT, 2, 700, ANY], EFORMAT, T_BAD[ANY]),
    ([OVERRUN | COEF | Q, 0, 2048, FAST], EFORMAT, T_OVERRUN),
    ([OVERRUN | COEF | Q, 0, 700, ANY], EFORMAT, T_OVERRUN),
    ([COEF | Q, 0, 2048, FAST], ERANGE, T_COEF),
    ([Q | SHORT, 0, 2048, FAST], ERANGE, T_Q),
    ([Q | SHORT, 0, 700, ANY], ERANGE, T_Q),
    ([SHORT | INTERNAL, 0, 3, ANY], ERANGE, T_SHORT),
    ([INTERNAL, 0, 700, ANY], ENODEV, T_INTERNAL),
])
def test_status_words_give_the_host_calls_text(status, code, text):
    assert codec.decode_n_status_error(np.array(status, np.uint32)) == code
    assert capi.lib().sela_hip_last_error().decode() == text


def test_status_error_of_a_null_pointer():
    assert capi.lib().sela_hip_decode_n_status_error(None) == EINVAL


def test_workspace_bytes_without_a_gpu():
    lib = capi.lib()
    ws = lib.sela_hip_decode_n_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for frames, ch, stride in [(0, 1, 1), (1, 1, 1), (1, 2, 2048), (3875, 2, 2048), (4097, 3, 777), (550_000, 2, 2048), (5, 8, 4096),
                               (5, 9, 4096), (7, 255, 65535)]:
        got = int(ws(frames, ch, stride))
        subs = frames * ch
        tiles = max(1, (frames + 4095) // 4096)
        # decoded subframes (int32) + one 8-byte record per subframe + counters + one 16-byte record per 4096 frames + the sample
        # offsets, and above 8 channels the combine's channel-major copy, each 256-aligned, and the base's alignment
        want = up(subs * stride * 4) + up(subs * 8) + up(32) + up(tiles * 16) + up((frames + 1) * 8) + 256
        if ch > 8:
            want += up(subs * stride * 4)
        assert got == want, (frames, ch, stride)
        # one int32 array of decoded samples for up to 8 channels (the i32 call's workspace plus the sample offsets)
        if ch <= 8:
            assert got == int(lib.sela_hip_decode_i32_workspace_bytes(frames, ch, stride)) + up((frames + 1) * 8)
    for a, b in [((3, 2, 2048), (4, 2, 2048)), ((4, 2, 2048), (4, 3, 2048)), ((4, 2, 2048), (4, 2, 4096)), ((4, 8, 100), (4, 9, 100)),
                 ((0, 1, 1), (1, 1, 1))]:
        assert int(ws(*a)) < int(ws(*b)), (a, b)
    assert int(ws(0xFFFFFFFF, 255, 0xFFFFFFFF)) == (1 << 64) - 1  # (beyond what any device holds: SIZE_MAX, never a wrapped size)


def test_the_new_kernels_spill_nothing():
    """The router and the int16 writer, from the shipped code object: no spill, no scratch; the names the existing tests count
    by substring gain no match."""
    from test_isa_handoffs import _kernel_resources

    res = _kernel_resources()
    for part in ("k_route_n", "k_interleave16"):
        names = [n for n in res if part in n]
        assert len(names) == 1, (part, names)
        r = res[names[0]]
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (names[0], r)
    assert res[[n for n in res if "k_interleave16" in n][0]]["lds"] <= 16 * 1024
    assert len([n for n in res if "k_index_samples" in n]) == 2
    assert len([n for n in res if "k_decode_framesILb0E" in n]) == 1
