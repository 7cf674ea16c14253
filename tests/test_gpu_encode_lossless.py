"""SELA_HIP_ENCODE_LOSSLESS: every *_opt encode call against the CPU model of the mode (tests/lossless_model.py,
pinned to the oracle and to the reference's decoder by tests/test_lossless_model_cpu.py) byte for byte -- on every kernel and
every form of the residue filter -- and through this project's own verifiers and decoders.  The cases hold frames with a tie in
a stored candidate, with a tie in a discarded one, and clean neighbours; the plain calls on the same inputs are the control."""
import ctypes as C

import numpy as np
import pytest

import corpus
import lossless_model as model
from gpu_common import _wrap_taps, gpu, teams  # noqa: F401
from oracle_lib import oracle
from sela_amd import capi, codec

pytestmark = pytest.mark.gpu

LOSSLESS = capi.ENCODE_LOSSLESS
POISON = 0xA5
A_LOSSY = [1, 4, 5, 6]  # frames 401, 1128, 1158, 1182 of the corpus within case A


@pytest.fixture(scope="module")
def streams():
    """case -> {False: (bytes, offsets) of the plain model, True: of the lossless one}; R: {False / True: the frame's bytes}."""
    o = oracle()
    out = {}
    for name, frames in model.cases().items():
        if name == "R":
            out[name] = {mode: model.encode_frame(o, frames[0], mode) for mode in (False, True)}
        else:
            out[name] = {mode: model.stream(o, frames, mode) for mode in (False, True)}
    return out


def _pcm(name):
    return model.interleaved(model.cases()[name])


def _same(got, want, label):
    frames, offs = got
    assert np.array_equal(np.asarray(offs, np.uint64), want[1]), (label, "offsets")
    assert np.asarray(frames).tobytes() == want[0].tobytes(), (label, "bytes")


def _fast(torch, pcm, lossless=True):
    """The 2048-sample device call -> (frames, offsets, encoder, EncodedFrames)."""
    enc = codec.Encoder(pcm.shape[0], pcm.shape[2], lossless=lossless)
    out = enc.encode(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    st = out.status.cpu().numpy()
    assert int(st[0]) & ~capi.FLAG_Q_RANGE == 0 and not st[1:].any(), st  # ([2], [3] stay zero)
    frames, offs = out.to_host()
    return frames, offs, enc, out


def _natural_forms(frames):
    """The residue filter's form of every block (ch0, ch1, difference per frame) by the rule of sela_encode_tail.inc."""
    o = oracle()
    forms = []
    for x in frames:
        for s in (x[0], x[1], (x[0] - x[1]).astype(np.int32)):
            order, _, _, a, _, _ = o.lpc_analyze(s, with_trace=True)
            forms.append(corpus.expected_form(a, order, s))
    return np.array(forms, np.uint8)


def _every_form(torch, streams):
    """Case A on the kernel that is selected, under sela_hip_debug_force_plain_fir 0, 1 and 2: the model's bytes, and the forms asked for."""
    lib = capi.lib()
    pcm = _pcm("A")
    natural = _natural_forms(model.cases()["A"])
    seen = set()
    try:
        for force in (0, 1, 2):
            lib.sela_hip_debug_force_plain_fir(force)
            frames, offs, enc, _ = _fast(torch, pcm)
            _same((frames, offs), streams["A"][True], ("A", force))
            counts = (C.c_uint32 * 3)()
            forms = np.zeros(len(natural), np.uint8)
            assert lib.sela_hip_debug_block_forms(enc.workspace.data_ptr(), len(pcm), 2, counts, forms.ctypes.data) == 0
            want = natural if force == 0 else (np.full_like(natural, 2) if force == 1 else np.maximum(natural, 1))
            assert np.array_equal(forms, want), (force, forms.tolist(), want.tolist())
            # (the blocks whose stored candidate holds a tie: ch1 of frame 1, ch0 of frames 4, 5, 6)
            seen |= {int(forms[b]) for b in (1 * 3 + 1, 4 * 3 + 0, 5 * 3 + 0, 6 * 3 + 0)}
    finally:
        lib.sela_hip_debug_force_plain_fir(0)
    assert seen == {0, 1, 2}, seen  # (they are one-pass blocks by the rule: all three forms have coded a tie)


# ---- 1. byte parity with the model: three kernels x three forms ------------------------------------------------------------------
def test_the_kernel_the_launch_size_picks_in_every_form(gpu, streams):  # noqa: F811
    assert capi.lib().sela_hip_debug_encode_kernel(10, 2) == 0  # (ten frames: k_encode_blocks)
    _every_form(gpu, streams)


def test_the_team_kernels_in_every_form(gpu, teams, streams):  # noqa: F811
    assert capi.lib().sela_hip_debug_encode_kernel(10, 2) == teams
    _every_form(gpu, streams)


# ---- 2. round trips, and the other device calls -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "M", "T"])
def test_fast_kernels_round_trip(gpu, streams, case):  # noqa: F811
    torch = gpu
    pcm = _pcm(case)
    nf, _, ch = pcm.shape
    frames, offs, enc, out = _fast(torch, pcm)
    _same((frames, offs), streams[case][True], case)
    d_pcm = torch.from_numpy(pcm).cuda()
    ver = codec.Verifier(nf, ch, 2048)
    ver.verify(out.frames, out.offsets, nf, d_pcm)
    ver.check()
    assert ver.lossy_frames() == 0
    dec = codec.Decoder(nf, ch)
    back = dec.decode(out.frames, out.offsets, nf)
    torch.cuda.synchronize()
    dec.check()
    assert np.array_equal(back.cpu().numpy(), pcm)


@pytest.mark.parametrize("wrap", [False, True], ids=["taps_by_the_bound", "wrap_around_taps"])
def test_wide_frames_through_the_i32_device_call(gpu, streams, wrap):  # noqa: F811
    torch = gpu
    x = np.ascontiguousarray(np.stack(model.cases()["W"]))
    _wrap_taps(wrap)
    try:
        enc = codec.Encoder32(len(x), 2, 2048, lossless=True)
        d_x = torch.from_numpy(x).cuda()
        frames, offsets, status = enc.encode(d_x)
        _same(enc.to_host(), streams["W"][True], ("W", wrap))
        assert not status.cpu().numpy()[1:].any()
        ver = codec.Verifier32(len(x), 2, 2048)
        ver.verify(frames, offsets, len(x), d_x)
        ver.check()
        assert ver.lossy_frames() == 0
        plain = codec.Encoder32(len(x), 2, 2048)  # the control: today's call loses frames 187, 642, 906 and 939
        frames, offsets, _ = plain.encode(d_x)
        _same(plain.to_host(), streams["W"][False], ("W plain", wrap))
        counts, _ = ver.verify(frames, offsets, len(x), d_x)
        assert (counts.cpu().numpy() != 0).tolist() == [False, True, True, True, True]
    finally:
        _wrap_taps(False)


@pytest.mark.parametrize("case, wrap", [("N1000", False), ("N300", False), ("N1000", True), ("N300", True)])
def test_short_frames_through_the_n_device_call(gpu, streams, case, wrap):  # noqa: F811
    torch = gpu
    pcm = _pcm(case)
    nf, n, ch = pcm.shape
    _wrap_taps(wrap)
    try:
        enc = codec.Encoder32(nf, ch, n, lossless=True)
        d_pcm = torch.from_numpy(pcm).cuda()
        frames, offsets, _ = enc.encode(d_pcm)
        _same(enc.to_host(), streams[case][True], (case, wrap))
        ver = codec.Verifier(nf, ch, n)
        ver.verify(frames, offsets, nf, d_pcm)
        ver.check()
        assert ver.lossy_frames() == 0
    finally:
        _wrap_taps(False)


# ---- 3. host calls and the one-launch form ----------------------------------------------------------------------------------------
def test_one_shot_host_calls(gpu, streams):  # noqa: F811
    o = oracle()
    r = model.cases()["R"][0]
    assert codec.encode_ragged(r, lossless=True) == streams["R"][True]
    assert codec.encode_ragged(r) == streams["R"][False] == o.frame_encode_ragged(r) != streams["R"][True]
    _same(codec.encode_host(_pcm("A"), lossless=True), streams["A"][True], "sela_hip_encode_opt")
    _same(codec.encode_i32(np.stack(model.cases()["A"]), lossless=True), streams["A"][True], "sela_hip_encode_i32_opt, 2048")
    _same(codec.encode_i32(np.stack(model.cases()["W"]), lossless=True), streams["W"][True], "sela_hip_encode_i32_opt, wide")
    _same(codec.encode_host(_pcm("N1000"), lossless=True), streams["N1000"][True], "sela_hip_encode_opt, 1000 samples")
    _same(codec.encode_i32(np.stack(model.cases()["N300"]), lossless=True), streams["N300"][True], "sela_hip_encode_i32_opt, 300 samples")


def _job(pcm, cuts, options):
    """begin(_opt) / one feed per piece / end -> (frames, offsets)."""
    lib = capi.lib()
    nf, _, ch = pcm.shape
    cap = int(lib.sela_hip_encode_bound_bytes(nf, ch))
    out = np.zeros(cap, np.uint8)
    offs = np.zeros(nf + 1, np.uint64)
    job = C.c_void_p()
    if options is None:
        capi.check(lib.sela_hip_encode_begin(C.byref(job), ch, nf, out.ctypes.data, cap, offs.ctypes.data))
    else:
        capi.check(lib.sela_hip_encode_begin_opt(C.byref(job), ch, nf, out.ctypes.data, cap, offs.ctypes.data, options))
    pieces = [np.ascontiguousarray(pcm[a:b]) for a, b in zip([0] + cuts, cuts + [nf])]  # (alive until the job ends)
    rc = 0
    for p in pieces:
        rc = rc or lib.sela_hip_encode_feed(job, p.ctypes.data, len(p), None, None)
    total = C.c_uint64(0)
    rc_end = lib.sela_hip_encode_end(job, None, C.byref(total))
    capi.check(rc)
    capi.check(rc_end)
    assert total.value == int(offs[nf])
    return out[: total.value].copy(), offs


@pytest.mark.parametrize("fused", [0, 1], ids=["three_kernels", "one_launch"])
def test_streaming_job_and_the_one_launch_form(gpu, streams, fused):  # noqa: F811
    lib = capi.lib()
    pcm = _pcm("A")
    lib.sela_hip_debug_encode_fused(fused)
    try:
        _same(_job(pcm, [6], LOSSLESS), streams["A"][True], "job, lossless")
        _same(_job(pcm, [6], 0), streams["A"][False], "job, options 0")
        _same(_job(pcm, [6], None), streams["A"][False], "job, plain")
        frames, offs, _, _ = _fast(gpu, pcm)  # (with the hook on: k_encode_blocks' one-launch form on device pointers)
        _same((frames, offs), streams["A"][True], "device call")
    finally:
        lib.sela_hip_debug_encode_fused(0)


def test_an_open_job_is_left_alone(gpu, streams):  # noqa: F811
    """A thread in the middle of a plain streaming job makes lossless one-shot calls: they take the any-length route, and the job
    goes on to write the plain stream."""
    lib = capi.lib()
    pcm = _pcm("A")
    nf, _, ch = pcm.shape
    cap = int(lib.sela_hip_encode_bound_bytes(nf, ch))
    out = np.zeros(cap, np.uint8)
    offs = np.zeros(nf + 1, np.uint64)
    job = C.c_void_p()
    first, rest = np.ascontiguousarray(pcm[:4]), np.ascontiguousarray(pcm[4:])
    capi.check(lib.sela_hip_encode_begin(C.byref(job), ch, nf, out.ctypes.data, cap, offs.ctypes.data))
    try:
        capi.check(lib.sela_hip_encode_feed(job, first.ctypes.data, 4, None, None))
        _same(codec.encode_host(pcm, lossless=True), streams["A"][True], "one-shot beside the job")
        capi.check(lib.sela_hip_encode_feed(job, rest.ctypes.data, nf - 4, None, None))
    finally:
        total = C.c_uint64(0)
        rc = lib.sela_hip_encode_end(job, None, C.byref(total))
    capi.check(rc)
    _same((out[: total.value], offs), streams["A"][False], "the job's own stream")


# ---- 4. baselines and argument errors ---------------------------------------------------------------------------------------------
def test_options_zero_is_the_plain_call_and_the_plain_call_still_loses_four_frames(gpu, streams):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    pcm = _pcm("A")
    nf, _, ch = pcm.shape
    frames, offs, enc, out = _fast(torch, pcm, lossless=False)
    _same((frames, offs), streams["A"][False], "sela_hip_encode_device")
    d_pcm = torch.from_numpy(pcm).cuda()
    ver = codec.Verifier(nf, ch, 2048)
    counts, _ = ver.verify(out.frames, out.offsets, nf, d_pcm)
    ver.check()
    assert np.flatnonzero(counts.cpu().numpy()).tolist() == A_LOSSY and ver.lossy_frames() == 4  # the control: the inputs bite
    # options = 0 through every *_opt call
    other = codec.Encoder(nf, ch)
    capi.check(lib.sela_hip_encode_device_opt(d_pcm.data_ptr(), nf, ch, other.frames.data_ptr(), other.capacity, other.offsets.data_ptr(), other.status.data_ptr(),
                                              other.workspace.data_ptr(), other.workspace.numel(), None, torch.cuda.current_stream().cuda_stream, 0))
    torch.cuda.synchronize()
    _same((other.frames[: len(frames)].cpu().numpy(), other.offsets[: nf + 1].cpu().numpy().view(np.uint64)), streams["A"][False], "device_opt, options 0")
    for name, call, pre in (("N1000", lib.sela_hip_encode_n_device_opt, _pcm), ("W", lib.sela_hip_encode_i32_device_opt, lambda c: np.stack(model.cases()[c]))):
        x = np.ascontiguousarray(pre(name))
        n = x.shape[1] if x.dtype == np.int16 else x.shape[2]
        e32 = codec.Encoder32(len(x), 2, n)
        d_x = torch.from_numpy(x).cuda()
        capi.check(call(d_x.data_ptr(), len(x), 2, n, e32.frames.data_ptr(), e32.capacity, e32.offsets.data_ptr(), e32.status.data_ptr(), e32.workspace.data_ptr(),
                        e32.workspace.numel(), torch.cuda.current_stream().cuda_stream, 0))
        e32.n_frames = len(x)
        _same(e32.to_host(), streams[name][False], (name, "options 0"))
    cap = int(lib.sela_hip_encode_bound_bytes(nf, ch))
    buf, o = np.zeros(cap, np.uint8), np.zeros(nf + 1, np.uint64)
    capi.check(lib.sela_hip_encode_opt(pcm.ctypes.data, nf, ch, 2048, buf.ctypes.data, cap, o.ctypes.data, 0))
    _same((buf[: int(o[nf])], o), streams["A"][False], "sela_hip_encode_opt, options 0")
    x = np.ascontiguousarray(np.stack(model.cases()["A"]))
    capi.check(lib.sela_hip_encode_i32_opt(x.ctypes.data, nf, ch, 2048, buf.ctypes.data, cap, o.ctypes.data, 0))
    _same((buf[: int(o[nf])], o), streams["A"][False], "sela_hip_encode_i32_opt, options 0")


def test_argument_errors_enqueue_nothing(gpu):  # noqa: F811
    torch = gpu
    lib = capi.lib()
    pcm = _pcm("N300")
    nf, n, ch = pcm.shape
    full = _pcm("A")[:2]
    d16 = torch.from_numpy(pcm).cuda()
    d32 = torch.from_numpy(np.ascontiguousarray(np.stack(model.cases()["N300"]))).cuda()
    dfull = torch.from_numpy(full).cuda()
    frames = torch.full((1 << 18,), POISON, dtype=torch.uint8, device="cuda")
    offs = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(int(lib.sela_hip_encode_workspace_bytes(2, 2)), int(lib.sela_hip_encode_i32_workspace_bytes(nf, ch, n))), dtype=torch.uint8, device="cuda")
    trace = torch.zeros(2 * 3 * C.sizeof(capi.Trace), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    out = (frames.data_ptr(), frames.numel(), offs.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel())

    def fast(options, tr=None):
        return lib.sela_hip_encode_device_opt(dfull.data_ptr(), 2, 2, *out, tr, stream, options)

    host_out, host_offs = np.full(1 << 18, POISON, np.uint8), np.full(8, 7, np.uint64)
    used = C.c_size_t(99)
    job = C.c_void_p()
    x32 = np.ascontiguousarray(np.stack(model.cases()["N300"]))
    lengths = np.array([n, n], np.uint32)
    calls = [
        (lambda: fast(2), -2), (lambda: fast(LOSSLESS | 2), -2), (lambda: fast(0x80000000), -2), (lambda: fast(2, trace.data_ptr()), -2),
        (lambda: fast(LOSSLESS, trace.data_ptr()), -2),  # the trace is the reference's arithmetic
        (lambda: lib.sela_hip_encode_n_device_opt(d16.data_ptr(), nf, ch, n, *out, stream, 2), -2),
        (lambda: lib.sela_hip_encode_i32_device_opt(d32.data_ptr(), nf, ch, n, *out, stream, LOSSLESS | 4), -2),
        (lambda: lib.sela_hip_encode_opt(pcm.ctypes.data, nf, ch, n, host_out.ctypes.data, host_out.size, host_offs.ctypes.data, 2), -2),
        (lambda: lib.sela_hip_encode_i32_opt(x32.ctypes.data, nf, ch, n, host_out.ctypes.data, host_out.size, host_offs.ctypes.data, 8), -2),
        (lambda: lib.sela_hip_encode_ragged_i32_opt(x32.ctypes.data, lengths.ctypes.data, 2, host_out.ctypes.data, host_out.size, C.byref(used), 2), -2),
        (lambda: lib.sela_hip_encode_begin_opt(C.byref(job), 2, 2, host_out.ctypes.data, host_out.size, host_offs.ctypes.data, 2), -2),
        # ... and what the namesakes refuse, with the option set
        (lambda: lib.sela_hip_encode_device_opt(dfull.data_ptr(), 2, 0, *out, None, stream, LOSSLESS), -2),
        (lambda: lib.sela_hip_encode_device_opt(dfull.data_ptr(), 2, 2, *out[:5], 16, None, stream, LOSSLESS), -4),
        (lambda: lib.sela_hip_encode_n_device_opt(d16.data_ptr(), nf, ch, 0, *out, stream, LOSSLESS), -2),
        (lambda: lib.sela_hip_encode_i32_device_opt(d32.data_ptr(), nf, ch, n, *out[:5], 16, stream, LOSSLESS), -4),
    ]
    for i, (call, code) in enumerate(calls):
        assert call() == code, i
    torch.cuda.synchronize()  # nothing was enqueued or written: every output is as it was
    assert (frames.cpu().numpy() == POISON).all() and (offs.cpu().numpy() == -1).all() and (status.cpu().numpy() == -1).all()
    assert (host_out == POISON).all() and (host_offs == 7).all() and used.value == 99 and not job.value
    # the same buffers take the call as it is meant
    assert fast(LOSSLESS) == 0
    torch.cuda.synchronize()
    assert codec.encode_status_error(status.cpu().numpy()) == 0 and int(offs[0].item()) == 0 and int(offs[2].item()) > 0


# ---- 5. graph capture -------------------------------------------------------------------------------------------------------------
def test_graph_replay_on_new_samples(gpu, streams):  # noqa: F811
    torch = gpu
    w = np.ascontiguousarray(np.stack(model.cases()["W"]))
    enc = codec.Encoder32(len(w), 2, 2048, lossless=True)
    d_x = torch.from_numpy(np.ascontiguousarray(w[::-1])).cuda()  # (captured on other samples: the frames in reverse)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.encode(d_x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enc.encode(d_x)
    d_x.copy_(torch.from_numpy(w))
    enc.frames.fill_(POISON)
    enc.status.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    _same(enc.to_host(), streams["W"][True], "replay")
