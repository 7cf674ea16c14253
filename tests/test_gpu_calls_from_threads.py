"""GPU tests, by subject: one-shot host-pointer calls from many threads at once, which the library merges into device batches
(sela_amd/csrc/sela_coalescer.h) -- the 32-bit calls of frame::FrameEncoder / FrameDecoder (sela_hip_encode_i32 /
sela_hip_decode_i32) and sela_hip_decode -- and one-shot calls made while the calling thread has a streaming job open.  Every
accepted call against the oracle, every refused call's code and its own thread's last error (include/sela_hip.h: "Every call
still gets exactly its own result and its own error")."""
import ctypes as C
import threading
import time

import numpy as np
import pytest
from oracle_lib import oracle
from sela_amd.synth import synth_frames, synth_pcm

from gpu_common import _build_frame, gpu  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

DECODE, ENCODE, DECODE32, ENCODE32 = 0, 1, 2, 3  # the coalescer's kinds (sela_hip_debug_coalesced)
BAD_DECODE_FLAGS = 1 | 2 | 8 | 32 | 128  # the oracle's Q_RANGE, COEF_OVERFLOW, RICE_OVERRUN, BAD_FRAME, SHORT_BLOCK


def _coalesced(kind):
    from sela_amd import capi

    b, r = C.c_longlong(-1), C.c_longlong(-1)
    capi.lib().sela_hip_debug_coalesced(kind, C.byref(b), C.byref(r))
    return b.value, r.value


def _last_error():
    from sela_amd import capi

    return capi.lib().sela_hip_last_error().decode("utf-8", "replace")


def _rounds(n_threads, rounds, phases):
    """Every phase(t, r, problems) of every round on n_threads threads.  A phase is a generator: what it does up to its `yield`
    (the call's inputs and buffers: numpy work under the GIL that would spread the threads' arrivals far apart) is done before
    the round starts, what follows (the library call, the checks) by all threads together."""
    barrier = threading.Barrier(n_threads, timeout=120)
    problems = []

    def body(t):
        try:
            for r in range(rounds):
                for phase in phases:
                    call = phase(t, r, problems)
                    next(call)
                    barrier.wait()
                    for _ in call:
                        pass
        except threading.BrokenBarrierError:
            problems.append("thread %d: the barrier broke" % t)
        except Exception as e:  # noqa: BLE001 -- reported below, from the test's thread
            problems.append("thread %d: %r" % (t, e))
            barrier.abort()

    threads = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(n_threads)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + 240
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    assert not any(th.is_alive() for th in threads), "a thread is stuck"
    return problems


def _oracle_decode_i32(blob, ch):
    """The oracle's channels of one frame and the flags it raised on the way."""
    o = oracle()
    b = np.frombuffer(blob, np.uint8).copy()
    out = np.zeros((ch, 65535), np.int32)
    counts = np.zeros(ch, np.uint32)
    fl = C.c_uint32(0)
    used = o._fdec32(b, ch, out, 65535, counts, C.byref(fl))
    assert used == len(blob)
    return [out[c, : int(counts[c])].copy() for c in range(ch)], fl.value


def _short(planar):
    """A block the frame encoder analyses (the difference signal of a stereo frame included) not longer than its own order:
    the reference reads past its vector, the library answers SELA_HIP_ERANGE."""
    o = oracle()
    ch, n = planar.shape
    signals = [planar[c] for c in range(ch)] + ([(planar[0].astype(np.int64) - planar[1]).astype(np.int32)] if ch == 2 else [])
    return any(o.lpc_analyze(s)[0] >= n for s in signals)


def _q_range_frame(ch, n, seed):
    """A frame of `ch` channels of n samples whose first channel holds a quantised reflection coefficient of 100 (the reference
    indexes past its tables): the oracle flags it, the library answers SELA_HIP_ERANGE."""
    rng = np.random.default_rng(seed)
    subs = [(c, 0, c, [5, 100, -7] if c == 0 else [9, -4], rng.integers(-300, 301, n)) for c in range(ch)]
    blob = _build_frame(subs)
    _, fl = _oracle_decode_i32(blob, ch)
    assert fl & 1 and not fl & (BAD_DECODE_FLAGS & ~1), hex(fl)
    return blob


# ---- a. sela_hip_encode_i32 / sela_hip_decode_i32 ------------------------------------------------------------------------------
# (kind, channels, samples per channel, threads); only calls of one shape share an encode batch, decode batches go by channels
SHAPES_32 = [("click", 1, 40, 6), ("any", 2, 1, 2), ("three", 3, 1000, 3), ("stereo_diff", 2, 2047, 3), ("mono", 1, 2049, 3),
             ("three", 3, 4096, 3), ("stereo_diff", 2, 20000, 4)]
POOL_32 = 40  # frames per shape; a call takes a run of them (wrapping round)


def _pool_32(kind, ch, n, seed):
    """int32 [POOL_32, ch, n] frames of one shape: synthetic audio (the second channel a near copy of the first for stereo_diff:
    difference coding wins), clicks in silence for 40 samples (a tone that short comes out at an order above its length), any
    values for one sample (every block of one sample is refused: its order is 1)."""
    rng = np.random.default_rng(seed)
    if kind == "click":
        x = np.zeros((POOL_32, ch, n), np.int32)
        x[np.arange(POOL_32), 0, rng.integers(0, n, POOL_32)] = rng.integers(-30000, 30001, POOL_32)
        return x
    if kind == "any":
        return rng.integers(-30000, 30001, (POOL_32, ch, n)).astype(np.int32)
    x = synth_pcm(POOL_32 * n, ch, seed).astype(np.int32).reshape(POOL_32, n, ch).transpose(0, 2, 1).copy()
    if kind == "stereo_diff":
        x[:, 1] = x[:, 0] - (synth_pcm(POOL_32 * n, 1, seed + 7, noise_shift=6)[:, 0].astype(np.int32) >> 9).reshape(POOL_32, n)
    return x


def _cases_32():
    """What test a needs, made before its threads start: every shape's frames, the oracle's bytes and channels of each (or the
    refusal), a frame the encoder must refuse among the clicks and a frame the decoder must refuse, per shape."""
    o = oracle()
    shapes = []
    for s, (kind, ch, n, _) in enumerate(SHAPES_32):
        x = _pool_32(kind, ch, n, 300 + 11 * s)
        short = [_short(f) for f in x]
        assert all(short) if n == 1 else not any(short), (kind, n)
        if n == 1:  # frames of one sample no encoder writes: order 0 (decoded like any other)
            rng = np.random.default_rng(17)
            blobs = [_build_frame([(c, 0, c, [], [int(rng.integers(-30000, 30001))]) for c in range(ch)]) for _ in range(POOL_32)]
        else:
            blobs = [o.frame_encode_i32(f) for f in x]
        decoded = []
        for b in blobs:
            chans, fl = _oracle_decode_i32(b, ch)
            assert not fl & BAD_DECODE_FLAGS and all(len(c) == n for c in chans), (kind, n, hex(fl))
            decoded.append(np.stack(chans))
        shapes.append(dict(ch=ch, n=n, x=x, blobs=blobs, decoded=decoded, short=short,
                           q_range=_q_range_frame(ch, n, 500 + s) if n > 1 else None))
    rng = np.random.default_rng(2)
    noise = rng.integers(-20000, 20000, (1, 40)).astype(np.int32)  # white noise: its order comes out at 40 or above
    assert _short(noise)
    return shapes, noise


def test_32_bit_calls_from_many_threads_stay_their_own(gpu):
    """24 threads, 6 rounds: sela_hip_encode_i32 then sela_hip_decode_i32 on frames of seven shapes (mono, stereo whose difference
    coding wins, three channels; 1, 40, 1000, 2047, 2049, 4096 samples; stereo 20000-sample calls of 16 frames, under the
    library's 2^20 samples for coalescing, and of 32, over it), 1 to 33 frames per call (33 are not coalesced), decode strides
    from the stream's largest length to a few hundred more.  Callers that must fail alone, on another thread each round: a
    white-noise block among clicks (ERANGE), frames_cap one byte short (ECAPACITY) beside neighbours with exactly the oracle's
    bytes, a broken sync word (EFORMAT), a coefficient of 100 (ERANGE), a stride one short (ECAPACITY).  Every accepted call is
    the oracle's, every refused one gets its code and its own last error, and batches that held such a caller were retried."""
    from sela_amd import capi

    lib = capi.lib()
    shapes, noise = _cases_32()
    owner = [s for s, (_, _, _, k) in enumerate(SHAPES_32) for _ in range(k)]  # thread -> shape
    n_threads, rounds = len(owner), 6
    assert n_threads == 24
    of_shape = lambda s: [t for t in range(n_threads) if owner[t] == s]  # noqa: E731
    # the callers that must fail, per round, each on a thread of its own (and on another one every round)
    encoders_ok = [t for t in range(n_threads) if SHAPES_32[owner[t]][2] > 1]
    decoders = [t for t in range(n_threads) if SHAPES_32[owner[t]][2] > 1]
    dec_plan = [["format"], ["range", "stride"], ["range"], ["format", "stride"], ["range"], ["format", "range"]]
    enc_role, dec_role = [{} for _ in range(rounds)], [{} for _ in range(rounds)]
    for r in range(rounds):
        enc_role[r][of_shape(0)[r]] = "noise"
        if r % 2:
            others = [t for t in encoders_ok if owner[t] != 0]
            enc_role[r][others[(5 * r) % len(others)]] = "cap"
        free = [t for t in decoders if t not in enc_role[r]]
        for j, what in enumerate(dec_plan[r]):
            dec_role[r][free[(7 * r + 5 * j) % len(free)]] = what
    for r in range(1, rounds):
        assert not set(enc_role[r]) & set(enc_role[r - 1]) and not set(dec_role[r]) & set(dec_role[r - 1])

    def frames_per_call(t, r):
        if SHAPES_32[owner[t]][2] == 20000:
            return 16 if (t + r) % 2 else 32  # 640,000 samples: coalesced; 1,280,000: over the limit, on its own
        return (1, 7, 32, 33, 16, 3, 25, 2)[(3 * t + r) % 8]

    def pick(t, r, k):
        start = (t * 13 + r * 7) % POOL_32
        return [(start + i) % POOL_32 for i in range(k)]

    def encode(t, r, problems):
        s = shapes[owner[t]]
        ch, n = s["ch"], s["n"]
        idx = pick(t, r, frames_per_call(t, r))
        k = len(idx)
        role = enc_role[r].get(t)
        x = np.ascontiguousarray(s["x"][idx])
        if role == "noise":
            x[k // 2, 0] = noise[0]
        exact = sum(len(s["blobs"][i]) for i in idx)
        cap = exact - 1 if role == "cap" else exact if (t + r) % 2 == 0 else int(lib.sela_hip_encode_bound_bytes_n(k, ch, n))
        out = np.full(max(cap, 1), 0xEE, np.uint8)
        offs = np.zeros(k + 1, np.uint64)
        yield
        rc = lib.sela_hip_encode_i32(x.ctypes.data, k, ch, n, out.ctypes.data, cap, offs.ctypes.data)
        err = _last_error() if rc else ""
        want = -6 if role == "noise" or s["short"][idx[0]] else -4 if role == "cap" else 0
        why = {-6: "not longer than its predictor order", -4: "frames_out too small", 0: ""}[want]
        if rc != want or why not in err:
            problems.append("encode t%d r%d (%d x %d x %d, %s): rc %d, %r" % (t, r, k, ch, n, role, rc, err))
        elif rc == 0:
            want_bytes = b"".join(s["blobs"][i] for i in idx)
            if offs.tolist() != np.cumsum([0] + [len(s["blobs"][i]) for i in idx]).tolist() or out[:exact].tobytes() != want_bytes:
                problems.append("encode t%d r%d (%d x %d x %d): not the oracle's bytes" % (t, r, k, ch, n))

    def decode(t, r, problems):
        s = shapes[owner[t]]
        ch, n = s["ch"], s["n"]
        idx = pick(t, r, frames_per_call(t, r))
        k = len(idx)
        role = dec_role[r].get(t)
        blobs = [s["blobs"][i] for i in idx]
        bad = (t + r) % k
        if role == "range":
            blobs[bad] = s["q_range"]
        frames = np.frombuffer(b"".join(blobs), np.uint8).copy()
        offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
        if role == "format":
            frames[int(offs[bad])] ^= 0xFF
        stride = n - 1 if role == "stride" else n + (0, 1, 37, 300)[(t + 2 * r) % 4]
        out = np.full((k, ch, stride), 0x7A7A7A7A, np.int32)
        counts = np.full((k, ch), 0xFFFFFFFF, np.uint32)
        yield
        rc = lib.sela_hip_decode_i32(frames.ctypes.data, offs.ctypes.data, k, ch, out.ctypes.data, stride, counts.ctypes.data)
        err = _last_error() if rc else ""
        want, why = {"format": (-5, "malformed"), "range": (-6, "quantised reflection coefficient"), "stride": (-4, "stride"), None: (0, "")}[role]
        if rc != want or why not in err:
            problems.append("decode t%d r%d (%d x %d x %d, %s): rc %d, %r" % (t, r, k, ch, n, role, rc, err))
        elif rc == 0:
            for f, i in enumerate(idx):
                want_f = s["decoded"][i]
                if not (counts[f] == n).all() or not np.array_equal(out[f, :, :n], want_f):
                    problems.append("decode t%d r%d (%d x %d x %d): frame %d is not the oracle's" % (t, r, k, ch, n, f))
                    break

    before = {kind: _coalesced(kind) for kind in (DECODE32, ENCODE32)}
    problems = _rounds(n_threads, rounds, [encode, decode])
    assert not problems, problems
    for kind in (DECODE32, ENCODE32):
        (b0, r0), (b1, r1) = before[kind], _coalesced(kind)
        assert b1 > b0 and r1 >= r0 + 1 and r1 - r0 <= b1 - b0, (kind, before[kind], (b1, r1))


# ---- b. sela_hip_decode: a coefficient out of range in a batch of 2048-sample frames ---------------------------------------------
def test_16_bit_decode_calls_with_a_coefficient_out_of_range_among_them(gpu):
    """sela_hip_decode from 24 threads, 6 rounds, stereo and mono callers of 1 to 33 frames.  Among them: stereo callers with a
    frame whose coefficient is 100 (SELA_HIP_ERANGE, the job's verdict on the Q_RANGE flag), callers with a broken sync word
    (SELA_HIP_EFORMAT), and one caller per round whose stream turns to 1000-sample frames after its first frame (the any-length
    route: the oracle's samples at the sela_hip_index_samples layout).  Each fails -- or takes its route -- alone: every other
    caller gets the oracle's samples, and the batches that held such a caller were retried call by call."""
    from sela_amd import capi, codec

    lib = capi.lib()
    o = oracle()
    pools = {}
    for ch, track in ((2, 71), (1, 72)):
        pcm = synth_frames(40, ch, track)
        blobs = [o.frame_encode(pcm[f]) for f in range(40)]
        decoded = []
        for b in blobs:
            d, used = o.frame_decode(b, ch)
            assert used == len(b)
            decoded.append(d)
        pools[ch] = (blobs, decoded)
    odd_pcm = synth_pcm(1000, 2, 73)
    odd = o.frame_encode(odd_pcm)
    odd_back, used = o.frame_decode(odd, 2, n=1000)
    assert used == len(odd) and np.array_equal(odd_back, odd_pcm)
    q_range = _q_range_frame(2, 2048, 74)
    # alone first: the fast decoder flags the coefficient, the call says SELA_HIP_ERANGE
    with pytest.raises(capi.SelaHipError) as err:
        codec.decode_host(np.frombuffer(q_range, np.uint8).copy(), np.array([0, len(q_range)], np.uint64), 2)
    assert err.value.code == -6 and "quantised reflection coefficient" in str(err.value)

    n_threads, rounds = 24, 6
    channels = [1 if t % 6 == 5 else 2 for t in range(n_threads)]
    stereo = [t for t in range(n_threads) if channels[t] == 2]
    role = [{} for _ in range(rounds)]
    for r in range(rounds):
        picks = [stereo[(r * 5 + j * 7) % len(stereo)] for j in range(4)]
        assert len(set(picks)) == 4
        role[r][picks[0]] = "odd"
        role[r][picks[1]] = "range"
        if r % 2 == 0:
            role[r][picks[2]] = "range"
        else:
            role[r][picks[2]] = "format"
    for r in range(rounds):
        mono = [t for t in range(n_threads) if channels[t] == 1]
        role[r][mono[r % len(mono)]] = "format"
    for r in range(1, rounds):
        assert not {t for t, w in role[r].items() if w != "format"} & {t for t, w in role[r - 1].items() if w != "format"}

    def decode(t, r, problems):
        ch = channels[t]
        blobs_pool, decoded_pool = pools[ch]
        k = 1 + (5 * t + 3 * r) % 33
        what = role[r].get(t)
        if what == "odd":
            k = max(k, 2)
        start = (t * 11 + r * 3) % 40
        idx = [(start + i) % 40 for i in range(k)]
        blobs = [blobs_pool[i] for i in idx]
        wants = [decoded_pool[i] for i in idx]
        bad = (t + r) % k
        if what == "odd":
            blobs[1], wants[1] = odd, odd_back
        elif what == "range":
            blobs[bad] = q_range
        frames = np.frombuffer(b"".join(blobs), np.uint8).copy()
        offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
        if what == "format":
            frames[int(offs[bad])] ^= 0xFF
        total = sum(len(w) for w in wants)
        out = np.full((max(total, k * 2048), ch), 0x5A5A, np.int16)  # (sela_hip.h: max(n_frames * 2048, sample_offsets[n_frames]))
        yield
        rc = lib.sela_hip_decode(frames.ctypes.data, offs.ctypes.data, k, ch, out.ctypes.data)
        err = _last_error() if rc else ""
        want, why = {"format": (-5, "malformed"), "range": (-6, "quantised reflection coefficient"), "odd": (0, ""), None: (0, "")}[what]
        if rc != want or why not in err:
            problems.append("t%d r%d (%d x %d, %s): rc %d, %r" % (t, r, k, ch, what, rc, err))
            return
        if rc == 0:
            if what == "odd":
                so = np.zeros(k + 1, np.uint64)
                lib.sela_hip_index_samples(frames.ctypes.data, offs.ctypes.data, k, ch, so.ctypes.data)
                if so.tolist() != np.cumsum([0] + [len(w) for w in wants]).tolist():
                    problems.append("t%d r%d: the stream's layout is not the oracle's" % (t, r))
            if not np.array_equal(out[:total], np.concatenate(wants)):
                problems.append("t%d r%d (%d x %d, %s): not the oracle's samples" % (t, r, k, ch, what))

    b0, r0 = _coalesced(DECODE)
    problems = _rounds(n_threads, rounds, [decode])
    assert not problems, problems
    b1, r1 = _coalesced(DECODE)
    assert b1 > b0 and r1 >= r0 + 1 and r1 - r0 <= b1 - b0, ((b0, r0), (b1, r1))


# ---- c. one-shot calls while the thread's streaming job is open --------------------------------------------------------------
@pytest.mark.parametrize("job_kind", ["encode", "decode"])
def test_one_shot_32_bit_calls_leave_the_threads_open_job_alone(gpu, job_kind):
    """begin, feed half; then sela_hip_encode_i32 / sela_hip_decode_i32 on a 1000-sample stereo frame, sela_hip_encode_ragged_i32
    and sela_hip_decode on a stream of 1000-sample frames (the oracle's answers) and sela_hip_decode on 2048-sample frames
    (SELA_HIP_EINVAL: the 16-bit one-shot calls refuse while a job is open); the job must still be open -- a second begin on
    the thread is refused -- and feeding the rest and ending it gives the oracle's bytes / samples.  (Were the job torn down by
    a one-shot call, its handle would point at buffers that are gone: the test then ends the probing job and stops, without
    touching the old handle again.)"""
    from sela_amd import capi

    lib = capi.lib()
    o = oracle()
    ch, n = 2, 8
    pcm = synth_frames(n, ch, 81)
    want_frames, want_offs, _ = o.encode_frames(pcm)
    want_pcm, _ = o.decode_frames(want_frames, want_offs, ch)
    assert np.array_equal(want_pcm, pcm)
    job = C.c_void_p()
    if job_kind == "encode":
        out = np.zeros(int(lib.sela_hip_encode_bound_bytes(n, ch)), np.uint8)
        offs = np.zeros(n + 1, np.uint64)
        capi.check(lib.sela_hip_encode_begin(C.byref(job), ch, n, out.ctypes.data, out.nbytes, offs.ctypes.data))
        feed = lambda a, b: lib.sela_hip_encode_feed(job, pcm[a:b].ctypes.data, b - a, None, None)  # noqa: E731
        end = lambda: lib.sela_hip_encode_end(job, None, None)  # noqa: E731
    else:
        back = np.zeros_like(pcm)
        stream = np.ascontiguousarray(want_frames)
        o_all = np.ascontiguousarray(want_offs)
        pieces = [np.ascontiguousarray(o_all[a: b + 1]) for a, b in ((0, n // 2), (n // 2, n))]
        capi.check(lib.sela_hip_decode_begin(C.byref(job), ch, n, back.ctypes.data))
        feed = lambda a, b: lib.sela_hip_decode_feed(job, stream.ctypes.data, pieces[a // (n // 2)].ctypes.data, b - a, None)  # noqa: E731
        end = lambda: lib.sela_hip_decode_end(job, None)  # noqa: E731
    capi.check(feed(0, n // 2))

    # the one-shot calls, each against the oracle
    x = np.ascontiguousarray(synth_pcm(1000, 2, 82).T.astype(np.int32))
    x[1] = x[0] - (x[1] >> 9)
    want = o.frame_encode_i32(x)
    got = np.zeros(int(lib.sela_hip_encode_bound_bytes_n(1, 2, 1000)), np.uint8)
    go = np.zeros(2, np.uint64)
    assert lib.sela_hip_encode_i32(x.ctypes.data, 1, 2, 1000, got.ctypes.data, got.nbytes, go.ctypes.data) == 0, _last_error()
    assert go.tolist() == [0, len(want)] and got[: len(want)].tobytes() == want
    f32 = np.frombuffer(want, np.uint8).copy()
    o32 = np.array([0, len(want)], np.uint64)
    wide = np.zeros((1, 2, 1100), np.int32)
    counts = np.zeros((1, 2), np.uint32)
    assert lib.sela_hip_decode_i32(f32.ctypes.data, o32.ctypes.data, 1, 2, wide.ctypes.data, 1100, counts.ctypes.data) == 0, _last_error()
    chans, _ = _oracle_decode_i32(want, 2)
    assert counts.tolist() == [[1000, 1000]] and all(np.array_equal(wide[0, c, :1000], chans[c]) for c in range(2))
    ragged = [x[0], x[1, :700]]
    want_r = o.frame_encode_ragged(ragged)
    flat = np.concatenate(ragged).astype(np.int32)
    lengths = np.array([1000, 700], np.uint32)
    rbuf = np.zeros(4 + int(lib.sela_hip_encode_bound_bytes_n(1, 1, 1000)) + int(lib.sela_hip_encode_bound_bytes_n(1, 1, 700)), np.uint8)
    used = C.c_size_t(0)
    assert lib.sela_hip_encode_ragged_i32(flat.ctypes.data, lengths.ctypes.data, 2, rbuf.ctypes.data, rbuf.nbytes, C.byref(used)) == 0, _last_error()
    assert rbuf[: used.value].tobytes() == want_r
    odd_pcm = synth_pcm(3000, 2, 83).reshape(3, 1000, 2)
    odd_blobs = [o.frame_encode(odd_pcm[f]) for f in range(3)]
    odd = np.frombuffer(b"".join(odd_blobs), np.uint8).copy()
    odd_offs = np.cumsum([0] + [len(b) for b in odd_blobs]).astype(np.uint64)
    odd_back = np.zeros((3 * 2048, 2), np.int16)
    assert lib.sela_hip_decode(odd.ctypes.data, odd_offs.ctypes.data, 3, 2, odd_back.ctypes.data) == 0, _last_error()
    assert np.array_equal(odd_back[:3000], np.concatenate([o.frame_decode(b, 2, n=1000)[0] for b in odd_blobs]))

    # the job is still open: a second one on this thread is refused
    other = C.c_void_p()
    rc = lib.sela_hip_decode_begin(C.byref(other), ch, 0, None)
    if rc == 0:
        lib.sela_hip_decode_end(other, None)
        pytest.fail("a one-shot call closed the thread's open %s job (a second begin succeeded); its handle is not touched again" % job_kind)
    assert rc == -2 and "open job" in _last_error()
    # ... and the one-shot calls on 2048-sample frames say so themselves
    std = np.zeros((1, 2048, 2), np.int16)
    one = np.ascontiguousarray(want_frames[: int(want_offs[1])])
    assert lib.sela_hip_decode(one.ctypes.data, np.array([0, len(one)], np.uint64).ctypes.data, 1, 2, std.ctypes.data) == -2
    assert "open job" in _last_error()
    f16 = np.zeros(int(lib.sela_hip_encode_bound_bytes(1, 2)), np.uint8)
    o16 = np.zeros(2, np.uint64)
    assert lib.sela_hip_encode(pcm[:1].ctypes.data, 1, 2, 2048, f16.ctypes.data, f16.nbytes, o16.ctypes.data) == -2
    assert "open job" in _last_error()

    capi.check(feed(n // 2, n))
    capi.check(end())
    if job_kind == "encode":
        assert np.array_equal(offs, want_offs) and out[: int(want_offs[n])].tobytes() == want_frames.tobytes()
    else:
        assert np.array_equal(back, want_pcm)


# ---- d. the error of a stream whose offsets fall ---------------------------------------------------------------------------------
def test_decode_with_an_odd_first_frame_and_falling_offsets_reports_its_own_error(gpu):
    """sela_hip_decode on a stream whose first frame is not 2048 samples and whose frame offsets decrease: SELA_HIP_EFORMAT,
    and the thread's last error says so -- not what the thread's previous failure said."""
    from sela_amd import capi

    lib = capi.lib()
    o = oracle()
    a = o.frame_encode(synth_pcm(1000, 2, 91))
    b = o.frame_encode(synth_pcm(1000, 2, 92))
    frames = np.frombuffer(a + b, np.uint8).copy()
    pcm = np.zeros((2 * 2048, 2), np.int16)
    assert lib.sela_hip_decode(frames.ctypes.data, np.array([0, len(a) + len(b)], np.uint64).ctypes.data, 1, 0, pcm.ctypes.data) == -2
    before = _last_error()
    assert before
    falling = np.array([0, len(a), len(a) - 4], np.uint64)
    assert lib.sela_hip_decode(frames.ctypes.data, falling.ctypes.data, 2, 2, pcm.ctypes.data) == -5
    assert _last_error() != before and "offsets" in _last_error()
