"""Hand-built subframes for every compiled copy of the decoder's synthesis (sela_synth.h, sela_decode_core.inc), built once on the
CPU, with the oracle's answer beside them.  Not a test file: tests/test_synth_cases.py shows that the cases are what they are
called, tests/test_gpu_synth_matrix.py runs them through every kernel in both recurrence forms, and test_gpu_synth_roles.py and
test_gpu_step_up_orders.py take their builders from here.

A case is one subframe, (label, order, q, residues, res_k or None) and what it is meant to be:
  seams      every order across the step-up's seams, coefficients random, all -64 and all 63 (decoder_frames), and 47 .. 49 for
             the class boundary at 48;
  folded     (a) the folded form throughout: every sample below 2^23 (asserted here);
  residue    (b) one residue of 2^23 or more in a named block: the block starts in the exact form;
  leaves     (c) residues below 2^23 whose SAMPLES reach 2^23 in a named block: the block is run folded, found out and run again;
  exact      (d) a predictor whose table does not fit the fold: exact from the first block.
Whether a 2048-sample subframe is parsed just in time or parked in the workspace is a matter of its words alone (coefficient
words + 2 + residue words against kStreamCap = 1072).  The workspace cases are cases (a) to (c) again under a Rice parameter no
encoder would pick (17: 2048 x 18 bits are 1152 words); one value is there whatever the parameter: a residue of 2^29 + 5 costs
64 (k + 1) + 2^(30 - k) / 32 words, 1344 at the least.  For the same reason the plateau of _leaves_in_block is two residues
long in the just-in-time cases (thirty of 2^23 - 1 cannot be carried in 1072 words either).

Every expectation is the oracle's (oracle_lib.oracle()); nothing here touches a GPU."""
import ctypes as C
import functools
from typing import NamedTuple, Optional

import numpy as np

import wide_cases as wc
from gpu_common import _build_frame, _subframe_words  # noqa: F401  (re-exported for the tests of the cases)
from oracle_lib import oracle

P23 = 1 << 23
N = 2048
PLAN_WORDS = 1072                      # kStreamCap: the words of a subframe the just-in-time parse holds
COEF_OVERFLOW = 2
ORDERS = [1, 2, 3, 31, 32, 33, 60, 61, 62, 63, 64, 65, 66, 99, 100]
KINDS = ("random", "all -64", "all 63")
BOUNDARY_ORDERS = [47, 48, 49]         # ring 64 / group 16 up to 48, group 4 from 49
CLASS_ORDERS = [48, 60, 61, 62, 100]   # 64 / 16, 64 / 4, 128 / 16 (three of it)
WORKSPACE_ORDERS = [60, 61, 100]
WORKSPACE_K = 17
HAND_OVER_VALUES = (P23, -P23, (1 << 24) + 3, wc.P29 + 5)
HAND_OVER_BLOCKS = (0, 1, 2, 31)
LENGTHS = [65, 129, 191, 192, 2049, 2113, 4095]
LENGTH_ORDERS = [61, 100]
TAIL_LENGTHS = [n for n in LENGTHS if n >= 2049]
WIDE_CHANNELS = (9, 10)


class Case(NamedTuple):
    label: str
    order: int
    q: np.ndarray
    residues: np.ndarray
    res_k: Optional[int]
    kind: str = "seam"             # seam | folded | residue | leaves | exact
    block: Optional[int] = None    # the block the case names: where the first residue or sample of 2^23 or more lies
    at: Optional[int] = None       # that residue's or sample's index
    mode: str = "jit"              # jit | workspace: what the subframe's words make of a 2048-sample frame


class Frame(NamedTuple):
    label: str
    blob: bytes
    channels: int
    n: int
    cases: tuple                   # the Case of every channel (None: a difference subframe)
    mode: str                      # jit | workspace: what its cases say
    pcm: np.ndarray                # the oracle's int16 [n, channels] (n != 2048: its 32-bit samples, narrowed)
    wide: tuple                    # the oracle's int32 samples per channel
    flags: int                     # the oracle's flags (both of its decoders agree: asserted)


class Stream(NamedTuple):
    label: str
    blobs: tuple                   # whole-track stream: 2048-sample frames, then the long (or only) last frame
    channels: int
    case: Case                     # the last frame's hard subframe
    pcm: np.ndarray                # the oracle's int16 [samples, channels] of the whole stream


# ---- the builders that test_gpu_synth_roles.py and test_gpu_step_up_orders.py had -----------------------------------------------------
def _q(order, rng):
    q = wc.fold_coefficients(order, rng)
    assert wc.fits_fold(oracle().lpc_coeffs(order, q)), order  # the synthesis starts in the folded form
    return q


def _quiet(n, rng):
    return rng.integers(-200, 201, n).astype(np.int32)


def _leaves_in_block(order, q, block, n, rng, plateau=30):
    """Residues below 2^23 in size whose SAMPLES reach 2^23 first inside `block`: quiet noise, then a plateau of 2^23 - 1 from
    the block's tenth sample on (the strong first coefficient of fold_coefficients carries it past the range)."""
    o = oracle()
    r = _quiet(n, rng)
    r[64 * block + 10: 64 * block + 10 + plateau] = P23 - 1
    assert np.abs(r.astype(np.int64)).max() < P23
    s = o.lpc_synth(order, q, r).astype(np.int64)
    first = int(np.flatnonzero(np.abs(s) >= P23)[0])
    assert first // 64 == block, (order, block, first)
    return r


def _seam_q(order, kind, rng):
    if kind == "random":
        return rng.integers(-64, 64, order).astype(np.int32)
    return np.full(order, -64 if kind == "all -64" else 63, np.int32)


def first_beyond(order, q, residues):
    """index of the first residue or sample of 2^23 or more in size (the folded form's two tests, synth_mac), or None"""
    r = np.asarray(residues, np.int64)
    s = oracle().lpc_synth(order, q, np.asarray(residues, np.int32)).astype(np.int64)
    hit = np.flatnonzero((np.abs(r) >= P23) | (np.abs(s) >= P23))
    return int(hit[0]) if len(hit) else None


def oracle_frame(blob, ch, n):
    """-> (int16 [n, ch], int32 per channel, flags): frame::FrameDecoder as the oracle restates it.  A 2048-sample frame goes
    through both of its decoders (the int16 one keeps the reference's x86 result of a predictor beyond int64); any other length
    through the any-length one, narrowed as the reference's writer narrows."""
    o = oracle()
    b = np.frombuffer(blob, np.uint8).copy()
    out = np.zeros((ch, n), np.int32)
    counts = np.zeros(ch, np.uint32)
    fl32 = C.c_uint32(0)
    assert o._fdec32(b, ch, out, n, counts, C.byref(fl32)) == len(blob) and (counts == n).all()
    wide = tuple(out[c].copy() for c in range(ch))
    if n == N:
        pcm = np.zeros((N, ch), np.int16)
        fl16 = C.c_uint32(0)
        assert o._fdec(b, ch, pcm, C.byref(fl16)) == len(blob)
        assert fl16.value == fl32.value, (fl16.value, fl32.value)
    else:
        pcm = np.ascontiguousarray(out.T.astype(np.int16))
    for a in (pcm,) + wide:
        a.setflags(write=False)
    return pcm, wide, fl32.value


def _frame(label, cases, subframes, res_k=None, n=N):
    blob = _build_frame(subframes, res_k)
    pcm, wide, flags = oracle_frame(blob, len(subframes), n)
    mode = "workspace" if any(c is not None and c.mode == "workspace" for c in cases) else "jit"
    return Frame(label, blob, len(subframes), n, tuple(cases), mode, pcm, wide, flags)


def _plain(cases, res_k=None, n=N, label=None):
    """one ordinary subframe per case, channel c = case c"""
    return _frame(label or " | ".join(c.label for c in cases), cases, [(c, 0, c, case.q, case.residues) for c, case in enumerate(cases)], res_k, n)


def _partnered(cases):
    """every case with a different one on the other channel: each is channel 0 once and channel 1 once"""
    n = len(cases)
    return [(cases[b], cases[(b + max(n // 2, 1)) % n]) for b in range(n)]


# ---- seams ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seam_frame(order, kind):
    rng = np.random.default_rng(1000 + order)
    qs = [_seam_q(order, kind, rng) for _ in range(2)]
    cases = [Case(f"order {order}, {kind}", order, qs[c], rng.integers(-300, 300, N).astype(np.int32), None) for c in range(2)]
    return _plain(cases, label=f"order {order}, {kind}")


@functools.lru_cache(maxsize=None)
def decoder_frames():
    """tuple of (label, q of channel 0, q of channel 1, frame bytes, the oracle's int16 [2048, 2], its int32 per channel, its flags)"""
    out = []
    for order in ORDERS:
        for kind in KINDS:
            f = _seam_frame(order, kind)
            out.append((f.label, f.cases[0].q, f.cases[1].q, f.blob, f.pcm, list(f.wide), f.flags))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def seam_frames():
    """decoder_frames() as Frames, and orders 47 .. 49 with random coefficients"""
    return tuple(_seam_frame(order, kind) for order in ORDERS for kind in KINDS) + tuple(_seam_frame(order, "random") for order in BOUNDARY_ORDERS)


# ---- classes x hand-over --------------------------------------------------------------------------------------------------------------
def _exact_q(order, rng):
    """Coefficients whose Q35 predictor does not fit the fold and stays inside int64 (random ones within the tables stay far
    below 2^55 at every order): the tables' two ends in random order on as many leading stages as int64 bears, small ones behind."""
    o = oracle()
    for m in range(order, 0, -1):
        for _ in range(8):
            q = rng.integers(-6, 7, order).astype(np.int32)
            q[:m] = rng.choice([-64, 63], m)
            qq = np.zeros(100, np.int32)
            qq[:order] = q
            a = np.zeros(101, np.int64)
            fl = C.c_uint32(0)
            o._coeffs(order, qq, a, C.byref(fl))
            if fl.value == 0 and not wc.fits_fold(a[: order + 1]):
                return q
    raise AssertionError(order)


def _hard_cases(order, n, rng, leave_blocks, values=(), plateau=30):
    """(a), (b) for (value, block) in `values`, (c) for the blocks of `leave_blocks`"""
    q = _q(order, rng)
    r = _quiet(n, rng)
    assert np.abs(oracle().lpc_synth(order, q, r).astype(np.int64)).max() < P23 and first_beyond(order, q, r) is None
    out = [Case(f"order {order}, n {n}, folded", order, q, r, None, "folded")]
    for v, block in values:
        q, r = _q(order, rng), _quiet(n, rng)
        at = 64 * block + int(rng.integers(0, 64))
        r[at] = v
        assert first_beyond(order, q, r) == at
        long = abs(v) >= wc.P29  # (no Rice parameter carries it in 1072 words)
        out.append(Case(f"order {order}, n {n}, residue {v} in block {block}", order, q, r, None, "residue", block, at, "workspace" if long else "jit"))
    for block in leave_blocks:
        q = _q(order, rng)
        r = _leaves_in_block(order, q, block, n, rng, plateau)
        out.append(Case(f"order {order}, n {n}, samples leave in block {block}", order, q, r, None, "leaves", block, first_beyond(order, q, r), "workspace" if plateau > 2 else "jit"))
    return out


@functools.lru_cache(maxsize=None)
def class_cases():
    out = []
    for i, order in enumerate(CLASS_ORDERS):
        rng = np.random.default_rng(7000 + order)
        values = [(v, HAND_OVER_BLOCKS[(j + i) % 4]) for j, v in enumerate(HAND_OVER_VALUES)]
        out += _hard_cases(order, N, rng, (1, 2), values, plateau=2)
        out.append(Case(f"order {order}, exact from the first block", order, _exact_q(order, rng), _quiet(N, rng), None, "exact"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def workspace_cases():
    """(a) to (c) of the class cases at orders 60, 61 and 100 under the forced Rice parameter: the same residues, the same samples"""
    return tuple(c._replace(label=c.label + f", k = {WORKSPACE_K}", res_k=WORKSPACE_K, mode="workspace")
                 for c in class_cases() if c.order in WORKSPACE_ORDERS and c.kind != "exact" and c.mode == "jit")


@functools.lru_cache(maxsize=None)
def class_frames():
    """stereo frames of the class cases: the just-in-time ones, then those that no parameter keeps out of the workspace"""
    jit = [c for c in class_cases() if c.mode == "jit"]
    long = [c for c in class_cases() if c.mode == "workspace"]
    return tuple(_plain(pair) for pair in _partnered(jit) + _partnered(long))


@functools.lru_cache(maxsize=None)
def workspace_frames():
    return tuple(_plain(pair, WORKSPACE_K) for pair in _partnered(list(workspace_cases())))


@functools.lru_cache(maxsize=None)
def stereo_frames():
    """Every 2048-sample stereo frame in the order of one launch: every workspace-mode frame between two just-in-time frames."""
    frames = seam_frames() + class_frames() + workspace_frames()
    jit = [f for f in frames if f.mode == "jit"]
    parked = [f for f in frames if f.mode == "workspace"]
    assert len(jit) > len(parked)
    out = []
    for i, f in enumerate(jit):
        out.append(f)
        if i < len(parked):
            out.append(parked[i])
    return tuple(out)


def hard_frames():
    """the stereo frames of the class and workspace cases (all clean), in launch order"""
    return tuple(f for f in stereo_frames() if f.cases[0].kind != "seam")


def stream_of(frames):
    blobs = [f.blob for f in frames]
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def narrow_frames(ch):
    """frames of `ch` channels (1, 3) from the same class and workspace cases, each case once at least"""
    out = []
    pools = ([c for c in class_cases() if c.mode == "jit"], None), ([c for c in class_cases() if c.mode == "workspace"], None), (list(workspace_cases()), WORKSPACE_K)
    for pool, res_k in pools:
        for i in range(0, len(pool), ch):
            out.append(_plain([pool[(i + c) % len(pool)] for c in range(ch)], res_k))
    return tuple(out)


# ---- frames of more than eight channels -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_frames(ch):
    """Four frames of `ch` channels whose subframes cycle through the class cases: three of just-in-time cases, the first with
    two difference subframes under hand-over parents (a wide residue; samples that leave), one of cases parked in the workspace."""
    rng = np.random.default_rng(7100 + ch)
    jit = [c for c in class_cases() if c.mode == "jit"]
    parked = [c for c in class_cases() if c.mode == "workspace"] + list(workspace_cases())
    out, at = [], 3 * ch  # (the two channel counts start at different cases)
    for f in range(4):
        pool = jit if f < 3 else parked
        cases = [pool[(at + c) % len(pool)] for c in range(ch)]
        at += ch
        subs = [(c, 0, c, case.q, case.residues) for c, case in enumerate(cases)]
        if f == 0:
            for c, kind in ((ch - 1, "residue"), (ch - 2, "leaves")):
                parent = next(p for p in range(ch - 2) if cases[p].kind == kind)
                subs[c] = (c, 1, parent, np.zeros(0, np.int32), _quiet(N, rng))
                cases[c] = None
        out.append(_frame(f"{ch} channels, frame {f}", cases, subs, WORKSPACE_K if f == 3 else None))
    return tuple(out)


# ---- run-time lengths -----------------------------------------------------------------------------------------------------------------
def leave_blocks(n):
    """(odd, even): the blocks in which the samples of a run-time length leave the range -- block 1 and the last even block that
    holds the plateau of thirty and ten samples in front of it (block 0 below three blocks); no odd one where block 1 is too short"""
    fits = [b for b in range((n + 63) // 64) if 64 * b + 41 <= n]
    odd = [b for b in fits if b % 2 == 1][:1]
    even = [b for b in fits if b % 2 == 0][-1:]
    return tuple(odd + even)


@functools.lru_cache(maxsize=None)
def length_cases(n):
    out = []
    for order in LENGTH_ORDERS:
        if order >= n:  # (a block not longer than its order: refused, tested elsewhere)
            continue
        out += _hard_cases(order, n, np.random.default_rng(7200 + 10 * n + order), leave_blocks(n))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def length_frames():
    """stereo frames of every run-time length"""
    return tuple(_plain(pair, n=n) for n in LENGTHS for pair in _partnered(list(length_cases(n))))


# ---- whole-track streams with a hand-built last frame ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_streams(ch):
    """ch 1: mono; ch 2: the hard subframe and a difference channel under it.  Two ordinary 2048-sample frames and a last frame
    of every run-time length from 2049 up, and single frames of 191 samples."""
    rng = np.random.default_rng(7300 + ch)
    front_cases = [c for c in class_cases() if c.kind == "folded" and c.order in (61, 100)]
    front = [_plain([front_cases[(f + c) % 2] for c in range(ch)]) for f in range(2)]
    out = []
    for n in TAIL_LENGTHS + [191]:
        for case in length_cases(n):
            subs = [(0, 0, 0, case.q, case.residues)] + ([(1, 1, 0, np.zeros(0, np.int32), _quiet(n, rng))] if ch == 2 else [])
            last = _frame(case.label, [case, None][:ch], subs, n=n)
            assert last.flags == 0
            frames = (front if n > N else []) + [last]
            pcm = np.concatenate([f.pcm for f in frames])
            pcm.setflags(write=False)
            out.append(Stream(case.label, tuple(f.blob for f in frames), ch, case, pcm))
    return tuple(out)
