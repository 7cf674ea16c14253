"""Inputs beyond 24 bits, shared by the oracle-versus-reference tests and the GPU tests of 25- to 31-bit audio.  Not a test file.

The decoder's folded synthesis keeps a residue only mod 2^29 and its samples only while |s| < 2^23 (sela_decode_core.inc,
synth_mac), so what matters here: residues at k * 2^29 + d, at the zig-zag's edge (|r| < 2^30 for the reference's int32
zig-zag, -2^30 the last value it takes), around 2^28 (where the prediction's 29 bits end) and at the range check's own
edges +-(2^23 - 1) / +-2^23; samples of every width from 24 to 31 bits."""
import numpy as np

P29, P30, P31 = 1 << 29, 1 << 30, 1 << 31

# residue values for the synthesis (any int32: the stage has no zig-zag) ...
STAGE_RESIDUES = [P29 + 5, -P29 + 5, P29 - 7, -P29 - 7, 2 * P29 - 3, -2 * P29 + 3, 3 * P29 + 11, -4 * P29 + 9, P30 - 1, -(P30 - 1), -P30,
                  (1 << 28) + 1, (1 << 28) - 1, -(1 << 28) + 1, -(1 << 28) - 1, (1 << 23) - 1, -(1 << 23) + 1, 1 << 23, -(1 << 23)]
# ... and those a Rice stream of the format can carry (|r| < 2^30, and -2^30)
FRAME_RESIDUES = [r for r in STAGE_RESIDUES if -P30 <= r < P30]

# orders on both sides of every ring / group of the synthesis (<= 48: 64 / 16, <= 60: 64 / 4, else 128 / 16)
ORDERS = [0, 1, 2, 47, 48, 49, 60, 61, 64, 65, 100]


def fold_coefficients(order, rng):
    """Quantised coefficients whose Q35 predictor fits the folded form (|a| < 2^55: the synthesis starts folded): order 1 the
    encoder's pick for the impulse frame below, order 2 a pair from the issue's model, longer ones a strong first reflection
    coefficient and small others."""
    if order == 0:
        return np.zeros(0, np.int32)
    if order == 1:
        return np.array([26], np.int32)
    if order == 2:
        return np.array([-40, 10], np.int32)
    q = rng.integers(-6, 7, order).astype(np.int32)
    q[0] = rng.integers(-64, -40)
    return q


def fits_fold(a):
    """The folded form's test on a Q35 predictor (build_synth_table): every a = ah * 2^32 + al with ah in [-2^23, 2^23)."""
    a = np.asarray(a, np.int64)
    ah = (a - a.astype(np.uint64).astype(np.uint32).view(np.int32).astype(np.int64)) >> 32
    return bool(np.all((ah >= -(1 << 23)) & (ah < (1 << 23))))


def placements(n):
    """Where a wide residue goes in a vector of n: lane 0 of the first block, lane 63, and in the second block of a ring of 128."""
    return sorted({p for p in (0, 63, 128 + 64 + 20) if p < n} or {0})


def stage_cases(n, rng, values=STAGE_RESIDUES):
    """(name, residues int32[n]): small noise with one wide value at one placement."""
    out = []
    for v in values:
        for p in placements(n):
            r = rng.integers(-200, 201, n).astype(np.int32)
            r[p] = v
            out.append((f"{v}@{p}", r))
    return out


def impulse_frame_signal():
    """The frame an encoder really writes with a residue of 2^29 + 5: 2048 zeros, s[700] = 2^29 + 5, s[1500] = -1000 -- order 1
    (q = 26), residue 536870917 at sample 700."""
    s = np.zeros(2048, np.int32)
    s[700] = P29 + 5
    s[1500] = -1000
    return s


def wide_signals(n, seed):
    """(name, int32[n]) mono signals of 24 to 31 bits.  Some the format cannot carry (a residue >= 2^30 -- sample 0 is its own
    residue -- or a Rice stream beyond the u16 word count): an encoder refuses those."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    out = []
    x = np.zeros(n, np.int64)
    x[700 * n // 2048] = P29 + 5
    x[1500 * n // 2048] = -1000
    out.append(("impulse", x))
    for i, v in enumerate((P29 + 3, -P29 - 7, P29 - 11, -P29 + 2)):
        x = np.zeros(n, np.int64)
        for p in (63, 64 + 17, 1000 + 64 * i):
            if p < n:
                x[p] = v
        out.append((f"impulses {v}", x))
    for v in (P29, -P29, P30 - 1000, -(P30 - 1000), -P30, P30, P31 - 1, -(P31 - 1)):
        out.append((f"dc {v}", np.full(n, v, np.int64)))
    for bits in (25, 28, 30, 31):  # sparse clicks at this width (31: full scale)
        x = np.zeros(n, np.int64)
        idx = rng.integers(1, n, max(1, n // 200)) if n > 1 else np.zeros(0, np.int64)
        x[idx] = rng.integers(-(1 << (bits - 1)) + 1, 1 << (bits - 1), len(idx))
        out.append((f"sparse {bits}-bit", x))
    for bits in (24, 25, 26, 27, 28, 29, 30, 31):  # tones at every width
        amp = (1 << (bits - 1)) - 1
        x = np.round(amp * 0.9 * np.sin(t * 0.031 + 0.3) + rng.normal(0, amp / 5000 + 1, n))
        out.append((f"tone {bits}-bit", np.clip(x, -amp, amp)))
    out.append(("dc 2^29 + sine", P29 + np.round((1 << 20) * np.sin(t * 0.02))))
    out.append(("noise 25-bit", rng.integers(-(1 << 24), 1 << 24, n)))
    out.append(("noise 30-bit", rng.integers(-(1 << 29), 1 << 29, n)))
    return [(name, np.asarray(x, np.int64).astype(np.int32)) for name, x in out]


def wrapping_stereo(n, seed):
    """(name, int32[2, n]) stereo pairs whose difference ch0 - ch1 wraps int32 (src/frame/frame_encoder.cpp:22-24 computes it in
    int32).  No encoder can code one: a residue is s - pred with |pred| < 2^28 (29 bits of a Q35 sum), so |s| <= 2^30 + 2^28 on
    both channels, and a difference beyond int32 then wraps to at least 2^30 - 2^28 in size and leaves a residue the zig-zag
    cannot take.  The decoder's side of the wrap (frame_decoder.cpp:65) comes from crafted frames: stereo_wrap_subframes."""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(0, P31 - 1, n).astype(np.int64)
    idx = rng.integers(1, n, max(1, n // 150))
    clicks = np.zeros(n, np.int64)
    clicks[idx] = rng.integers(P30, P30 + (1 << 28), len(idx))
    out = [("ramp, mirrored", np.stack([ramp, -ramp])),
           ("ramp, down and up", np.stack([ramp // 2 + P29, -(ramp // 2) - P29 + 3])),
           ("clicks against their negatives", np.stack([clicks, -clicks + rng.integers(-3, 4, n)]))]
    return [(name, np.asarray(x, np.int64).astype(np.int32)) for name, x in out]


def stereo_wrap_subframes(o, n, seed):
    """(subframes, want_wrap): a crafted stereo frame -- (channel, type, parent, q, residues) -- whose channel 1 is a difference
    subframe under a wide parent: parent samples near +-2^30 (order 2, residues +-(2^30 - 1)) and differences at -+2^30, so
    that parent - difference wraps int32 on the decoder's side."""
    rng = np.random.default_rng(seed)
    q0 = np.array([-40, 10], np.int32)
    r0 = rng.integers(-300, 301, n).astype(np.int32)
    pos = rng.integers(0, n, max(2, n // 30))
    r0[pos] = np.where(rng.random(len(pos)) < 0.5, P30 - 1, -(P30 - 1))
    parent = o.lpc_synth(2, q0, r0)
    d = rng.integers(-50, 51, n).astype(np.int32)
    d[pos] = np.where(parent[pos] >= 0, -P30, P30 - 1)
    wraps = int(((parent.astype(np.int64) - d) > P31 - 1).sum() + ((parent.astype(np.int64) - d) < -P31).sum())
    return [(0, 0, 0, q0, r0), (1, 1, 0, np.zeros(0, np.int32), d)], wraps


def frame_bytes(o, subframes, res_k=None):
    """On-disk frame bytes (src/file/sela_file.cpp:115-135) from (channel, type, parent, q, residues) tuples, Rice-coded by the
    oracle.  (gpu_common._build_frame does the same; this one needs no GPU test module.)"""
    import struct

    out = struct.pack("<I", 0xAA55FF00)
    for channel, typ, parent, q, res in subframes:
        ck, cw = o.rice_encode(np.asarray(q, np.int32))
        rk, rw = o.rice_encode(np.asarray(res, np.int32))
        out += struct.pack("<BBBBHB", channel, typ, parent, ck, len(cw), len(q)) + cw.astype("<u4").tobytes()
        out += struct.pack("<BHH", rk, len(rw), len(res)) + rw.astype("<u4").tobytes()
    return out


def encoder_refuses(o, planar):
    """Whether frame::FrameEncoder cannot code planar int32 [channels, n] in the format: a block not longer than its own order
    (the reference reads past its vector), a residue beyond the int32 zig-zag (|r| >= 2^30 but -2^30), or a Rice stream beyond
    the u16 word count -- of a channel, or of the difference an exactly-stereo frame also tries.  The oracle's frame encoder
    must not be called on such a frame."""
    ch, n = planar.shape
    signals = [planar[c] for c in range(ch)]
    if ch == 2:
        signals.append((planar[0].astype(np.int64) - planar[1]).astype(np.int32))
    for s in signals:
        order, _, r = o.lpc_analyze(s)
        if order >= n or r.min() < -P30 or r.max() >= P30:
            return True
        if len(o.rice_encode(r)[1]) > 65535:
            return True
    return False
