"""The second pass of frame::FrameDecoder (src/frame/frame_decoder.cpp:40-69) as the 2048-sample kernels restate it -- the stereo
and the general form of k_decode_frames, the in-place pass of k_decode_frames_wide, the three loops of k_verify_frames and
k_verify_compare behind the wide kernel -- on every subframe layout of topology_cases.py: subframes out of channel order, a
difference in front of its parent, parents above and below their dependants, two differences under one parent, parents in
the other round of the eight waves, parent - difference beyond int16, a subframe on the serial parse.

All accepted cases of one channel count are one stream: one launch per call.  The expectation is always the CPU oracle's PCM
(topology_cases.accepted_stream, pinned to the reference by test_oracle_topologies.py), never another GPU call; what the
verify calls must report for planted differences is computed in numpy from (oracle PCM, planted PCM) alone."""
import functools

import numpy as np
import pytest

import topology_cases as tc
from gpu_common import gpu  # noqa: F401
from sela_amd import capi, codec
from test_gpu_verify_device import FAST, GUARD, NO_DIFF, _Device, _decode_n, _per_frame

pytestmark = pytest.mark.gpu

EFORMAT = -5
CHANNELS = tc.accepted_channels()  # 2: the stereo forms; 3, 5, 8: the general loops; 9, 12: k_decode_frames_wide, k_verify_compare


def _on_device(torch, stream, offs):
    frames = torch.from_numpy(np.array(stream)).cuda()
    o = torch.from_numpy(np.array(offs).view(np.int64)).cuda()
    return frames, o


def _accepted(ch):
    """topology_cases.accepted_stream with the stream and its offsets as copies of the test's own; the oracle's PCM stays the shared,
    read-only one."""
    cs, stream, offs, want = tc.accepted_stream(ch)
    return cs, np.array(stream), np.array(offs), want


def _standard_offsets(n):
    return np.arange(n + 1, dtype=np.uint64) * np.uint64(tc.N)


def _same_frames(got, want, cases, which=None):
    got = np.asarray(got).reshape(want.shape)
    for f in range(len(want)) if which is None else which:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, (cases[f][0], len(bad), bad[:4].tolist())


# ---- a. decode, accepted cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", CHANNELS)
def test_accepted_layouts_decode_to_the_oracles_pcm(gpu, ch):  # noqa: F811
    torch = gpu
    cs, stream, offs, want = _accepted(ch)
    n = len(cs)
    frames, o = _on_device(torch, stream, offs)
    # sela_hip_decode_device
    dec = codec.Decoder(n, ch)
    back = dec.decode(frames, o, n)
    torch.cuda.synchronize()
    dec.check()
    assert dec.status.cpu().numpy()[:2].tolist() == [0, 0]
    _same_frames(back.cpu().numpy(), want, cs)
    # sela_hip_decode_n_device, at the frames' own stride and at a larger one
    for stride in (tc.N, 3000):
        pcm, so, st = _decode_n(torch, stream, offs, ch, stride)
        assert codec.decode_n_status_error(st) == 0 and int(st[0]) == 0 and int(st[1]) == 0 and int(st[3]) == FAST, (stride, st)
        assert np.array_equal(so, _standard_offsets(n)), stride
        _same_frames(pcm[: n * tc.N].cpu().numpy(), want, cs)
    # sela_hip_decode_payload_n_device
    dn = codec.DecoderN(n, ch, tc.N)
    pcm, so, fo, count = dn.decode_payload(frames)
    torch.cuda.synchronize()
    st = dn.status.cpu().numpy().view(np.uint32)
    assert codec.decode_n_status_error(st) == 0 and int(st[3]) == FAST and int(count.item()) == n
    assert np.array_equal(fo.cpu().numpy().view(np.uint64), offs) and np.array_equal(so.cpu().numpy().view(np.uint64), _standard_offsets(n))
    _same_frames(pcm[: n * tc.N].cpu().numpy(), want, cs)
    # sela_hip_decode (the host pipeline: per-frame flags)
    _same_frames(codec.decode_host(stream, offs, ch), want, cs)


# ---- b. verify, the PCM as the oracle decodes it ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", CHANNELS)
def test_verify_finds_nothing_in_the_oracles_pcm(gpu, ch):  # noqa: F811
    cs, stream, offs, want = _accepted(ch)
    n = len(cs)
    for stride in (tc.N, 3000):
        counts, first, st = _Device(gpu, n, ch, stride).verify(stream, offs, want)
        assert st.tolist() == [0, 0, 0, FAST], (stride, st)
        assert (counts == 0).all(), (stride, [(cs[f][0], int(counts[f]), int(first[f])) for f in np.flatnonzero(counts)])
        assert (first == NO_DIFF).all(), stride


# ---- c. verify, planted differences -------------------------------------------------------------------------------------------------------
def _roles(case):
    subs = case[2]
    return {"dependent": tc.dependent_channels(subs), "parent": tc.parent_channels(subs), "unrelated": tc.unrelated_channels(subs)}


def _planted(ch, cs, pcm, seed):
    """A copy of pcm [frames, 2048, ch] with values changed in dependent channels, their parents' channels and channels that are
    neither: samples 0, 1 and 2047 of the first frame, the last one and two inner ones, and 30 random places."""
    rng = np.random.default_rng(seed)
    n = len(cs)
    spots, hit = set(), set()
    for f in (0, n - 1, n // 2, 1):
        for role, chans in _roles(cs[f]).items():
            for c in chans[:1]:
                spots |= {(f, i, c) for i in (0, 1, tc.N - 1)}
                hit.add(role)
    for _ in range(30):
        f = int(rng.integers(n))
        roles = [(r, c) for r, c in _roles(cs[f]).items() if c]
        role, chans = roles[int(rng.integers(len(roles)))]
        spots.add((f, int(rng.integers(tc.N)), int(chans[int(rng.integers(len(chans)))])))
        hit.add(role)
    assert hit == {"dependent", "parent", "unrelated"}, hit
    out = pcm.copy()
    bits = out.view(np.uint16)
    for f, i, c in sorted(spots):
        bits[f, i, c] ^= np.uint16(rng.integers(1, 1 << 16))
    return out


def _expected(want, changed):
    """(diff_counts, first_diff, lossy frames) as sela_hip.h defines them, from the two PCMs alone."""
    n, _, ch = want.shape
    counts, first = _per_frame((changed != want).reshape(-1, ch), _standard_offsets(n), ch)
    return counts, first, int((counts != 0).sum())


def _all_of_one_dependent_channel(cs, pcm):
    n = len(cs)
    f = next(f for f in range(1, n - 1) if _roles(cs[f])["dependent"])
    c = _roles(cs[f])["dependent"][-1]
    out = pcm.copy()
    out.view(np.uint16)[f, :, c] ^= np.uint16(0x8001)
    return out, f, c


@pytest.mark.parametrize("ch", CHANNELS)
def test_verify_finds_planted_differences_where_they_are(gpu, ch):  # noqa: F811
    cs, stream, offs, want = _accepted(ch)
    n = len(cs)
    dev = _Device(gpu, n, ch, tc.N)
    changed = _planted(ch, cs, want, 100 + ch)
    want_counts, want_first, lossy = _expected(want, changed)
    assert want_counts[0] >= 3 and want_counts[-1] >= 3 and lossy >= 4 and int(want_counts.sum()) >= 36
    counts, first, st = dev.verify(stream, offs, changed)
    assert np.array_equal(counts, want_counts), [(cs[f][0], int(counts[f]), int(want_counts[f])) for f in np.flatnonzero(counts != want_counts)]
    assert np.array_equal(first, want_first), [(cs[f][0], int(first[f]), int(want_first[f])) for f in np.flatnonzero(first != want_first)]
    assert st.tolist() == [0, 0, lossy, FAST]
    # every value of one dependent channel
    changed, f, c = _all_of_one_dependent_channel(cs, want)
    want_counts, want_first, lossy = _expected(want, changed)
    assert int(want_counts[f]) == tc.N and int(want_first[f]) == c and lossy == 1
    counts, first, st = dev.verify(stream, offs, changed)
    assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first) and st.tolist() == [0, 0, 1, FAST], (cs[f][0], int(counts[f]), int(first[f]))


# ---- d. the other loops and calls ---------------------------------------------------------------------------------------------------------
def test_a_stereo_pcm_off_the_16_byte_boundary(gpu):  # noqa: F811
    """k_verify_frames' scalar loop on stereo (PCM 2 and 6 bytes off a 16-byte boundary), with channel 0 under channel 1, the
    swapped orders and the wrapping frames in it -- the PCM as it is, then with planted differences."""
    torch = gpu
    ch = 2
    cs, stream, offs, want = _accepted(ch)
    n = len(cs)
    lib = capi.lib()
    frames, o = _on_device(torch, stream, offs)
    ws = torch.empty(int(lib.sela_hip_verify_workspace_bytes(n, ch, tc.N)), dtype=torch.uint8, device="cuda")
    for changed in (want, _planted(ch, cs, want, 7), _all_of_one_dependent_channel(cs, want)[0]):
        want_counts, want_first, lossy = _expected(want, changed)
        flat = np.array(changed).reshape(-1)
        for shift in (1, 3):  # int16 elements off the allocation's start
            room = torch.zeros(len(flat) + 8, dtype=torch.int16, device="cuda")
            room[shift: shift + len(flat)].copy_(torch.from_numpy(flat))
            before = room.clone()
            assert room.data_ptr() % 16 == 0
            counts = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
            first = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
            status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
            capi.check(lib.sela_hip_verify_device(frames.data_ptr(), o.data_ptr(), n, ch, tc.N, room.data_ptr() + 2 * shift, counts.data_ptr(),
                                                  first.data_ptr(), None, status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert torch.equal(room, before)
            got_counts, got_first = counts.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32)
            assert np.array_equal(got_counts[:n], want_counts), (shift, [(cs[f][0], int(got_counts[f]), int(want_counts[f])) for f in np.flatnonzero(got_counts[:n] != want_counts)])
            assert np.array_equal(got_first[:n], want_first), shift
            assert (counts.cpu().numpy()[n:] == -1).all() and (first.cpu().numpy()[n:] == -1).all()
            assert status.cpu().numpy().tolist() == [0, 0, lossy, FAST], shift


@pytest.mark.parametrize("ch", CHANNELS)
def test_the_host_pointer_and_the_payload_call(gpu, ch):  # noqa: F811
    """sela_hip_verify and sela_hip_verify_payload_device on the same streams."""
    torch = gpu
    cs, stream, offs, want = _accepted(ch)
    n = len(cs)
    frames, _ = _on_device(torch, stream, offs)
    ver = codec.Verifier(n, ch, tc.N)
    for changed in (want, _planted(ch, cs, want, 300 + ch)):
        want_counts, want_first, lossy = _expected(want, changed)
        counts, first, got_lossy = codec.verify_host(stream, offs, ch, changed)
        assert np.array_equal(counts, want_counts) and np.array_equal(first, want_first) and got_lossy == lossy
        c, f, count = ver.verify_payload(frames, torch.from_numpy(np.array(changed)).cuda())
        ver.check()
        assert int(count.item()) == n and ver.route() == FAST and ver.lossy_frames() == lossy
        assert np.array_equal(c.cpu().numpy().view(np.uint32), want_counts) and np.array_equal(f.cpu().numpy().view(np.uint32), want_first)


# ---- e. refused layouts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", tc.REFUSED_CHANNELS)
def test_refused_layouts_are_reported_and_their_neighbours_decoded(gpu, ch):  # noqa: F811
    """One channel named twice, a difference under itself, under another difference (chains included: refused by policy in
    these kernels), under a channel the frame has not, and a type the format has not: BAD_FRAME, counted once per frame; the
    accepted frames on both sides decode and verify as ever.  Nothing is asserted about a refused frame's own samples."""
    torch = gpu
    cs, mask, stream, offs, want = tc.refused_stream(ch)
    stream, offs = np.array(stream), np.array(offs)
    n = len(cs)
    good, n_bad = np.flatnonzero(mask), int((~mask).sum())
    frames, o = _on_device(torch, stream, offs)
    dec = codec.Decoder(n, ch)
    back = dec.decode(frames, o, n)
    torch.cuda.synchronize()
    with pytest.raises(capi.SelaHipError) as e:
        dec.check()
    assert e.value.code == EFORMAT
    st = dec.status.cpu().numpy().view(np.uint32)
    assert int(st[0]) == capi.FLAG_BAD_FRAME and int(st[1]) == n_bad, st
    _same_frames(back.cpu().numpy(), want, cs, good)
    with pytest.raises(capi.SelaHipError) as e:
        codec.decode_host(stream, offs, ch)
    assert e.value.code == EFORMAT
    pcm, so, dst = _decode_n(torch, stream, offs, ch, tc.N)
    assert codec.decode_n_status_error(dst) == EFORMAT
    assert int(dst[0]) == capi.FLAG_BAD_FRAME and int(dst[1]) == n_bad and int(dst[3]) == FAST, dst
    assert np.array_equal(so, _standard_offsets(n))
    _same_frames(pcm[: n * tc.N].cpu().numpy(), want, cs, good)
    counts, first, st = _Device(torch, n, ch, tc.N).verify(stream, offs, want)
    assert (int(st[0]), int(st[1]), int(st[3])) == (int(dst[0]), int(dst[1]), int(dst[3])), (st, dst)
    assert codec.decode_n_status_error(st) == EFORMAT
    assert (counts[good] == 0).all() and (first[good] == NO_DIFF).all(), [(cs[f][0], int(counts[f])) for f in good if counts[f]]


# ---- f. the serial parse between two frames on the fast plan --------------------------------------------------------------------------
# (layout of ACCEPTED_LAYOUTS / SERIAL_LAYOUTS, position of the long subframe): a parent with a dependant behind it; a dependant
# in k_decode_frames' general pass; the parent that the wide kernel's second round decodes
_SERIAL_BETWEEN = {2: (tc.SERIAL_LAYOUTS[2][0][1], 0), 8: (tc.ACCEPTED_LAYOUTS[8][0][1], 4), 9: (tc.ACCEPTED_LAYOUTS[9][0][1], 8)}


@functools.lru_cache(maxsize=None)
def _serial_between_fast(ch):
    """Three frames of one layout, the middle one with a subframe beyond the 1072-word plan -> (blobs, stream, offsets, oracle PCM),
    computed once per channel count and read-only."""
    from oracle_lib import oracle

    o = oracle()
    layout, pos = _SERIAL_BETWEEN[ch]
    blobs = []
    for f in range(3):
        scales = {pos: tc.LONG} if f == 1 else None
        blob = tc.wc.frame_bytes(o, tc.subframes(layout, tc.ORDINARY, 7000 + 10 * ch + f, scales))
        words = tc.subframe_words(blob, ch)
        assert [p for p in range(ch) if words[p] > tc.PLAN_WORDS] == ([pos] if f == 1 else []), (ch, f, words)
        blobs.append(blob)
    stream = np.frombuffer(b"".join(blobs), np.uint8).copy()
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    pcm = np.stack([o.frame_decode(b, ch)[0] for b in blobs])
    for a in (stream, offs, pcm):
        a.setflags(write=False)
    return blobs, stream, offs, pcm


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("ch", sorted(_SERIAL_BETWEEN))
def test_a_serial_parse_between_two_fast_frames_in_one_launch(gpu, ch, form):  # noqa: F811
    """The workspace hand-over behind the serial parse (lane 0 stores the residues, the wave reads them back) is one fence in
    k_decode_frames, k_decode_frames_wide and k_verify_frames: one launch whose middle workgroup takes it while its
    neighbours run the fast plan, in both recurrence forms, against the oracle's PCM."""
    torch = gpu
    _, stream, offs, want = _serial_between_fast(ch)
    stream, offs = np.array(stream), np.array(offs)  # (copies of the test's own; the oracle's PCM stays the shared one)
    n = 3
    frames, o = _on_device(torch, stream, offs)
    labels = [("fast",), ("serial",), ("fast",)]
    # differences in every frame, the serial one's long channel and its relatives among them
    changed = want.copy()
    bits = changed.view(np.uint16)
    for f, i, c, x in ((0, 5, 0, 1), (1, 0, ch - 1, 0x8000), (1, 777, 0, 3), (1, tc.N - 1, 1, 0xFFFF), (2, tc.N - 1, ch - 1, 0x10)):
        bits[f, i, c] ^= np.uint16(x)
    want_counts, want_first, lossy = _expected(want, changed)
    assert want_counts.tolist() == [1, 3, 1] and lossy == 3
    lib = capi.lib()
    lib.sela_hip_debug_decode_recurrence(form)
    try:
        dec = codec.Decoder(n, ch)
        back = dec.decode(frames, o, n)
        torch.cuda.synchronize()
        dec.check()
        assert dec.status.cpu().numpy()[:2].tolist() == [0, 0]
        _same_frames(back.cpu().numpy(), want, labels)
        pcm, so, st = _decode_n(torch, stream, offs, ch, tc.N)
        assert codec.decode_n_status_error(st) == 0 and int(st[0]) == 0 and int(st[1]) == 0 and int(st[3]) == FAST, st
        assert np.array_equal(so, _standard_offsets(n))
        _same_frames(pcm[: n * tc.N].cpu().numpy(), want, labels)
        ver = codec.Verifier(n, ch, tc.N)
        for p, counts_want, first_want, lossy_want in ((want, np.zeros(n, np.uint32), np.full(n, NO_DIFF, np.uint32), 0), (changed, want_counts, want_first, lossy)):
            counts, first = ver.verify(frames, o, n, torch.from_numpy(np.array(p)).cuda())
            ver.check()
            assert ver.status.cpu().numpy().view(np.uint32).tolist() == [0, 0, lossy_want, FAST]
            assert np.array_equal(counts.cpu().numpy().view(np.uint32), counts_want), counts
            assert np.array_equal(first.cpu().numpy().view(np.uint32), first_want), first
    finally:
        lib.sela_hip_debug_decode_recurrence(-1)
