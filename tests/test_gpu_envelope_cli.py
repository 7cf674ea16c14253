"""`sela_mi355x -w [--bucket B] in.sela out.env` (sela::envelopeFile): a 32-byte header and the records of
sela_hip_envelope on the track's grid.  The header's fields and the records are held against codec.envelope_host and
codec.track_envelope on the file's own payload, and those against numpy on the WAV's data."""
import struct

import numpy as np
import pytest

from gpu_common import _build, _write_wav, gpu  # noqa: F401
from sela_amd import codec
from sela_amd.synth import synth_frames
from test_gpu_pcm_cli import _cli, _samples, _write_wide

pytestmark = pytest.mark.gpu


def _read_env(path):
    raw = open(path, "rb").read()
    magic, channels, bucket, samples, rate, bits = struct.unpack("<8sIIQII", raw[:32])
    assert magic == b"SELAENV1" and bits == 16
    records = np.frombuffer(raw[32:], codec.ENVELOPE_DTYPE)
    assert len(records) == -(-samples // bucket) * channels
    return channels, bucket, samples, rate, records.reshape(-1, channels)


def _payload(path, channels):
    """the frames of a .sela file as the library's own index finds them (the 15-byte header skipped)"""
    payload = np.frombuffer(open(path, "rb").read(), np.uint8)[15:].copy()
    offs = codec.index_frames(payload, len(payload) // (4 + 12 * channels), channels)  # (no more frames than fit: the walk ends at the file's end)
    return payload, offs


def _numpy_envelope(pcm, bucket):
    v = pcm.astype(np.int64)
    out = np.zeros((-(-len(v) // bucket), v.shape[1]), codec.ENVELOPE_DTYPE)
    for b in range(len(out)):
        w = v[b * bucket: (b + 1) * bucket]
        out["min"][b], out["max"][b], out["sum"][b], out["sum_squares"][b] = w.min(0), w.max(0), w.sum(0), (w * w).sum(0)
    return out


@pytest.mark.parametrize("tail", [False, True])
def test_the_file_holds_the_header_and_the_track_s_records(gpu, tmp_path, tail):  # noqa: F811
    _build()
    pcm = synth_frames(4, 2, 21).reshape(-1, 2)[: 3 * 2048 + 777].copy()
    pcm[:, 1] //= 3
    wav, sela = tmp_path / "in.wav", tmp_path / "in.sela"
    _write_wav(wav, pcm)
    assert _cli(*(("-e", "--keep-tail", "--lossless") if tail else ("-e", "--lossless")), wav, sela).returncode == 0
    held = pcm if tail else pcm[: 3 * 2048]
    payload, offs = _payload(sela, 2)
    so = codec.index_samples(payload, offs, 2)[0]
    assert int(so[-1]) == len(held)
    for args, bucket in ((("-w",), 256), (("-w", "--bucket", "32"), 32), (("-w", "--bucket", "2048"), 2048)):
        env = tmp_path / f"out{bucket}.env"
        r = _cli(*args, sela, env)
        assert r.returncode == 0, r.stdout + r.stderr
        channels, got_bucket, samples, rate, records = _read_env(env)
        assert (channels, got_bucket, samples, rate) == (2, bucket, len(held), 44100)
        want = codec.track_envelope(codec.envelope_host(payload, offs, 2, bucket), so, bucket)
        for name in codec.ENVELOPE_DTYPE.names:
            assert np.array_equal(records[name], want[name]), (bucket, name)
            assert np.array_equal(records[name], _numpy_envelope(held, bucket)[name]), (bucket, name, "against the WAV")


def test_a_24_bit_file_and_a_bucket_outside_the_set_are_refused(gpu, tmp_path):  # noqa: F811
    _build()
    wav, sela = tmp_path / "in24.wav", tmp_path / "in24.sela"
    _write_wide(wav, _samples(2, 24, 5), 24)
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    r = _cli("-w", sela, tmp_path / "out.env")
    assert r.returncode == 1, r.stdout + r.stderr
    assert "24-bit" in r.stderr and str(sela) in r.stderr and "16-bit" in r.stderr, r.stderr
    r = _cli("-w", "--bucket", "48", sela, tmp_path / "out.env")
    assert r.returncode == 1, r.stdout + r.stderr
    assert "48" in r.stderr and "32, 64, 128, 256, 512, 1024, 2048" in r.stderr, r.stderr
    assert not (tmp_path / "out.env").exists()
    for args in (("-w", sela), ("-w", "--bucket", "64", sela)):
        r = _cli(*args)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-w [--bucket B]" in r.stdout, (args, r.stdout, r.stderr)
