"""`sela_mi355x -W [--bucket B] in.sela out.env` (sela::envelopeWideFile): the verb goes by the file's own header.
A 16-bit file takes -w's path and writes -w's bytes; a 24-bit file, a --whole one as it stands, writes the wide file: the same
32-byte header with 24 for its last word, then the 32-byte records of sela_hip_envelope_i32 on the track's grid -- held against
numpy over the WAV's samples.  -w itself still refuses such a file in its old words."""
import struct

import numpy as np
import pytest

from gpu_common import _build, _write_wav, gpu  # noqa: F401
from sela_amd import codec
from sela_amd.synth import synth_frames
from test_gpu_levels32 import _record
from test_gpu_pcm_cli import _cli, _samples, _write_wide

pytestmark = pytest.mark.gpu


def _read_wide_env(path):
    raw = open(path, "rb").read()
    magic, channels, bucket, samples, rate, bits = struct.unpack("<8sIIQII", raw[:32])
    assert magic == b"SELAENV1"
    records = np.frombuffer(raw[32:], codec.ENVELOPE32_DTYPE)
    assert len(records) == -(-samples // bucket) * channels
    return channels, bucket, samples, rate, bits, records.reshape(-1, channels)


def _numpy_envelope32(x, bucket):
    """x: int32 [n, channels] -> ENVELOPE32_DTYPE [ceil(n / bucket), channels], the energy in Python's integers"""
    out = np.zeros((-(-len(x) // bucket), x.shape[1]), codec.ENVELOPE32_DTYPE)
    for b in range(len(out)):
        for c in range(x.shape[1]):
            w = x[b * bucket: (b + 1) * bucket, c]
            _, _, total, energy = _record(w)
            out[b, c] = (int(w.min()), int(w.max()), total, energy & ((1 << 64) - 1), energy >> 64)
    return out


def test_a_16_bit_file_writes_the_bytes_of_the_narrow_verb(gpu, tmp_path):  # noqa: F811
    _build()
    pcm = synth_frames(4, 2, 22).reshape(-1, 2)[: 3 * 2048 + 777].copy()
    wav, sela = tmp_path / "in.wav", tmp_path / "in.sela"
    _write_wav(wav, pcm)
    assert _cli("-e", "--keep-tail", "--lossless", wav, sela).returncode == 0
    for args in ((), ("--bucket", "32")):
        small, large = _cli("-w", *args, sela, tmp_path / "w.env"), _cli("-W", *args, sela, tmp_path / "W.env")
        assert small.returncode == large.returncode == 0, large.stdout + large.stderr
        assert open(tmp_path / "w.env", "rb").read() == open(tmp_path / "W.env", "rb").read()
        assert large.stdout.replace("W.env", "w.env") == small.stdout


@pytest.mark.parametrize("whole", [False, True])
def test_a_24_bit_file_writes_the_wide_file(gpu, tmp_path, whole):  # noqa: F811
    _build()
    x = _samples(2, 24, 6)  # (3 * 2048 + 100 samples)
    wav, sela = tmp_path / "in24.wav", tmp_path / "in24.sela"
    _write_wide(wav, x, 24)
    assert _cli("-e", *(("--whole",) if whole else ()), "--lossless", wav, sela).returncode == 0
    held = x if whole else x[: 3 * 2048]
    for args, bucket in (((), 256), (("--bucket", "32"), 32), (("--bucket", "2048"), 2048)):
        env = tmp_path / f"out{bucket}.env"
        r = _cli("-W", *args, sela, env)
        assert r.returncode == 0 and "(24-bit)" in r.stdout, r.stdout + r.stderr
        channels, got_bucket, samples, rate, bits, records = _read_wide_env(env)
        assert (channels, got_bucket, samples, rate, bits) == (2, bucket, len(held), 48000, 24)
        want = _numpy_envelope32(held, bucket)
        for name in codec.ENVELOPE32_DTYPE.names:
            assert np.array_equal(records[name], want[name]), (bucket, name)
    # -w on that file still refuses in its old words, with its old exit code
    r = _cli("-w", sela, tmp_path / "narrow.env")
    assert r.returncode == 1 and "24-bit" in r.stderr and str(sela) in r.stderr and "the envelope is taken of 16-bit streams only" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "narrow.env").exists()


def test_a_bucket_outside_the_set_is_refused_with_the_set_named(gpu, tmp_path):  # noqa: F811
    _build()
    wav, sela = tmp_path / "in24.wav", tmp_path / "in24.sela"
    _write_wide(wav, _samples(2, 24, 5), 24)
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    r = _cli("-W", "--bucket", "48", sela, tmp_path / "out.env")
    assert r.returncode == 1, r.stdout + r.stderr
    assert "48" in r.stderr and "32, 64, 128, 256, 512, 1024, 2048" in r.stderr, r.stderr
    assert not (tmp_path / "out.env").exists()
    for args in (("-W", sela), ("-W", "--bucket", "64", sela)):
        r = _cli(*args)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-W [--bucket B]" in r.stdout, (args, r.stdout, r.stderr)
