"""`sela_mi355x -d --start S --count N in.sela out.wav` (sela::decodeFileRange over sela_hip_decode_windows): the
samples S .. S + N - 1 per channel of plain -d's WAV, cut at the stream's end, in a WAV whose header says what it holds."""
import os
import struct
import subprocess

import numpy as np
import pytest

from gpu_common import gpu  # noqa: F401
from sela_amd.synth import synth_pcm
from test_host_cpp import HOST, _build, _write_wav

pytestmark = pytest.mark.gpu

CLI = os.path.join(HOST, "sela_mi355x")


def _read_wav(path):
    """-> (int16 [samples, channels], the header's fields)"""
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data"
    riff, = struct.unpack_from("<I", raw, 4)
    fmt_len, kind, ch, rate, byte_rate, align, bits = struct.unpack_from("<IhHIIHH", raw, 16)
    data, = struct.unpack_from("<I", raw, 40)
    assert (fmt_len, kind, bits, align, byte_rate) == (16, 1, 16, ch * 2, rate * ch * 2)
    assert riff == 36 + data and len(raw) == 44 + data
    return np.frombuffer(raw, "<i2", offset=44).reshape(-1, ch), dict(rate=rate, channels=ch, data=data)


@pytest.fixture(scope="module")
def files(gpu, tmp_path_factory):  # noqa: F811
    _build()
    d = tmp_path_factory.mktemp("range_cli")
    wav, sela, whole = d / "in.wav", d / "in.sela", d / "whole.wav"
    _write_wav(wav, synth_pcm(4 * 2048, 2, 23))
    for args in (("-e", wav, sela), ("-d", sela, whole)):
        r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout, r.stderr)
    pcm, head = _read_wav(whole)
    assert pcm.shape == (4 * 2048, 2)
    return d, sela, pcm, head


def _range(files, start, count, name):
    d, sela, _, _ = files
    out = d / name
    r = subprocess.run([CLI, "-d", "--start", str(start), "--count", str(count), str(sela), str(out)], capture_output=True, text=True)
    return r, out


def test_a_range_is_that_range_of_the_whole_decode(files):
    _, _, pcm, head = files
    r, out = _range(files, 3000, 5000, "mid.wav")
    assert r.returncode == 0, (r.stdout, r.stderr)
    got, h = _read_wav(out)
    assert h == dict(rate=head["rate"], channels=2, data=5000 * 4)
    assert np.array_equal(got, pcm[3000:8000])
    r, out = _range(files, 0, 4 * 2048, "all.wav")
    assert r.returncode == 0 and np.array_equal(_read_wav(out)[0], pcm)


def test_a_count_past_the_end_is_cut_at_the_end(files):
    _, _, pcm, _ = files
    r, out = _range(files, 8000, 5000, "tail.wav")
    assert r.returncode == 0, (r.stdout, r.stderr)
    got, h = _read_wav(out)
    assert h["data"] == (4 * 2048 - 8000) * 4 and np.array_equal(got, pcm[8000:])
    r, out = _range(files, 4 * 2048 - 1, 2 ** 63, "last.wav")
    assert r.returncode == 0 and np.array_equal(_read_wav(out)[0], pcm[-1:])


def test_a_start_at_the_end_fails_and_writes_nothing(files):
    for start in (4 * 2048, 4 * 2048 + 1, 2 ** 62):
        r, out = _range(files, start, 10, "none.wav")
        assert r.returncode == 1 and "past the end" in r.stderr, (r.returncode, r.stdout, r.stderr)
        assert not os.path.exists(out)
