"""`sela_mi355x -d --start S --count N` on 24- and 32-bit .sela files (sela::decodeWideFileRange over sela_hip_decode_windows_i32,
DESIGN.md 5.23): the WAV that comes back carries the file's own width and holds exactly the slice of the input's data chunk --
and of what plain -d writes; the samples behind the last whole frame are absent, as plain -d drops them; a start at the stream's
end is decodeFileRange's refusal; a 16-bit file still goes through decodeFileRange, to the same bytes."""
import struct

import numpy as np
import pytest

from gpu_common import _build, _write_wav, gpu  # noqa: F401
from sela_amd import codec
from sela_amd.synth import synth_frames
from test_gpu_pcm_cli import _cli, _samples, _write_wide

pytestmark = pytest.mark.gpu

N = 2048
STREAM = 3 * N  # samples per channel of the three whole frames: the 100 behind them are dropped by -e
RANGES = [(0, 1), (2047, 3), (2048, 2048), (5000, 10 ** 6), (6144, 1)]


def _header(channels, bits, data_bytes, rate=48000):
    b = bits // 8
    return (b"RIFF" + struct.pack("<I", 36 + data_bytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * channels * b, channels * b, bits) + b"data"
            + struct.pack("<I", data_bytes))


@pytest.mark.parametrize("bits", [24, 32])
def test_ranges_of_a_wide_file(gpu, tmp_path, bits):  # noqa: F811
    _build()
    channels, b = 2, bits // 8
    data = _write_wide(tmp_path / "in.wav", _samples(channels, bits, 60 + bits), bits)
    assert len(data) == (STREAM + 100) * channels * b
    out = _cli("-e", "--lossless", tmp_path / "in.wav", tmp_path / "in.sela")
    assert out.returncode == 0, out.stdout + out.stderr
    out = _cli("-d", tmp_path / "in.sela", tmp_path / "whole.wav")
    assert out.returncode == 0, out.stdout + out.stderr
    whole = open(tmp_path / "whole.wav", "rb").read()
    assert whole[44:] == data[: STREAM * channels * b]
    for k, (start, count) in enumerate(RANGES):
        path = tmp_path / f"r{k}.wav"
        out = _cli("-d", "--start", start, "--count", count, tmp_path / "in.sela", path)
        if start >= STREAM:  # 6144: the stream's end -- the 100-sample tail is not in the file
            assert out.returncode == 1 and "past the end" in (out.stdout + out.stderr) and str(STREAM) in (out.stdout + out.stderr) and not path.exists(), out.stdout + out.stderr
            continue
        assert out.returncode == 0 and f"({bits}-bit)" in out.stdout, out.stdout + out.stderr
        got = open(path, "rb").read()
        lo, hi = start * channels * b, min(start + count, STREAM) * channels * b
        assert got[:44] == _header(channels, bits, hi - lo), (start, count)
        assert got[44:] == data[lo:hi] and got[44:] == whole[44 + lo: 44 + hi], (start, count)
        assert f"{min(count, STREAM - start)} samples per channel" in out.stdout
    for start in (STREAM, STREAM + 1, STREAM + 100):
        out = _cli("-d", "--start", start, "--count", 10, tmp_path / "in.sela", tmp_path / "past.wav")
        assert out.returncode == 1 and "past the end" in (out.stdout + out.stderr) and not (tmp_path / "past.wav").exists(), (start, out.stdout, out.stderr)


def test_a_16_bit_file_still_gives_decodeFileRange_s_bytes(gpu, tmp_path):  # noqa: F811
    _build()
    pcm = synth_frames(3, 2, 78)
    _write_wav(str(tmp_path / "in.wav"), pcm.reshape(-1, 2))
    out = _cli("-e", tmp_path / "in.wav", tmp_path / "in.sela")
    assert out.returncode == 0, out.stdout + out.stderr
    frames, offs = codec.encode_host(pcm)
    back = codec.decode_host(frames, offs, 2).reshape(-1, 2)
    for k, (start, count) in enumerate(RANGES[:4]):
        path = tmp_path / f"r{k}.wav"
        out = _cli("-d", "--start", start, "--count", count, tmp_path / "in.sela", path)
        assert out.returncode == 0 and "\nDecoding: " in out.stdout and "-bit)" not in out.stdout, out.stdout + out.stderr
        got = open(path, "rb").read()
        want = back[start: min(start + count, STREAM)].tobytes()
        assert got[:44] == _header(2, 16, len(want), rate=44100) and got[44:] == want, (start, count)
