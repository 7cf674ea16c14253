"""Whole 24- and 32-bit WAV files through the CLI: -e --whole goes by the file's own header -- a 24- or 32-bit file
keeps its tail in a long last frame (sela_hip_encode_whole_pcm), a 16-bit file takes --keep-tail's path to --keep-tail's bytes --
and -v, -d and -d --start/--count read the tailed file without a flag: no tail reported, the data chunk back byte for byte, ranges in
front of, across, inside and past the tail."""
import os
import struct
import subprocess

import numpy as np
import pytest

import whole_pcm_cases as W
from gpu_common import HOST, _build, _write_wav, gpu  # noqa: F401
from sela_amd import codec
from sela_amd.synth import synth_pcm
from test_gpu_pcm_cli import _read_sela, _write_wide

pytestmark = pytest.mark.gpu

N = 2048


def _cli(*args):
    return subprocess.run([os.path.join(HOST, "sela_mi355x")] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _data_chunk(path):
    blob = open(path, "rb").read()
    at = blob.index(b"data")
    size = struct.unpack_from("<I", blob, at + 4)[0]
    assert len(blob) == at + 8 + size
    return blob[at + 8:]


@pytest.mark.parametrize("channels, bits, n", [(2, 24, 2 * N + 777), (1, 24, N + 5), (1, 32, 3 * N + 100), (2, 32, 1500)], ids=["stereo24", "mono24", "mono32", "stereo32_short"])
def test_whole_wide_files_through_the_cli(gpu, tmp_path, channels, bits, n):  # noqa: F811
    _build()
    b = bits // 8
    assert n % N
    x = W.track(n, channels, b, 1)
    data = _write_wide(tmp_path / "in.wav", x, bits)
    wav, sela, back = tmp_path / "in.wav", tmp_path / "whole.sela", tmp_path / "back.wav"
    out = _cli("-e", "--whole", "--lossless", wav, sela)
    assert out.returncode == 0 and "whole file" in out.stdout and " 0 samples per channel behind the last whole frame dropped" in out.stdout, out.stdout + out.stderr
    rate, sbits, sch, frames, payload = _read_sela(sela)
    want, want_offs = W.expected(n, channels, b, 1, True)
    assert (rate, sbits, sch, frames) == (48000, bits, channels, len(codec.whole_frames(n))) and payload.tobytes() == want
    verdict = _cli("-v", wav, sela)
    assert verdict.returncode == 0 and "tail:" not in verdict.stdout, verdict.stdout + verdict.stderr
    out = _cli("-d", sela, back)
    assert out.returncode == 0, out.stdout + out.stderr
    assert _data_chunk(back) == data
    # ranges: in front of the tail, across its start, inside it, across the stream's end, and past it
    base = N * (frames - 1)
    value = channels * b
    for start, count in ((0, 100), (max(base - 50, 0), 300), (base + 7, 333), (n - 10, 500)):
        part = tmp_path / "part.wav"
        out = _cli("-d", "--start", start, "--count", count, sela, part)
        assert out.returncode == 0, out.stdout + out.stderr
        kept = min(count, n - start)
        assert "%d samples per channel" % kept in out.stdout
        assert _data_chunk(part) == data[start * value: (start + kept) * value], (start, count)
    out = _cli("-d", "--start", n, "--count", 10, sela, tmp_path / "never.wav")
    assert out.returncode == 1 and "past the end" in out.stderr and not os.path.exists(tmp_path / "never.wav")


def test_whole_on_a_16_bit_file_gives_keep_tail_s_bytes(gpu, tmp_path):  # noqa: F811
    _build()
    pcm = synth_pcm(2 * N + 777, 2, 3)
    _write_wav(str(tmp_path / "in.wav"), pcm)
    for flags in ([], ["--lossless"]):
        a, b = _cli("-e", "--whole", *flags, tmp_path / "in.wav", tmp_path / "a.sela"), _cli("-e", "--keep-tail", *flags, tmp_path / "in.wav", tmp_path / "b.sela")
        assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout, a.stdout + a.stderr + b.stdout + b.stderr
        assert open(tmp_path / "a.sela", "rb").read() == open(tmp_path / "b.sela", "rb").read()
    frames, offs = codec.encode_whole_host(pcm, lossless=True)
    assert open(tmp_path / "a.sela", "rb").read()[15:] == frames.tobytes()
