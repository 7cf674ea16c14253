"""`sela_mi355x -m in.sela` (sela::measureFile): one line per channel with the exact integers of sela_hip_levels
folded over the file's frames, then dBFS peak, dBFS RMS and DC; a last line for the track.  The integers are held against numpy on
the WAV's own data chunk."""
import math
import re

import numpy as np
import pytest

from gpu_common import _build, _write_wav, gpu  # noqa: F401
from sela_amd.synth import synth_frames
from test_gpu_pcm_cli import _cli, _samples, _write_wide

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^(channel (\d+)|track): peak=(\d+) samples=(\d+) sum=(-?\d+) sum_squares=(\d+) peak_dbfs=(\S+) rms_dbfs=(\S+) dc=(\S+)")


def _parse(stdout):
    out = {}
    for line in stdout.splitlines():
        m = LINE.match(line)
        if m:
            out[m.group(2) if m.group(2) is not None else "track"] = ([int(m.group(k)) for k in (3, 4, 5, 6)], [float(m.group(k)) for k in (7, 8, 9)], line)
    return out


def test_a_whole_file_with_its_tail(gpu, tmp_path):  # noqa: F811
    _build()
    pcm = synth_frames(4, 2, 21).reshape(-1, 2)[: 3 * 2048 + 777].copy()
    pcm[:, 1] //= 3  # (two channels that differ in level)
    wav, sela = tmp_path / "in.wav", tmp_path / "whole.sela"
    _write_wav(wav, pcm)
    assert _cli("-e", "--keep-tail", "--lossless", wav, sela).returncode == 0
    r = _cli("-m", sela)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _parse(r.stdout)
    assert sorted(got) == ["0", "1", "track"], r.stdout
    v = pcm.astype(np.int64)
    for c in (0, 1):
        want = [int(np.abs(v[:, c]).max()), len(v), int(v[:, c].sum()), int((v[:, c] * v[:, c]).sum())]
        assert got[str(c)][0] == want, (c, got[str(c)], want)
        peak_db, rms_db, dc = got[str(c)][1]
        assert abs(peak_db - 20 * math.log10(want[0] / 32768)) < 0.006 and abs(rms_db - 10 * math.log10(want[3] / want[1] / 32768 ** 2)) < 0.006
        assert abs(dc - want[2] / want[1]) < 0.00006
    assert got["track"][0] == [int(np.abs(v).max()), v.size, int(v.sum()), int((v * v).sum())]
    assert r.stdout.splitlines()[-1].startswith("track: ") and r.stdout.splitlines()[-1].endswith("(3 frames, 0 silent)")  # (two of 2048 and the long last one of 2048 + 777)


def test_a_24_bit_file_is_refused_by_name(gpu, tmp_path):  # noqa: F811
    _build()
    wav, sela = tmp_path / "in24.wav", tmp_path / "in24.sela"
    _write_wide(wav, _samples(2, 24, 5), 24)
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    r = _cli("-m", sela)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "24-bit" in r.stderr and str(sela) in r.stderr and "16-bit" in r.stderr, r.stderr


def test_two_paths_are_the_usage_text(gpu, tmp_path):  # noqa: F811
    _build()
    for args in (("-m", tmp_path / "a.sela", tmp_path / "b.sela"), ("-m",)):
        r = _cli(*args)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-m path/to/input.sela" in r.stdout, (args, r.stdout, r.stderr)
