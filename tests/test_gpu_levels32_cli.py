"""`sela_mi355x -M in.sela` (sela::measureWideFile): -m by the file's own header.  A 24- or 32-bit file prints one
line per channel with the exact integers of sela_hip_levels_i32 folded over the file's frames -- the sum of squares in 128 bits,
printed whole -- then dBFS peak and RMS against the file's own full scale and DC; a 16-bit file prints what -m prints.  The
integers are held against numpy on the WAV's own data chunk."""
import math

import numpy as np
import pytest

from gpu_common import _build, _write_wav, gpu  # noqa: F401
from sela_amd.synth import synth_frames
from test_gpu_levels_cli import _parse
from test_gpu_pcm_cli import _cli, _samples, _write_wide

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bits", [24, 32])
def test_a_whole_wide_file_with_its_tail(gpu, tmp_path, bits):  # noqa: F811
    _build()
    x = np.concatenate([_samples(2, bits, 30 + bits), _samples(2, bits, 31 + bits)])[: 3 * 2048 + 777].copy()
    x[:, 1] //= 3  # (two channels that differ in level)
    wav, sela = tmp_path / "in.wav", tmp_path / "whole.sela"
    _write_wide(wav, x, bits)
    r = _cli("-e", "--whole", "--lossless", wav, sela)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("-M", sela)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Measuring (%d-bit): " % bits in r.stdout
    got = _parse(r.stdout)
    assert sorted(got) == ["0", "1", "track"], r.stdout
    full = 1 << (bits - 1)
    columns = [[int(s) for s in x[:, c]] for c in (0, 1)]
    for c in (0, 1):
        v = columns[c]
        want = [max(abs(s) for s in v), len(v), sum(v), sum(s * s for s in v)]
        assert got[str(c)][0] == want, (c, got[str(c)], want)
        peak_db, rms_db, dc = got[str(c)][1]
        assert abs(peak_db - 20 * math.log10(want[0] / full)) < 0.006 and abs(rms_db - 10 * math.log10(want[3] / want[1] / full ** 2)) < 0.006
        assert abs(dc - want[2] / want[1]) < 0.00006
    both = columns[0] + columns[1]
    assert got["track"][0] == [max(abs(s) for s in both), len(both), sum(both), sum(s * s for s in both)]
    assert r.stdout.splitlines()[-1].startswith("track: ") and r.stdout.splitlines()[-1].endswith("(3 frames, 0 silent)")  # (two of 2048 and the long last one of 2048 + 777)
    print(bits, "track energy 2^%.1f" % math.log2(got["track"][0][3]))


def test_a_16_bit_file_prints_what_m_prints(gpu, tmp_path):  # noqa: F811
    _build()
    pcm = synth_frames(4, 2, 22).reshape(-1, 2)[: 3 * 2048 + 777].copy()
    wav, sela = tmp_path / "in.wav", tmp_path / "whole.sela"
    _write_wav(wav, pcm)
    assert _cli("-e", "--keep-tail", "--lossless", wav, sela).returncode == 0
    small, large = _cli("-m", sela), _cli("-M", sela)
    assert small.returncode == large.returncode == 0, large.stdout + large.stderr
    assert large.stdout == small.stdout and large.stderr == small.stderr and "sum_squares=" in large.stdout


def test_no_path_and_two_paths_are_the_usage_text(gpu, tmp_path):  # noqa: F811
    _build()
    for args in (("-M", tmp_path / "a.sela", tmp_path / "b.sela"), ("-M",)):
        r = _cli(*args)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-M path/to/input.sela" in r.stdout and "-m path/to/input.sela" in r.stdout, (args, r.stdout, r.stderr)
