"""No GPU: `--lossless` is `sela_mi355x -e`'s alone.  Anywhere else -- `-E --lossless` above all, which is out of scope -- it is
refused with the usage text, not ignored, and nothing is written."""
import os
import subprocess

import numpy as np

from test_host_cpp import HOST, _build, _write_wav

CLI = os.path.join(HOST, "sela_mi355x")


def test_lossless_is_refused_where_it_does_not_belong(tmp_path):
    _build()
    wav = tmp_path / "in.wav"
    _write_wav(wav, np.zeros((2048, 2), np.int16))
    for args in (("-E", "--lossless", tmp_path, wav), ("-E", tmp_path, "--lossless", wav), ("-E", tmp_path, wav, "--lossless"),
                 ("-e", wav, "--lossless", tmp_path / "x.sela"), ("-e", "--lossless", wav), ("-d", "--lossless", wav, tmp_path / "x.wav"),
                 ("-v", "--lossless", wav, wav)):
        r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-e [--lossless]" in r.stdout, (args, r.stdout, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["in.wav"]
