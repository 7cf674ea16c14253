"""`sela_mi355x -e --pair-channels [--lossless]`: a 6-channel WAV comes back from `-d` sample for sample, the
.sela's payload is the model's stream (tests/paired_model.py), and the flag is refused, with the usage text and nothing written,
wherever it does not belong."""
import os
import subprocess

import numpy as np
import pytest

import paired_model as model
from oracle_lib import oracle
from test_host_cpp import HOST, _build, _write_wav

CLI = os.path.join(HOST, "sela_mi355x")


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.gpu
@pytest.mark.parametrize("lossless", [False, True], ids=["plain", "lossless"])
def test_six_channel_wav_round_trip(tmp_path, lossless):
    _build()
    frames = model.cases()["S6"][:6]
    pcm = model.interleaved(frames).reshape(-1, 6)  # [6 * 2048, 6]
    wav, sela, back = tmp_path / "in.wav", tmp_path / "out.sela", tmp_path / "back.wav"
    _write_wav(wav, pcm)
    r = _run("-e", "--pair-channels", *(["--lossless"] if lossless else []), wav, sela)
    assert r.returncode == 0, (r.stdout, r.stderr)
    blob, _ = model.stream(oracle(), frames, lossless)
    data = sela.read_bytes()
    assert data[:4] == b"SeLa" and data[10] == 6 and int.from_bytes(data[11:15], "little") == len(frames)
    assert data[15:] == blob.tobytes()
    if lossless:
        r = _run("-d", sela, back)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert np.array_equal(np.frombuffer(back.read_bytes()[44:], "<i2").reshape(-1, 6), pcm)
        r = _run("-v", wav, sela)
        assert r.returncode == 0, (r.stdout, r.stderr)


def test_pair_channels_is_refused_where_it_does_not_belong(tmp_path):
    """No GPU is asked for: every form ends at the usage text."""
    _build()
    wav = tmp_path / "in.wav"
    _write_wav(wav, np.zeros((2048, 6), np.int16))
    x = tmp_path / "x.sela"
    for args in (("-E", "--pair-channels", tmp_path, wav), ("-E", tmp_path, "--pair-channels", wav), ("-E", tmp_path, wav, "--pair-channels"),
                 ("-e", wav, "--pair-channels", x), ("-e", wav, x, "--pair-channels"), ("-e", "--pair-channels", wav),
                 ("-e", "--lossless", "--pair-channels", wav, x), ("-e", "--pair-channels", wav, "--lossless", x),
                 ("-e", "--pair-channels", wav, x, "--lossless"), ("-e", "--pair-channels", "--pair-channels", wav, x),
                 ("-e", "--pair-channels", "--lossless", wav), ("-e", "--pair-channels", "--lossless", "--lossless", wav, x),
                 ("-d", "--pair-channels", wav, tmp_path / "x.wav"), ("-v", "--pair-channels", wav, wav), ("-p", "--pair-channels", wav)):
        r = _run(*args)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-e [--lossless]" in r.stdout and "-e --pair-channels [--lossless]" in r.stdout, (args, r.stdout, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["in.wav"]
