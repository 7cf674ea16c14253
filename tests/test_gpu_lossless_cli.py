"""`sela_mi355x -e --lossless in.wav out.sela` (sela::encodeFile with the lossless option): the file verifies clean
where plain `-e` leaves four lossy frames, and the reference's own decoder gives the WAV back.  (Where `--lossless` does not
belong it is refused: tests/test_lossless_cli_usage.py, no GPU.)"""
import os
import subprocess

import numpy as np
import pytest

import lossless_model as model
from gpu_common import MAIN_ON_HOST, gpu  # noqa: F401
from oracle_lib import oracle, reference
from test_host_cpp import HOST, _build, _write_wav

pytestmark = pytest.mark.gpu

CLI = os.path.join(HOST, "sela_mi355x")


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)


def test_lossless_file_verifies_clean_and_the_reference_decodes_it(gpu, tmp_path):  # noqa: F811
    _build()
    o = oracle()
    pcm = model.interleaved(model.cases()["A"])
    wav, plain, lossless, back = tmp_path / "in.wav", tmp_path / "plain.sela", tmp_path / "lossless.sela", tmp_path / "back.wav"
    _write_wav(wav, pcm.reshape(-1, 2))

    r = _run("-e", "--lossless", wav, lossless)
    assert r.returncode == 0 and "Encoding (lossless): " in r.stdout, r.stdout + r.stderr
    r = _run("-v", wav, lossless)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "verified 10 frames: 0 differ", r.stdout + r.stderr

    r = _run("-e", wav, plain)  # the control: today's stream of the same WAV
    assert r.returncode == 0, r.stderr
    r = _run("-v", wav, plain)
    assert r.returncode == 3 and r.stdout.splitlines()[-1] == "verified 10 frames: 4 differ", r.stdout + r.stderr
    assert [line.split(":")[0] for line in r.stdout.splitlines() if line.startswith("frame ")] == ["frame 1", "frame 4", "frame 5", "frame 6"]

    # the payloads are the model's streams: the plain one the reference's bit for bit, the lossless one equal in size
    want_plain, _ = model.stream(o, model.cases()["A"], False)
    want, offs = model.stream(o, model.cases()["A"], True)
    assert plain.read_bytes()[15:] == want_plain.tobytes()
    assert lossless.read_bytes()[:15] == plain.read_bytes()[:15] and lossless.read_bytes()[15:] == want.tobytes()
    assert os.path.getsize(lossless) == os.path.getsize(plain)

    # the reference's decoder on the file's frames (its library, where built), and its unchanged main.cpp on the file
    ref = reference()
    if ref is not None:
        got, _ = ref.decode_frames(want, offs, 2, threads=2)
        assert np.array_equal(got, pcm)
    got, _ = o.decode_frames(want, offs, 2, threads=2)
    assert np.array_equal(got, pcm)
    if os.path.exists(MAIN_ON_HOST):
        r = subprocess.run([MAIN_ON_HOST, "-d", str(lossless), str(back)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == wav.read_bytes()
    r = _run("-d", lossless, back)
    assert r.returncode == 0 and back.read_bytes() == wav.read_bytes()
