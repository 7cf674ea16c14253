"""`sela_mi355x -v in.wav in.sela` (sela::verifyFile): one line per frame that comes back different, one for the WAV's tail, and the
exit code says which of the two happened."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import corpus
from gpu_common import gpu  # noqa: F401
from oracle_lib import oracle
from sela_amd.synth import synth_pcm
from test_host_cpp import HOST, ROOT, _build, _write_wav

pytestmark = pytest.mark.gpu

CLI = os.path.join(HOST, "sela_mi355x")


def _run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)


def test_a_wav_with_a_tail(gpu, tmp_path):  # noqa: F811
    _build()
    n = 9 * 2048 + 777
    wav, sela = tmp_path / "in.wav", tmp_path / "out.sela"
    _write_wav(wav, synth_pcm(n, 2, 17))
    r = _run("-e", wav, sela)
    assert r.returncode == 0, r.stderr
    r = _run("-v", wav, sela)
    assert r.returncode == 4, r.stdout + r.stderr
    assert "tail: 777 samples per channel beyond the last whole frame are not in the .sela" in r.stdout.splitlines()
    assert "verified 9 frames: 0 differ" in r.stdout.splitlines()
    assert not [line for line in r.stdout.splitlines() if line.startswith(("frame ", "header:"))]


def test_whole_frames_with_a_lossy_one_a_clean_file_and_a_changed_sample(gpu, tmp_path):  # noqa: F811
    _build()
    with open(os.path.join(ROOT, "tests", "golden", "verify_corpus.json")) as fh:
        fx = json.load(fh)
    pcm = corpus.build(fx["frames"], fx["seed"])
    entry = fx["lossy"][2]  # (the frame with the fewest differing values)
    picked = [0, 1, entry["frame"], 2, 3]
    frames = pcm[picked]
    back, _ = oracle().decode_frames(*oracle().encode_frames(frames, threads=4)[:2], 2, threads=4)
    lossy = np.flatnonzero((back != frames).reshape(len(picked), -1).any(1)).tolist()
    assert 2 in lossy
    wav, sela = tmp_path / "lossy.wav", tmp_path / "lossy.sela"
    _write_wav(wav, frames.reshape(-1, 2))
    assert _run("-e", wav, sela).returncode == 0
    r = _run("-v", wav, sela)
    assert r.returncode == 3, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    want = f"frame 2: {entry['count']} values differ, first at index {entry['first']} (sample {entry['first'] // 2}, channel {entry['first'] % 2})"
    assert want in lines, lines
    assert [line.split(":")[0] for line in lines if line.startswith("frame ")] == [f"frame {f}" for f in lossy]
    assert f"verified 5 frames: {len(lossy)} differ" in lines and not [line for line in lines if line.startswith("tail:")]

    # a clean one: exit 0
    clean = frames[[f for f in range(5) if f not in lossy]]
    wav2, sela2 = tmp_path / "clean.wav", tmp_path / "clean.sela"
    _write_wav(wav2, clean.reshape(-1, 2))
    assert _run("-e", wav2, sela2).returncode == 0
    r = _run("-v", wav2, sela2)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == f"verified {len(clean)} frames: 0 differ"

    # the same .sela against a WAV with one sample changed: that frame, that index
    changed = clean.copy()
    f, i, c = len(clean) - 1, 1234, 1
    changed[f, i, c] ^= 0x40
    wav3 = tmp_path / "changed.wav"
    _write_wav(wav3, changed.reshape(-1, 2))
    r = _run("-v", wav3, sela2)
    assert r.returncode == 3, r.stdout + r.stderr
    assert f"frame {f}: 1 values differ, first at index {i * 2 + c} (sample {i}, channel {c})" in r.stdout.splitlines()
    assert r.stdout.splitlines()[-1] == f"verified {len(clean)} frames: 1 differ"

    # headers that disagree: another rate
    wav4 = tmp_path / "rate.wav"
    _write_wav(wav4, clean.reshape(-1, 2), rate=48000)
    r = _run("-v", wav4, sela2)
    assert r.returncode == 3 and "header: sample rate 48000 in the .wav, 44100 in the .sela" in r.stdout.splitlines()
    # errors stay errors
    assert _run("-v", tmp_path / "nothing.wav", sela2).returncode == 1


def test_a_sela_whose_frames_say_another_length(gpu, tmp_path):  # noqa: F811
    """Compared at the positions `-d` writes them."""
    from sela_amd import codec

    _build()
    n = 1500
    pcm = synth_pcm(3 * n, 2, 9).reshape(3, n, 2)
    blob, offs = codec.encode_host(pcm)
    sela, back, wav = tmp_path / "odd.sela", tmp_path / "back.wav", tmp_path / "changed.wav"
    sela.write_bytes(b"SeLa" + struct.pack("<IHBI", 44100, 16, 2, 3) + blob.tobytes())
    assert _run("-d", sela, back).returncode == 0
    r = _run("-v", back, sela)
    assert r.returncode == 0, r.stdout + r.stderr
    decoded = np.frombuffer(back.read_bytes()[44:], dtype="<i2").reshape(-1, 2).copy()
    decoded[n + 7, 0] ^= 1
    _write_wav(wav, decoded)
    r = _run("-v", wav, sela)
    assert r.returncode == 3 and "frame 1: 1 values differ, first at index 14 (sample 7, channel 0)" in r.stdout.splitlines(), r.stdout
