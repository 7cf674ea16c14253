"""`sela_mi355x -v in.wav in.sela` on 24- and 32-bit files (sela::verifyWideFile): routed by the WAV's own header as
-e is, the stream held against the WAV's packed data chunk by one sela_hip_verify_pcm call; the report and the exit codes are
verifyFile's.  The lossy frame is the reference's own (tests/golden/verify_wide.json)."""
import numpy as np
import pytest

from gpu_common import _build, gpu  # noqa: F401
from test_gpu_pcm_cli import N, _cli, _read_sela, _samples, _write_wide
from test_gpu_verify_i32_device import _fixture

pytestmark = pytest.mark.gpu


def _wide_fixture_frames():
    """frames 185 .. 189 of the widened corpus, interleaved [5 * 2048, 2]: frame 187 (here: 2) comes back with 9 values different"""
    fx, x = _fixture()
    entry = [e for e in fx["lossy"] if e["frame"] == 187][0]
    assert entry["count"] == 9
    return np.ascontiguousarray(x[185:190].transpose(0, 2, 1)).reshape(-1, 2)


def test_a_24_bit_file_with_the_references_lossy_frame(gpu, tmp_path):  # noqa: F811
    _build()
    x = _wide_fixture_frames()
    wav, sela, clean = tmp_path / "in.wav", tmp_path / "plain.sela", tmp_path / "lossless.sela"
    _write_wide(wav, x, 24)
    assert _cli("-e", wav, sela).returncode == 0
    r = _cli("-v", wav, sela)
    assert r.returncode == 3, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "frame 2: 9 values differ, first at index 3 (sample 1, channel 1)" in lines, lines
    assert [line for line in lines if line.startswith("frame ")] == ["frame 2: 9 values differ, first at index 3 (sample 1, channel 1)"]
    assert lines[-1] == "verified 5 frames: 1 differ" and not [line for line in lines if line.startswith(("tail:", "header:", "end:"))]

    # the lossless mode is the cure: exit 0
    assert _cli("-e", "--lossless", wav, clean).returncode == 0
    r = _cli("-v", wav, clean)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "verified 5 frames: 0 differ"

    # the same .sela against a WAV with one sample changed (in its sign byte): that frame, that index
    changed = x.copy()
    f, i, c = 4, 1234, 1
    changed[f * N + i, c] ^= 1 << 23
    wav2 = tmp_path / "changed.wav"
    _write_wide(wav2, changed, 24)
    r = _cli("-v", wav2, clean)
    assert r.returncode == 3, r.stdout + r.stderr
    assert f"frame {f}: 1 values differ, first at index {i * 2 + c} (sample {i}, channel {c})" in r.stdout.splitlines()
    assert r.stdout.splitlines()[-1] == "verified 5 frames: 1 differ"



def test_tails_ends_and_headers(gpu, tmp_path):  # noqa: F811
    _build()
    x = _wide_fixture_frames()
    wav, clean = tmp_path / "in.wav", tmp_path / "lossless.sela"
    _write_wide(wav, x, 24)
    assert _cli("-e", "--lossless", wav, clean).returncode == 0
    # a WAV with a tail: exit 4, and a shorter WAV: the samples the .sela holds beyond it
    wav3 = tmp_path / "tail.wav"
    _write_wide(wav3, np.concatenate([x, x[:777]]), 24)
    r = _cli("-v", wav3, clean)
    assert r.returncode == 4, r.stdout + r.stderr
    assert "tail: 777 samples per channel beyond the last whole frame are not in the .sela" in r.stdout.splitlines()
    assert "verified 5 frames: 0 differ" in r.stdout.splitlines()
    wav4 = tmp_path / "short.wav"
    _write_wide(wav4, x[: 4 * N + 48], 24)
    r = _cli("-v", wav4, clean)
    assert r.returncode == 3, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "end: the .sela holds 2000 samples per channel beyond the end of the .wav" in lines
    assert "frame 4: 4000 values differ, first at index 96 (sample 48, channel 0)" in lines and lines[-1] == "verified 5 frames: 1 differ"

    # headers that disagree: another rate
    wav5 = tmp_path / "rate.wav"
    _write_wide(wav5, x, 24, rate=44100)
    r = _cli("-v", wav5, clean)
    assert r.returncode == 3 and "header: sample rate 44100 in the .wav, 48000 in the .sela" in r.stdout.splitlines()



def test_widths_that_disagree(gpu, tmp_path):  # noqa: F811
    """a usage-level error (exit 1) that names both widths"""
    _build()
    x = _wide_fixture_frames()[: 2 * N]
    wav, clean = tmp_path / "in.wav", tmp_path / "lossless.sela"
    _write_wide(wav, x, 24)
    assert _cli("-e", "--lossless", wav, clean).returncode == 0
    wav32, sela32 = tmp_path / "in32.wav", tmp_path / "in32.sela"
    _write_wide(wav32, x, 32)
    assert _cli("-e", "--lossless", wav32, sela32).returncode == 0
    for a, b, wav_bits, sela_bits in ((wav, sela32, 24, 32), (wav32, clean, 32, 24)):
        r = _cli("-v", a, b)
        assert r.returncode == 1, r.stdout + r.stderr
        assert f"{wav_bits}-bit" in r.stderr and f"{sela_bits}-bit" in r.stderr, r.stderr
    # errors stay errors
    assert _cli("-v", tmp_path / "nothing.wav", clean).returncode == 1


@pytest.mark.parametrize("channels, bits, extensible", [(2, 24, True), (1, 32, False), (3, 32, False)], ids=["extensible24", "mono32", "three32"])
def test_encode_then_verify(gpu, tmp_path, channels, bits, extensible):  # noqa: F811
    _build()
    x = _samples(channels, bits, 90 + bits + channels)  # (3 frames and 100 samples more)
    wav, sela = tmp_path / "in.wav", tmp_path / "out.sela"
    _write_wide(wav, x, bits, extensible)
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    assert _read_sela(sela)[:4] == (48000, bits, channels, 3)
    r = _cli("-v", wav, sela)
    assert r.returncode == 4, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "tail: 100 samples per channel beyond the last whole frame are not in the .sela" in lines and lines[-1] == "verified 3 frames: 0 differ"
    assert not [line for line in lines if line.startswith(("frame ", "header:"))]
    # whole frames only: exit 0; then the last value of the file changed
    whole = x[: 3 * N].copy()
    _write_wide(wav, whole, bits, extensible)
    r = _cli("-v", wav, sela)
    assert r.returncode == 0, r.stdout + r.stderr
    whole[-1, channels - 1] ^= 1
    _write_wide(wav, whole, bits, extensible)
    r = _cli("-v", wav, sela)
    assert r.returncode == 3, r.stdout + r.stderr
    assert f"frame 2: 1 values differ, first at index {N * channels - 1} (sample {N - 1}, channel {channels - 1})" in r.stdout.splitlines()
