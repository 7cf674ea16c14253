"""`sela_mi355x -C in.sela [in.wav]` (sela::digestWideFile): -c by the file's own header.  For a 24- or 32-bit
file the CRC-32 of the packed samples it decodes to, its byte count and the frame count; with a WAV of that width also the CRC-32
of its data chunk, and exit 0 only if the two agree.  The figures are held against zlib on the WAV's own data chunk.  (A wide
file keeps its tail with `-e --whole`: --keep-tail itself keeps to 16-bit files.)"""
import zlib

import numpy as np
import pytest

from gpu_common import _build, _write_wav, gpu  # noqa: F401
from sela_amd.synth import synth_frames
from test_gpu_digest_cli import WAV_LINE, _figures
from test_gpu_pcm_cli import _cli, _write_wide

pytestmark = pytest.mark.gpu

N_SAMPLES = 3 * 2048 + 777


@pytest.fixture(scope="module")
def tracks(tmp_path_factory):
    """3 frames and 777 samples of stereo music as a 24-bit and as a 32-bit WAV (28-bit amplitudes), and as a 16-bit one: written
    once, never changed.  bits -> (path, the data chunk's bytes)"""
    d = tmp_path_factory.mktemp("digest_pcm_cli")
    pcm = synth_frames(4, 2, 29).reshape(-1, 2)[:N_SAMPLES].astype(np.int32)
    rng = np.random.default_rng(29)
    out = {}
    for bits, shift in ((24, 8), (32, 12)):
        x = (pcm << shift) | rng.integers(0, 1 << shift, pcm.shape).astype(np.int32)
        out[bits] = (d / f"in{bits}.wav", _write_wide(d / f"in{bits}.wav", x, bits))
    _write_wav(d / "in16.wav", pcm.astype(np.int16))
    out[16] = (d / "in16.wav", np.ascontiguousarray(pcm.astype(np.int16), "<i2").tobytes())
    return out


@pytest.mark.parametrize("keep", [False, True], ids=["whole frames", "tail kept"])
@pytest.mark.parametrize("bits", [24, 32])
def test_a_wide_file_alone_and_against_its_wav(gpu, tracks, tmp_path, bits, keep):  # noqa: F811
    _build()
    wav, data = tracks[bits]
    sela = tmp_path / "out.sela"
    assert _cli("-e", *(("--whole",) if keep else ()), "--lossless", wav, sela).returncode == 0
    per = 2 * (bits // 8)
    held = data if keep else data[: 3 * 2048 * per]
    assert len(data) == N_SAMPLES * per
    r = _cli("-C", sela)
    assert r.returncode == 0 and f"Digest ({bits}-bit)" in r.stdout, r.stdout + r.stderr
    assert _figures(r.stdout) == (zlib.crc32(held), len(held), 3), r.stdout
    assert "beyond 24 bits" not in r.stdout and "wav:" not in r.stdout
    r = _cli("-C", sela, wav)
    m = WAV_LINE.search(r.stdout)
    assert m and (int(m.group(1), 16), int(m.group(2))) == (zlib.crc32(held), len(held)), r.stdout
    assert _figures(r.stdout) == (zlib.crc32(held), len(held), 3), r.stdout
    assert r.returncode == 0 and "match" in r.stdout and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    assert ("left out" in r.stdout) == (not keep)
    if not keep:
        assert f"({777 * per} bytes behind the last whole frame left out)" in r.stdout
    # ... and what -d writes has that CRC
    back = tmp_path / "back.wav"
    assert _cli("-d", sela, back).returncode == 0
    assert back.read_bytes()[-len(held):] == held
    # -c itself stays what it is: the file is refused by name
    r = _cli("-c", sela)
    assert r.returncode == 1 and f"{bits}-bit" in r.stderr and str(sela) in r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("bits", [24, 32])
def test_one_flipped_byte_is_found(gpu, tracks, tmp_path, bits):  # noqa: F811
    _build()
    wav, _ = tracks[bits]
    sela = tmp_path / "out.sela"
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    assert _cli("-C", sela, wav).returncode == 0
    blob = bytearray(sela.read_bytes())
    blob[len(blob) // 2] ^= 0x10  # (in the middle of a frame's residues)
    bad = tmp_path / "bad.sela"
    bad.write_bytes(bytes(blob))
    r = _cli("-C", bad, wav)
    assert r.returncode != 0, r.stdout + r.stderr


def test_a_32_bit_stream_read_as_24_bit_says_how_many_samples_lay_beyond(gpu, tracks, tmp_path):  # noqa: F811
    """the .sela header's width rewritten from 32 to 24: the samples are digested as their low three bytes, and counted"""
    _build()
    wav, data = tracks[32]
    sela = tmp_path / "out.sela"
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    blob = bytearray(sela.read_bytes())
    assert blob[8:10] == bytes([32, 0])
    blob[8:10] = bytes([24, 0])
    narrow = tmp_path / "narrow.sela"
    narrow.write_bytes(bytes(blob))
    x = np.frombuffer(data[: 3 * 2048 * 8], "<i4")
    low = np.ascontiguousarray(x.view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    beyond = int(((x < -(1 << 23)) | (x >= (1 << 23))).sum())
    assert beyond > 0
    r = _cli("-C", narrow)
    assert r.returncode == 0 and _figures(r.stdout) == (zlib.crc32(low), len(low), 3), r.stdout + r.stderr
    assert f"{beyond} samples beyond 24 bits" in r.stdout, r.stdout


def test_a_16_bit_file_prints_what_c_prints(gpu, tracks, tmp_path):  # noqa: F811
    _build()
    wav, data = tracks[16]
    sela = tmp_path / "out.sela"
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    for args in ((sela,), (sela, wav)):
        a, b = _cli("-c", *args), _cli("-C", *args)
        assert a.returncode == b.returncode == 0 and a.stdout == b.stdout and a.stderr == b.stderr, (a.stdout, b.stdout, b.stderr)
    held = data[: 3 * 2048 * 4]
    assert _figures(b.stdout) == (zlib.crc32(held), len(held), 3)


def test_a_wav_of_another_width_is_refused_by_name(gpu, tracks, tmp_path):  # noqa: F811
    _build()
    sela = tmp_path / "out.sela"
    assert _cli("-e", "--lossless", tracks[24][0], sela).returncode == 0
    for other in (32, 16):
        r = _cli("-C", sela, tracks[other][0])
        assert r.returncode == 1, r.stdout + r.stderr
        assert "24-bit" in r.stderr and f"{other}-bit" in r.stderr, r.stderr


def test_no_path_and_three_paths_are_the_usage_text(gpu, tmp_path):  # noqa: F811
    _build()
    for args in (("-C",), ("-C", tmp_path / "a.sela", tmp_path / "b.wav", tmp_path / "c.wav")):
        r = _cli(*args)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-C path/to/input.sela [path/to/input.wav]" in r.stdout, (args, r.stdout, r.stderr)
