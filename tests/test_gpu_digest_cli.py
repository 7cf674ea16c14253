"""`sela_mi355x -c in.sela [in.wav]` (sela::digestFile): the CRC-32 of the PCM the file decodes to, its byte count
and the frame count; with a WAV also the CRC-32 of its data chunk, and exit 0 only if the two agree.  The figures are held
against zlib on the WAV's own data chunk."""
import re
import zlib

import numpy as np
import pytest

from gpu_common import _build, _write_wav, gpu  # noqa: F401
from sela_amd.synth import synth_frames
from test_gpu_pcm_cli import _cli, _samples, _write_wide

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^crc32=([0-9a-f]{8}) bytes=(\d+) frames=(\d+)$", re.M)
WAV_LINE = re.compile(r"^wav: crc32=([0-9a-f]{8}) bytes=(\d+)", re.M)


def _figures(stdout):
    m = LINE.search(stdout)
    assert m, stdout
    return int(m.group(1), 16), int(m.group(2)), int(m.group(3))


@pytest.fixture(scope="module")
def track(tmp_path_factory):
    """3 frames and 777 samples of stereo music as a WAV: written once, never changed."""
    pcm = synth_frames(4, 2, 21).reshape(-1, 2)[: 3 * 2048 + 777].copy()
    wav = tmp_path_factory.mktemp("digest_cli") / "in.wav"
    _write_wav(wav, pcm)
    return wav, np.ascontiguousarray(pcm, "<i2")


def test_the_digest_of_an_encoded_file_is_zlibs(gpu, track, tmp_path):  # noqa: F811
    _build()
    wav, pcm = track
    sela = tmp_path / "lossless.sela"
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    r = _cli("-c", sela)
    assert r.returncode == 0, r.stdout + r.stderr
    whole_frames = pcm[: 3 * 2048].tobytes()
    assert _figures(r.stdout) == (zlib.crc32(whole_frames), len(whole_frames), 3), r.stdout
    # ... and what -d writes has that CRC
    out = tmp_path / "back.wav"
    assert _cli("-d", sela, out).returncode == 0
    assert out.read_bytes()[-len(whole_frames):] == whole_frames


@pytest.mark.parametrize("flags", [("--lossless",), (), ("--keep-tail", "--lossless")])
def test_a_file_against_its_wav(gpu, track, tmp_path, flags):  # noqa: F811
    _build()
    wav, pcm = track
    sela = tmp_path / "out.sela"
    assert _cli("-e", *flags, wav, sela).returncode == 0
    keep = "--keep-tail" in flags
    held = pcm.tobytes() if keep else pcm[: 3 * 2048].tobytes()
    r = _cli("-c", sela, wav)
    m = WAV_LINE.search(r.stdout)
    assert m and (int(m.group(1), 16), int(m.group(2))) == (zlib.crc32(held), len(held)), r.stdout
    crc, total, frames = _figures(r.stdout)
    assert (total, frames) == (len(held), 3)
    # (the plain stream is the reference's, which is not lossless on every frame of every track: on this one `-v` finds no frame
    # that differs, so all three agree with the WAV)
    assert r.returncode == 0 and crc == zlib.crc32(held) and "match" in r.stdout, r.stdout + r.stderr
    assert ("left out" in r.stdout) == (not keep)


def test_one_flipped_byte_is_found(gpu, track, tmp_path):  # noqa: F811
    _build()
    wav, _ = track
    sela = tmp_path / "out.sela"
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    assert _cli("-c", sela, wav).returncode == 0
    blob = bytearray(sela.read_bytes())
    blob[len(blob) // 2] ^= 0x10  # (in the middle of a frame's residues)
    bad = tmp_path / "bad.sela"
    bad.write_bytes(bytes(blob))
    r = _cli("-c", bad, wav)
    assert r.returncode != 0, r.stdout + r.stderr


def test_a_24_bit_file_is_refused_by_name(gpu, tmp_path):  # noqa: F811
    _build()
    wav, sela = tmp_path / "in24.wav", tmp_path / "in24.sela"
    _write_wide(wav, _samples(2, 24, 5), 24)
    assert _cli("-e", "--lossless", wav, sela).returncode == 0
    r = _cli("-c", sela)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "24-bit" in r.stderr and str(sela) in r.stderr and "16-bit" in r.stderr, r.stderr


def test_no_path_and_three_paths_are_the_usage_text(gpu, tmp_path):  # noqa: F811
    _build()
    for args in (("-c",), ("-c", tmp_path / "a.sela", tmp_path / "b.wav", tmp_path / "c.wav")):
        r = _cli(*args)
        assert r.returncode == 2 and "Usage:" in r.stdout and "-c path/to/input.sela [path/to/input.wav]" in r.stdout, (args, r.stdout, r.stderr)
