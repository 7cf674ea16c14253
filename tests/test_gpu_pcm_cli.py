"""24- and 32-bit WAV files through the CLI: -e, -e --lossless and -d are routed by what the file's own header says;
the .sela payload is sela_hip_encode_i32's on the unpacked samples, the WAV that comes back is the canonical 44-byte PCM header and
the input's first whole frames byte for byte; a 16-bit file takes the path it always took, to the same bytes; every other verb
keeps its behaviour (for a 24-bit WAV: the reader's refusal)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from gpu_common import HOST, _build, _write_wav, gpu  # noqa: F401
from sela_amd import codec
from sela_amd.synth import synth_frames

pytestmark = pytest.mark.gpu

N = 2048
PCM_GUID = bytes([0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def _cli(*args):
    return subprocess.run([os.path.join(HOST, "sela_mi355x")] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _samples(channels, bits, seed):
    """3 frames and 100 samples more, int32 [3 * 2048 + 100, channels]: the synthetic music widened to `bits`, noise in the low bits"""
    rng = np.random.default_rng(seed)
    pcm = synth_frames(4, channels, seed).reshape(-1, channels)[: 3 * N + 100].astype(np.int32)
    shift = min(bits - 16, 12)  # (a 32-bit container holds 28-bit amplitudes: full scale is beyond what the format's residues carry)
    return (pcm << shift) | rng.integers(0, 1 << shift, pcm.shape).astype(np.int32)


def _packed(x, b):
    u = np.ascontiguousarray(x, np.int32).view(np.uint32)
    return np.stack([(u >> np.uint32(8 * k)).astype(np.uint8) for k in range(b)], axis=-1).reshape(-1).tobytes()


def _write_wide(path, x, bits, extensible=False, rate=48000):
    b, ch = bits // 8, x.shape[1]
    data = _packed(x, b)
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else 1, ch, rate, rate * ch * b, ch * b, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, 3) + PCM_GUID
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return data


def _read_sela(path):
    blob = open(path, "rb").read()
    assert blob[:4] == b"SeLa"
    rate, bits, channels, frames = struct.unpack("<IHBI", blob[4:15])
    return rate, bits, channels, frames, np.frombuffer(blob[15:], np.uint8)


@pytest.mark.parametrize("channels, bits, extensible", [(2, 24, False), (2, 24, True), (1, 32, False)], ids=["stereo24", "extensible24", "mono32"])
def test_wide_files_through_the_cli(gpu, tmp_path, channels, bits, extensible):  # noqa: F811
    _build()
    b = bits // 8
    x = _samples(channels, bits, 40 + bits + channels)
    data = _write_wide(tmp_path / "in.wav", x, bits, extensible)
    planar = np.ascontiguousarray(x[: 3 * N].reshape(3, N, channels).transpose(0, 2, 1))
    for flags, lossless in (([], False), (["--lossless"], True)):
        out = _cli("-e", *flags, tmp_path / "in.wav", tmp_path / "out.sela")
        assert out.returncode == 0, out.stdout + out.stderr
        assert "100 samples per channel behind the last whole frame dropped" in out.stdout
        rate, sbits, sch, frames, payload = _read_sela(tmp_path / "out.sela")
        assert (rate, sbits, sch, frames) == (48000, bits, channels, 3)
        want, offs = codec.encode_i32(planar, lossless=lossless)
        assert np.array_equal(payload, want), lossless
    # (out.sela is the lossless one now)
    out = _cli("-d", tmp_path / "out.sela", tmp_path / "back.wav")
    assert out.returncode == 0, out.stdout + out.stderr
    back = open(tmp_path / "back.wav", "rb").read()
    kept = 3 * N * channels * b
    assert back[:44] == (b"RIFF" + struct.pack("<I", 36 + kept) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, 48000, 48000 * channels * b, channels * b, bits)
                         + b"data" + struct.pack("<I", kept))
    assert back[44:] == data[:kept]


def test_a_16_bit_file_takes_the_path_it_always_took(gpu, tmp_path):  # noqa: F811
    _build()
    pcm = synth_frames(3, 2, 77)
    _write_wav(str(tmp_path / "in.wav"), pcm.reshape(-1, 2))
    out = _cli("-e", tmp_path / "in.wav", tmp_path / "out.sela")
    assert out.returncode == 0 and "Encoding: " in out.stdout, out.stdout + out.stderr
    rate, bits, channels, frames, payload = _read_sela(tmp_path / "out.sela")
    want, offs = codec.encode_host(pcm)
    assert (rate, bits, channels, frames) == (44100, 16, 2, 3) and np.array_equal(payload, want)
    out = _cli("-d", tmp_path / "out.sela", tmp_path / "back.wav")
    assert out.returncode == 0 and "Decoding: " in out.stdout, out.stdout + out.stderr
    back = open(tmp_path / "back.wav", "rb").read()
    assert back[44:] == codec.decode_host(want, offs, 2).tobytes()
    assert struct.unpack("<H", back[34:36])[0] == 16


def test_keep_tail_on_a_24_bit_file_is_still_the_readers_refusal(gpu, tmp_path):  # noqa: F811
    _build()
    _write_wide(tmp_path / "in.wav", _samples(2, 24, 5), 24)
    out = _cli("-e", "--keep-tail", tmp_path / "in.wav", tmp_path / "out.sela")
    assert out.returncode == 1 and "Only 16bits per sample wav is supported." in out.stderr, out.stdout + out.stderr
