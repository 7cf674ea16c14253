"""`sela_mi355x -s in.sela out.sela`: a file with a flipped sync word, a file cut in the middle of a frame and
a clean one -- the exit codes, the report's numbers against codec.salvage_frames on the same bytes, the salvaged files read to
their end by -d with the surviving frames' PCM in order, and the clean file written back byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_common import gpu  # noqa: F401
from sela_amd import codec
from sela_amd.synth import synth_pcm
from test_host_cpp import HOST, _build, _write_wav


def _report(text):
    announced, found = map(int, re.search(r"announced (\d+) frames, found (\d+)", text).groups())
    gaps = [tuple(map(int, g)) for g in re.findall(r"gap: file offset (\d+), (\d+) bytes, before frame (\d+)", text)]
    return announced, found, gaps, int(re.search(r"trailing: (\d+) bytes", text).group(1))


def _wav_frames(path, channels):
    with open(path, "rb") as f:
        data = f.read()
    return np.frombuffer(data[44:], "<i2").reshape(-1, 2048, channels)


@pytest.mark.gpu
def test_salvage_verb(gpu, tmp_path):  # noqa: F811
    _build()
    cli = os.path.join(HOST, "sela_mi355x")
    wav, clean = tmp_path / "in.wav", tmp_path / "clean.sela"
    _write_wav(wav, synth_pcm(12 * 2048, 2, 41))
    r = subprocess.run([cli, "-e", str(wav), str(clean)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = clean.read_bytes()
    offs = [int(o) for o in codec.index_frames(np.frombuffer(data[15:], np.uint8), 12, 2)]
    assert len(offs) == 13 and 15 + offs[12] == len(data)
    flipped = bytearray(data)
    flipped[15 + offs[5]] ^= 0xFF
    copies = {"flipped": (bytes(flipped), 2, [f for f in range(12) if f != 5]), "cut": (data[:15 + (offs[9] + offs[10]) // 2], 2, list(range(9))),
              "clean": (data, 0, list(range(12)))}
    r = subprocess.run([cli, "-d", str(clean), str(tmp_path / "clean.wav")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    original = _wav_frames(tmp_path / "clean.wav", 2)
    assert original.shape[0] == 12
    for name, (blob, code, survivors) in copies.items():
        src, dst, back = tmp_path / (name + ".sela"), tmp_path / (name + ".salvaged.sela"), tmp_path / (name + ".wav")
        src.write_bytes(blob)
        r = subprocess.run([cli, "-s", str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == code, (name, r.stdout, r.stderr)
        announced, found, gaps, trailing = _report(r.stdout)
        records, totals = codec.salvage_frames(np.frombuffer(blob[15:], np.uint8), 2)
        assert announced == 12 and found == len(records) == len(survivors) and trailing == len(blob) - 15 - int(totals[3])
        assert gaps == [(15 + int(rec["offset"]) - int(rec["skipped_before"]), int(rec["skipped_before"]), f) for f, rec in enumerate(records) if rec["skipped_before"]]
        assert [int(o) for o in records["offset"]] == [offs[f] for f in survivors]
        salvaged = dst.read_bytes()
        assert salvaged[:11] == blob[:11] and int.from_bytes(salvaged[11:15], "little") == found
        assert salvaged[15:] == b"".join(data[15 + offs[f]:15 + offs[f + 1]] for f in survivors)
        if name == "clean":
            assert salvaged == blob
        r = subprocess.run([cli, "-d", str(dst), str(back)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr)
        assert np.array_equal(_wav_frames(back, 2), original[survivors]), name
    # -C and -v read the salvaged file to its end: all 11 frames, where the damaged file gives them 5
    for path, frames in ((tmp_path / "flipped.salvaged.sela", 11), (tmp_path / "flipped.sela", 5)):
        r = subprocess.run([cli, "-C", str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and "frames=%d\n" % frames in r.stdout, (r.stdout, r.stderr)
        r = subprocess.run([cli, "-v", str(wav), str(path)], capture_output=True, text=True)
        assert r.returncode == 3 and "verified %d frames" % frames in r.stdout, (r.stdout, r.stderr)  # (3: the .wav has 12)
    # a file that is no .sela, and one without a frame: exit 1
    junk = tmp_path / "junk.sela"
    junk.write_bytes(b"RIFF" + bytes(64))
    assert subprocess.run([cli, "-s", str(junk), str(tmp_path / "junk.out")], capture_output=True, text=True).returncode == 1
    junk.write_bytes(data[:15] + bytes(4096))
    r = subprocess.run([cli, "-s", str(junk), str(tmp_path / "junk.out")], capture_output=True, text=True)
    assert r.returncode == 1 and _report(r.stdout)[1] == 0 and not (tmp_path / "junk.out").exists()
