"""`sela_mi355x -s --any-byte in.sela out.sela`: a 12-frame file whose payload lost ONE byte.  Plain -s keeps
the frames in front of the damage only; --any-byte keeps what the model of the rule says, and -d reads its output to the end.
On an intact file both give exit 0 and the same output; the flag with any other verb is a usage error."""
import os
import subprocess

import numpy as np
import pytest

import salvage_unaligned_cases as ua
from gpu_common import gpu  # noqa: F401
from sela_amd import codec
from sela_amd.synth import synth_pcm
from test_gpu_salvage_cli import _report, _wav_frames
from test_host_cpp import HOST, _build, _write_wav


@pytest.mark.gpu
def test_salvage_any_byte_verb(gpu, tmp_path):  # noqa: F811
    _build()
    cli = os.path.join(HOST, "sela_mi355x")
    wav, clean = tmp_path / "in.wav", tmp_path / "clean.sela"
    _write_wav(wav, synth_pcm(12 * 2048, 2, 42))
    r = subprocess.run([cli, "-e", str(wav), str(clean)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = clean.read_bytes()
    offs = [int(o) for o in codec.index_frames(np.frombuffer(data[15:], np.uint8), 12, 2)]
    assert len(offs) == 13 and 15 + offs[12] == len(data)
    r = subprocess.run([cli, "-d", str(clean), str(tmp_path / "clean.wav")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    original = _wav_frames(tmp_path / "clean.wav", 2)

    # one byte dropped: the first of frame 5
    at = 15 + offs[5]
    dropped = tmp_path / "dropped.sela"
    dropped.write_bytes(data[:at] + data[at + 1:])
    body = np.frombuffer(dropped.read_bytes()[15:], np.uint8)
    want, want_totals = ua.model(body.tobytes(), 2, len(body) // 28)

    word_out, any_out = tmp_path / "word.sela", tmp_path / "any.sela"
    r = subprocess.run([cli, "-s", str(dropped), str(word_out)], capture_output=True, text=True)
    announced, found, gaps, trailing = _report(r.stdout)
    assert r.returncode == 2 and announced == 12 and found == 5 and gaps == [] and trailing == len(body) - offs[5], (r.stdout, r.stderr)
    assert word_out.read_bytes()[15:] == data[15:15 + offs[5]], "the frames in front only"

    r = subprocess.run([cli, "-s", "--any-byte", str(dropped), str(any_out)], capture_output=True, text=True)
    assert r.returncode == 2 and "\nSalvaging (any byte): %s\n" % dropped in r.stdout, (r.stdout, r.stderr)  # (behind the banner line)
    announced, found, gaps, trailing = _report(r.stdout)
    assert announced == 12 and found == want_totals[0] == len(want) and trailing == len(body) - want_totals[3]
    assert gaps == [(15 + o - skipped, skipped, f) for f, (o, skipped, _) in enumerate(want) if skipped], "gaps in bytes, at file offsets"
    # frame 5 is no frame any more; frames 6 .. 11, one byte off the word grid, are found
    assert [o for o, _, _ in want] == offs[:5] + [o - 1 for o in offs[6:12]] and gaps == [(15 + offs[5], offs[6] - 1 - offs[5], 5)]
    salvaged = any_out.read_bytes()
    assert salvaged[:11] == data[:11] and int.from_bytes(salvaged[11:15], "little") == 11
    assert salvaged[15:] == b"".join(body[o:o + n].tobytes() for o, _, n in want)
    back = tmp_path / "any.wav"
    r = subprocess.run([cli, "-d", str(any_out), str(back)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decoded = _wav_frames(back, 2)
    assert np.array_equal(decoded, original[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]])

    # an intact file: exit 0 and identical output from both
    outs = []
    for flags in ([], ["--any-byte"]):
        dst = tmp_path / ("intact%d.sela" % len(flags))
        r = subprocess.run([cli, "-s"] + flags + [str(clean), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0 and _report(r.stdout) == (12, 12, [], 0), (r.stdout, r.stderr)
        outs.append(dst.read_bytes())
    assert outs[0] == outs[1] == data

    # the flag is -s's alone
    for args in (["-d", "--any-byte", str(clean), str(tmp_path / "x.wav")], ["-s", str(clean), "--any-byte", str(tmp_path / "x.sela")],
                 ["-C", "--any-byte", str(clean)], ["-s", "--any-byte", str(clean)]):
        r = subprocess.run([cli] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "Usage:" in r.stdout and "announced" not in r.stdout, (args, r.stdout)
    assert "-s --any-byte " in subprocess.run([cli], capture_output=True, text=True).stdout
