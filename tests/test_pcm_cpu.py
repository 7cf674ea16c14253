"""CPU-only: the two stand-alone programs of the packed-PCM work, each built with -fsanitize=address,undefined and
run directly -- tests/c/pcm_layout.cpp replays k_pcm_unpack / k_pcm_pack from sela_pcm_layout.h (every byte written once, none
outside, every dword read aligned and holding input), tests/c/wav_probe.cpp holds file::probeWav against headers it writes."""
import os
import subprocess

from test_host_cpp import HOST, ROOT, _build

SAN = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _compile(tmp_path, name, sources, flags):
    exe = os.path.join(str(tmp_path), name)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra"] + SAN + flags + sources + ["-o", exe])
    return exe


def test_pcm_layout(tmp_path):
    exe = _compile(tmp_path, "pcm_layout", [os.path.join(ROOT, "tests", "c", "pcm_layout.cpp")], ["-I" + os.path.join(ROOT, "sela_amd", "csrc")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "pcm_layout ok: 216 shapes" in out.stdout, out.stdout + out.stderr


def test_wav_probe(tmp_path):
    _build()  # (wide.cpp's file functions call the library: it is linked, not run)
    lib_dir = os.path.join(ROOT, "sela_amd")
    exe = _compile(tmp_path, "wav_probe", [os.path.join(ROOT, "tests", "c", "wav_probe.cpp"), os.path.join(HOST, "src", "wide.cpp")],
                   ["-pthread", "-I" + os.path.join(HOST, "include"), "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lsela_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath-link," + ROCM + "/lib", "-L" + ROCM + "/lib", "-lamdhip64", "-Wl,-rpath," + ROCM + "/lib"])
    scratch = tmp_path / "wavs"
    scratch.mkdir()
    out = subprocess.run([exe, str(scratch)], capture_output=True, text=True)
    assert out.returncode == 0 and "wav_probe ok" in out.stdout, out.stdout + out.stderr
