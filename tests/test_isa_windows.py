"""The shipped gfx950 code object, asked about k_window_frames: the window kernel is the decoder with a clipped
store, and it is only as cheap as the decoder while it keeps the decoder's registers and LDS.  No GPU needed: llvm-readelf on the
library, the way tests/test_isa_verify.py asks about k_verify_frames."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sela_amd", "libsela_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# the decoder's LDS records (sela_decode_core.inc): DecSubframeLds, DecWaveScratch
SUBFRAME_LDS, WAVE_SCRATCH = (1072 + 4) * 4, 192 * 8


def decode_lds_bytes_for(channels, waves):
    """decode_lds_bytes_for (sela_decode_core.inc), restated"""
    return channels * SUBFRAME_LDS + waves * WAVE_SCRATCH + channels * 4 + waves * 4


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """kernel name -> its register, spill and static-LDS counts, from the notes of every gfx950 code object in the library"""
    tools = {t: os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools.values()):
        pytest.skip("no built library or no LLVM tools")
    d = tmp_path_factory.mktemp("isa_windows")
    fat = str(d / "fat.bin")
    subprocess.check_call([tools["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fat, LIB])
    blob = open(fat, "rb").read()
    magic, starts, at = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (at := blob.find(magic, at)) >= 0:
        starts.append(at)
        at += 1
    out = {}
    for k, begin in enumerate(starts):
        part, co = str(d / f"b{k}.bin"), str(d / f"d{k}.co")
        with open(part, "wb") as f:
            f.write(blob[begin: starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        cur = {}
        for line in subprocess.check_output([tools["llvm-readelf"], "--notes", co], text=True).splitlines():
            text = line.strip().lstrip("- ")
            for key in (".name", ".vgpr_count", ".vgpr_spill_count", ".group_segment_fixed_size"):
                if text.startswith(key + ":"):
                    cur[key] = text.split(":", 1)[1].strip()
            if text.startswith(".wavefront_size"):
                out[cur[".name"]] = {"vgpr": int(cur[".vgpr_count"]), "vgpr_spill": int(cur[".vgpr_spill_count"]), "lds": int(cur[".group_segment_fixed_size"])}
                cur = {}
    return out


def test_one_window_kernel_under_a_name_no_other_budget_claims(resources):
    assert len([n for n in resources if "k_window_frames" in n]) == 1, [n for n in resources if "window" in n]
    # the strings tests/test_isa_handoffs.py and tests/test_isa_verify.py select kernels by still select what they selected
    for claimed in ("k_decode_frames", "k_verify_frames", "k_decode_subframes32", "k_stage_in"):
        assert not [n for n in resources if claimed in n and "window" in n]


def test_window_frames_keeps_the_decoder_s_registers_and_lds(resources):
    """72 VGPRs and at most one spilled -- the budget of k_decode_frames, on which seven waves per SIMD rest -- and no static LDS:
    the launch's dynamic LDS is decode_lds_bytes_for itself, 14 stereo workgroups per CU, as the decoder."""
    r = resources[next(n for n in resources if "k_window_frames" in n)]
    d = resources[next(n for n in resources if "k_decode_framesILb0E" in n)]
    print("k_window_frames", r, "k_decode_frames<false>", d)
    assert r["vgpr"] <= 72 and r["vgpr_spill"] <= 1, r
    assert r["lds"] == 0, r
    from sela_amd import capi

    lds = capi.lib().sela_hip_debug_window_lds_bytes
    for channels in range(1, 9):
        assert int(lds(channels)) == decode_lds_bytes_for(channels, channels), channels
    assert int(lds(0)) == 0 and int(lds(9)) == 0
    assert 160 * 1024 // int(lds(2)) == 14
