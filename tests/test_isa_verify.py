"""The shipped gfx950 code object, asked about k_verify_frames: the fused verification kernel is the decoder
with a compare where it stores, and it is only as cheap as the decoder while it keeps the decoder's occupancy and writes no PCM.
No GPU needed: llvm-readelf and llvm-objdump on the library."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sela_amd", "libsela_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# the decoder's LDS records (sela_decode_core.inc): DecSubframeLds, DecWaveScratch
SUBFRAME_LDS, WAVE_SCRATCH = (1072 + 4) * 4, 192 * 8


def decode_lds_bytes_for(channels, waves):
    """decode_lds_bytes_for (sela_decode.hip), restated"""
    return channels * SUBFRAME_LDS + waves * WAVE_SCRATCH + channels * 4 + waves * 4


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    tools = {t: os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools.values()):
        pytest.skip("no built library or no LLVM tools")
    d = tmp_path_factory.mktemp("isa_verify")
    fat = str(d / "fat.bin")
    subprocess.check_call([tools["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fat, LIB])
    blob = open(fat, "rb").read()
    magic, starts, at = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (at := blob.find(magic, at)) >= 0:
        starts.append(at)
        at += 1
    out = []
    for k, begin in enumerate(starts):
        part, co = str(d / f"b{k}.bin"), str(d / f"d{k}.co")
        with open(part, "wb") as f:
            f.write(blob[begin: starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        out.append(co)
    return tools, out


def _resources(code_objects):
    tools, cos = code_objects
    out = {}
    for co in cos:
        cur = {}
        for line in subprocess.check_output([tools["llvm-readelf"], "--notes", co], text=True).splitlines():
            text = line.strip().lstrip("- ")
            for key in (".name", ".private_segment_fixed_size", ".vgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size"):
                if text.startswith(key + ":"):
                    cur[key] = text.split(":", 1)[1].strip()
            if text.startswith(".wavefront_size"):
                out[cur[".name"]] = {"vgpr": int(cur[".vgpr_count"]), "vgpr_spill": int(cur[".vgpr_spill_count"]), "lds": int(cur[".group_segment_fixed_size"])}
                cur = {}
    return out


def _disassembly(code_objects, part):
    """the instructions (mnemonic, operands) of the one function whose name contains `part`"""
    tools, cos = code_objects
    head = re.compile(r"^([0-9a-fA-F]+) <([^>]+)>:")
    insn = re.compile(r"^\t(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
    found = {}
    for co in cos:
        cur = None
        for line in subprocess.check_output([tools["llvm-objdump"], "-d", co], text=True).splitlines():
            h = head.match(line)
            if h:
                cur = h.group(2) if part in h.group(2) else None
                if cur:
                    found[cur] = []
                continue
            m = insn.match(line)
            if m and cur:
                found[cur].append((m.group(1), m.group(2)))
    assert len(found) == 1, (part, list(found))
    return next(iter(found.values()))


def test_the_new_kernels_are_there_under_names_no_other_budget_claims(code_objects):
    res = _resources(code_objects)
    for name in ("k_verify_frames", "k_verify_compare", "k_verify_combine"):
        assert len([n for n in res if name in n]) == 1, (name, [n for n in res if name in n])
    # the strings tests/test_isa_handoffs.py selects kernels by still select what they selected
    for claimed in ("k_decode_framesILb0E", "k_decode_frames_wide", "k_stage_in", "k_decode_subframes32"):
        assert not [n for n in res if claimed in n and "verify" in n]
    assert len([n for n in res if "k_decode_framesILb0E" in n]) == 1


def test_verify_frames_keeps_the_decoder_s_registers_and_lds(code_objects):
    """72 VGPRs and at most one spilled: the budget of k_decode_frames, on which seven waves per SIMD rest; no static LDS at all
    (the reduction's words lie in the waves' synthesis tables), so the launch's dynamic LDS is decode_lds_bytes_for itself --
    14 stereo workgroups per CU, as the decoder."""
    res = _resources(code_objects)
    r = res[next(n for n in res if "k_verify_frames" in n)]
    d = res[next(n for n in res if "k_decode_framesILb0E" in n)]
    print("k_verify_frames", r, "k_decode_frames<false>", d)
    assert r["vgpr"] <= 72 and r["vgpr_spill"] <= 1, r
    assert d["vgpr"] <= 72 and d["vgpr_spill"] <= 1, d
    assert r["lds"] <= 16 * 8, r  # (static: nothing beyond what the reductions need)
    # what the launch asks for (launch_verify_frames takes its dynamic LDS from the function behind this hook)
    from sela_amd import capi

    lds = capi.lib().sela_hip_debug_verify_lds_bytes
    for channels in range(1, 9):
        got = int(lds(channels))
        assert 0 < got <= decode_lds_bytes_for(channels, channels) + 16 * channels, (channels, got)
    assert 160 * 1024 // int(lds(2)) == 160 * 1024 // decode_lds_bytes_for(2, 2) == 14
    assert int(lds(0)) == 0 and int(lds(9)) == 0


def test_verify_frames_writes_two_words_per_frame_and_no_pcm(code_objects):
    """Its global stores: diff_count[f] and first_diff[f] (one dword each, thread 0), and the serial-parse fallback's residues into
    the workspace (dword stores in parse_stream_serial, twice inlined: the coefficient and the residue stream).  No 16-byte
    store (the decoder's stereo PCM), no short store (its other channel counts)."""
    f = _disassembly(code_objects, "k_verify_frames")
    stores = [x for x in f if x[0].startswith(("global_store", "flat_store", "buffer_store"))]
    print("stores in k_verify_frames:", stores)
    assert stores, "the per-frame words are stored somewhere"
    assert all(x[0] in ("global_store_dword", "flat_store_dword") for x in stores), stores
    assert not [x for x in f if "store_short" in x[0] or "store_dwordx4" in x[0] or "store_byte" in x[0]]
    assert 2 <= len(stores) <= 2 + 4, stores
    d = _disassembly(code_objects, "k_decode_framesILb0E")
    assert [x for x in d if x[0] in ("global_store_dwordx4", "flat_store_dwordx4")], "the decoder this is held against stores its stereo PCM 16 bytes at a time"
    # ... and it loads what the decoder stores: the original, 16 bytes per thread
    assert [x for x in f if x[0] in ("global_load_dwordx4", "flat_load_dwordx4")]
