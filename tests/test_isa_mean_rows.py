"""The block mean of k_encode_teams with teams of 16 (the headline's encode kernel) runs on DPP rows, and the kernel keeps the
budgets its occupancy needs.  No GPU needed: llvm-objdump / llvm-readelf on the .so that travels to the GPU box.

A team of 16 is one DPP row, so the mean's strictly ordered FP64 chain (src/lpc/residue_generator.cpp:27-30) takes its
operands by row_newbcast straight from the lane that converted the sample: 16 v_fmac_f64 (x * 1.0 + sum, which rounds as the
add does) per 16 samples, no LDS and no barrier.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sela_amd", "libsela_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
TEAMS16 = "_ZN4sela14k_encode_teamsILi0ELi16E"  # the product instantiation (kMode 0, teams of 16)
HEAD = re.compile(r"^[0-9a-fA-F]+ <([^>]+)>:")


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools):
        pytest.skip("no built library or no LLVM tools")
    d = tmp_path_factory.mktemp("mean_rows")
    fat = str(d / "fat.bin")
    subprocess.check_call([tools[0], "--dump-section", ".hip_fatbin=" + fat, LIB])
    blob = open(fat, "rb").read()
    magic, starts, at = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (at := blob.find(magic, at)) >= 0:
        starts.append(at)
        at += 1
    cos = []
    for k, begin in enumerate(starts):
        part, co = str(d / f"b{k}.bin"), str(d / f"d{k}.co")
        with open(part, "wb") as f:
            f.write(blob[begin: starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        cos.append(co)
    return tools, cos


def _function(code_objects, prefix):
    tools, cos = code_objects
    body, cur = {}, None
    for co in cos:
        for line in subprocess.check_output([tools[2], "-d", co], text=True).splitlines():
            h = HEAD.match(line)
            if h:
                cur = h.group(1)
                body[cur] = []
            elif cur and line.startswith("\t"):
                body[cur].append(line.strip())
    names = [n for n in body if n.startswith(prefix)]
    assert len(names) == 1, names
    return body[names[0]]


def _resources(code_objects, prefix):
    tools, cos = code_objects
    found, cur = [], {}
    for co in cos:
        for line in subprocess.check_output([tools[3], "--notes", co], text=True).splitlines():
            text = line.strip().lstrip("- ")
            for key in (".name", ".private_segment_fixed_size", ".vgpr_count", ".vgpr_spill_count", ".group_segment_fixed_size"):
                if text.startswith(key + ":"):
                    cur[key] = text.split(":", 1)[1].strip()
            if text.startswith(".wavefront_size"):
                if cur[".name"].startswith(prefix):
                    found.append({"vgpr": int(cur[".vgpr_count"]), "vgpr_spill": int(cur[".vgpr_spill_count"]),
                                  "scratch": int(cur[".private_segment_fixed_size"]), "lds": int(cur[".group_segment_fixed_size"])})
                cur = {}
    assert len(found) == 1, (prefix, found)
    return found[0]


def test_teams16_mean_is_one_row_broadcast_fma_per_sample(code_objects):
    """Two chunks of 64 samples per loop trip: 128 v_fmac_f64 with a row_newbcast source, 8 for each of the 16 row lanes -- in
    each of the loop's two copies (stereo frames, whose samples are loaded as pairs, and every other channel count)."""
    insns = _function(code_objects, TEAMS16)
    chain = [i for i in insns if i.startswith("v_fmac_f64_dpp")]
    assert len(chain) == 2 * 128, len(chain)
    assert all(re.search(r"row_newbcast:\d+ row_mask:0xf bank_mask:0xf", i) for i in chain), chain[:4]
    lanes = [int(re.search(r"row_newbcast:(\d+)", i).group(1)) for i in chain]
    assert lanes == list(range(16)) * 16, lanes
    # one accumulator through each copy's chain
    assert all(len({i.split()[1] for i in half}) == 1 for half in (chain[:128], chain[128:])), chain[:4]


def test_teams16_keeps_its_occupancy_budgets(code_objects):
    """Three waves per SIMD (168 VGPRs) and twelve per CU (LDS), no spill, no scratch -- as tests/test_isa_handoffs.py pins."""
    r = _resources(code_objects, TEAMS16)
    assert r["vgpr"] <= 168 and r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] <= 160 * 1024 // 12, r
