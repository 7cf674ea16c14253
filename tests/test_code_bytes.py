"""Bytes of code of the timed kernels and of the synthesis instantiations in the shipped gfx950 code objects, read from their
symbol tables by tools/kernel_resources.py: a guard against code growth (profiles/r12/README.md has the table these bounds come
from, the tree's own sizes with about 5 % of head-room).  Round 12 halved the 16-bit synthesize<2, 16, ...> by running one copy of
the block's text for both roles of the ring of 128's registers; written out once per role it is 24 KB again.  No GPU needed."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sela_amd", "libsela_hip.so")

# name prefix -> bytes allowed for every function of that name in every code object (tree: the figure in the comment)
KERNELS = {
    "sela::k_encode_teams<0, 16>": 66800,        # 63,652
    "sela::k_encode_teams<0, 8>": 57800,         # 55,072
    "sela::k_encode_blocks<0, false>": 51500,    # 49,024
    "sela::k_decode_frames<false>": 15200,       # 14,512
}
# the 16-bit instantiations (kOut32 = false: what k_decode_frames, the verifier and the window decoder call) ...
SYNTHESIS = {
    "sela::synthesize<1, 16, ": 7960,            # 7,412 .. 7,576
    "sela::synthesize<1, 4, ": 8550,             # 8,112 .. 8,136
    "sela::synthesize<2, 16, ": 11920,           # 11,092 .. 11,352 (the parent: 23,692 .. 24,212)
}
# ... and the 32-bit ones, which keep the parent's text (sela_synth.h says why): two copies of the ring-of-128 block
SYNTHESIS_32 = {
    "sela::synthesize<1, 16, ": 8550,            # 7,512 .. 8,144
    "sela::synthesize<1, 4, ": 9130,             # 8,156 .. 8,696
    "sela::synthesize<2, 16, ": 25670,           # 22,988 .. 24,452
}


@pytest.fixture(scope="module")
def code_bytes():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    needed = [os.path.join(tool.LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in needed):
        pytest.skip("no built library or no LLVM tools")
    return tool.code_bytes(LIB)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_a_timed_kernel_stays_within_its_code_bytes(code_bytes, name):
    rows = [r for r in code_bytes if r[1] == name and r[2]]
    assert len(rows) == 1, (name, rows)
    assert 0 < rows[0][3] <= KERNELS[name], rows


@pytest.mark.parametrize("wide", [False, True], ids=["16-bit", "32-bit"])
@pytest.mark.parametrize("prefix", sorted(SYNTHESIS))
def test_the_synthesis_instantiations_stay_within_their_code_bytes(code_bytes, prefix, wide):
    tail, bounds = (", true>", SYNTHESIS_32) if wide else (", false>", SYNTHESIS)
    rows = [r for r in code_bytes if r[1].startswith(prefix) and r[1].endswith(tail) and not r[2]]
    # sela_decode.hip, sela_decode32.hip, the verifier and the window decoders each compile their own copies
    assert len(rows) >= 4, (prefix, rows)
    for r in rows:
        assert 0 < r[3] <= bounds[prefix], r
