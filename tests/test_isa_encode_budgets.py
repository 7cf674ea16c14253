"""The register and scratch budgets of the three encode kernels, from the code object's metadata (no GPU needed: llvm-readelf on
the built library, the figures tools/kernel_resources.py prints).

The residue filter's coefficient lives in a vector register pair instead of a scalar one, and the tail's addresses are bases
with constant offsets: that must not cost k_encode_teams<0,16> its three waves per SIMD, nor any of the three
a spilled register more than they had before.
"""
from test_isa_mean_rows import TEAMS16, _resources, code_objects  # noqa: F401  (fixture and helpers)

TEAMS8 = "_ZN4sela14k_encode_teamsILi0ELi8E"
BLOCKS = "_ZN4sela15k_encode_blocksILi0ELb0E"
# bytes of scratch per lane in the build of the commit before this change (fe9d4ae's kernels, unchanged since)
TEAMS8_SCRATCH_BEFORE = 48
BLOCKS_SCRATCH_BEFORE = 0


def test_teams16_fits_three_waves_per_simd_without_scratch(code_objects):  # noqa: F811
    r = _resources(code_objects, TEAMS16)
    assert r["vgpr"] <= 168 and r["scratch"] == 0 and r["vgpr_spill"] == 0, r


def test_teams8_and_blocks_spill_no_more_than_before(code_objects):  # noqa: F811
    r8 = _resources(code_objects, TEAMS8)
    rb = _resources(code_objects, BLOCKS)
    assert r8["vgpr"] <= 168 and r8["scratch"] <= TEAMS8_SCRATCH_BEFORE, r8
    assert rb["vgpr"] <= 168 and rb["scratch"] <= BLOCKS_SCRATCH_BEFORE, rb
