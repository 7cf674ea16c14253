"""The shipped gfx950 code object, asked about the kernels of sela_hip_verify_i32_device: k_verify32_direct
compares from the subframes as decoded and stores no sample, it loads the original 16 bytes at a time where the rows allow it,
nothing spills, and the decode kernels the call is built on are the parent's, register for register.  No GPU needed:
llvm-readelf and llvm-objdump on the library."""
from test_isa_verify import _disassembly, _resources, code_objects  # noqa: F401

# one name each: the templates by their mangled argument (ILb1E: the int4 rows, ILb0E: sample by sample)
NEW_KERNELS = ("k_verify32_begin", "k_verify32_directILb1E", "k_verify32_directILb0E", "k_verify32_gate", "k_verify32_restILb1E", "k_verify32_restILb0E",
               "k_verify32_sum")

# read from the parent commit's build (tools/kernel_resources.py): VGPRs and static LDS of the kernels this call shares
PARENT = {
    "k_decode_subframes32ILb1E": (69, 5840),
    "k_decode_subframes32ILb0E": (56, 5840),
    "k_generic_decode": (36, 1832),
    "k_generic_combineILb1E": (32, 1024),
    "k_generic_combineILb0E": (50, 1024),
}


def _one(res, part):
    names = [n for n in res if part in n]
    assert len(names) == 1, (part, names)
    return res[names[0]]


def test_every_new_kernel_is_there_once_and_none_spills(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for part in NEW_KERNELS:
        r = _one(res, part)
        print(part, r)
        assert r["vgpr_spill"] == 0, (part, r)
        assert r["vgpr"] <= 64, (part, r)  # (eight waves per SIMD: these kernels wait for memory, nothing else)
    assert len([n for n in res if "k_verify32" in n]) == len(NEW_KERNELS)
    # the strings other budgets select kernels by select nothing here
    for claimed in ("k_verify_frames", "k_verify_compare", "k_verify_combine", "k_decode_subframes32", "k_generic_pack", "k_decode_frames", "k_stage_in"):
        assert not [n for n in res if claimed in n and "k_verify32" in n]


def test_the_shared_decode_kernels_keep_the_parent_s_registers_and_lds(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for part, (vgpr, lds) in PARENT.items():
        r = _one(res, part)
        assert (r["vgpr"], r["lds"], r["vgpr_spill"]) == (vgpr, lds, 0), (part, r)


def test_the_direct_kernel_stores_words_only_and_loads_the_original_16_bytes_at_a_time(code_objects):  # noqa: F811
    """Its global stores: the frame's mark (set or cleared) and the slice's two words -- dword stores only, four of them.  No
    wider store, no loop of stores: no decoded sample leaves the registers."""
    for part, vector in (("k_verify32_directILb1E", True), ("k_verify32_directILb0E", False)):
        f = _disassembly(code_objects, part)
        stores = [x for x in f if x[0].startswith(("global_store", "flat_store", "buffer_store", "scratch_store"))]
        print(part, "stores:", stores)
        assert stores and all(x[0] in ("global_store_dword", "flat_store_dword") for x in stores), stores
        assert len(stores) <= 4, stores
        wide = [x for x in f if x[0] in ("global_load_dwordx4", "flat_load_dwordx4")]
        assert bool(wide) == vector, (part, wide)
        if vector:  # the subframe as decoded, its parent's and the original: each 16 bytes per lane
            assert len(wide) >= 3, wide
    r = _disassembly(code_objects, "k_verify32_restILb1E")
    assert [x for x in r if x[0] in ("global_load_dwordx4", "flat_load_dwordx4")]
