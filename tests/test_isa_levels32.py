"""The shipped gfx950 code object, asked about the kernels of sela_hip_levels_i32_device: k_level32_direct
reduces from the subframes as decoded and stores no sample -- its stores are words of partial records and a frame's mark --, it
loads 16 bytes at a time where the rows allow it, and neither it nor k_level32_rest spills or uses scratch memory.  No GPU needed:
llvm-readelf and llvm-objdump on the library.  (Vector loads and stores only are looked at.)"""
from test_isa_verify import _disassembly, _resources, code_objects  # noqa: F401

# one name each: the templates by their mangled argument (ILb1E: the int4 rows, ILb0E: sample by sample)
NEW_KERNELS = ("k_level32_begin", "k_level32_directILb1E", "k_level32_directILb0E", "k_level32_restILb1E", "k_level32_restILb0E", "k_level32_sum")


def _one(res, part):
    names = [n for n in res if part in n]
    assert len(names) == 1, (part, names)
    return res[names[0]]


def test_every_new_kernel_is_there_once_under_a_name_no_other_budget_claims(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for part in NEW_KERNELS:
        print(part, _one(res, part))
    for name in ("k_level32_begin", "k_level32_direct", "k_level32_rest", "k_level32_sum"):
        assert [n for n in res if name in n], name
    assert len([n for n in res if "k_level32" in n]) == len(NEW_KERNELS)
    # the strings other budgets select kernels by select nothing here, and still select what they selected
    for claimed in ("k_level_frames", "k_level_channels", "k_level_count", "k_verify", "k_decode_subframes32", "k_generic_pack", "k_decode_frames", "k_stage_in"):
        assert not [n for n in res if claimed in n and "k_level32" in n], claimed
    for name in ("k_level_frames", "k_level_channels", "k_level_count", "k_verify32_sum", "k_verify32_gate"):
        assert len([n for n in res if name in n]) == 1, name


def test_the_reductions_do_not_spill(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for part in NEW_KERNELS[1:5]:
        r = _one(res, part)
        assert r["vgpr_spill"] == 0 and r.get("scratch", 0) == 0, (part, r)
        f = _disassembly(code_objects, part)
        assert not [x for x in f if x[0].startswith(("scratch_", "buffer_store", "buffer_load"))], part


def test_the_reductions_store_words_of_records_only(code_objects):  # noqa: F811
    """Their global stores: a word of a partial record (8 bytes, one of threads 0 .. 3) and, in the direct kernel, the frame's
    mark (a dword, set or cleared).  Nothing wider, no loop of sample stores: no decoded sample leaves the registers."""
    for part, vector in (("k_level32_directILb1E", True), ("k_level32_directILb0E", False), ("k_level32_restILb1E", True), ("k_level32_restILb0E", False)):
        f = _disassembly(code_objects, part)
        stores = [x for x in f if x[0].startswith(("global_store", "flat_store"))]
        print(part, "stores:", stores)
        assert stores and all(x[0] in ("global_store_dword", "flat_store_dword", "global_store_dwordx2", "flat_store_dwordx2") for x in stores), stores
        assert [x for x in stores if x[0].endswith("dwordx2")], "a partial record leaves as 8-byte words"
        assert len(stores) <= 6, stores
        wide = [x for x in f if x[0] in ("global_load_dwordx4", "flat_load_dwordx4")]
        assert bool(wide) == vector, (part, wide)
    s = _disassembly(code_objects, "k_level32_sum")
    stores = [x for x in s if x[0].startswith(("global_store", "flat_store"))]
    assert [x[0] for x in stores] in (["global_store_dwordx2"], ["flat_store_dwordx2"]), stores
