"""The shipped gfx950 code object, asked about k_envelope32_direct and k_envelope32_rest: the envelope kernels of
24- and 32-bit streams write finished records and nothing else, keep no partial result anywhere, and use no scratch.  No GPU
needed: llvm-readelf and llvm-objdump on the library.  (Vector stores and loads only are looked at.)"""
import pytest

from test_isa_verify import _disassembly, _resources, code_objects  # noqa: F401

KERNELS = ("k_envelope32_directILb1E", "k_envelope32_directILb0E", "k_envelope32_restILb1E", "k_envelope32_restILb0E")
# what the build shows
VGPRS = {"k_envelope32_directILb1E": 28, "k_envelope32_directILb0E": 25, "k_envelope32_restILb1E": 33, "k_envelope32_restILb0E": 25}


def test_the_new_kernels_are_there_under_names_no_other_budget_claims(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for name in KERNELS:
        assert len([n for n in res if name in n]) == 1, (name, [n for n in res if name in n])
    assert len([n for n in res if "k_envelope32" in n]) == len(KERNELS)
    # the strings the other ISA tests select kernels by still select what they selected
    for claimed in ("k_level", "k_verify", "k_digest", "k_decode_frames", "k_stage_in", "k_window", "window", "k_envelope_frames", "k_envelope_channels"):
        assert not [n for n in res if claimed in n and "k_envelope32" in n], claimed
    assert len([n for n in res if "k_envelope_frames" in n]) == 1 and len([n for n in res if "k_envelope_channels" in n]) == 1
    assert len([n for n in res if "k_level32_directILb1E" in n]) == 1 and len([n for n in res if "k_verify32_restILb1E" in n]) == 1


def test_no_scratch_and_no_spilled_register(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for name in KERNELS:
        r = res[next(n for n in res if name in n)]
        print(name, r)
        assert r["vgpr_spill"] == 0, (name, r)
        f = _disassembly(code_objects, name)
        assert f and not [x for x in f if x[0].startswith("scratch_") or (x[0].startswith("buffer_") and "offen" in x[1])], name
        assert r["vgpr"] == VGPRS[name], (name, r)
    # static LDS: the layout judge's tables by channel in the direct kernel (256 x (4 + 4 + 2 + 2) + 4 bytes), none in the rest kernel
    for name in KERNELS:
        r = res[next(n for n in res if name in n)]
        assert r["lds"] <= (3080 if "direct" in name else 0), (name, r)


@pytest.mark.parametrize("name", KERNELS)
def test_the_stores_are_record_words_and_the_mark(code_objects, name):  # noqa: F811
    """k_envelope32_direct stores a dword (the frame's mark) and 8-byte words (the records, the zero words); k_envelope32_rest
    8-byte words only.  No 16-byte store (a decoded sample row), no short or byte store."""
    f = _disassembly(code_objects, name)
    stores = [x for x in f if x[0].startswith(("global_store", "flat_store", "buffer_store"))]
    print("stores in", name, stores)
    assert [x for x in stores if x[0] in ("global_store_dwordx2", "flat_store_dwordx2")], "a record leaves as 8-byte words"
    allowed = ("global_store_dwordx2", "flat_store_dwordx2") + (("global_store_dword", "flat_store_dword") if "direct" in name else ())
    assert all(x[0] in allowed for x in stores), stores
    if "direct" in name:
        assert [x for x in stores if x[0] in ("global_store_dword", "flat_store_dword")], "the mark"
    # the loads: int4 in the vector form, dwords in the other (beside the bookkeeping's)
    loads = [x[0] for x in f if x[0].startswith(("global_load", "flat_load"))]
    assert ("global_load_dwordx4" in loads or "flat_load_dwordx4" in loads) == name.endswith("ILb1E"), loads
