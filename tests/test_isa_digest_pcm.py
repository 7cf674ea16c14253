"""The shipped gfx950 code object, asked about the kernels of sela_hip_digest_pcm_device: k_digest32_tiles packs a
tile of the subframes as decoded in LDS and takes its CRC there -- its global stores are the frame's mark and the tile's word, no
decoded byte --, it reads the image 16 bytes at a time, has no float instruction (no division by the channel count either), and
neither spills nor uses scratch memory; the folds it shares with the 16-bit digest stay free of floats and atomics.  No GPU needed:
llvm-readelf and llvm-objdump on the library.  (Vector loads and stores only are looked at.)"""
from test_isa_digest import re_float
from test_isa_verify import _disassembly, _resources, code_objects  # noqa: F401

# one name each: the template by its mangled arguments (<bytes per sample, rest>)
DIRECT = ("k_digest32_tilesILi3ELb0EE", "k_digest32_tilesILi4ELb0EE")
REST = ("k_digest32_tilesILi3ELb1EE", "k_digest32_tilesILi4ELb1EE")
NEW_KERNELS = ("k_digest32_begin",) + DIRECT + REST


def _one(res, part):
    names = [n for n in res if part in n]
    assert len(names) == 1, (part, names)
    return res[names[0]]


def test_every_new_kernel_is_there_once_under_a_name_no_other_budget_claims(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for part in NEW_KERNELS:
        print(part, _one(res, part))
    assert len([n for n in res if "k_digest32" in n]) == len(NEW_KERNELS)
    # the strings other budgets select kernels by select nothing here, and still select what they selected
    for claimed in ("k_digest_frames", "k_digest_pcm", "k_digest_slices", "k_digest_fold", "k_digest_track", "k_verify", "k_level", "k_decode_frames",
                    "k_decode_subframes32", "k_stage_in", "k_generic_pack", "k_pcm_pack", "k_pcm_unpack"):
        assert not [n for n in res if claimed in n and "k_digest32" in n], claimed
    for name in ("k_digest_frames", "k_digest_pcm", "k_digest_slices", "k_digest_fold", "k_digest_track", "k_verify32_gate"):
        assert len([n for n in res if name in n]) == 1, name


def test_the_tile_kernels_do_not_spill(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for part in DIRECT + REST:
        r = _one(res, part)
        assert r["vgpr_spill"] == 0 and r.get("scratch", 0) == 0, (part, r)
        assert r["lds"] <= 24 * 1024, (part, r)  # the image (16 KiB and a line), the judge's tables: six workgroups a compute unit
        f = _disassembly(code_objects, part)
        assert not [x for x in f if x[0].startswith(("scratch_", "buffer_store", "buffer_load"))], part


def test_the_direct_kernel_stores_a_mark_and_a_word_and_no_pcm(code_objects):  # noqa: F811
    """Its global stores: the frame's mark (set or cleared) and the tile's raw CRC, dwords (or 8-byte words); its other writes are
    atomics on the control word and the status words.  No byte store, no 12- or 16-byte store: k_pcm_pack's are gone."""
    for part in DIRECT + REST:
        f = _disassembly(code_objects, part)
        stores = [x for x in f if x[0].startswith(("global_store", "flat_store"))]
        print(part, "stores:", stores)
        assert stores and all(x[0] in ("global_store_dword", "flat_store_dword", "global_store_dwordx2", "flat_store_dwordx2") for x in stores), stores
        assert len(stores) <= (3 if part in DIRECT else 1), stores
        assert not [x for x in f if re_float(x[0])], (part, [x for x in f if re_float(x[0])][:4])
        # the image goes through the CRC 16 bytes at a time; the subframes come in as int4 where the rows allow it
        assert [x for x in f if x[0] == "ds_read_b128"], part
        assert [x for x in f if x[0] in ("global_load_dwordx4", "flat_load_dwordx4")], part
        atomics = [x for x in f if "atomic" in x[0] and x[0].startswith(("global_", "flat_"))]
        assert len(atomics) <= (4 if part.startswith("k_digest32_tilesILi3") else 3) - (0 if part in DIRECT else 1), (part, atomics)
    for part in DIRECT[1:] + REST[1:]:  # four bytes a sample: whole dwords into the image, and nothing counted
        f = _disassembly(code_objects, part)
        assert not [x for x in f if x[0].startswith("ds_write_b8")], part


def test_the_folds_have_no_float_and_no_atomic(code_objects):  # noqa: F811
    for name in ("k_digest32_begin", "k_digest_fold", "k_digest_track", "k_digest_slices"):
        k = _disassembly(code_objects, name)
        if name != "k_digest_slices":  # (its 64-bit division by the slice size is the compiler's reciprocal-and-correct sequence; a CRC never passes through it)
            assert not [x for x in k if re_float(x[0])], (name, [x for x in k if re_float(x[0])][:4])
        assert not [x for x in k if "atomic" in x[0]], name
