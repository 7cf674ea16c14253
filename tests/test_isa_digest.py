"""The shipped gfx950 code object, asked about k_digest_frames: the fused digest kernel is the decoder with a
CRC where it stores, and it is only as cheap as the decoder while it keeps the decoder's occupancy and writes no PCM.
No GPU needed: llvm-readelf and llvm-objdump on the library.  (Vector stores and loads only are looked at.)"""
from test_isa_verify import _disassembly, _resources, code_objects, decode_lds_bytes_for  # noqa: F401


def test_the_new_kernels_are_there_under_names_no_other_budget_claims(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for name in ("k_digest_frames", "k_digest_pcm", "k_digest_slices", "k_digest_fold", "k_digest_track"):
        assert len([n for n in res if name in n]) == 1, (name, [n for n in res if name in n])
    for claimed in ("k_decode_frames", "k_decode_subframes32", "k_stage_in", "k_verify", "k_level"):
        assert not [n for n in res if claimed in n and "k_digest" in n]


def test_digest_frames_keeps_the_decoder_s_registers_and_lds(code_objects):  # noqa: F811
    """72 VGPRs and none spilled to memory: the budget of k_decode_frames, on which seven waves per SIMD rest; static LDS of at
    most 128 bytes (the waves' words lie in their synthesis tables), so the launch's dynamic LDS is the level kernel's."""
    res = _resources(code_objects)
    r = res[next(n for n in res if "k_digest_frames" in n)]
    d = res[next(n for n in res if "k_decode_framesILb0E" in n)]
    print("k_digest_frames", r, "k_decode_frames<false>", d)
    assert r["vgpr"] <= 72 and r["vgpr_spill"] == 0, r
    assert r["lds"] <= 128, r
    from sela_amd import capi

    lds = capi.lib().sela_hip_debug_digest_lds_bytes
    for channels in range(1, 9):
        assert 0 < int(lds(channels)) <= decode_lds_bytes_for(channels, channels)
        assert int(lds(channels)) == int(capi.lib().sela_hip_debug_levels_lds_bytes(channels))
    assert 160 * 1024 // int(lds(2)) == 160 * 1024 // decode_lds_bytes_for(2, 2)
    assert int(lds(0)) == 0 and int(lds(9)) == 0


def test_digest_frames_writes_a_record_and_no_pcm(code_objects):  # noqa: F811
    """Its global stores: the frame's record as one 8-byte word, and the serial-parse fallback's residues into the workspace (dword
    stores in parse_stream_serial, twice inlined).  No 16-byte store (the decoder's stereo PCM), no short store, no byte store --
    and no float instruction and no atomic in the kernels that take the CRC of bytes in memory and fold the records."""
    f = _disassembly(code_objects, "k_digest_frames")
    stores = [x for x in f if x[0].startswith(("global_store", "flat_store"))]
    print("stores in k_digest_frames:", stores)
    assert [x for x in stores if x[0] in ("global_store_dwordx2", "flat_store_dwordx2")], "the record leaves as one 8-byte word"
    assert all(x[0] in ("global_store_dword", "flat_store_dword", "global_store_dwordx2", "flat_store_dwordx2") for x in stores), stores
    assert len(stores) <= 1 + 4, stores
    for name in ("k_digest_pcm", "k_digest_slices", "k_digest_fold", "k_digest_track"):
        k = _disassembly(code_objects, name)
        if name != "k_digest_slices":  # (its 64-bit division by the slice size is the compiler's reciprocal-and-correct sequence; a CRC never passes through it)
            assert not [x for x in k if re_float(x[0])], (name, [x for x in k if re_float(x[0])][:4])
        assert not [x for x in k if "atomic" in x[0]], name
        assert [x for x in k if x[0].startswith("global_load_dwordx4")] or name != "k_digest_pcm", "the lines are read 16 bytes at a time"


def re_float(mnemonic):
    return mnemonic.startswith("v_") and any(t in mnemonic for t in ("_f16", "_f32", "_f64")) and "cvt" not in mnemonic
