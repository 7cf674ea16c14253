"""The shipped gfx950 code object, asked about k_envelope_frames: the fused envelope kernel is the decoder with a
reduction per bucket where it stores, and it is only as cheap as the decoder while it keeps the decoder's occupancy and writes no
PCM.  No GPU needed: llvm-readelf and llvm-objdump on the library.  (Vector stores and loads only are looked at.)"""
import pytest

from test_isa_verify import _disassembly, _resources, code_objects, decode_lds_bytes_for  # noqa: F401


def test_the_new_kernels_are_there_under_names_no_other_budget_claims(code_objects):  # noqa: F811
    res = _resources(code_objects)
    for name in ("k_envelope_frames", "k_envelope_channels"):
        assert len([n for n in res if name in n]) == 1, (name, [n for n in res if name in n])
    # the strings the other ISA tests select kernels by still select what they selected
    for claimed in ("k_level", "k_verify", "k_digest", "k_decode_frames", "k_stage_in"):
        assert not [n for n in res if claimed in n and "k_envelope" in n]
    assert len([n for n in res if "k_decode_framesILb0E" in n]) == 1 and len([n for n in res if "k_level_frames" in n]) == 1
    assert len([n for n in res if "k_verify_frames" in n]) == 1 and len([n for n in res if "k_digest_frames" in n]) == 1


def test_envelope_frames_keeps_the_decoder_s_registers_and_lds(code_objects):  # noqa: F811
    """72 VGPRs and at most one spilled: the budget of k_decode_frames, on which seven waves per SIMD rest; static LDS of at most
    128 bytes (nothing crosses waves behind the barrier: no partial results at all), so the launch's dynamic LDS is
    decode_lds_bytes_for itself -- 14 stereo workgroups per CU, as the decoder."""
    res = _resources(code_objects)
    r = res[next(n for n in res if "k_envelope_frames" in n)]
    d = res[next(n for n in res if "k_decode_framesILb0E" in n)]
    print("k_envelope_frames", r, "k_decode_frames<false>", d)
    assert r["vgpr"] <= 72 and r["vgpr_spill"] <= 1, r
    assert d["vgpr"] <= 72 and d["vgpr_spill"] <= 1, d
    assert r["lds"] <= 128, r
    from sela_amd import capi

    lds = capi.lib().sela_hip_debug_envelope_lds_bytes
    for channels in range(1, 9):
        got = int(lds(channels))
        assert 0 < got <= decode_lds_bytes_for(channels, channels), (channels, got)
        assert got == int(capi.lib().sela_hip_debug_verify_lds_bytes(channels)) == int(capi.lib().sela_hip_debug_levels_lds_bytes(channels))
    assert 160 * 1024 // int(lds(2)) == 160 * 1024 // decode_lds_bytes_for(2, 2) == 14
    assert int(lds(0)) == 0 and int(lds(9)) == 0


def test_envelope_frames_writes_records_and_no_pcm(code_objects):  # noqa: F811
    """Its global stores: one 8-byte word of a record per lane (the stereo form, the form for other channel counts, the zero
    records behind the frame's end), and the serial-parse fallback's residues into the workspace (dword stores in
    parse_stream_serial).  No 16-byte store (the decoder's stereo PCM), no short store (its other channel counts), no byte store."""
    f = _disassembly(code_objects, "k_envelope_frames")
    stores = [x for x in f if x[0].startswith(("global_store", "flat_store"))]
    print("stores in k_envelope_frames:", stores)
    assert stores, "the records are stored somewhere"
    assert not [x for x in stores if "store_short" in x[0] or "store_dwordx4" in x[0] or "store_byte" in x[0] or "store_dwordx3" in x[0]], stores
    assert [x for x in stores if x[0] in ("global_store_dwordx2", "flat_store_dwordx2")], "a record leaves as 8-byte words"
    assert all(x[0] in ("global_store_dword", "flat_store_dword", "global_store_dwordx2", "flat_store_dwordx2") for x in stores), stores
    d = _disassembly(code_objects, "k_decode_framesILb0E")
    assert [x for x in d if x[0] in ("global_store_dwordx4", "flat_store_dwordx4")], "the decoder this is held against stores its stereo PCM 16 bytes at a time"


def test_envelope_channels_writes_whole_words_too(code_objects):  # noqa: F811
    f = _disassembly(code_objects, "k_envelope_channels")
    stores = [x for x in f if x[0].startswith(("global_store", "flat_store"))]
    assert stores and all(x[0] in ("global_store_dwordx2", "flat_store_dwordx2") for x in stores), stores
