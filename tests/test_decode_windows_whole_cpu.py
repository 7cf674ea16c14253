"""No GPU: what the whole-track window calls decide before a device is asked for, and what their kernels are in
the shipped code object.  The sizing function; every argument error of sela_hip_decode_windows_whole_device and
sela_hip_decode_windows_whole with its code -- the conditions, codes and texts of the 5.17 calls, on made-up addresses (every row
ends in a refusal, so nothing is dereferenced and nothing is launched); the host call's plan under ASan + UBSan in a stand-alone
program; the three new kernels' registers, scratch and stores."""
import os
import shutil
import subprocess

import pytest

from sela_amd import capi
from test_decode_windows_cpu import DEVICE_ARGS, DEVICE_REFUSALS, HOST_ARGS, HOST_REFUSALS, A, cover
from test_isa_verify import _disassembly, code_objects  # noqa: F401
from test_isa_handoffs import _kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -2, -4
I16, F32 = 0, 1


def workspace_bytes(n_windows, window_samples, channels):
    return int(capi.lib().sela_hip_decode_windows_whole_workspace_bytes(n_windows, window_samples, channels))


def device_call(short=0, **changes):
    a = dict(DEVICE_ARGS)
    assert not set(changes) - set(a)
    a.update(changes)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(workspace_bytes(a["n_windows"], a["window_samples"], a["channels"]) - short, 0)
    lib = capi.lib()
    rc = lib.sela_hip_decode_windows_whole_device(*[a[k] for k, _ in DEVICE_ARGS])
    return rc, lib.sela_hip_last_error().decode()


def host_call(**changes):
    a = dict(HOST_ARGS)
    assert not set(changes) - set(a)
    a.update(changes)
    lib = capi.lib()
    rc = lib.sela_hip_decode_windows_whole(*[a[k] for k, _ in HOST_ARGS])
    return rc, lib.sela_hip_last_error().decode()


def test_the_sizing_function_is_the_header_s_formula():
    """The existing call's bytes, a copy of each descriptor (16) and a record of its share of the last frame (32), per channel a
    record (16) and 4096 decoded 32-bit samples, and the alignment of the four pieces."""
    lib = capi.lib()
    for n_windows, window_samples, channels in ((1, 1, 1), (4, 777, 2), (64, 2050, 3), (256, 16000, 2), (3, 1 << 24, 8), (0, 5, 2), (8192, 16000, 2)):
        base = int(lib.sela_hip_decode_windows_workspace_bytes(n_windows, window_samples, channels))
        assert base == n_windows * cover(window_samples) * channels * 2048 * 4 + n_windows * 4 + 256
        want = base + n_windows * (48 + channels * (16 + 4 * 4096)) + 1024
        assert workspace_bytes(n_windows, window_samples, channels) == want, (n_windows, window_samples, channels)
    # ... which is what the capacity check goes by.  (Only refused calls are made here.)
    for window_samples in (1, 2, 2049, 2050):
        rc, text = device_call(window_samples=window_samples, short=1)
        assert rc == ECAPACITY and "sela_hip_decode_windows_whole_workspace_bytes()" in text
    # the existing call's workspace is too small for this one
    rc, text = device_call(workspace_bytes=int(lib.sela_hip_decode_windows_workspace_bytes(4, 777, 2)))
    assert rc == ECAPACITY


WHOLE_DEVICE_REFUSALS = [(c, code, text.replace("sela_hip_decode_windows_workspace_bytes()", "sela_hip_decode_windows_whole_workspace_bytes()"))
                         for c, code, text in DEVICE_REFUSALS]


@pytest.mark.parametrize("changes,code,text", WHOLE_DEVICE_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _, _ in WHOLE_DEVICE_REFUSALS])
def test_device_call_refuses_what_the_existing_call_refuses_with_its_code(changes, code, text):
    rc, said = device_call(**changes)
    assert rc == code and text in said, (rc, said)
    # the same condition, the same code from the existing call (its own workspace where the capacity is not the point)
    a = dict(DEVICE_ARGS)
    a.update({k: v for k, v in changes.items() if k != "short"})
    lib = capi.lib()
    if a["workspace_bytes"] is None:
        shaped = 1 <= a["channels"] <= 8 and 1 <= a["window_samples"] <= 1 << 24
        a["workspace_bytes"] = max(int(lib.sela_hip_decode_windows_workspace_bytes(a["n_windows"], a["window_samples"], a["channels"])) - changes.get("short", 0), 0) if shaped else 0
    assert lib.sela_hip_decode_windows_device(*[a[k] for k, _ in DEVICE_ARGS]) == code


def test_device_call_takes_every_alignment_its_elements_allow():
    assert device_call(d_out=A(4) + 2, short=1)[0] == ECAPACITY
    assert device_call(d_out=A(4) + 4, format=F32, short=1)[0] == ECAPACITY
    assert device_call(d_window_flags=0, short=1)[0] == ECAPACITY  # (NULL: no per-window flags)


@pytest.mark.parametrize("changes,text", HOST_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in HOST_REFUSALS])
def test_host_call_refuses_before_it_asks_for_a_device(changes, text):
    rc, said = host_call(**changes)
    assert rc == EINVAL and text in said, (rc, said)
    assert int(capi.lib().sela_hip_debug_windows_staged_bytes()) == 0


def test_host_call_of_no_windows_is_done_without_a_device():
    assert host_call(n_windows=0, windows=0, out=0)[0] == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_whole_call_s_host_plan_under_asan_and_ubsan(tmp_path):
    """plan_windows_whole (sela_window_plan.h), driven by tests/c/window_whole_plan.cpp on tables of real header bytes: which
    frames are staged, the compacted descriptors, windows entirely inside the tail, starts at the uint64 extremes, a table whose
    last frame is too short to hold a header."""
    exe = tmp_path / "window_whole_plan"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "sela_amd", "csrc"), os.path.join(ROOT, "tests", "c", "window_whole_plan.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])


# ---- the code object ------------------------------------------------------------------------------------------------------------
NEW_KERNELS = ("k_tailwin_plan", "k_tailwin_decode", "k_tailwin_store")


def test_every_new_kernel_is_there_once_spills_nothing_and_claims_no_other_budget_s_name():
    """The plan and the store use no scratch memory.  The decode kernel's private segment is the 12 bytes k_decode_subframes32
    has: the frame of the shared synthesis (sela_decode_core.inc's `synthesize`, a real call), which this kernel calls as that one
    does -- no register of the kernel is spilled into it, and it may not grow."""
    res = _kernel_resources()
    for part in NEW_KERNELS:
        names = [n for n in res if part in n]
        assert len(names) == 1, (part, names)
        r = res[names[0]]
        print(part, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (part, r)
        for claimed in ("k_window_frames", "k_decode_subframes32", "k_decode_frames", "k_verify"):
            assert claimed not in names[0]
    assert len([n for n in res if "k_tailwin" in n]) == len(NEW_KERNELS)
    one = lambda part: res[next(n for n in res if part in n)]  # noqa: E731
    assert one("k_tailwin_plan")["scratch"] == 0 and one("k_tailwin_store")["scratch"] == 0
    parent = one("k_decode_subframes32ILb1E")
    decode = one("k_tailwin_decode")
    assert decode["scratch"] <= parent["scratch"] <= 12, (decode, parent)
    # the decoder of any length's budget (tests/test_isa_handoffs.py): seven waves per SIMD
    assert decode["vgpr"] <= 72 and decode["lds"] <= 160 * 1024 // 28, decode


def test_the_store_kernel_stores_shorts_and_dwords_only(code_objects):  # noqa: F811
    f = _disassembly(code_objects, "k_tailwin_store")
    stores = [x for x in f if x[0].startswith(("global_store", "flat_store", "buffer_store", "scratch_store"))]
    print("k_tailwin_store stores:", stores)
    assert stores and all(x[0] in ("global_store_short", "global_store_dword", "flat_store_short", "flat_store_dword") for x in stores), stores
    assert any("short" in x[0] for x in stores) and any("dword" in x[0] for x in stores)
