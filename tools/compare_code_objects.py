#!/usr/bin/env python3
"""Do two builds of libsela_hip.so hold the same device code?  Both libraries' gfx950 code objects are taken out of their
.hip_fatbin sections (llvm-objcopy, clang-offload-bundler), disassembled (llvm-objdump -d) and compared function by function --
(index of the code object, function name) -> the list of (mnemonic, operands) -- so a function that several translation units
instantiate is compared copy by copy.  Prints how many functions of the first library are identical in the second, which differ,
which are gone and which are new; exit code 0 only if none differs and none is gone.  No GPU needed.
    python tools/compare_code_objects.py parent/sela_amd/libsela_hip.so sela_amd/libsela_hip.so
(the first library built from the parent commit by __graft_entry__.build_hip_library() in a checkout of its own)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def functions(lib):
    d = tempfile.mkdtemp()
    fat = os.path.join(d, "fat.bin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib])
    blob = open(fat, "rb").read()
    magic, starts, at = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (at := blob.find(magic, at)) >= 0:
        starts.append(at)
        at += 1
    head = re.compile(r"^([0-9a-fA-F]+) <([^>]+)>:")
    insn = re.compile(r"^\t(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
    out = {}
    for k, begin in enumerate(starts):
        part, co = os.path.join(d, "b%d.bin" % k), os.path.join(d, "d%d.co" % k)
        with open(part, "wb") as fh:
            fh.write(blob[begin: starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part, "--targets=" + TARGET, "--output=" + co])
        cur = None
        for line in subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True).splitlines():
            h = head.match(line)
            if h:
                cur = (k, h.group(2))
                out[cur] = []
                continue
            m = insn.match(line)
            if m and cur:
                out[cur].append((m.group(1), m.group(2)))
    return out, len(starts)


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    (a, a_objects), (b, b_objects) = functions(sys.argv[1]), functions(sys.argv[2])
    same = [n for n in a if n in b and a[n] == b[n]]
    differ = [n for n in a if n in b and a[n] != b[n]]
    gone = [n for n in a if n not in b]
    new = [n for n in b if n not in a]
    print("first: %d functions in %d code objects; second: %d in %d" % (len(a), a_objects, len(b), b_objects))
    print("identical %d (%d instructions), differ %d, gone %d, new %d" % (len(same), sum(len(a[n]) for n in same), len(differ), len(gone), len(new)))
    for label, names in (("differ", differ), ("gone", gone), ("new", new)):
        for k, name in names:
            print("%s: code object %d: %s" % (label, k, name))
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main())
