"""tools/kernel_resources.py [library] [--bytes-only]   (CPU only: reads the gfx950 code objects inside libsela_hip.so)

Prints, per kernel, the registers, spills, scratch and LDS from the code objects' metadata notes, and per kernel AND per
out-of-line device function the bytes of code from the code objects' symbol tables (profiles/r12/README.md has the table;
tests/test_code_bytes.py holds the sizes).  A device function that several translation units compile (synthesize<...>)
is listed once per code object.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
LIB = os.path.join(os.path.dirname(HERE), "sela_amd", "libsela_hip.so")
KEYS = (".name", ".private_segment_fixed_size", ".vgpr_count", ".vgpr_spill_count", ".group_segment_fixed_size", ".sgpr_spill_count")


def code_objects(lib, directory):
    """The gfx950 code objects of `lib` (one offload bundle per translation unit that has device code), unbundled into `directory`."""
    fat = os.path.join(directory, "fat.bin")
    subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib])
    blob = open(fat, "rb").read()
    magic, starts, at = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (at := blob.find(magic, at)) >= 0:
        starts.append(at)
        at += 1
    out = []
    for k, b in enumerate(starts):
        part, co = os.path.join(directory, f"b{k}.bin"), os.path.join(directory, f"dev{k}.co")
        with open(part, "wb") as f:
            f.write(blob[b: starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        out.append(co)
    return out


def demangle(names):
    if not names:
        return []
    tool = LLVM + "/llvm-cxxfilt"
    out = subprocess.check_output([tool if os.path.exists(tool) else "c++filt"], input="\n".join(names) + "\n", text=True).splitlines()
    return [n.split("(")[0].replace("void ", "") for n in out]


def resources(co):
    """[(mangled kernel name, {metadata key: value})] of one code object."""
    out, cur = [], {}
    for line in subprocess.check_output([LLVM + "/llvm-readelf", "--notes", co], text=True).splitlines():
        text = line.strip().lstrip("- ")
        for key in KEYS:
            if text.startswith(key + ":"):
                cur[key] = text.split(":", 1)[1].strip()
        if text.startswith(".wavefront_size"):
            out.append((cur[".name"], cur))
            cur = {}
    return out


def function_bytes(co):
    """[(mangled name, bytes of code)] of every function symbol of one code object: kernels and out-of-line device functions."""
    out = {}  # (a kernel is in .dynsym and in .symtab: once)
    for line in subprocess.check_output([LLVM + "/llvm-readelf", "-s", "--wide", co], text=True).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND" and f[2].isdigit() and int(f[2]) > 0:
            out[f[7]] = int(f[2])
    return list(out.items())


def code_bytes(lib=LIB):
    """[(code object index, demangled name without arguments, is a kernel, bytes)] for every function of the library's device code."""
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for k, co in enumerate(code_objects(lib, d)):
            kernels = {name for name, _ in resources(co)}
            fb = function_bytes(co)
            for (mangled, size), name in zip(fb, demangle([m for m, _ in fb])):
                rows.append((k, name, mangled in kernels, size))
    return rows


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    lib = args[0] if args else LIB
    with tempfile.TemporaryDirectory() as d:
        cos = code_objects(lib, d)
        if "--bytes-only" not in argv:
            for co in cos:
                res = resources(co)
                for (_, cur), n in zip(res, demangle([m for m, _ in res])):
                    print(f"{n:50s} vgpr {cur['.vgpr_count']:>4} vspill {cur['.vgpr_spill_count']:>3} sspill {cur['.sgpr_spill_count']:>3} "
                          f"scratch {cur['.private_segment_fixed_size']:>4} lds {cur['.group_segment_fixed_size']}")
    total = 0
    for k, name, is_kernel, size in sorted(code_bytes(lib), key=lambda r: (r[0], not r[2], -r[3])):
        print(f"code object {k:2d}  {'kernel  ' if is_kernel else 'function'}  {size:7d} B  {name}")
        total += size
    print(f"all device code: {total} B")


if __name__ == "__main__":
    main(sys.argv[1:])
