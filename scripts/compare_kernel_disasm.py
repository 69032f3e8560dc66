"""Per-kernel disassembly comparison of two builds of libradegs_hip.so (needs no GPU: build.py cross-compiles).

    python scripts/compare_kernel_disasm.py OLD.so NEW.so

For every gfx950 kernel symbol of OLD: is it in NEW, and are the instruction streams (`llvm-objdump -d` with addresses, encodings and the zero or
s_nop padding behind a kernel stripped, so a kernel that merely moved inside its code object compares equal) the same?  Kernels only NEW has are listed.  Exit status 1
when a kernel of OLD is missing from NEW or differs.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def kernels_of(lib):
    """{kernel symbol: [instruction lines]}"""
    tmp = tempfile.mkdtemp(prefix="radegs_dis_")
    try:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        data = open(fat, "rb").read()
        offs = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]   # one bundle per translation unit
        out = {}
        for n, o in enumerate(offs):
            end = offs[n + 1] if n + 1 < len(offs) else len(data)
            b, co = os.path.join(tmp, f"b{n}.bin"), os.path.join(tmp, f"b{n}.co")
            open(b, "wb").write(data[o:end])
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + b, "--output=" + co, "--unbundle"])
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co]).decode()
            names = set(re.findall(r"\.name:\s+(\S+)", notes))
            asm = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co]).decode()
            cur = None
            for line in asm.splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
                if m:
                    cur = m.group(1) if m.group(1) in names else None
                    if cur:
                        out[cur] = []
                elif cur and line.strip() and line.strip() != "...":   # "...": zero padding up to the next symbol's alignment
                    out[cur].append(re.sub(r"\s*//.*$", "", line).strip())   # the trailing comment is the address
        for ins in out.values():   # the padding behind a kernel can also be s_nop up to the next symbol's alignment: not part of the kernel
            while len(ins) > 1 and ins[-1] == "s_nop 0" and ins[-2] in ("s_nop 0", "s_endpgm"):
                ins.pop()
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    old, new = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    missing = sorted(k for k in old if k not in new)
    differ = sorted(k for k in old if k in new and old[k] != new[k])
    added = sorted(k for k in new if k not in old)
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW: {len(old) - len(missing) - len(differ)} identical, {len(differ)} differ, "
          f"{len(missing)} missing, {len(added)} new")
    for tag, ks in (("DIFFERS", differ), ("MISSING", missing), ("new", added)):
        for k in ks:
            print(f"  {tag}: {k}" + (f" ({len(new[k])} instructions)" if tag == "new" else ""))
    return 1 if (missing or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
