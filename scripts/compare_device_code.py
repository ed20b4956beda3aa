"""CPU only: do two builds of librwkv_hip.so hold the same device code?  Unbundles every gfx950 code object of both libraries and
compares the disassembly of every kernel symbol.

    python scripts/compare_device_code.py <a/librwkv_hip.so> <b/librwkv_hip.so>

The check of a host-side refactor: every kernel must come out identical.  Exit status 1 when a kernel differs or exists on one side only.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(lib, tmp):
    """{kernel symbol: disassembly text} over all code objects of the library's .hip_fatbin section (one bundle per translation unit)."""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, blob)]
    out = {}
    for i, a in enumerate(starts):
        part, co = os.path.join(tmp, f"bundle{i}.bin"), os.path.join(tmp, f"bundle{i}.co")
        open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}", f"--output={co}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True, check=True).stdout
        for sym, body in re.findall(r"^<([^>]+)>:\n(.*?)(?=^<|\Z)", text, flags=re.S | re.M):
            body = re.sub(r"\s*//.*", "", body)                 # objdump's address comments
            assert sym not in out, sym
            out[sym] = body
    return out


def main(a, b):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ka, kb = kernels(a, ta), kernels(b, tb)
    only = sorted(set(ka) ^ set(kb))
    differ = sorted(s for s in set(ka) & set(kb) if ka[s] != kb[s])
    print(f"{len(ka)} / {len(kb)} device symbols; {len(set(ka) & set(kb)) - len(differ)} identical, {len(differ)} differ, {len(only)} on one side only")
    for s in differ + only:
        print("  ", s)
    return 1 if differ or only else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
