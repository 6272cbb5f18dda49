"""Per-kernel resource table of a built library, for comparing two builds (no GPU needed).

    python tools/kernel_table.py LIB.so [--asm DIR] > table.tsv

One line per kernel over all of the library's gfx950 code objects: name, VGPRs, SGPRs, VGPR and
SGPR spills, private (scratch) and group (LDS) bytes, and the SHA-256 of its disassembly with
addresses stripped.  --asm DIR also writes each kernel's stripped disassembly to DIR/<sha of
name>.s.  Two trees that differ only in where code lives give the same table: `diff` them.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
KEYS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size")


def tool(name, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True, cwd=cwd).stdout


def main(lib, asm_dir=None):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))                  # (bundles are written beside the library)
        tool("llvm-objdump", "--offloading", "lib.so", cwd=tmp)        # one bundle per translation unit
        for co in sorted(f for f in os.listdir(tmp) if "amdgcn" in f):
            path = os.path.join(tmp, co)
            notes = tool("llvm-readelf", "--notes", path)
            res = {}
            for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
                res[name] = [re.search(r"^\s+%s:\s+(\d+)" % re.escape(k), blk, re.M).group(1) for k in KEYS]
            dis = tool("llvm-objdump", "-d", "--no-show-raw-insn", path)
            for sym, body in re.findall(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.M | re.S):
                if sym not in res:
                    continue
                text = re.sub(r"\s*// [0-9A-Fa-f]+:.*$", "", body, flags=re.M)    # the address comment of each line
                text = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<L>", text)               # branch targets as symbol + offset
                rows.append([sym, *res.pop(sym), hashlib.sha256(text.encode()).hexdigest()[:16]])
                if asm_dir:
                    os.makedirs(asm_dir, exist_ok=True)
                    open(os.path.join(asm_dir, hashlib.sha256(sym.encode()).hexdigest()[:16] + ".s"), "w").write(text)
            assert not res, f"kernels without disassembly: {sorted(res)}"
    for r in sorted(rows):
        print("\t".join(r))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[sys.argv.index("--asm") + 1] if "--asm" in sys.argv else None)
