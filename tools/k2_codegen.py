"""What the K2 kernels compile to: registers, spills, scratch, LDS, the vector-memory waits inside
the stream kernels' tile loop and its vector-ALU instruction counts.  CPU only (cross-compiles for gfx950).

    python tools/k2_codegen.py [--csrc DIR] [--git REV] [--keep-asm FILE]

Compiles csrc/uq_unbiased.hip device-only to assembly with build_ext.HIPCC_FLAGS (--git REV:
csrc/ as of that revision, in a temporary directory).  For every quantize_stream_kernel and
quantize_small_kernel instantiation it prints the code object's metadata (.vgpr_count,
.vgpr_spill_count, .sgpr_spill_count, .private_segment_fixed_size, .group_segment_fixed_size),
and for the tile loop of each (the largest depth-1 loop of the kernel, nested loops included)
every s_waitcnt that names vmcnt: its line in the kernel's assembly, its value and the
instruction that follows it.  Spills are read from the metadata only; the one mnemonic the tool
looks for is s_waitcnt.  It also counts the vector-ALU instructions (v_*) of each tile loop: all of
them, and those of the hot blocks a full regular tile runs per element (tile_loop_valu), which for
quantize_stream_kernel<1,1,1,1>, the bench step's instantiation, are listed block by block.

report() returns the same as a dict (tests/test_k2_codegen.py).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unbiased-quantization-distributed-mean-estimation_amd")
KEYS = (".vgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size")
KERNELS = ("quantize_stream_kernel", "quantize_small_kernel")
HOT_DETAIL = "quantize_stream_kernel<1,1,1,1>"      # the bench step's instantiation: hot path block by block


def _build_ext():
    from importlib import util
    spec = util.spec_from_file_location("_uq_build_ext", os.path.join(PKG, "build_ext.py"))
    be = util.module_from_spec(spec)
    spec.loader.exec_module(be)
    return be


def have_hipcc():
    try:
        return bool(_build_ext().hipcc()) and subprocess.run(
            [_build_ext().hipcc(), "--version"], capture_output=True).returncode == 0
    except (RuntimeError, OSError):
        return False


def compile_asm(csrc):
    be = _build_ext()
    flags = [f for f in be.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "uq_unbiased.s")
        subprocess.run([be.hipcc(), *flags, "--cuda-device-only", "-S", "-o", out,
                        os.path.join(csrc, "uq_unbiased.hip")], check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def checkout_csrc(rev, dst):
    rel = os.path.relpath(os.path.join(PKG, "csrc"), ROOT)
    names = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", rev, rel + "/"], check=True,
                           capture_output=True, text=True).stdout.split()
    for path in names:
        blob = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{path}"], check=True, capture_output=True).stdout
        with open(os.path.join(dst, os.path.basename(path)), "wb") as f:
            f.write(blob)


def instantiation(symbol):
    """'quantize_stream_kernel<1,1,1,1>' from the mangled name, None for any other kernel."""
    for k in KERNELS:
        m = re.search(r"\d+%sI((?:Lb[01]E)+)E" % k, symbol)
        if m:
            return "%s<%s>" % (k, ",".join(re.findall(r"Lb([01])E", m.group(1))))
    return None


def metadata(asm):
    """{symbol: {key: int}} from the amdhsa.kernels list of the code-object metadata."""
    out, cur = {}, None
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:"))
    for l in lines[start + 1:]:
        if l.startswith("  - ."):
            cur = {}
            l = "    " + l[4:]
        elif not l.startswith("  "):
            break
        m = re.match(r"    (\.\w+):\s+(\S+)\s*$", l)
        if m and cur is not None:
            if m.group(1) == ".name":
                out[m.group(2)] = cur
            elif m.group(1) in KEYS:
                cur[m.group(1)] = int(m.group(2))
    return out


def kernel_body(asm, symbol):
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].lstrip().startswith("s_endpgm"))
    while not lines[end].startswith(".Lfunc_end"):
        end += 1
    return lines[start:end]


_HDR = re.compile(r"^\.LBB(\d+_\d+):.*=>This Loop Header: Depth=1")
_IN = re.compile(r"(?:in Loop: Header=|Parent Loop )BB(\d+_\d+) Depth=1")


def _loop_owner(body):
    """For every line of the kernel the depth-1 loop it belongs to (from the assembler's loop
    comments, nested loops included), or None."""
    owner, cur, pend = [], None, False
    for l in body:
        s = l.strip()
        block_start = l.startswith(".LBB") or s.startswith("; %bb.")
        if block_start:
            cur, pend = None, True
            h = _HDR.match(l)
            if h:
                cur = h.group(1)
        if pend and (block_start or s.startswith(";")):
            m = _IN.search(l)
            if m:
                cur = m.group(1)
        elif s and not s.startswith(";"):
            pend = False
        owner.append(cur)
    return owner


def _tile_loop(owner):
    sizes = {}
    for o in owner:
        if o:
            sizes[o] = sizes.get(o, 0) + 1
    return max(sizes, key=sizes.get) if sizes else None


def tile_loop_waits(body):
    """Blocks of the kernel by depth-1 loop; the largest such loop is the tile loop.  Returns
    (header label, [(line, vmcnt, next instruction)])."""
    owner = _loop_owner(body)
    loop = _tile_loop(owner)
    if loop is None:
        return None, []
    waits = []
    for i, l in enumerate(body):
        s = l.strip()
        if owner[i] == loop and s.startswith("s_waitcnt") and "vmcnt" in s:
            nxt = next((b.strip() for b in body[i + 1:] if b.strip() and not b.strip().startswith(";")), "")
            waits.append((i + 1, int(re.search(r"vmcnt\((\d+)\)", s).group(1)), nxt.split(";")[0].strip()))
    return loop, waits


def tile_loop_valu(body):
    """Vector-ALU instructions (mnemonic v_*) of the tile loop, counted statically.

    in_loop: every v_* instruction in the loop's blocks, rare paths and nested loops included.
    hot: the v_* instructions of the straight-line blocks that every thread runs once per full,
    regular tile (kQItems = 16 elements), found by what only they hold:
      div4    the blocks with packed fmas (the Markstein quotients, four elements each).  Each of
              the loop's two tile_pass1 instantiations (FULL and padded) has its own identical
              copies; kQItems / 4 of them run per tile, and the cheapest that many are counted;
      pass 1  the block with kQItems v_floor_f32 and kQItems v_cvt_f64_f32 and no v_cvt_f32_f64,
              and the blocks after it through the first with an s_barrier (the wave scan, what
              the compiler sinks below it, the tile sums); of the two instantiations the cheaper
              one is the full tile's;
      pass 2  the blocks with v_cvt_f32_f64 and v_floor_f32 (the f32 crossing of the fp64 prefix),
              and the block the last of them falls into (the packing and the early codes store).
    The tie resolution and the staging are not in it.  Returns (in_loop, hot, [(block, part,
    v_* count)])."""
    owner = _loop_owner(body)
    loop = _tile_loop(owner)
    if loop is None:
        return 0, 0, []
    blocks, cur = [], None
    for i, l in enumerate(body):
        s = l.strip()
        if l.startswith(".LBB") or s.startswith("; %bb."):
            cur = None
            if owner[i] == loop:
                cur = {"name": l[1:l.index(":")].replace("; %", "") if l.startswith(".LBB") else s[3:s.index(":")],
                       "v": 0, "floor": 0, "to32": 0, "to64": 0, "pk": 0, "barrier": 0}
                blocks.append(cur)
            continue
        if cur is None or not s or s.startswith(";") or s.startswith("."):
            continue
        mn = s.split()[0]
        cur["v"] += mn.startswith("v_")
        cur["floor"] += mn.startswith("v_floor_f32")
        cur["to32"] += mn.startswith("v_cvt_f32_f64")
        cur["to64"] += mn.startswith("v_cvt_f64_f32")
        cur["pk"] += mn.startswith("v_pk_fma_f32")
        cur["barrier"] += mn == "s_barrier"
    in_loop = sum(b["v"] for b in blocks)
    path = [(b["name"], "div4", b["v"]) for b in sorted((b for b in blocks if b["pk"]), key=lambda b: b["v"])[:4]]
    inst = []
    for j, b in enumerate(blocks):
        if b["floor"] >= 16 and b["to64"] >= 16 and not b["to32"] and not b["pk"]:
            k = next((k for k in range(j, len(blocks)) if blocks[k]["barrier"]), j)
            inst.append(blocks[j:k + 1])
    if inst:
        run = min(inst, key=lambda r: sum(b["v"] for b in r))
        path += [(b["name"], "pass 1", b["v"]) for b in run if b["v"]]
    p2 = [j for j, b in enumerate(blocks) if b["to32"] and b["floor"]]
    path += [(blocks[j]["name"], "pass 2", blocks[j]["v"]) for j in p2]
    if p2 and p2[-1] + 1 < len(blocks):
        path.append((blocks[p2[-1] + 1]["name"], "pass 2 tail", blocks[p2[-1] + 1]["v"]))
    return in_loop, sum(n for _, _, n in path), path


def report(csrc=None, rev=None, keep_asm=None):
    if rev:
        with tempfile.TemporaryDirectory() as tmp:         # the sources include ../../include/uq_dme.h
            src = os.path.join(tmp, "pkg", "csrc")
            os.makedirs(src)
            os.symlink(os.path.join(ROOT, "include"), os.path.join(tmp, "include"))
            checkout_csrc(rev, src)
            asm = compile_asm(src)
    else:
        asm = compile_asm(csrc or os.path.join(PKG, "csrc"))
    if keep_asm:
        with open(keep_asm, "w") as f:
            f.write(asm)
    out = {}
    for sym, md in metadata(asm).items():
        name = instantiation(sym)
        if name is None:
            continue
        stream = name.startswith(KERNELS[0])
        body = kernel_body(asm, sym) if stream else []
        loop, waits = tile_loop_waits(body) if stream else (None, [])
        in_loop, hot, path = tile_loop_valu(body) if stream else (0, 0, [])
        out[name] = {"meta": md, "loop": loop, "waits": waits, "valu_loop": in_loop, "valu_hot": hot,
                     "hot_path": path}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc")
    ap.add_argument("--git")
    ap.add_argument("--keep-asm")
    a = ap.parse_args()
    rep = report(a.csrc, a.git, a.keep_asm)
    print("# csrc of %s" % (a.git or a.csrc or "the tree"))
    for name in sorted(rep):
        r = rep[name]
        print(name)
        for k in KEYS:
            print(f"    {k:<30}{r['meta'][k]}")
        if r["loop"] is None:
            continue
        print(f"    tile loop {r['loop']}: {len(r['waits'])} s_waitcnt naming vmcnt")
        for line, val, nxt in r["waits"]:
            print(f"        line {line:<6} vmcnt({val})  then  {nxt}")
        print(f"    v_* instructions in the tile loop: {r['valu_loop']}")
        print(f"    v_* instructions in the hot blocks (div4, pass 1, pass 2 of a full tile): {r['valu_hot']} per "
              f"thread and tile, {r['valu_hot'] / 16:.2f} per element")
        if name == HOT_DETAIL:
            for blk, part, n in r["hot_path"]:
                print(f"        {blk:<12}{part:<12}{n}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
