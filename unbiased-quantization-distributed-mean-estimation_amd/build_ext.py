"""Build the HIP C-ABI library in-tree (gfx950 only).

    python unbiased-quantization-distributed-mean-estimation_amd/build_ext.py

Output: unbiased-quantization-distributed-mean-estimation_amd/_build/libuq_dme.so
(git-ignored; it travels to the GPU box with the gpurun snapshot).
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import Sequence

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# csrc/*.hip: one device translation unit per scheme (hipcc).  csrc/*.cpp: host-only C++ (g++)
# linked into the same library: the MT19937 jump polynomials, and numpy's legacy RandomState
# samplers for the NMSE harness (uq_legacy_rng.cpp: -ffp-contract=off, every product and sum
# rounded on its own as in numpy's baseline build; log/exp from the host libm)
CSRC = os.path.join(PKG_DIR, "csrc")
OUT_DIR = os.path.join(PKG_DIR, "_build")
SO = os.path.join(OUT_DIR, "libuq_dme.so")

# -ffp-contract=off: the reference evaluates m*p, floor, subtract, (L1*sign)*(k)/m as
#   separate f32 ops; a fused multiply-add would change bits.
# -fhip-fp32-correctly-rounded-divide-sqrt: x/den and t/m must be IEEE divisions.
# -fno-gpu-flush-denormals-to-zero: torch CPU keeps f32 denormals.
HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
    "-fno-gpu-flush-denormals-to-zero", "-Wall",
]


HOST_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-ffp-contract=off", "-fno-fast-math"]


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


HEADER = os.path.join(PKG_DIR, "..", "include", "uq_dme.h")
ID_FILE = SO + ".build_id"


def build_id() -> str:
    """SHA-256 over the library's sources (csrc/*, include/uq_dme.h) and the compile flags:
    the identity of the binary they produce.  The library reports the id it was built from
    (uq_build_id), so a stale binary is detected by content, not by file times."""
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)) + [None]:
        path = HEADER if f is None else os.path.join(CSRC, f)
        h.update((os.path.basename(path) + "\0").encode())
        with open(path, "rb") as fh:
            h.update(fh.read())
    h.update("\0".join(HIPCC_FLAGS + HOST_FLAGS).encode())
    return h.hexdigest()


def needs_build() -> bool:
    if not os.path.exists(SO) or not os.path.exists(ID_FILE):
        return True
    with open(ID_FILE) as f:
        return f.read().strip() != build_id()


def _jobs(n: int) -> int:
    """Parallel compiles: one per translation unit, 16 at most, MAX_JOBS if set (never the CPU count)."""
    try:
        cap = int(os.environ.get("MAX_JOBS", ""))
    except ValueError:
        cap = 16
    return max(1, min(16, cap, n))


def build(force: bool = False, verbose: bool = False, src_dir: str = CSRC, out: str = SO,
          extra_flags: Sequence[str] = ()) -> str:
    """Compile every src_dir/*.hip (device translation units, hipcc) and src_dir/*.cpp (host,
    g++) to objects, in parallel, and link them into `out`.  The defaults build the package's
    library, and only those are skipped when the library on disk is current; another src_dir
    (csrc/ of another revision, a patched copy), `out` or extra_flags (-D...) is what the
    measurement tools use."""
    default = src_dir == CSRC and out == SO and not extra_flags
    if default and not force and not needs_build():
        return SO
    obj_dir = out + ".obj"
    os.makedirs(obj_dir, exist_ok=True)
    bid = build_id()
    cmds, objs = [], []
    for f in sorted(os.listdir(src_dir)):
        path = os.path.join(src_dir, f)
        obj = os.path.join(obj_dir, f + ".o")
        if f.endswith(".hip"):
            with open(path, "rb") as fh:
                owns_id = b"UQ_BUILD_ID" in fh.read()      # the unit that defines uq_build_id
            ident = [f'-DUQ_BUILD_ID="{bid}"'] if owns_id and default else []
            cmds.append([hipcc(), *[x for x in HIPCC_FLAGS if x != "-shared"], *extra_flags, *ident, "-c", "-o", obj, path])
        elif f.endswith(".cpp"):
            cmds.append([os.environ.get("CXX", "g++"), *HOST_FLAGS, "-c", "-o", obj, path])
        else:
            continue
        objs.append(obj)
    if not any(o.endswith(".hip.o") for o in objs):
        raise RuntimeError(f"no .hip source in {src_dir}")

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(_jobs(len(cmds))) as pool:
        list(pool.map(run, cmds))
    tmp = out + ".tmp"
    run([hipcc(), *HIPCC_FLAGS, "-o", tmp, *objs, "-lpthread"])
    os.replace(tmp, out)
    if default:
        with open(ID_FILE, "w") as f:
            f.write(bid + "\n")
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
