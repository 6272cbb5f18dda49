"""Times of Scalar_quantize and DRIVE_quantize_Hadamard.

GPU (default): the drop-ins per call at each --dims (one client per call, host overhead
included; "ms_per_call": 48 calls back to back, "ms_synced": each call waited for, as
tools/dropin_latency.py), and one batch of --batch clients x --batch-dim per scheme through
scalar_quantize / drive_quantize with px_seeds (the call and a synchronise; Scalar's includes
its read-back of the end states).
--ref: the reference's own functions on this container's CPU, one thread (the reference is
importable here, never on the GPU machine).

    python tools/rand_schemes_times.py [--out profiles/NAME.json]
    PYTHONDONTWRITEBYTECODE=1 python tools/rand_schemes_times.py --ref [--out profiles/NAME.json]"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference/NMSE_Results/Codes"


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def ref_times(dims):
    sys.path.insert(0, REF)
    import All_Schemes as AS  # noqa: E402  (the reference, this container only)
    torch.set_num_threads(1)
    res = {"tool": "rand_schemes_times --ref", "host": cpu_name(), "threads": 1, "ms_per_call": {}}
    rng = np.random.default_rng(0)
    for d in dims:
        x = torch.from_numpy(rng.standard_normal(d).astype(np.float32))
        for name, f, bits in (("Scalar_quantize", AS.Scalar_quantize, 2),
                              ("DRIVE_quantize_Hadamard", AS.DRIVE_quantize_Hadamard, 1)):
            f(x, bits)
            k = 20 if d <= 4096 else 3
            t0 = time.perf_counter()
            for _ in range(k):
                f(x, bits)
            res["ms_per_call"][f"{name}/d={d}"] = round((time.perf_counter() - t0) / k * 1e3, 4)
    return res


def gpu_times(dims, n, bd):
    import uqdme
    res = {"tool": "rand_schemes_times", "gpu": torch.cuda.get_device_name(0), "ms_per_call": {}, "ms_synced": {},
           "batch_ms": {}}
    for d in dims:
        vs = [torch.randn(d, device="cuda") for _ in range(16)]
        for name, f, bits in (("Scalar_quantize", uqdme.Scalar_quantize, 2),
                              ("DRIVE_quantize_Hadamard", uqdme.DRIVE_quantize_Hadamard, 1)):
            for _ in range(3):
                y = f(vs[0], bits)
            torch.cuda.synchronize()
            k = 48
            t0 = time.perf_counter()
            for i in range(k):
                y = f(vs[i % 16], bits)
            torch.cuda.synchronize()
            res["ms_per_call"][f"{name}/d={d}"] = round((time.perf_counter() - t0) / k * 1e3, 4)
            t0 = time.perf_counter()
            for i in range(k):
                y = f(vs[i % 16], bits)
                torch.cuda.synchronize()
            res["ms_synced"][f"{name}/d={d}"] = round((time.perf_counter() - t0) / k * 1e3, 4)
            del y
    if n:
        x = torch.randn((n, bd), device="cuda")
        seeds = np.arange(n)
        for name, f in (("scalar_quantize", lambda: uqdme.scalar_quantize(x, 2, px_seeds=seeds)),
                        ("drive_quantize", lambda: uqdme.drive_quantize(x, px_seeds=seeds))):
            ts = []
            for it in range(5):                     # the first two warm up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                y = f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                del y
            res["batch_ms"][f"{name}/{n}x{bd}"] = {"min": round(min(ts[2:]), 3), "max": round(max(ts[2:]), 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="2048,1048576,4194304")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batch-dim", type=int, default=1 << 20)
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = [int(v) for v in a.dims.split(",")]
    res = ref_times(dims) if a.ref else gpu_times(dims, a.batch, a.batch_dim)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
