"""Times of Kashin_quantize.

GPU (default): the drop-in per call at each --dims (one client per call, host overhead and the
copy of the NumPy result included; every call waits for the GPU), with warm run tables (those of
all 100 seeds a call can draw built before, kashin.warm_run_tables) and with cold ones
(kashin.clear_run_tables() before each call: the host's jump-aheads and the upload are in),
EDEN_quantize_Hadamard beside it; the same at --sweep-dims for run lengths of 8, 32 and 128
generator blocks; one batch of --batch clients x --batch-dim through kashin_quantize (the call
and a synchronise, tables warm).
--ref: the reference's own function on this container's CPU, one thread (the reference is
importable here, never on the GPU machine).

    python tools/kashin_times.py [--out profiles/kashin_times.json]
    PYTHONDONTWRITEBYTECODE=1 python tools/kashin_times.py --ref [--out profiles/kashin_ref_cpu.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.rand_schemes_times import cpu_name  # noqa: E402

REF = "/root/reference/NMSE_Results/Codes"
RUN_BLOCKS = (8, 32, 128)


def ref_times(dims):
    sys.path.insert(0, REF)
    import All_Schemes as AS  # noqa: E402  (the reference, this container only)
    torch.set_num_threads(1)
    res = {"tool": "kashin_times --ref", "host": cpu_name(), "threads": 1, "ms_per_call": {}}
    rng = np.random.default_rng(0)
    for d in dims:
        x = rng.standard_normal(d).astype(np.float32)
        for bits in (1, 2):
            AS.Kashin_quantize(x, bits)
            k = 20 if d <= 4096 else 3
            ts = []
            for _ in range(k):
                t0 = time.perf_counter()
                AS.Kashin_quantize(x, bits)
                ts.append((time.perf_counter() - t0) * 1e3)
            res["ms_per_call"][f"Kashin_quantize/bits={bits}/d={d}"] = {"median": round(float(np.median(ts)), 4),
                                                                       "min": round(min(ts), 4)}
    return res


def med(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def dropin_ms(f, vs, k, before=None):
    ts = []
    for i in range(k):
        if before is not None:
            before()
        t0 = time.perf_counter()
        f(vs[i % len(vs)], 1)
        ts.append((time.perf_counter() - t0) * 1e3)
    return med(ts)


def gpu_times(dims, sweep_dims, n, bd):
    import uqdme
    from uqdme_amd import kashin
    res = {"tool": "kashin_times", "gpu": torch.cuda.get_device_name(0), "default_run_words": kashin.DEFAULT_RUN_WORDS,
           "dropin_ms": {}, "sweep_ms": {}, "batch_ms": {}}
    for d in dims:
        vs = [torch.randn(d, device="cuda") for _ in range(8)]
        kashin.warm_run_tables(d)               # warm: whichever of the 100 seeds a call draws
        for _ in range(3):
            uqdme.Kashin_quantize(vs[0], 1)
            uqdme.EDEN_quantize_Hadamard(vs[0], 1)
        res["dropin_ms"][f"Kashin_quantize/warm/d={d}"] = dropin_ms(uqdme.Kashin_quantize, vs, 32)
        res["dropin_ms"][f"Kashin_quantize/cold/d={d}"] = dropin_ms(uqdme.Kashin_quantize, vs, 6, kashin.clear_run_tables)
        res["dropin_ms"][f"EDEN_quantize_Hadamard/d={d}"] = dropin_ms(uqdme.EDEN_quantize_Hadamard, vs, 32)
    default = kashin.DEFAULT_RUN_WORDS
    for d in sweep_dims:
        vs = [torch.randn(d, device="cuda") for _ in range(8)]
        for blocks in RUN_BLOCKS:
            kashin.DEFAULT_RUN_WORDS = blocks * kashin.MT_BLOCK
            kashin.clear_run_tables()
            kashin.warm_run_tables(d)
            for _ in range(3):
                uqdme.Kashin_quantize(vs[0], 1)
            res["sweep_ms"][f"warm/blocks={blocks}/d={d}"] = dropin_ms(uqdme.Kashin_quantize, vs, 32)
            res["sweep_ms"][f"cold/blocks={blocks}/d={d}"] = dropin_ms(uqdme.Kashin_quantize, vs, 6, kashin.clear_run_tables)
    kashin.DEFAULT_RUN_WORDS = default
    kashin.clear_run_tables()
    if n:                                       # (workspace: four [n][D] f32 buffers, D = 2 bd for a power of two)
        x = torch.randn((n, bd), device="cuda")
        seeds = np.arange(n) % 100
        ts = []
        for it in range(5):                     # the first two warm up (and build the 100 seeds' tables)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = uqdme.kashin_quantize(x, 1, seeds=seeds, return_info=True)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            del y
        res["batch_ms"][f"kashin_quantize/{n}x{bd}"] = {"first": round(ts[0], 3), "min": round(min(ts[2:]), 3),
                                                        "max": round(max(ts[2:]), 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="2048,1048576,4194304")
    ap.add_argument("--sweep-dims", default="1048576,4194304")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batch-dim", type=int, default=1 << 20)
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = [int(v) for v in a.dims.split(",") if v]
    res = ref_times(dims) if a.ref else gpu_times(dims, [int(v) for v in a.sweep_dims.split(",") if v], a.batch,
                                                  a.batch_dim)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
