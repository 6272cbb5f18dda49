"""Times of EDEN at a fractional rate beside the 2-bit call, in one process on one GPU.

Warm 2-bit and 1.5-bit calls alternate (the 2-bit call runs code this rate does not touch, so it is
the baseline): EDEN_quantize_Hadamard per call at each --dims (host overhead and the copy of the
NumPy result included), the --batch x --batch-dim round trip (eden_compress + eden_decompress and a
synchronise), and the first fractional call for a new (D, threshold), which builds its mask rows.

    python tools/eden_frac_times.py [--out profiles/eden_frac_times.json]

Per-kernel times of the round trip come from one profiler run per rate, each a run of its own
(--round-trip BITS runs nothing but that rate's round trips), and --summarize joins the two
kernel_stats tables:

    rocprofv3 --kernel-trace --stats -d DIR/b2 -o s --output-format csv -- python tools/eden_frac_times.py --round-trip 2
    rocprofv3 --kernel-trace --stats -d DIR/b15 -o s --output-format csv -- python tools/eden_frac_times.py --round-trip 1.5
    python tools/eden_frac_times.py --summarize DIR/b2 DIR/b15 --out profiles/eden_frac_kernel_stats.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]        # noqa: E731
    return {"median": round(float(np.median(ts)), 4), "p10": round(q(0.1), 4), "p90": round(q(0.9), 4),
            "min": round(ts[0], 4), "max": round(ts[-1], 4), "n": len(ts)}


def round_trips(bits, n, d, iters):
    """nothing but `iters` warm round trips of one rate (for a kernel trace)"""
    import uqdme  # noqa: F401  (makes the package importable as uqdme_amd)
    from uqdme_amd import eden as ED
    x = torch.randn((n, d), device="cuda")
    seeds = np.arange(n) % 100
    for _ in range(iters):
        out = ED.eden_decompress(ED.eden_compress(x, bits, seeds=seeds))
        torch.cuda.synchronize()
        del out


def kernel_stats(d):
    """{kernel name: (calls, average ns)} of the *kernel_stats.csv under d"""
    import csv
    import glob
    paths = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert len(paths) == 1, (d, paths)
    with open(paths[0]) as fh:
        return {r["Name"]: (int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(fh)}


def summarize(dirs, iters):
    """Per round trip (kernels that ran once or more per round trip: the tables' builders ran once
    per process and are listed apart), microseconds: each kernel's time at 2 bits and at the
    fractional rate; a fractional instance stands beside the kernel whose place it takes."""
    import re
    a, b = (kernel_stats(d) for d in dirs)

    def short(name):
        return re.sub(r"\(.*", "", name.replace("void ", "").replace("(anonymous namespace)::", ""))

    def base(name):
        return short(name).replace("_frac_kernel", "_kernel")
    rows, once = {}, {}
    for side, tab in (("bits=2", a), ("bits=1.5", b)):
        for name, (calls, avg) in tab.items():
            if calls < iters:
                once.setdefault(side, {})[short(name)] = {"calls": calls, "avg_us": round(avg / 1e3, 1)}
                continue
            if name.startswith("void at::") or "rocclr" in name:      # torch's own kernels, runtime copies
                continue
            key = base(name)                           # a fractional instance beside the 2-bit kernel whose place it takes
            key = {"eden_dotbins_kernel": "eden_dotbins_kernel<3>", "fwht_low4096_kernel<false, false>": "fwht_low4096_kernel<2, false, false>",
                   "fwht_low16k_kernel": "fwht_low16k_kernel<2>"}.get(key, key)
            rows.setdefault(key, {})[side] = {"kernel": short(name), "us_per_round_trip": round(avg * calls / iters / 1e3, 1)}
    tot = {s_: round(sum(r[s_]["us_per_round_trip"] for r in rows.values() if s_ in r), 1) for s_ in ("bits=2", "bits=1.5")}
    return {"tool": "eden_frac_times --summarize", "iters": iters, "per_round_trip": rows, "sum_us": tot, "once_per_process": once}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="2048,1048576,4194304")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batch-dim", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--round-trips", type=int, default=40, help="timed round trips per rate (alternating)")
    ap.add_argument("--round-trip", type=float, default=None, help="only warm round trips of this rate (for a trace)")
    ap.add_argument("--iters", type=int, default=12, help="round trips of --round-trip; calls per kernel for --summarize")
    ap.add_argument("--summarize", nargs=2, default=None, metavar=("DIR_2BIT", "DIR_FRAC"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarize:
        txt = json.dumps(summarize(a.summarize, a.iters), indent=1)
        print(txt)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(txt + "\n")
        return
    if a.round_trip is not None:
        bits = int(a.round_trip) if a.round_trip == int(a.round_trip) else a.round_trip
        round_trips(bits, a.batch, a.batch_dim, a.iters)
        return
    import uqdme
    from uqdme_amd import eden as ED
    res = {"tool": "eden_frac_times", "gpu": torch.cuda.get_device_name(0), "dropin_ms": {}, "first_call_ms": {},
           "round_trip_ms": {}}
    for d in [int(v) for v in a.dims.split(",") if v]:
        vs = [torch.randn(d, device="cuda") for _ in range(8)]
        for bits in (2, 1.5):                     # warm: the tables of all 100 seeds a call can draw
            for _ in range(3):
                uqdme.EDEN_quantize_Hadamard(vs[0], bits)
        ts = {2: [], 1.5: []}
        for i in range(a.calls):
            for bits in (2, 1.5):
                t0 = time.perf_counter()
                uqdme.EDEN_quantize_Hadamard(vs[i % 8], bits)
                ts[bits].append((time.perf_counter() - t0) * 1e3)
        res["dropin_ms"][f"bits=2/d={d}"] = med(ts[2])
        res["dropin_ms"][f"bits=1.5/d={d}"] = med(ts[1.5])
        first = []
        for k in range(3):                        # a rate never seen: the 100 seeds' mask rows are built
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            uqdme.EDEN_quantize_Hadamard(vs[0], 1.61 + 0.01 * k)
            first.append((time.perf_counter() - t0) * 1e3)
        res["first_call_ms"][f"new rate, 100 rows/d={d}"] = med(first)
        first = []
        for k in range(3):                        # a seed outside 0..99: one row
            x = vs[0].view(1, -1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ED.eden_quantize(x, 1.5, seeds=[1000 + k])
            torch.cuda.synchronize()
            first.append((time.perf_counter() - t0) * 1e3)
        res["first_call_ms"][f"new seed, 1 row (and its sign row)/d={d}"] = med(first)
    if a.batch:
        x = torch.randn((a.batch, a.batch_dim), device="cuda")
        seeds = np.arange(a.batch) % 100
        ts = {2: [], 1.5: []}
        for it in range(a.round_trips + 2):       # the first two rounds warm up
            for bits in (2, 1.5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = ED.eden_decompress(ED.eden_compress(x, bits, seeds=seeds))
                torch.cuda.synchronize()
                if it >= 2:
                    ts[bits].append((time.perf_counter() - t0) * 1e3)
                del out
        for bits in (2, 1.5):
            res["round_trip_ms"][f"bits={bits}/{a.batch}x{a.batch_dim}"] = med(ts[bits])
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
