"""Times of EDEN's coordinate drop: randperm_prefix, the drop-in with pdrop = 0.5, and one batch.

All in one process, medians of --reps timed repetitions after --warmup untimed ones, each repetition
synchronised (the figure is what a caller waits for).  Per shape, beside the GPU figure:
  host_ms      torch.randperm(D) on this machine's host plus the upload of its prefix: what the kernels replace
  pdrop0_ms    the same EDEN call at pdrop = 0, which runs exactly what ran before the drop existed: the
               difference is the cost of the drop
randperm_prefix is timed twice: `call_ms`, the public call on a CPU generator (the state's upload and the
generator's jump-ahead on the host included), and `device_ms`, the kernels alone on states already on the
device (HIP events around uq_randperm_prefix).

    python tools/eden_drop_times.py [--out profiles/eden_drop_times.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(f, reps, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


def event_ms(f, reps, warmup):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="2048,1048576,4194304")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batch-dim", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import uqdme
    from uqdme_amd import _mtstate, randperm
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"tool": "eden_drop_times", "gpu": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "host_threads": torch.get_num_threads(), "randperm_prefix": {}, "dropin": {}, "batch": {}}
    g = torch.Generator()
    g.manual_seed(1)
    for D in (int(v) for v in a.dims.split(",")):
        for k in (D // 2, D - 1):
            words = np.stack([_mtstate.generator_words(g)[1]])
            sd = torch.from_numpy(words.view(np.int32)).to(dev)
            row = {
                "call_ms": median_ms(lambda: randperm.randperm_prefix(D, k, generator=g), a.reps, a.warmup),
                "device_ms": event_ms(lambda: randperm.prefix_from_states(sd, 1, D, k, dev), a.reps, a.warmup),
                "bits_only_device_ms": event_ms(lambda: randperm.prefix_from_states(sd, 1, D, k, dev, index=False, bits=True),
                                                a.reps, a.warmup),
                "host_ms": median_ms(lambda: torch.randperm(D, generator=g)[:k].to(dev), a.reps, a.warmup),
                "plan": randperm.last_plan(),
            }
            res["randperm_prefix"][f"D={D}/k={k}"] = row
            print(D, k, row, flush=True)
        x = torch.randn(D, device=dev)
        row = {"pdrop0.5_ms": median_ms(lambda: uqdme.EDEN_quantize_Hadamard(x, 1, 0.5), a.reps, a.warmup),
               "pdrop0_ms": median_ms(lambda: uqdme.EDEN_quantize_Hadamard(x, 1), a.reps, a.warmup),
               "host_ms": res["randperm_prefix"][f"D={D}/k={D // 2}"]["host_ms"]}
        res["dropin"][f"d={D}"] = row
        print(D, row, flush=True)
        del x
    if a.batch:
        n, d = a.batch, a.batch_dim
        x = torch.randn((n, d), device=dev)
        seeds = np.arange(n) % 100
        row = {"pdrop0.5_ms": median_ms(lambda: uqdme.eden_quantize(x, 1, seeds=seeds, pdrop=0.5, generator=g), a.reps, a.warmup),
               "pdrop0_ms": median_ms(lambda: uqdme.eden_quantize(x, 1, seeds=seeds), a.reps, a.warmup),
               "host_jumps_ms": median_ms(lambda: randperm.client_states(n, d, generator=g), a.reps, a.warmup),
               "host_ms_per_client": res["randperm_prefix"].get(f"D={d}/k={d // 2}", {}).get("host_ms")}
        t = torch.Generator()
        t.set_state(g.get_state())
        sd = torch.from_numpy(randperm.client_states(n, d, generator=g).view(np.int32)).to(dev)
        row["drop_rows_device_ms"] = event_ms(
            lambda: randperm.prefix_from_states(sd, n, d, d // 2, dev, index=False, bits=True), a.reps, a.warmup)
        row["plan"] = randperm.last_plan()
        # what was timed is checked: the index rows of the first and the last client against torch.randperm
        idx = randperm.prefix_from_states(sd, n, d, d // 2, dev)[0]
        for j in range(n):
            ref = torch.randperm(d, generator=t)
            if j in (0, n - 1) and not torch.equal(idx[j].cpu(), ref[:d // 2]):
                raise SystemExit(f"batch {n} x {d}: client {j}'s permutation differs from torch.randperm")
        if not torch.equal(t.get_state(), g.get_state()):
            raise SystemExit(f"batch {n} x {d}: the generator is not where {n} torch.randperm calls leave it")
        row["checked_clients"] = [0, n - 1]
        res["batch"][f"{n}x{d}"] = row
        print(n, d, row, flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
