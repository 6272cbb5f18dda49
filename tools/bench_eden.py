"""Time EDEN + RHT (uq_eden_f32) on a resident synthetic batch.

    python tools/bench_eden.py --clients 1024 --dim 1048576 --bits 1

    python tools/bench_eden.py --parent-lib OLD.so [--reps 20] [--json OUT.json]

--parent-lib: another build of the library (build_ext.build(src_dir=..., out=...) of an earlier
revision).  Its sender (uq_eden_compress_f32 / uq_eden_compress_frac_f32; the norm alone through
uq_eden_norm_f32 mode 2) takes turns with this tree's, call for call in one process, each on a
workspace and outputs of its own, device events around each call, the order swapped every
repetition, over the shapes that take the segmented chains (AB_SHAPES).  Compress only: the
receiver's transform would dilute a difference in the sender.  Per shape: median and 10th / 90th
percentile of both, whether both wrote the same bits, and `within_noise`: this tree's median is at
most the parent's plus the parent's own 10th-90th percentile spread in that run.

    python tools/bench_eden.py --packed [--parent-lib OLD.so] [--reps 30] [--json OUT.json]

--packed: compress -> decompress through a u8 message and through a bit-packed one (uq_eden_*_packed_f32), the same
way: in turns in one process, workspaces and outputs of their own, device events, the order swapped every repetition
(at least 30), over PACKED_SHAPES; the packed calls under test hook bit 0 (the converter fallback) join as a third,
and with --parent-lib the parent build's u8 round trip as a fourth.  Writes
profiles/eden_packed_times.json."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (clients, dim, bits; bits None: the norm alone).  DESIGN.md §4.3's dispatch table: the per-call
# drop-ins, config C4, the largest segmented dot, the largest segmented norm batch, two fractional rates
AB_SHAPES = [(n, d, b) for n, d in ((1, 1 << 20), (1, 1 << 22), (101, 1 << 22), (128, 1 << 20)) for b in (1, 2)]
AB_SHAPES += [(256, 1 << 14, None), (1, 1 << 20, 1.5), (101, 1 << 22, 1.5)]


def sender_call(lib, x, bits, tab, rows, sb, mb):
    """(run, outputs): the sender of the ctypes library `lib` on x [n, d], on a workspace of its own."""
    from uqdme_amd import _runtime
    p, sp = _runtime.ptr, _runtime.stream_ptr(x.device)
    n, d = x.shape
    nb = ctypes.c_size_t()
    size_fn = lib.uq_eden_norm_workspace_bytes if bits is None else lib.uq_eden_workspace_bytes
    assert size_fn(n, d, ctypes.byref(nb)) == 0
    ws = torch.zeros(max(1, nb.value), dtype=torch.uint8, device=x.device)
    scale = torch.empty(n, dtype=torch.float32, device=x.device)        # (the norm alone: the norms)
    bins = torch.empty((n, d), dtype=torch.uint8, device=x.device)
    if bits is None:
        run = lambda: lib.uq_eden_norm_f32(p(x), n, d, 2, p(scale), p(ws), ws.numel(), sp)
    elif mb is not None:
        run = lambda: lib.uq_eden_compress_frac_f32(p(x), n, d, p(tab), p(rows), p(sb), p(mb), p(rows), p(bins), p(scale),
                                                    p(ws), ws.numel(), sp)
    else:
        run = lambda: lib.uq_eden_compress_f32(p(x), n, d, bits, p(tab), p(rows), p(bins), p(scale), p(ws), ws.numel(), sp)

    def checked():
        rc = run()
        assert rc == 0, rc
    return checked, (bins, scale)


def bench_ab(a):
    import uqdme  # noqa: F401  (loads the package as uqdme_amd)
    from uqdme_amd import _lib, eden
    libs = {"new": _lib.load(), "parent": ctypes.CDLL(a.parent_lib)}
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith("uq_eden_"):
            fn = getattr(libs["parent"], name)
            fn.restype, fn.argtypes = res, args
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(3)
    results = []
    for n, d, bits in AB_SHAPES:
        x = torch.randn(n, d, generator=g, device=dev)
        seeds = torch.arange(min(n, 100))
        rows = (torch.arange(n) % 100).to(torch.int32).to(dev)
        tab = sb = mb = None
        if bits is not None:
            tab = eden.rht_signs(seeds, d, dev)
            sb = eden.rht_sign_bits(tab)
            if bits not in (1, 2):
                mb = eden.eden_mask_bits(seeds, d, eden._threshold(bits - 1.0), dev)
        calls = {k: sender_call(lib, x, bits, tab, rows, sb, mb) for k, lib in libs.items()}
        for run, _ in calls.values():
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for rep in range(a.reps):
            for k in ("new", "parent")[::1 if rep % 2 == 0 else -1]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[k][0]()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        outs = [calls[k][1] for k in ("new", "parent")]
        same = bool(torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)) and
                    (bits is None or torch.equal(outs[0][0], outs[1][0])))
        ms = {k: {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4),
                  "p90": round(float(np.percentile(v, 90)), 4)} for k, v in times.items()}
        par = ms["parent"]
        row = {"clients": n, "d": d, "bits": bits, "call": "uq_eden_norm_f32 mode 2" if bits is None else "compress",
               "ms": ms, "same_bits": same,
               "within_noise": ms["new"]["median"] <= par["median"] + (par["p90"] - par["p10"])}
        print(json.dumps(row), flush=True)
        results.append(row)
        del x, tab, sb, mb, calls, outs
        torch.cuda.empty_cache()
    res = {"tool": "bench_eden --parent-lib", "reps": a.reps, "shapes": results,
           "all_same_bits": all(r["same_bits"] for r in results), "all_within_noise": all(r["within_noise"] for r in results)}
    print(json.dumps({k: v for k, v in res.items() if k != "shapes"}))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


# --packed: the batch shape the project measures at both integer rates, and a short-row batch (KE2+4 over 8 chunks)
PACKED_SHAPES = [(1024, 1 << 20, 1), (1024, 1 << 20, 2), (1024, 1 << 14, 1), (1024, 1 << 14, 2)]


def round_trip_call(lib, x, bits, tab, rows, sb, packed):
    """(run, outputs): compress -> decompress of the ctypes library `lib` on x [n, d] through a message of its own
    (u8 bins, or payload rows), on a workspace of its own."""
    from uqdme_amd import _runtime
    p, sp = _runtime.ptr, _runtime.stream_ptr(x.device)
    n, d = x.shape
    nb = ctypes.c_size_t()
    assert lib.uq_eden_workspace_bytes(n, d, ctypes.byref(nb)) == 0
    if packed:
        pb = ctypes.c_size_t()
        assert lib.uq_eden_packed_workspace_bytes(n, d, bits, ctypes.byref(pb)) == 0
        nb = pb
    ws = torch.zeros(max(1, nb.value), dtype=torch.uint8, device=x.device)
    scale = torch.empty(n, dtype=torch.float32, device=x.device)
    out = torch.empty((n, d), dtype=torch.float32, device=x.device)
    if packed:
        pitch = (d // 32) * (1 if bits == 1 else 2)
        msg = torch.empty((n, pitch), dtype=torch.int32, device=x.device)
        pbits = torch.empty(n, dtype=torch.int64, device=x.device)

        def run():
            rc = lib.uq_eden_compress_packed_f32(p(x), n, d, bits, p(tab), p(rows), p(sb), None, None, None, p(msg), p(pbits),
                                                 p(scale), p(ws), ws.numel(), sp)
            assert rc == 0, rc
            rc = lib.uq_eden_decompress_packed_f32(p(msg), p(scale), n, d, bits, p(tab), p(rows), p(sb), None, None, None,
                                                   p(out), p(ws), ws.numel(), sp)
            assert rc == 0, rc
    else:
        msg = torch.empty((n, d), dtype=torch.uint8, device=x.device)

        def run():
            rc = lib.uq_eden_compress_f32_sb(p(x), n, d, bits, p(tab), p(rows), p(sb), p(msg), p(scale), p(ws), ws.numel(), sp)
            assert rc == 0, rc
            rc = lib.uq_eden_decompress_f32_sb(p(msg), p(scale), n, d, bits, p(tab), p(rows), p(sb), p(out), p(ws), ws.numel(),
                                               sp)
            assert rc == 0, rc
    return run, (out, scale, msg)


def bench_packed(a):
    """u8 and packed compress -> decompress of this build, taking turns in one process (and, with --parent-lib, the
    parent build's u8 round trip as a third: the u8 path itself has not moved).  The yardstick of a packed form is the
    u8 form of the same build in the same run: `within_noise` = the packed median is at most the u8 median plus the
    u8 form's own 10th-90th percentile spread."""
    import uqdme  # noqa: F401
    from uqdme_amd import _lib, eden
    lib = _lib.load()
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        for name, (res, args) in _lib.SIGNATURES.items():
            if name.startswith("uq_eden_") and hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(3)
    names = {1: "fused", 2: "converter"}
    results = []
    for n, d, bits in PACKED_SHAPES:
        x = torch.randn(n, d, generator=g, device=dev)
        rows = (torch.arange(n) % 100).to(torch.int32).to(dev)
        tab = eden.rht_signs(torch.arange(100), d, dev)
        sb = eden.rht_sign_bits(tab)
        calls = {"u8": round_trip_call(lib, x, bits, tab, rows, sb, False),
                 "packed": round_trip_call(lib, x, bits, tab, rows, sb, True)}
        # the fallback of the fused forms: the same packed calls under test hook bit 0 (u8 bins + converter)
        conv_run, conv_out = round_trip_call(lib, x, bits, tab, rows, sb, True)

        def via_converter(run=conv_run):
            prev = lib.uq_test_set_eden_hooks(1)
            try:
                run()
            finally:
                lib.uq_test_set_eden_hooks(prev)
        calls["packed_converter"] = (via_converter, conv_out)
        if parent is not None:
            calls["parent_u8"] = round_trip_call(parent, x, bits, tab, rows, sb, False)
        order = list(calls)
        for k in ["packed_converter"] + [k for k in calls if k != "packed_converter"]:      # (the hooked one first:
            for _ in range(3):                                                              # the plans read below are
                calls[k][0]()                                                               # the unhooked call's)
        calls["packed"][0]()
        torch.cuda.synchronize()
        buf = (ctypes.c_int64 * 4)()
        forms = []
        for op in (0, 1):                                           # the packed call's last plans: sender, receiver
            assert lib.uq_test_last_eden_packed_plan(op, buf, 4) == 0
            forms.append(names.get(int(buf[1]), "none"))
        times = {k: [] for k in calls}
        for rep in range(a.reps):
            for k in order[::1 if rep % 2 == 0 else -1]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[k][0]()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        ref = calls["u8"][1]
        same = {k: bool(torch.equal(o[0].view(torch.int32), ref[0].view(torch.int32)) and
                        torch.equal(o[1].view(torch.int32), ref[1].view(torch.int32))) for k, (_, o) in calls.items() if k != "u8"}
        if parent is not None:
            same["parent_u8"] = same["parent_u8"] and bool(torch.equal(calls["parent_u8"][1][2], ref[2]))
        ms = {k: {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4),
                  "p90": round(float(np.percentile(v, 90)), 4)} for k, v in times.items()}
        u8 = ms["u8"]
        row = {"clients": n, "d": d, "bits": bits, "call": "compress -> decompress", "sender": forms[0], "receiver": forms[1],
               "message_bytes": {"u8": n * d, "packed": n * d * bits // 8}, "ms": ms, "same_bits": same,
               "packed_minus_u8_ms": round(ms["packed"]["median"] - u8["median"], 4),
               "converter_minus_u8_ms": round(ms["packed_converter"]["median"] - u8["median"], 4),
               "within_noise": ms["packed"]["median"] <= u8["median"] + (u8["p90"] - u8["p10"])}
        if parent is not None:
            par = ms["parent_u8"]
            row["u8_within_noise_of_parent"] = u8["median"] <= par["median"] + (par["p90"] - par["p10"])
        print(json.dumps(row), flush=True)
        results.append(row)
        del x, tab, sb, calls, ref
        torch.cuda.empty_cache()
    res = {"tool": "bench_eden --packed", "reps": a.reps, "shapes": results,
           "all_same_bits": all(all(r["same_bits"].values()) for r in results),
           "fused_within_noise": all(r["within_noise"] for r in results if r["sender"] == r["receiver"] == "fused")}
    print(json.dumps({k: v for k, v in res.items() if k != "shapes"}))
    path = a.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eden_packed_times.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=1 << 20)
    ap.add_argument("--bits", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="an earlier build whose sender is timed beside this tree's")
    ap.add_argument("--reps", type=int, default=20, help="--parent-lib: alternations per shape")
    ap.add_argument("--json", default=None, help="--parent-lib: also write the result here")
    ap.add_argument("--packed", action="store_true",
                    help="u8 and bit-packed compress -> decompress taking turns (with --parent-lib: the parent's u8 too); "
                         "writes profiles/eden_packed_times.json unless --json names another file")
    a = ap.parse_args()
    if a.packed:
        if a.reps < 30:
            a.reps = 30
        return bench_packed(a)
    if a.parent_lib:
        return bench_ab(a)
    import uqdme
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(a.clients, a.dim, generator=g, device="cuda")
    seeds = torch.randint(0, 100, (a.clients,), generator=torch.Generator().manual_seed(5))
    for _ in range(2):
        uqdme.eden_quantize(x, a.bits, seeds=seeds)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        uqdme.eden_quantize(x, a.bits, seeds=seeds)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    print(json.dumps({"tool": "bench_eden", "clients": a.clients, "d": a.dim, "bits": a.bits, "ms_per_call": round(ms, 4),
                      "M_vectors_per_s": round(a.clients / ms / 1e3, 6)}))


if __name__ == "__main__":
    main()
