"""Time the QUIC-FL sender (uq_quicfl_compress_f32) and receiver on a resident synthetic batch,
on the synthetic sender tables of tests/golden/quicfl_tables.py and the reference's receiver
tables (tests/golden/quicfl_recv_vectors.npz).  Also times one message per call (the drop-in's
QuicFLSender.compress, host work included).

    python tools/bench_quicfl.py --clients 1024 --dim 1048576 --bits 1

    python tools/bench_quicfl.py --packed [--parent-lib OLD.so] [--reps 30] [--json OUT.json]

--packed: the u8 message, the packed message (uq_quicfl_compress_packed_f32 -> uq_quicfl_receive_packed_f32) and
the packed message through the converter path (uq_test_set_quicfl_packed_hooks bit 0), compress then receive
through the C ABI, taking turns in one process over PACKED_SHAPES, device events around each round trip; with
--parent-lib (another build of the library) that build's u8 round trip as a fourth.  Median and 10th / 90th
percentile per contender; the yardstick of a packed form is the u8 form of the same run.  Writes
profiles/quicfl_packed_times.json."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def make_sender(uqdme, bits):
    from quicfl_tables import DATA, sender_tables
    X, p = sender_tables(bits)
    return uqdme.QuicFLSender(tables={bits: (X, p, DATA[bits])})


def recv_table(bits):
    return np.load(os.path.join(ROOT, "tests", "golden", "quicfl_recv_vectors.npz"))[f"recv{bits}"]


def digest(msg, out):
    import hashlib
    h = hashlib.sha256()
    for t in (msg.X, msg.exact_mask, msg.exact_dense(), msg.scale, out):
        t = t.contiguous()
        t = t.view(torch.int32) if t.dtype == torch.float32 else t
        w = torch.arange(t.shape[-1], device=t.device, dtype=torch.int64) % 65521 + 1
        rows = (t.to(torch.int64) * w).sum(dim=-1) if t.dim() > 1 else t.to(torch.int64)
        h.update(rows.cpu().numpy().tobytes())
    h.update(np.asarray(msg.exact_count).tobytes())
    return h.hexdigest()[:16]


def timed(f, steps):
    f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


PACKED_SHAPES = ((1024, 1 << 20, 1), (1024, 1 << 20, 2), (128, 1 << 20, 1))       # (clients, dim, bits)


def round_trip_call(lib, uqdme, snd, rt, x, bits, packed):
    """compress -> receive of the whole batch through `lib`'s C ABI on preallocated buffers -> (run, outputs)"""
    from uqdme_amd import quicfl as Q
    from uqdme_amd._runtime import ptr, stream_ptr
    n, d = x.shape
    dev = x.device
    a = Q._send_prologue(x, bits, list(range(n)), [123] * n, snd, list(range(1000, 1000 + n)), None, 2, packed)
    D = a.D
    ev = torch.empty((n, D), dtype=torch.float32, device=dev)
    scale = torch.empty(n, dtype=torch.float32, device=dev)
    pre = torch.empty((n, D), dtype=torch.float32, device=dev)
    rinfo = torch.zeros(n, dtype=torch.int32, device=dev)
    cnt = a.dout[n:2 * n]
    tab = torch.as_tensor(rt, dtype=torch.float32).to(dev).contiguous()
    seeds32 = a.ps.to(torch.int32).to(dev)
    wb = ctypes.c_size_t()
    wsf = lib.uq_quicfl_receive_packed_workspace_bytes if packed else lib.uq_quicfl_receive_workspace_bytes
    assert wsf(n, D, ctypes.byref(wb)) == 0
    rws = torch.empty(max(int(wb.value), 1), dtype=torch.uint8, device=dev)
    st = stream_ptr(dev)
    if packed:
        pay = torch.zeros((n, bits * ((D + 31) // 32)), dtype=torch.int32, device=dev)
        eidx = torch.empty((n, D), dtype=torch.int32, device=dev)
        pbits = torch.zeros(n, dtype=torch.int64, device=dev)
        keep = (a, ev, scale, pre, rinfo, tab, seeds32, rws, pay, eidx, pbits)

        def run():
            rc = lib.uq_quicfl_compress_packed_f32(*a.head, *a.gens, ptr(pay), bits, ptr(eidx), ptr(ev), ptr(cnt), ptr(pbits),
                                                   ptr(scale), ptr(a.info), *a.tail)
            assert rc == 0, rc
            rc = lib.uq_quicfl_receive_packed_f32(ptr(pay), bits, n, D, ptr(tab), tab.shape[0], tab.shape[1], ptr(seeds32), ptr(eidx),
                                                  ptr(ev), ptr(cnt), ptr(scale), ptr(pre), ptr(rinfo), ptr(rws), wb.value, st)
            assert rc == 0, rc
        return run, (pre, scale, cnt, keep)
    X = torch.empty((n, D), dtype=torch.uint8, device=dev)
    mask = torch.empty((n, D), dtype=torch.uint8, device=dev)
    keep = (a, ev, scale, pre, rinfo, tab, seeds32, rws, X, mask)

    def run():
        rc = lib.uq_quicfl_compress_f32(*a.head, *a.gens, ptr(X), 1, ptr(mask), ptr(ev), ptr(cnt), ptr(scale), ptr(a.info), *a.tail)
        assert rc == 0, rc
        rc = lib.uq_quicfl_receive_ws_f32(ptr(X), 1, n, D, ptr(tab), tab.shape[0], tab.shape[1], ptr(seeds32), ptr(mask), ptr(ev), 1,
                                          ptr(cnt), ptr(scale), ptr(pre), ptr(rinfo), ptr(rws), wb.value, st)
        assert rc == 0, rc
    return run, (pre, scale, cnt, keep)


def bench_packed(a):
    import uqdme
    from uqdme_amd import _lib
    lib = _lib.load()
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        for name, (res, args) in _lib.SIGNATURES.items():
            if name.startswith("uq_quicfl_") and hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, args
    names = {1: "fused", 2: "converter"}
    forms_q = {1: "one-wave", 2: "team", 3: "jump"}
    g = torch.Generator(device="cuda").manual_seed(3)
    results = []
    for n, d, bits in PACKED_SHAPES:
        snd, rt = make_sender(uqdme, bits), recv_table(bits)
        x = torch.randn(n, d, generator=g, device="cuda")
        calls = {"u8": round_trip_call(lib, uqdme, snd, rt, x, bits, False),
                 "packed": round_trip_call(lib, uqdme, snd, rt, x, bits, True)}
        conv_run, conv_out = round_trip_call(lib, uqdme, snd, rt, x, bits, True)

        def via_converter(run=conv_run):
            prev = lib.uq_test_set_quicfl_packed_hooks(1)
            try:
                run()
            finally:
                lib.uq_test_set_quicfl_packed_hooks(prev)
        calls["packed_converter"] = (via_converter, conv_out)
        if parent is not None:
            calls["parent_u8"] = round_trip_call(parent, uqdme, snd, rt, x, bits, False)
        order = list(calls)
        for k in ["packed_converter"] + [k for k in calls if k != "packed_converter"]:
            for _ in range(3):
                calls[k][0]()
        calls["packed"][0]()
        torch.cuda.synchronize()
        buf, qb = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 6)()
        forms, qforms = [], []
        for side in (0, 1):                                         # the packed call's last plans: sender, receiver
            assert lib.uq_test_last_quicfl_packed_plan(side, buf, 4) == 0 and lib.uq_test_last_quicfl_plan(side, qb, 6) == 0
            forms.append(names.get(int(buf[1]), "none"))
            qforms.append(forms_q.get(int(qb[0]), "none"))
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
                        torch.equal(o[1].view(torch.int32), ref[1].view(torch.int32)) and torch.equal(o[2], ref[2]))
                for k, (_, o) in calls.items() if k != "u8"}
        ms = {k: {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4),
                  "p90": round(float(np.percentile(v, 90)), 4)} for k, v in times.items()}
        u8 = ms["u8"]
        D = ref[0].shape[1]
        exact = int(ref[2].sum().item())
        row = {"clients": n, "d": d, "bits": bits, "call": "compress -> receive", "quicfl_forms": qforms, "sender": forms[0],
               "receiver": forms[1], "message_bytes": {"u8": 2 * n * D + 4 * exact, "packed": n * D * bits // 8 + 8 * exact},
               "ms": ms, "same_bits": same, "packed_minus_u8_ms": round(ms["packed"]["median"] - u8["median"], 4),
               "converter_minus_u8_ms": round(ms["packed_converter"]["median"] - u8["median"], 4),
               "within_noise": ms["packed"]["median"] <= u8["median"] + (u8["p90"] - u8["p10"])}
        if parent is not None:
            par = ms["parent_u8"]
            row["u8_within_noise_of_parent"] = u8["median"] <= par["median"] + (par["p90"] - par["p10"])
        print(json.dumps(row), flush=True)
        results.append(row)
        del x, calls, ref, conv_out, conv_run
        torch.cuda.empty_cache()
    res = {"tool": "bench_quicfl --packed", "reps": a.reps, "shapes": results,
           "all_same_bits": all(all(r["same_bits"].values()) for r in results),
           "fused_within_noise": all(r["within_noise"] for r in results)}
    print(json.dumps({k: v for k, v in res.items() if k != "shapes"}))
    with open(a.json or os.path.join(ROOT, "profiles", "quicfl_packed_times.json"), "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=1 << 20)
    ap.add_argument("--bits", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--per-call", type=int, default=5, help="single-message compress calls to time (0: skip)")
    ap.add_argument("--digest", action="store_true", help="add a digest of the messages and the decompressed batch")
    ap.add_argument("--packed", action="store_true", help="u8, packed and packed-through-the-converter round trips taking turns")
    ap.add_argument("--parent-lib", default=None, help="--packed: an earlier build whose u8 round trip is timed beside")
    ap.add_argument("--reps", type=int, default=30, help="--packed: alternations per shape")
    ap.add_argument("--json", default=None, help="--packed: write the result here instead of profiles/")
    a = ap.parse_args()
    if a.packed:
        return bench_packed(a)
    import uqdme
    snd = make_sender(uqdme, a.bits)
    rt = recv_table(a.bits)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(a.clients, a.dim, generator=g, device="cuda")
    seeds = list(range(a.clients))
    rots = [123] * a.clients
    pxs = list(range(1000, 1000 + a.clients))
    holder = {}

    def comp():
        holder["m"] = uqdme.quicfl_compress(x, a.bits, seeds, rots, sender=snd, px_seeds=pxs)

    ms_c = timed(comp, a.steps)
    msg = holder["m"]
    ms_d = timed(lambda: uqdme.quicfl_decompress_messages(msg, rt), a.steps)
    res = {"tool": "bench_quicfl", "clients": a.clients, "d": a.dim, "bits": a.bits, "compress_ms": round(ms_c, 4),
           "decompress_ms": round(ms_d, 4), "exact_per_client": float(msg.exact_count.float().mean()),
           "M_vectors_per_s_compress": round(a.clients / ms_c / 1e3, 6)}
    if a.digest:                           # to compare library variants' outputs (tools/exp/variants.py)
        res["digest"] = digest(msg, uqdme.quicfl_decompress_messages(msg, rt))
    if a.per_call:
        v = x[0].clone()
        data = {"vec": v, "seed": 7, "nbits": a.bits, "rotation_seed": 123}
        snd.compress(data)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.per_call):
            snd.compress(data)
        torch.cuda.synchronize()
        res["compress_per_call_ms"] = round((time.perf_counter() - t0) * 1e3 / a.per_call, 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
