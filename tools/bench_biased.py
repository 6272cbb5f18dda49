"""Time the biased type quantizer (uq_type_biased_f32) on resident synthetic batches.

    python tools/bench_biased.py --clients 1024 --dim 1048576 --dist normal --ties torch

dist: normal (no ties at the threshold), smallint (integers in [-3, 3]: every client
ambiguous, KB7 replays torch's topk for each), bernoulli (0/1 with p = 0.7).

    python tools/bench_biased.py --codes --reps 20 [--parent-lib OLD.so] [--json OUT.json]

--codes times the forms of the call in one process, alternating them repetition by repetition
(device events around each call): out only (uq_type_biased_f32), out + codes and codes only
(uq_type_biased_codes_f32), the client mean over the float batch, and the mean from the codes;
median and 10th / 90th percentile of each, and the UQR1 bits per coordinate of biased codes at
R = 1 and 2 (8 clients).  --parent-lib: another build of the library (build_ext.build(src_dir=
..., out=...) of an earlier revision) whose uq_type_biased_f32 takes a turn in the same loop, on
a workspace of its own: the out-only call before and after a change, side by side."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parent_call(path, x, out, m, T, policy):
    """uq_type_biased_f32 of the library at `path` on (x, out), with its own zero-filled workspace."""
    lib = ctypes.CDLL(path)
    i32, i64, p, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    lib.uq_biased_workspace_bytes.argtypes = [i64, i64, i32, ctypes.POINTER(sz)]
    lib.uq_type_biased_f32.argtypes = [p, p, i64, i64, i64, i32, i32, p, p, p, sz, p]
    n, d = x.shape
    nb = sz()
    assert lib.uq_biased_workspace_bytes(n, d, T, ctypes.byref(nb)) == 0
    ws = torch.zeros(nb.value, dtype=torch.uint8, device=x.device)

    def run():
        rc = lib.uq_type_biased_f32(x.data_ptr(), out.data_ptr(), n, d, m, T, policy, None, None, ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return run


def bench_codes(uqdme, a, x, out, m, bits):
    from uqdme_amd import _lib, _runtime
    from uqdme_amd.biased import _TIES
    lib, dev = _lib.load(), x.device
    n, d = x.shape
    T, policy = a.torch_threads, _TIES[a.ties]
    codes = torch.empty((n, d), dtype=torch.int8, device=dev)
    kmax = torch.empty(n, dtype=torch.int32, device=dev)
    l1 = torch.empty(n, dtype=torch.float32, device=dev)
    est = torch.empty(d, dtype=torch.float32, device=dev)
    ws = _runtime.workspace_for("uq_biased_codes_workspace_bytes", dev, n, d, T)
    p, sp = _runtime.ptr, _runtime.stream_ptr(dev)

    def enc(o):
        _lib.check(lib.uq_type_biased_codes_f32(p(x), p(o), p(codes), p(kmax), n, d, m, T, policy, p(l1), None, p(ws),
                                                ws.numel(), sp), "uq_type_biased_codes_f32")

    forms = {
        "out_only": lambda: uqdme.biased_quantize(x, m=m, torch_threads=T, ties=a.ties, out=out),
        "out_and_codes": lambda: enc(out),
        "codes_only": lambda: enc(None),
        "client_mean_floats": lambda: uqdme.client_mean(out, n, est=est),
        "mean_from_codes": lambda: _lib.check(lib.uq_codes_mean_form_f32(p(codes), d, None, d, p(l1), p(kmax), n, d, m, 1,
                                                                         float(n), 0, p(est), sp), "uq_codes_mean_form_f32"),
    }
    if a.parent_lib:
        forms["out_only_parent"] = parent_call(a.parent_lib, x, out, m, T, policy)
    for f in forms.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    order = list(forms)
    for rep in range(a.reps):
        if a.parent_lib:           # the two out-only calls next to each other, taking turns to go first
            pair = ["out_only", "out_only_parent"][::1 if rep % 2 == 0 else -1]
            order = pair + [k for k in forms if k not in pair]
        for k in order:
            f = forms[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    uqdme.check_status()
    # the codes-only pipeline gives the float pipeline's mean, on this very batch
    uqdme.biased_quantize(x, m=m, torch_threads=T, ties=a.ties, out=out)
    ref = uqdme.client_mean(out, n).clone()
    enc(None)
    forms["mean_from_codes"]()
    same = bool(torch.equal(ref.view(torch.int32), est.view(torch.int32)))
    bpc = {}
    for R in (1, 2):
        tc = uqdme.biased_quantize_encode(x[:8], R, torch_threads=T, ties=a.ties)
        bpc[f"R{R}"] = round(uqdme.encode_messages(tc).bits_per_dim(), 4)
        bpc[f"R{R}_exact_zero_signs"] = round(uqdme.encode_messages(tc, exact_zero_signs=True).bits_per_dim(), 4)
    res = {"tool": "bench_biased --codes", "clients": n, "d": d, "bits": bits, "dist": a.dist, "ties": a.ties,
           "reps": a.reps, "flagged_clients": int((kmax > 127).sum()), "mean_from_codes_equals_float_mean": same,
           "uqr1_bits_per_coordinate": bpc,
           "ms": {k: {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4),
                      "p90": round(float(np.percentile(v, 90)), 4)} for k, v in times.items()}}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=1 << 20)
    ap.add_argument("--bits", type=float, default=1)
    ap.add_argument("--dist", default="normal", choices=["normal", "smallint", "bernoulli"])
    ap.add_argument("--ties", default="torch", choices=["torch", "lowest"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--torch-threads", type=int, default=1)
    ap.add_argument("--codes", action="store_true", help="time out only / out + codes / codes only + mean, alternating")
    ap.add_argument("--reps", type=int, default=20, help="--codes: alternating repetitions per form")
    ap.add_argument("--parent-lib", default=None, help="--codes: an earlier build whose out-only call is timed beside")
    ap.add_argument("--json", default=None, help="--codes: also write the result here")
    a = ap.parse_args()
    import uqdme
    bits = int(a.bits) if float(a.bits).is_integer() else a.bits
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(3)
    n, d = a.clients, a.dim
    if a.dist == "normal":
        x = torch.randn(n, d, generator=g, device=dev)
    elif a.dist == "smallint":
        x = torch.randint(-3, 4, (n, d), generator=g, device=dev).float()
    else:
        x = (torch.rand(n, d, generator=g, device=dev) < 0.7).float()
    out = torch.empty_like(x)
    m = uqdme.rate_to_m(bits, d)
    if a.codes:
        return bench_codes(uqdme, a, x, out, m, bits)
    for _ in range(2):
        uqdme.biased_quantize(x, m=m, torch_threads=a.torch_threads, ties=a.ties, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        uqdme.biased_quantize(x, m=m, torch_threads=a.torch_threads, ties=a.ties, out=out)
    e1.record()
    torch.cuda.synchronize()
    uqdme.check_status()
    ms = e0.elapsed_time(e1) / a.steps
    _, info = uqdme.biased_quantize(x, m=m, torch_threads=a.torch_threads, ties=a.ties, out=out, return_info=True)
    amb = int(((info[:, 1] & 1) != 0).sum())
    print(json.dumps({"tool": "bench_biased", "clients": n, "d": d, "bits": bits, "dist": a.dist, "ties": a.ties,
                      "ms_per_call": round(ms, 4), "M_vectors_per_s": round(n / ms / 1e3, 6),
                      "GB_per_s_x_plus_out": round(8.0 * n * d / ms / 1e6, 1), "ambiguous_clients": amb}))


if __name__ == "__main__":
    main()
