"""Host-side mirror of the reference's quantizer interface, backed by HIP kernels.

Drop-in:
    Type_unbiased_quantize(input_vector, bits_per_dimension=1)
        == NMSE_Results/Codes/All_Schemes.py:609-641, same name, argument meaning,
        return type (new f32 tensor of shape (d,) on the GPU), RNG use (one draw from
        torch's global CPU generator per call, AS:634) and errors (KeyError for an
        unknown rate, AS:622; RuntimeError for non-1-D input, AS:635).

Batched APIs (what the DME harness and the bench use):
    quantize_dequantize(x[n, d], bits | m=, X[n])       -> q[n, d]
    client_mean(q[n, d], n_div, est=None)                 -> est[d]   (ND:137-138)
    quantize_mean(x[n, d], bits, X[n], n_div, est=None)   -> est[d]
    l1_torch_order(x[n, d], torch_threads)                -> l1[n]    (AS:624)

Every path calls the C-ABI in include/uq_dme.h; nothing here computes on the CPU.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, _runtime
from ._runtime import (as_batch_f32, as_vector_f32, check_status, get_torch_threads, ptr,  # noqa: F401 (re-exports)
                       set_torch_threads, stream_ptr, workspace_for)
from .codes import TypeCodes, form_index
from .outpool import POOL
from .rates import RATE_TABLE, rate_to_m

__all__ = [
    "Type_unbiased_quantize", "quantize_dequantize", "client_mean", "quantize_mean", "quantize_encode", "decode",
    "codes_mean",
    "l1_torch_order", "draw_uniforms", "set_torch_threads", "get_torch_threads",
]


def draw_uniforms(n: int, generator: torch.Generator | None = None) -> torch.Tensor:
    """n draws of AS:634's X from a CPU generator; torch.rand(n) equals n successive
    torch.rand(1) calls, so this reproduces a per-client loop of the reference."""
    return torch.rand(n, generator=generator, dtype=torch.float32)


def _prologue(x, bits, m, torch_threads, X, generator, dev):
    """-> (x as f32 [n, d] on dev, m, T, X flat f32 with one draw per row, where it was given or
    drawn: on the host unless the caller passed a device tensor)."""
    x = as_batch_f32(x, dev)
    n, d = x.shape
    mm = int(m) if m is not None else rate_to_m(bits, d)
    T = get_torch_threads() if torch_threads is None else int(torch_threads)
    if X is None:
        X = draw_uniforms(n, generator)
    X = torch.as_tensor(X, dtype=torch.float32).reshape(-1)
    if X.numel() != n:
        raise ValueError("X must have one draw per row")
    return x, mm, T, X


def _quantize_vec(v, m, X0: float, T, dev, out=None):
    """One contiguous f32 vector on dev with its draw by value (uq_type_unbiased_vec_f32): the
    call is the kernel chain alone -- no host-to-device copy of X, no workspace fill; same
    kernels and bits as a one-row batch (0.20 -> 0.15 ms at 2^22)."""
    if out is None:
        out = torch.empty_like(v)
    ws = workspace_for("uq_workspace_bytes", dev, 1, v.numel(), T)
    _lib.check(_lib.load().uq_type_unbiased_vec_f32(ptr(v), ptr(out), v.numel(), m, X0, T, ptr(ws), ws.numel(),
                                                    stream_ptr(dev)), "uq_type_unbiased_vec_f32")
    return out


def l1_torch_order(x, torch_threads: int | None = None) -> torch.Tensor:
    """AS:624 `|x|.sum()` per row, bit-identical to torch CPU with `torch_threads` threads."""
    dev = _runtime.device()
    x = as_batch_f32(x, dev)
    n, d = x.shape
    T = get_torch_threads() if torch_threads is None else int(torch_threads)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    ws = workspace_for("uq_workspace_bytes", dev, n, d, T)
    _lib.check(_lib.load().uq_l1_torch_order_f32(ptr(x), n, d, T, ptr(out), ptr(ws), ws.numel(),
                                                 stream_ptr(dev)), "uq_l1_torch_order_f32")
    return out


def quantize_dequantize(x, bits_per_dimension=1, X=None, *, m: int | None = None,
                        torch_threads: int | None = None, l1=None, out=None,
                        return_l1: bool = False, generator: torch.Generator | None = None):
    """Batched `Type_unbiased_quantize`: row j of `x` is quantized with uniform X[j].

    X defaults to n fresh draws from the CPU generator (global one unless given)."""
    dev = _runtime.device()
    x, mm, T, X = _prologue(x, bits_per_dimension, m, torch_threads, X, generator, dev)
    n, d = x.shape
    token = None
    if out is None:
        (out,), token = POOL.acquire(dev, [((n, d), torch.float32)])     # probed placement for big batches
    elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous f32 tensor like x")
    if n == 1 and d > 0 and l1 is None and not return_l1 and X.device.type == "cpu":
        return _quantize_vec(x, mm, X.item(), T, dev, out)   # one vector with its draw on the host
    X = X.to(dev)
    if l1 is not None:
        l1 = torch.as_tensor(l1, dtype=torch.float32).reshape(-1).to(dev).contiguous()
        if l1.numel() != n:
            raise ValueError("l1 must have one value per row")
    l1_out = torch.empty(n, dtype=torch.float32, device=dev) if return_l1 else None
    ws = workspace_for("uq_workspace_bytes", dev, n, d, T)
    POOL.timed(token, lambda: _lib.check(_lib.load().uq_type_unbiased_f32(
        ptr(x), ptr(out), n, d, mm, ptr(X), ptr(l1), ptr(l1_out), T, ptr(ws), ws.numel(), stream_ptr(dev)),
        "uq_type_unbiased_f32"))
    return (out, l1_out) if return_l1 else out


def quantize_encode(x, bits_per_dimension=1, X=None, *, m: int | None = None, torch_threads: int | None = None,
                    l1=None, return_q: bool = False, generator: torch.Generator | None = None):
    """Quantize a batch and emit type codes (codes.TypeCodes); optionally also q.

    Same numerics as quantize_dequantize: decode(codes) == q bit-for-bit."""
    dev = _runtime.device()
    x, mm, T, X = _prologue(x, bits_per_dimension, m, torch_threads, X, generator, dev)
    n, d = x.shape
    X = X.to(dev)
    if l1 is not None:
        l1 = torch.as_tensor(l1, dtype=torch.float32).reshape(-1).to(dev).contiguous()
    specs = [((n, d), torch.int8)] + ([((n, d), torch.float32)] if return_q else [])
    bufs, token = POOL.acquire(dev, specs)                      # probed placement for big batches
    codes = bufs[0]
    q = bufs[1] if return_q else None
    overflow = torch.zeros(n, dtype=torch.int32, device=dev)     # per-client kmax (128 = overflow)
    l1_out = torch.empty(n, dtype=torch.float32, device=dev)
    ws = workspace_for("uq_workspace_bytes", dev, n, d, T)
    POOL.timed(token, lambda: _lib.check(_lib.load().uq_type_unbiased_codes_f32(
        ptr(x), ptr(q), ptr(codes), ptr(overflow), n, d, mm, ptr(X), ptr(l1), ptr(l1_out), T, ptr(ws),
        ws.numel(), stream_ptr(dev)), "uq_type_unbiased_codes_f32"))
    tc = TypeCodes(codes=codes, l1=l1_out, m=mm, overflow=overflow)
    return (tc, q) if return_q else tc


def decode(tc) -> torch.Tensor:
    """Rebuild the dequantized batch from type codes in their form: bit-identical to
    quantize_dequantize (tc.form "unbiased") or biased_quantize ("biased")."""
    dev = _runtime.device()
    codes = tc.codes.to(dev).contiguous()
    l1 = tc.l1.to(device=dev, dtype=torch.float32).contiguous()
    n, d = codes.shape
    out = torch.empty((n, d), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().uq_codes_decode_form_f32(ptr(codes), ptr(l1), n, d, int(tc.m), form_index(tc.form), ptr(out),
                                                    stream_ptr(dev)), "uq_codes_decode_form_f32")
    return out


def codes_mean(tc, n_div, est=None, accumulate: bool = False, q=None) -> torch.Tensor:
    """ND:137-138 from type codes: est (+)= decode(codes)[j] / n_div over clients j in order,
    bit-identical to client_mean(decode(tc), n_div), in the codes' form (tc.form).  q: the
    dequantized batch [n, d] beside the codes; a client whose codes must not be decoded
    (tc.overflow == 128) is then read from it."""
    dev = _runtime.device()
    codes = tc.codes.to(dev).contiguous()
    l1 = tc.l1.to(device=dev, dtype=torch.float32).contiguous()
    n, d = codes.shape
    if est is None:
        est = torch.empty(d, dtype=torch.float32, device=dev)
        accumulate = False
    kmax = tc.overflow.to(device=dev, dtype=torch.int32).contiguous()
    if q is not None:
        q = q.to(device=dev, dtype=torch.float32).contiguous()
        if q.shape != codes.shape:
            raise ValueError("q must have the codes' shape")
    _lib.check(_lib.load().uq_codes_mean_form_f32(ptr(codes), d, ptr(q), d, ptr(l1), ptr(kmax), n, d, int(tc.m),
                                                  form_index(tc.form), float(n_div), int(bool(accumulate)), ptr(est),
                                                  stream_ptr(dev)), "uq_codes_mean_form_f32")
    return est


def client_mean(q, n_div, est=None, accumulate: bool = False) -> torch.Tensor:
    """ND:137-138: est (+)= q[j] / n_div over rows j in order (f32).

    `q` may be a column block of a wider row-major batch (unit column stride, any row
    stride); with accumulate=True the sum continues from `est` bit-for-bit."""
    dev = _runtime.device()
    if not torch.is_tensor(q):
        q = torch.as_tensor(np.asarray(q), dtype=torch.float32)
    if q.dim() != 2:
        raise ValueError("expected a 2-D [n, d] batch")
    q = q.to(device=dev, dtype=torch.float32)
    if q.shape[1] > 0 and (q.stride(1) != 1 or q.stride(0) < q.shape[1]):
        q = q.contiguous()
    n, d = q.shape
    ld = q.stride(0) if n > 0 else d
    if est is None:
        est = torch.empty(d, dtype=torch.float32, device=dev)
        accumulate = False
    elif est.shape != (d,) or est.dtype != torch.float32 or est.device != q.device or not est.is_contiguous():
        raise ValueError("est must be a contiguous f32 vector of length d on the same device")
    _lib.check(_lib.load().uq_client_mean_f32(ptr(q), n, d, max(ld, d), float(n_div), int(bool(accumulate)),
                                              ptr(est), stream_ptr(dev)), "uq_client_mean_f32")
    return est


def quantize_mean(x, bits_per_dimension=1, X=None, n_div=None, *, m: int | None = None,
                  torch_threads: int | None = None, est=None, accumulate: bool = False, out=None):
    """Quantize every row and fold it into the client-ordered mean (ND:133-138)."""
    dev = _runtime.device()
    x, mm, T, X = _prologue(x, bits_per_dimension, m, torch_threads, X, None, dev)
    n, d = x.shape
    X = X.to(dev)
    if n_div is None:
        n_div = n
    if est is None:
        est = torch.empty(d, dtype=torch.float32, device=dev)
        accumulate = False
    token = None
    if out is None:
        (out,), token = POOL.acquire(dev, [((n, d), torch.float32)])     # scratch q: probed placement
    ws = workspace_for("uq_workspace_bytes", dev, n, d, T)
    POOL.timed(token, lambda: _lib.check(_lib.load().uq_type_unbiased_mean_f32(
        ptr(x), ptr(out), n, d, mm, ptr(X), ptr(None), T, float(n_div), int(bool(accumulate)), ptr(est),
        ptr(ws), ws.numel(), stream_ptr(dev)), "uq_type_unbiased_mean_f32"))
    return est


def Type_unbiased_quantize(input_vector, bits_per_dimension=1):
    """Drop-in for NMSE_Results/Codes/All_Schemes.py:609 (same name: the Flower client
    derives directory names from `__name__`, FLM:177).

    AS:611  takes `input_vector` as f32 on the device (the input is only read; the result
            is always a new tensor, as the reference's copy guarantees: the kernels write a
            new output, and d == 0 returns a clone)
    AS:622  unknown `bits_per_dimension` -> KeyError (checked before any work)
    AS:634  consumes exactly one draw of torch's global CPU generator
    Returns a new f32 tensor of shape (d,) on the GPU."""
    dev = _runtime.device()
    l_rate = RATE_TABLE[bits_per_dimension]          # KeyError like the reference
    v = as_vector_f32(input_vector, dev, name="Type_unbiased_quantize",
                      hint=" (the reference fails at torch.cat for other ranks)")
    d = v.numel()
    X = torch.rand(1)                                   # AS:634 (global CPU generator)
    if d == 0:
        return v.clone()
    return _quantize_vec(v, int(l_rate * d), X.item(), get_torch_threads(), dev)
