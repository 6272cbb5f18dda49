"""What every scheme's host code needs around a C-ABI call (include/uq_dme.h): the device, raw
pointers, the stream, the per-(device, stream) workspace with its cached size queries, the
torch-CPU thread count that fixes the summation orders, and the two input fronts (a batch
[n, d], a drop-in's vector).  A leaf module: it imports only _lib.
"""
from __future__ import annotations

import ctypes
import functools
import os
import threading

import numpy as np
import torch

from . import _lib

_ws_lock = threading.Lock()
_ws_cache: dict = {}
_torch_threads_override = None


def set_torch_threads(t):
    """Pin the torch-CPU summation order used for L1 (AS:624).  None -> follow
    torch.get_num_threads() at call time, i.e. what the CPU reference would do in
    this process."""
    global _torch_threads_override
    _torch_threads_override = None if t is None else int(t)


def get_torch_threads() -> int:
    if _torch_threads_override is not None:
        return _torch_threads_override
    env = os.environ.get("UQDME_TORCH_THREADS")
    if env:
        return int(env)
    return int(torch.get_num_threads())


def device() -> torch.device:
    """The current GPU.  (Callers write _runtime.device(): many of them take a `device` argument.)"""
    if not torch.cuda.is_available():
        raise RuntimeError("uqdme requires a ROCm GPU (no CPU fallback by design)")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr(dev: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


@functools.lru_cache(maxsize=1024)
def workspace_bytes(size_fn_name: str, *shape: int) -> int:
    """The library's `size_fn_name(*shape, &bytes)` (uq_*_workspace_bytes), asked once per shape."""
    out = ctypes.c_size_t(0)
    _lib.check(getattr(_lib.load(), size_fn_name)(*shape, ctypes.byref(out)), size_fn_name)
    return int(out.value)


def workspace_for(size_fn_name: str, dev: torch.device, *shape: int) -> torch.Tensor:
    """The workspace of (dev, current stream), at least as large as `size_fn_name` asks for
    `shape`: one tensor per (device, stream), grown on demand (stream-ordered reuse).  One
    Python frame per call on purpose: the drop-ins at small d are host-bound."""
    nbytes = workspace_bytes(size_fn_name, *shape)
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    with _ws_lock:
        ws = _ws_cache.get(key)
        if ws is None or ws.numel() < nbytes:
            # zero-filled once: the C-ABI requires a zeroed control block on first use
            ws = torch.zeros(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
            _ws_cache[key] = ws
        return ws


def check_status() -> None:
    """Synchronise the current stream and raise if an in-kernel wait timed out."""
    dev = device()
    for (idx, sp), ws in list(_ws_cache.items()):
        if idx == dev.index and sp == torch.cuda.current_stream(dev).cuda_stream:
            _lib.check(_lib.load().uq_check_status(ptr(ws), stream_ptr(dev)), "uq_check_status")


def as_batch_f32(x, dev) -> torch.Tensor:
    """A batch (tensor or array-like) as a contiguous f32 [n, d] tensor on the device."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x), dtype=torch.float32)
    if x.dim() != 2:
        raise ValueError("expected a 2-D [n, d] batch")
    return x.to(device=dev, dtype=torch.float32).contiguous()


def as_vector_f32(v, dev, *, name: str | None = None, hint: str = "") -> torch.Tensor:
    """A drop-in's input vector (tensor or array-like) as f32 on the device, never a device-side
    copy of a tensor that is f32 there already (the kernels only read it).
    With `name` (the unbiased, biased, Scalar and DRIVE drop-ins): other ranks than 1 raise
    RuntimeError as the reference does, `hint` ending the message, and the result is contiguous.
    Without (EDEN, QUIC-FL, whose reference flattens): any shape, flattened."""
    if torch.is_tensor(v):
        v = v.detach().to(device=dev, dtype=torch.float32)
    else:
        v = torch.tensor(np.asarray(v), dtype=torch.float32, device=dev)
    if name is None:
        return v.reshape(-1)
    if v.dim() != 1:
        raise RuntimeError(f"{name} expects a 1-D vector{hint}")
    return v.contiguous()
