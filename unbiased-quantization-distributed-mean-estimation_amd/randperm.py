"""torch.randperm(D)[:k] of a CPU generator, computed on the GPU (uq_randperm_prefix).

The reference's EDEN receiver drops coordinates by `torch.randperm(dim)[:round(dim * pdrop)]` on the
global CPU generator (AS:419-423).  For D < 2^32 / 20 torch's CPU randperm is a forward Fisher-Yates
shuffle that takes D - 1 words of the generator whatever the prefix; the kernels compute the prefix
from the generator's state without the serial chain (csrc/uq_randperm_kernels.h), bit for bit, and
the generator is moved on by jump-ahead.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, _mtstate, _runtime
from ._runtime import ptr, stream_ptr

__all__ = ["randperm_prefix", "last_plan", "MAX_D"]

MAX_D = 0xFFFFFFFF // 20           # torch.randperm takes another algorithm from here on


def words_taken(D: int) -> int:
    """Generator words one torch.randperm(D) takes."""
    return max(0, int(D) - 1)


def client_states(n: int, D: int, generator=None, px_states=None) -> np.ndarray:
    """uint32 [n, 626]: where each client's permutation starts.  px_states: as given (checked).  Else
    client j starts j (D - 1) words into the generator's stream (n successive torch.randperm(D)
    calls), and the generator (torch's global CPU generator when None) is left n (D - 1) words on.
    One host jump-ahead per client after the first, and one for the generator."""
    if px_states is not None:
        w = np.ascontiguousarray(np.asarray(px_states, np.uint32).reshape(n, _mtstate.STATE_WORDS))
        for r in w:
            _mtstate.check_state(r)
        return w
    gen = torch.default_generator if generator is None else generator
    st, w0 = _mtstate.generator_words(gen)
    step = words_taken(D)
    out = np.empty((n, _mtstate.STATE_WORDS), np.uint32)
    cur = w0
    for j in range(n):
        out[j] = cur
        if step:
            cur = _mtstate.advance_words(cur, step)
    if step and n:
        _mtstate.set_generator_words(gen, st, cur)
    return out


def _workspace(dev, n: int, D: int, k: int, workspace_bytes):
    if workspace_bytes is None:
        return _runtime.workspace_for("uq_randperm_prefix_workspace_bytes", dev, n, D, k)
    return torch.zeros(max(int(workspace_bytes), 1), dtype=torch.uint8, device=dev)


def prefix_from_states(states_dev, n: int, D: int, k: int, dev, *, index: bool = True, bits: bool = False,
                       workspace_bytes=None):
    """uq_randperm_prefix on device states [n, 626] -> (index int64 [n, k] or None, bits int32 [n, ceil(D / 32)]
    or None)."""
    idx = torch.empty((n, k), dtype=torch.int64, device=dev) if index else None
    bt = torch.empty((n, (D + 31) // 32), dtype=torch.int32, device=dev) if bits else None
    if n:
        ws = _workspace(dev, n, D, k, workspace_bytes)
        _lib.check(_lib.load().uq_randperm_prefix(ptr(states_dev), n, D, k, ptr(idx), ptr(bt), ptr(ws), ws.numel(),
                                                  stream_ptr(dev)), "uq_randperm_prefix")
    return idx, bt


def randperm_prefix(D: int, k: int, n: int = 1, *, generator=None, px_states=None, return_bits: bool = False,
                    workspace_bytes=None):
    """int64 [n, k] on the GPU: row j = torch.randperm(D)[:k] of the j-th of n successive calls on `generator`
    (torch's global CPU generator when None), bit for bit; the generator is left n (D - 1) words on, where
    those calls leave it (D <= 1 takes no word; k does not matter).  px_states [n, 626] (left, next, the 624
    state words: torch's CPU generator state) starts each row from a state of its own instead and touches no
    generator.  return_bits=True: (index, bits int32 [n, ceil(D / 32)]), the same set with coordinate i at bit
    i % 32 of word i // 32 and every other bit 0.  workspace_bytes: a private workspace of that size instead
    of the stream's shared one (a batch that does not fit is processed in groups of clients).
    D must be below 2^32 / 20, where torch.randperm changes algorithm."""
    D, k, n = int(D), int(k), int(n)
    if D < 0 or n < 0 or not 0 <= k <= D:
        raise ValueError("randperm_prefix needs D >= 0, n >= 0 and 0 <= k <= D")
    if D >= MAX_D:
        raise ValueError("randperm_prefix needs D < 2^32 / 20 (torch.randperm changes algorithm there)")
    dev = _runtime.device()
    states = client_states(n, D, generator, px_states)
    sd = torch.from_numpy(states.view(np.int32)).to(dev) if n else None
    idx, bt = prefix_from_states(sd, n, D, k, dev, bits=return_bits, workspace_bytes=workspace_bytes)
    return (idx, bt) if return_bits else idx


def last_plan() -> dict:
    """uq_test_last_randperm_plan of this thread's last call."""
    f = (ctypes.c_int64 * 6)()
    _lib.check(_lib.load().uq_test_last_randperm_plan(f, 6), "uq_test_last_randperm_plan")
    return dict(zip(("form", "runs", "run_blocks", "group", "K", "groups"), (int(v) for v in f)))
