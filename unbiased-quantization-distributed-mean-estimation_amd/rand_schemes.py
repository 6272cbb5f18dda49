"""Scalar_quantize and DRIVE_quantize_Hadamard on the GPU: the two baselines whose randomness is
torch.rand_like drawn from the global CPU generator (one MT19937 word per element).

    Scalar_quantize(input_vector, bits_per_dimension=1)           drop-in for AS:755-790
    DRIVE_quantize_Hadamard(input_vector, bits_per_dimension=1)   drop-in for AS:707-752
        (AS = NMSE_Results/Codes/All_Schemes.py.)  Both take the state of torch.default_generator,
        draw the reference's words from it on the GPU and leave it exactly where the reference
        leaves it; they return a new f32 tensor on the GPU.
    scalar_quantize(x[n, d], bits, px_states= | px_seeds= | generator=) -> (q, new_states, info)
    drive_quantize(x[n, d], px_states= | px_seeds= | generator=)        -> (q, new_states[, S])
        the batch forms.  Client j's words come from px_states[j] ([626] = left, next, state
        words of a torch CPU generator, see _mtstate.generator_words), from a fresh generator seeded
        with px_seeds[j], or from `generator`, where client j starts where clients 0..j-1 leave the
        stream (the drivers' order) and the generator ends where the last client leaves it.

Scalar takes d words per client, or none when the client is constant (max == min, AS:763), so
with `generator=` its clients run one after another, each waiting for the state the one before
left: px_states is its batch form.  DRIVE always takes drive_words(d), so with `generator=` the
host places every client by jump-ahead and the batch runs at once.

Bit-identical to the reference on torch CPU (tests/golden/rand_schemes_vectors.* and
rand_schemes_edges.*).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, _runtime
from ._mtstate import STATE_WORDS, advance_generator, generator_words, set_generator_words, upload_generators
from ._runtime import as_batch_f32, as_vector_f32, ptr, stream_ptr, workspace_for

__all__ = ["Scalar_quantize", "DRIVE_quantize_Hadamard", "scalar_quantize", "drive_quantize", "drive_words",
           "SCALAR_CONSTANT"]

SCALAR_CONSTANT = 1                # UQ_SCALAR_CONSTANT: max == min, out = x, no word taken


def drive_words(d: int) -> int:
    """Generator words DRIVE takes for one vector of d coordinates (uq_drive_words)."""
    w = ctypes.c_int64(0)
    _lib.check(_lib.load().uq_drive_words(int(d), ctypes.byref(w)), "uq_drive_words")
    return int(w.value)


def _one_source(px_states, px_seeds, generator):
    if sum(v is not None for v in (px_states, px_seeds, generator)) != 1:
        raise ValueError("exactly one of px_states, px_seeds and generator")


def _nlevels(bits_per_dimension):
    return 2 ** bits_per_dimension - 1                                  # AS:771


def scalar_quantize(x, bits_per_dimension, *, px_states=None, px_seeds=None, generator=None):
    """Scalar_quantize (AS:755-790) on every row of x [n, d] -> (q [n, d], new_states [n, 626]
    uint32 on the host, info [n] int32 on the host: SCALAR_CONSTANT where the row's max == min).
    A constant row comes back unchanged and its generator untouched.  2**bits - 1 < 1 (AS:772):
    q is a copy of x, no word is taken and new_states are the given ones (None for px_seeds)."""
    _one_source(px_states, px_seeds, generator)
    dev = _runtime.device()
    x = as_batch_f32(x, dev)
    n, d = x.shape
    nl = _nlevels(bits_per_dimension)
    if generator is not None:                       # the drivers' order: each client after the one before
        st, words = generator_words(generator)
        q = torch.empty_like(x)
        states = np.empty((n, STATE_WORDS), np.uint32)
        info = np.zeros(n, np.int32)
        for j in range(n):
            qj, new, inf = scalar_quantize(x[j:j + 1], bits_per_dimension, px_states=words[None, :])
            q[j], states[j], info[j] = qj[0], new[0], inf[0]
            words = new[0]
        set_generator_words(generator, st, words)
        return q, states, info
    if nl < 1 or n == 0 or d == 0:
        given = None if px_states is None else np.array(px_states, np.uint32).reshape(n, STATE_WORDS)
        return x.clone(), given, np.zeros(n, np.int32)
    _, st_in, seeds = upload_generators(n, px_states, px_seeds, dev)
    q = torch.empty_like(x)
    dout = torch.empty(n * (1 + STATE_WORDS), dtype=torch.int32, device=dev)      # info, then the end states
    ws = workspace_for("uq_rand_workspace_bytes", dev, n, d)
    _lib.check(_lib.load().uq_scalar_quantize_f32(
        ptr(x), ptr(q), n, d, float(np.float32(nl)), ptr(st_in), ptr(seeds), ptr(dout[n:]), ptr(dout), ptr(ws),
        ws.numel(), stream_ptr(dev)), "uq_scalar_quantize_f32")
    hout = dout.cpu().numpy()
    return q, hout[n:].reshape(n, STATE_WORDS).view(np.uint32).copy(), hout[:n].copy()


def drive_quantize(x, *, px_states=None, px_seeds=None, generator=None, return_scale: bool = False):
    """DRIVE_quantize_Hadamard (AS:707-752) on every row of x [n, d] -> (q [n, d], new_states
    [n, 626] int32 on the device, viewed as the uint32 words), and with return_scale the chunks'
    S [n, ceil(d / 2048)] (AS:741).  Every client takes drive_words(d) words.  Nothing here
    waits for the GPU."""
    _one_source(px_states, px_seeds, generator)
    dev = _runtime.device()
    x = as_batch_f32(x, dev)
    n, d = x.shape
    if generator is not None:
        words = drive_words(d)
        g = torch.Generator()
        g.set_state(generator.get_state())
        px_states = np.empty((n, STATE_WORDS), np.uint32)
        for j in range(n):                          # client j starts drive_words(d) * j words on
            px_states[j] = generator_words(g)[1]
            advance_generator(g, words)
    q = torch.empty_like(x)
    nch = (d + 2047) // 2048
    S = torch.empty((n, nch), dtype=torch.float32, device=dev) if return_scale else None
    st_out = torch.empty((n, STATE_WORDS), dtype=torch.int32, device=dev)
    if n and d:
        _, st_in, seeds = upload_generators(n, px_states, px_seeds, dev)
        ws = workspace_for("uq_rand_workspace_bytes", dev, n, d)
        _lib.check(_lib.load().uq_drive_hadamard_f32(
            ptr(x), ptr(q), n, d, ptr(st_in), ptr(seeds), ptr(st_out), ptr(S), ptr(ws), ws.numel(),
            stream_ptr(dev)), "uq_drive_hadamard_f32")
    elif px_states is not None:
        st_out = torch.from_numpy(np.array(px_states, np.uint32).reshape(n, STATE_WORDS).view(np.int32)).to(dev)
    if generator is not None:
        generator.set_state(g.get_state())
    return (q, st_out, S) if return_scale else (q, st_out)


def Scalar_quantize(input_vector, bits_per_dimension=1):
    """Drop-in for AS:755-790: stochastic uniform rounding between min and max on 2**bits - 1
    intervals.  The d uniforms are torch.rand_like's words of torch's global CPU generator,
    which is left where the reference leaves it: d words on, or untouched when the vector is
    constant (AS:763) or 2**bits - 1 < 1 (AS:772), which return a copy.  Returns a new f32
    tensor of shape (d,) on the GPU; d = 0 returns an empty one."""
    dev = _runtime.device()
    v = as_vector_f32(input_vector, dev, name="Scalar_quantize")
    if v.numel() == 0 or _nlevels(bits_per_dimension) < 1:
        return v.clone()
    gen = torch.default_generator
    st, words = generator_words(gen)
    q, new, _ = scalar_quantize(v.view(1, -1), bits_per_dimension, px_states=words[None, :])
    set_generator_words(gen, st, new[0])            # read back: the count depends on the data
    return q.view(-1)


def DRIVE_quantize_Hadamard(input_vector, bits_per_dimension=1):
    """Drop-in for AS:707-752 (bits_per_dimension is unused there as well): random signs, the
    reference's pair steps, one scale per 2048-coordinate chunk, sign quantization and back.
    Takes drive_words(d) words of torch's global CPU generator, which is moved on by jump-ahead
    without waiting for the GPU.  Returns a new f32 tensor of shape (d,) on the GPU."""
    dev = _runtime.device()
    v = as_vector_f32(input_vector, dev, name="DRIVE_quantize_Hadamard")
    if v.numel() == 0:
        return v.clone()
    gen = torch.default_generator
    _, words = generator_words(gen)
    q, _ = drive_quantize(v.view(1, -1), px_states=words[None, :])
    advance_generator(gen, drive_words(v.numel()))
    return q.view(-1)
