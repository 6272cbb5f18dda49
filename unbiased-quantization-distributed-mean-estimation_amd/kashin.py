"""Kashin's representation with stochastic quantization on the GPU -- the reference's last
baseline (AS = NMSE_Results/Codes/All_Schemes.py).

Drop-in:
    Kashin_quantize(input_vector, bits_per_dimension=1)
        == AS:834-854: one torch.randint(0, 100) draw of the global CPU generator per call (the
        quantizer's seed, AS:841), KashinStochasticQuantizationSender.compress then the receiver's
        decompress, returns a NumPy f32 array of length d.  Raises RuntimeError where the
        reference's torch.bernoulli does (an all-zero vector, a NaN or an inf, every d = 1), after
        the draw.

Batched:
    kashin_quantize(x[n, d], bits, seeds[n])   -> out[n, d]
    kashin_compress(x[n, d], bits, seeds[n])   -> KashinMessage(bins u8 [n, D], mn[n], step[n], seeds, nbits, d)
    kashin_decompress(msg)                     -> out[n, d]
    kashin_padded_dim(d)                       -> D (AS:202-210)
    kashin_quantize and kashin_compress also take niters, eta, delta and err (keyword-only, the
    reference's 3, 0.9, 1.0 and 1e-6); err > 1 is refused: the reference then leaves the loop after
    its first transform, by a test the device loop skips.  At 8 bits the reference can emit bin 256
    (DESIGN.md §4.8): kashin_quantize and the drop-in carry it, a u8 message stores 255 and flags
    KASHIN_BIN_RANGE.

The loop of AS:212-239 (three forward transforms, the exit test after the second) runs on the
device without a host wait.  The quantizer's bernoulli stream starts from a generator seeded with
xxh64(str(seed)) % 2^16, seed one of 100 values: its states at the starts of runs of `run_words`
coordinates are computed once per (prng seed, D, run_words) on the host by jump-ahead, cached, and
every run of a message starts at once (one wave each).  Bit-identical to the reference on torch
CPU (tests/golden/kashin_vectors.*).
"""
from __future__ import annotations

import ctypes
import functools
import threading
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _runtime
from ._mtstate import STATE_WORDS, advance_generator, generator_words
from ._runtime import as_batch_f32, as_vector_f32, ptr, stream_ptr, workspace_for
from .eden import _seeds, _sign_rows

__all__ = ["Kashin_quantize", "kashin_quantize", "kashin_compress", "kashin_decompress", "kashin_padded_dim",
           "KashinMessage", "KASHIN_BAD_P", "KASHIN_BIN_RANGE", "warm_run_tables", "clear_run_tables"]

KASHIN_BAD_P = 1                   # UQ_KASHIN_BAD_P: torch.bernoulli would raise
KASHIN_BIN_RANGE = 2               # UQ_KASHIN_BIN_RANGE: a bin above 255 (8 bits only)
ROTATION_SEED = 123                # AS:843
ETA, DELTA, ERR, NITERS = 0.9, 1.0, 1e-6, 3        # AS:245, AS:251, AS:845
MT_BLOCK = 624
# A run's length in generator words.  Measured on the drop-in at d = 2^20 and 2^22 with warm and cold
# tables for 8, 32 and 128 blocks (profiles/kashin_times.json).
DEFAULT_RUN_WORDS = 32 * MT_BLOCK


class _LRU:
    """Run tables kept between calls, bounded by bytes (least recently used first out; the newest
    entry always stays).  eden._SignCache is the model."""

    def __init__(self, budget_bytes: int):
        self.budget, self.items, self.bytes = budget_bytes, OrderedDict(), 0
        self.lock = threading.Lock()

    def get(self, key):
        with self.lock:
            hit = self.items.get(key)
            if hit is None:
                return None
            self.items.move_to_end(key)
            return hit[0]

    def put(self, key, value, nbytes: int):
        with self.lock:
            old = self.items.pop(key, None)
            if old is not None:
                self.bytes -= old[1]
            self.items[key] = (value, nbytes)
            self.bytes += nbytes
            while self.bytes > self.budget and len(self.items) > 1:
                _, (_, b) = self.items.popitem(last=False)
                self.bytes -= b

    def clear(self):
        with self.lock:
            self.items.clear()
            self.bytes = 0


_host_runs = _LRU(1 << 30)         # (prng seed, D, run_words) -> uint32 [R, 626] on the host
_dev_runs = _LRU(1 << 30)          # (device, prng seeds, D, run_words) -> int32 [rows, R, 626] on the device


def clear_run_tables() -> None:
    """Forget every cached run table (the measurement tool's cold case)."""
    _host_runs.clear()
    _dev_runs.clear()


@functools.lru_cache(maxsize=None)
def kashin_padded_dim(d: int) -> int:
    """AS:202-210 (uq_kashin_padded_dim): a power of two doubles; else the next power of two,
    doubled again when d / D > 0.85."""
    D = ctypes.c_int64(0)
    _lib.check(_lib.load().uq_kashin_padded_dim(int(d), ctypes.byref(D)), "uq_kashin_padded_dim")
    return int(D.value)


@functools.lru_cache(maxsize=4096)
def prng_seed(seed: int) -> int:
    """AS:68: xxhash.xxh64(str(seed)).intdigest() % 2**16."""
    s = str(int(seed)).encode()
    return int(_lib.load().uq_xxh64(s, len(s), 0)) % 65536


def run_table(prng: int, D: int, run_words: int) -> np.ndarray:
    """uint32 [ceil(D / run_words), 626]: the states (left, next, 624 words) of a CPU generator
    seeded with `prng` at words 0, run_words, 2 run_words, ... of its stream."""
    key = (int(prng), int(D), int(run_words))
    tab = _host_runs.get(key)
    if tab is None:
        R = -(-D // run_words)
        g = torch.Generator()
        g.manual_seed(int(prng))
        tab = np.empty((R, STATE_WORDS), np.uint32)
        for r in range(R):
            tab[r] = generator_words(g)[1]
            if r + 1 < R:
                advance_generator(g, run_words)
        _host_runs.put(key, tab, tab.nbytes)
    return tab


def _runs_for(seeds: torch.Tensor, D: int, run_words: int, dev):
    """(device tables int32 [rows, R, 626], row per client int32 [n] or None when client j reads
    row j) for the clients' seeds; a batch's tables go up in one copy."""
    prngs = [prng_seed(int(s)) for s in seeds.tolist()]
    uniq = sorted(set(prngs))
    key = (dev.index, tuple(uniq), D, run_words)
    tab = _dev_runs.get(key)
    if tab is None:
        host = np.stack([run_table(p, D, run_words) for p in uniq])
        tab = torch.from_numpy(host.view(np.int32)).to(dev)
        _dev_runs.put(key, tab, host.nbytes)
    if len(prngs) == 1:
        return tab, None
    index = {p: i for i, p in enumerate(uniq)}
    return tab, torch.tensor([index[p] for p in prngs], dtype=torch.int32).to(dev)


def warm_run_tables(d: int, run_words=None) -> None:
    """Build and upload the run tables of all 100 seeds the drop-in can draw for vectors of d
    coordinates, so that no later call pays for one (a call with a seed it has not seen yet does)."""
    dev = _runtime.device()
    for s in range(100):
        _runs_for(torch.tensor([s]), kashin_padded_dim(d), _run_words(run_words), dev)


def _bits(bits) -> int:
    if not isinstance(bits, (int, np.integer)) or not 1 <= bits <= 8:
        raise ValueError("Kashin bits must be an integer in 1..8 (the bins are bytes)")
    return int(bits)


def _run_words(run_words) -> int:
    w = DEFAULT_RUN_WORDS if run_words is None else int(run_words)
    if w < 1:
        raise ValueError("run_words must be >= 1")
    return w


@dataclass
class KashinMessage:
    bins: torch.Tensor      # u8 [n, D]
    mn: torch.Tensor        # f32 [n]
    step: torch.Tensor      # f32 [n]
    seeds: torch.Tensor     # int64 [n] (the quantizers' seeds)
    nbits: int
    dim: int
    info: torch.Tensor = None       # int32 [n]: KASHIN_BAD_P where the reference raises
    iters: torch.Tensor = None      # int32 [n]: forward transforms run


def _sender(name, x, bits_per_dimension, seeds, generator, niters, eta, delta, err, run_words, head, tail):
    """uq_kashin_<name>(x, *head, n, d, D, the loop's and the quantizer's arguments, *tail, workspace, stream)."""
    if np.float32(err) > np.float32(1.0):            # before anything is drawn (uq_kashin_* refuse it as well)
        raise ValueError("Kashin err must be <= 1 as f32: above it the reference exits after its first transform "
                         "(AS:236 at i = 0), a test the device loop does not evaluate")
    dev = _runtime.device()
    x = as_batch_f32(x, dev)
    nb = _bits(bits_per_dimension)
    n, d = x.shape
    s = _seeds(seeds, n, generator)
    if int(niters) < 1:
        raise ValueError("niters must be >= 1")
    D = kashin_padded_dim(d) if d else 0
    outs = [make(n, d, D, dev) for make in head + tail]
    if n and d:
        rw = _run_words(run_words)
        tab, rows = _sign_rows(torch.full((n,), ROTATION_SEED, dtype=torch.int64), D, dev)
        runs, run_row = _runs_for(s, D, rw, dev)
        ws = workspace_for("uq_kashin_workspace_bytes", dev, n, D)
        fn = f"uq_kashin_{name}"
        _lib.check(getattr(_lib.load(), fn)(ptr(x), *map(ptr, outs[:len(head)]), n, d, D, int(niters), float(eta),
                                            float(delta), float(err), 2 ** nb, ptr(tab), ptr(rows), ptr(runs), ptr(run_row), rw,
                                            *map(ptr, outs[len(head):]), ptr(ws), ws.numel(), stream_ptr(dev)), fn)
    return x, s, nb, outs


def _f32n(n, d, D, dev):
    return torch.empty(n, dtype=torch.float32, device=dev)


def _i32n(n, d, D, dev):
    return torch.zeros(n, dtype=torch.int32, device=dev)


def kashin_compress(x, bits_per_dimension=1, seeds=None, *, generator=None, niters: int = NITERS, eta: float = ETA,
                    delta: float = DELTA, err: float = ERR, run_words=None) -> KashinMessage:
    """KashinStochasticQuantizationSender.compress (AS:249-261) for every row of x [n, d].  Nothing
    waits for the GPU: msg.info flags the rows the reference raises on.  eta and delta are the
    sender's constructor arguments (AS:245), niters and err its data['niters'] and data['err'];
    err > 1 raises ValueError."""
    def bins(n, d, D, dev):
        return torch.empty((n, D), dtype=torch.uint8, device=dev)
    x, s, nb, (b, mn, step, info, iters) = _sender("compress_f32", x, bits_per_dimension, seeds, generator, niters,
                                                   eta, delta, err, run_words, (),
                                                   (bins, _f32n, _f32n, _i32n, _i32n))
    return KashinMessage(bins=b, mn=mn, step=step, seeds=s, nbits=nb, dim=x.shape[1], info=info, iters=iters)


def kashin_decompress(msg: KashinMessage) -> torch.Tensor:
    """KashinStochasticQuantizationReceiver.decompress (AS:269-274) for every row."""
    dev = _runtime.device()
    bins = msg.bins.to(device=dev, dtype=torch.uint8).contiguous()
    mn = msg.mn.to(device=dev, dtype=torch.float32).contiguous()
    step = msg.step.to(device=dev, dtype=torch.float32).contiguous()
    n, D = bins.shape
    d = int(msg.dim)
    out = torch.empty((n, d), dtype=torch.float32, device=dev)
    if n and d:
        tab, rows = _sign_rows(torch.full((n,), ROTATION_SEED, dtype=torch.int64), D, dev)
        ws = workspace_for("uq_kashin_workspace_bytes", dev, n, D)
        _lib.check(_lib.load().uq_kashin_decompress_f32(ptr(bins), ptr(mn), ptr(step), n, d, D, ptr(tab), ptr(rows),
                                                        ptr(out), ptr(ws), ws.numel(), stream_ptr(dev)),
                   "uq_kashin_decompress_f32")
    return out


def _raise_flagged(info) -> None:
    bad = np.flatnonzero(np.asarray(info.cpu()) & KASHIN_BAD_P)
    if bad.size:
        raise RuntimeError("Expected p_in >= 0 && p_in <= 1 to be true, but got false (torch.bernoulli in the "
                           f"reference's stochastic quantizer, AS:80): row {int(bad[0])}" +
                           (f" and {bad.size - 1} more" if bad.size > 1 else ""))


def kashin_quantize(x, bits_per_dimension=1, seeds=None, *, generator=None, niters: int = NITERS, eta: float = ETA,
                    delta: float = DELTA, err: float = ERR, run_words=None, return_info: bool = False):
    """Kashin_quantize for every row of x [n, d] (quantizer seed per row; seeds=None draws them as n
    successive AS:841 draws from `generator` or the global one).  return_info: (out, info [n]
    int32, iters [n] int32) on the device without waiting for the GPU; else out, after a check
    of info that raises RuntimeError for a row the reference raises on.  niters, eta, delta and
    err as in kashin_compress."""
    def out(n, d, D, dev):
        return torch.empty((n, d), dtype=torch.float32, device=dev)

    def none(n, d, D, dev):
        return None
    _, _, _, (q, _, _, info, iters) = _sender("f32", x, bits_per_dimension, seeds, generator, niters, eta, delta, err,
                                             run_words, (out,), (none, none, _i32n, _i32n))
    if return_info:
        return q, info, iters
    _raise_flagged(info)
    return q


def Kashin_quantize(input_vector, bits_per_dimension=1):
    """Drop-in for AS:834 (same name for the drivers' result keys).  Draws the quantizer's seed
    from torch's global CPU generator like the reference (AS:841), also when the call then raises,
    and returns a NumPy f32 array (AS:854).  d = 0 returns an empty array after the draw."""
    dev = _runtime.device()
    v = as_vector_f32(input_vector, dev)
    seed = int(torch.randint(0, 100, (1,)).item())
    q, info, _ = kashin_quantize(v.view(1, -1), bits_per_dimension, seeds=[seed], return_info=True)
    # through pinned memory, as the EDEN drop-in returns its result
    host = torch.empty(q.numel(), dtype=torch.float32, pin_memory=True)
    host.copy_(q.view(-1))
    _raise_flagged(info)
    return host.numpy()
