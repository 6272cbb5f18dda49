"""EDEN with the randomized Hadamard transform on the GPU — SURVEY §8(f) row 2 (baseline).

Drop-in:
    EDEN_quantize_Hadamard(input_vector, bits_per_dimension=1)
        == NMSE_Results/Codes/All_Schemes.py:792-811: one torch.randint(0, 100) draw of the
        global CPU generator per call (the rotation seed, AS:797), EdenSender.compress then
        EdenReceiver.decompress, returns a NumPy f32 array of length d (AS:811).
        bits_per_dimension: 1, 2, or any rate between them (EdenSender.stochastic_quantize,
        AS:352-368: the 2-bit table for a seeded bernoulli(bits - 1) share of the coordinates,
        the 1-bit table for the rest; no further draw of the global generator).

Batched:
    eden_quantize(x[n, d], bits, seeds[n])              -> out[n, d]
    eden_compress(x[n, d], bits, seeds[n])              -> EdenMessage(bins u8 [n, D], scale[n], seeds, d)
    eden_decompress(msg)                                -> out[n, d]
    randperm_prefix(D, k, n)                            -> torch.randperm(D)[:k] of the CPU generator (randperm.py)

Coordinate drop (AS:413-423): a message with pdrop > 0 has round(D * pdrop) coordinates of its rotated
vector zeroed by the receiver (torch.randperm(D) on the global CPU generator, D - 1 words) and the rest
divided by 1 - pdrop.  The reference's rates below 1 bit are that drop on a 1-bit message:
EDEN_quantize_Hadamard(v, 1, pdrop=1 - r) is the reference's EDEN_quantize_Hadamard(v, r), bit for bit.

Numerics: rotation (MT19937 diagonal, f32 butterflies a+b / (a+b)-2b, / f32(sqrt(D))), the
norm (torch CPU order), the bins and the scale (its torch.dot in MKL sdot's order on the fixtures'
host, oracle/uq_eden.py:torch_dot) are bit-identical to the reference, and with them the outputs.
Only the 1- and 2-bit tables exist in the reference, so the rates are 1, 2 and what lies between them; a fractional message's nbits is the reference's tuple
(1, 2, p_high).  The spelling bits_per_dimension < 1 raises ValueError: write bits 1 with pdrop = 1 - bits.
"""
from __future__ import annotations

import ctypes
import math
import threading
import weakref
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _mtstate, _runtime, randperm
from ._runtime import as_batch_f32, as_vector_f32, ptr, stream_ptr, workspace_for

__all__ = ["EDEN_quantize_Hadamard", "eden_quantize", "eden_compress", "eden_decompress", "eden_pack", "eden_unpack",
           "eden_drop_form", "eden_with_pdrop",
           "EdenMessage", "eden_mask_bits", "eden_mask_ranks", "packed_words",
           "rht_signs", "padded_dim", "randomized_hadamard_transform", "randomized_inverse_hadamard_transform"]

_SEEDS = 100                       # AS:797 torch.randint(0, 100)
_cache_lock = threading.Lock()


class _SignCache:
    """Device sign tables kept between calls, bounded by BYTES (least recently used first out):
    the shared table of seeds 0..99 per (device, D) and the rows of other seeds (single seeds
    of the drop-ins, sets of <= 4 seeds such as QUIC-FL's fixed 123).  The newest entry always
    stays, so a table larger than the budget is still reused by the next call with that key.
    The per-call row-index tensors (4 bytes each) are cached apart, by count."""

    def __init__(self, budget_bytes: int = 2 << 30, max_rows: int = 4096):
        from collections import OrderedDict
        self.budget, self.max_rows = budget_bytes, max_rows
        self.tabs = OrderedDict()      # key -> (tensor, nbytes)
        self.rows = OrderedDict()      # key -> small int32 device tensor
        self.bytes = 0

    def get(self, key):
        hit = self.tabs.get(key)
        if hit is None:
            return None
        self.tabs.move_to_end(key)
        return hit[0]

    def put(self, key, tab):
        nb = tab.numel() * tab.element_size()
        old = self.tabs.pop(key, None)
        if old is not None:
            self.bytes -= old[1]
        self.tabs[key] = (tab, nb)
        self.bytes += nb
        while self.bytes > self.budget and len(self.tabs) > 1:
            _, (_, b) = self.tabs.popitem(last=False)
            self.bytes -= b

    def row(self, key, make):
        r = self.rows.get(key)
        if r is None:
            r = make()
            self.rows[key] = r
            while len(self.rows) > self.max_rows:
                self.rows.popitem(last=False)
        else:
            self.rows.move_to_end(key)
        return r

    def clear(self):
        self.tabs.clear()
        self.rows.clear()
        self.bytes = 0


_signs = _SignCache()


def padded_dim(d: int) -> int:
    """AS:128 / AS:359: the next power of two (d itself when it is one)."""
    return 1 if d <= 1 else 1 << (int(d) - 1).bit_length()


def rht_signs(seeds, D: int, device=None) -> torch.Tensor:
    """int8 [len(seeds), D] RHT diagonals (AS:117-120) generated on the GPU."""
    dev = device or _runtime.device()
    s = torch.as_tensor(seeds, dtype=torch.int32).reshape(-1).to(dev)
    out = torch.empty((s.numel(), D), dtype=torch.int8, device=dev)
    _lib.check(_lib.load().uq_rht_signs(ptr(s), s.numel(), D, ptr(out), stream_ptr(dev)), "uq_rht_signs")
    return out


def _shared_table(D: int, dev):
    key = (dev.index, D, "ref")
    with _cache_lock:
        tab = _signs.get(key)
        if tab is None:
            tab = rht_signs(torch.arange(_SEEDS), D, dev)
            _signs.put(key, tab)
        return tab


def _sign_rows(seeds: torch.Tensor, D: int, dev):
    """(table, row index per client).  Seeds 0..99 (the reference's range) share one cached
    table per (device, D); other seeds get rows of their own (cached for single seeds and sets
    of up to four, within the cache's byte budget)."""
    seeds_cpu = seeds.to("cpu", torch.int64).reshape(-1)
    in_range = bool(((seeds_cpu >= 0) & (seeds_cpu < _SEEDS)).all())
    if seeds_cpu.numel() == 1:                       # the per-vector drop-ins
        sd = int(seeds_cpu[0])
        if in_range:
            tab = _shared_table(D, dev)
            with _cache_lock:
                return tab, _signs.row((dev.index, sd), lambda: torch.tensor([sd], dtype=torch.int32, device=dev))
        key = (dev.index, D, "one", sd)
        with _cache_lock:
            tab = _signs.get(key)
            if tab is None:
                tab = rht_signs(seeds_cpu, D, dev)
                _signs.put(key, tab)
            return tab, _signs.row((dev.index, "zero"), lambda: torch.zeros(1, dtype=torch.int32, device=dev))
    if in_range:
        return _shared_table(D, dev), seeds_cpu.to(torch.int32).to(dev)
    uniq, inv = torch.unique(seeds_cpu, return_inverse=True)
    if uniq.numel() <= 4:                 # a few other seeds (e.g. QUIC-FL's fixed 123, AS:822): cached too
        key = (dev.index, D, tuple(uniq.tolist()))
        with _cache_lock:
            tab = _signs.get(key)
            if tab is None:
                tab = rht_signs(uniq, D, dev)
                _signs.put(key, tab)
        return tab, inv.to(torch.int32).to(dev)
    return rht_signs(uniq, D, dev), inv.to(torch.int32).to(dev)


def rht_sign_bits(tab: torch.Tensor) -> torch.Tensor:
    """int32 [rows, ceil(D / 32)]: the diagonal rows of `tab` as bits (bit set where the sign is
    -1), which the EDEN passes that apply the diagonal read instead of the int8 rows."""
    rows, D = tab.shape
    out = torch.empty((rows, (D + 31) // 32), dtype=torch.int32, device=tab.device)
    _lib.check(_lib.load().uq_rht_sign_bits(ptr(tab), rows, D, ptr(out), stream_ptr(tab.device)),
               "uq_rht_sign_bits")
    return out


_bits_of: dict = {}          # id(table) -> (weak reference to the table, its bit rows)


def _bits_for(tab: torch.Tensor) -> torch.Tensor:
    """The bit rows of a sign table, kept exactly as long as the table itself lives."""
    with _cache_lock:
        e = _bits_of.get(id(tab))
        if e is not None and e[0]() is tab:
            return e[1]
    bits = rht_sign_bits(tab)
    k = id(tab)
    with _cache_lock:
        _bits_of[k] = (weakref.ref(tab, lambda _r, k=k: _bits_of.pop(k, None)), bits)
    return bits


def _sign_rows_bits(seeds: torch.Tensor, D: int, dev):
    """(table, row index per client, the table's rows as bits)."""
    tab, rows = _sign_rows(seeds, D, dev)
    return tab, rows, _bits_for(tab)


def _seeds(seeds, n, generator=None):
    if seeds is None:
        return torch.randint(0, _SEEDS, (n,), generator=generator)     # n successive AS:797 draws
    s = torch.as_tensor(seeds, dtype=torch.int64).reshape(-1)
    if s.numel() != n:
        raise ValueError("one seed per row")
    return s


def _bits(bits):
    """1, 2, or the reference's message tuple (1, 2, p_high) for 1 < bits < 2 (AS:386-390: p_high =
    nbits - floor(nbits) as a Python double).  Anything else has no table in the reference."""
    if isinstance(bits, (tuple, list)):              # a fractional message's nbits (AS:390; a list: through JSON)
        try:
            ok = len(bits) == 3 and bits[0] == 1 and bits[1] == 2 and 0.0 < float(bits[2]) < 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("an EDEN message's nbits tuple must be (1, 2, p_high) with 0 < p_high < 1")
        return (1, 2, float(bits[2]))
    if isinstance(bits, (str, bytes)):               # float() would parse "1"; the reference compares numbers
        raise ValueError("EDEN's bits_per_dimension must be a number")
    try:
        b = float(bits)                              # Python numbers, NumPy scalars, 0-d tensors
    except (TypeError, ValueError):
        raise ValueError("EDEN's bits_per_dimension must be a number") from None
    if b == 1.0 or b == 2.0:
        return int(b)
    if 1.0 < b < 2.0:
        return (1, 2, b - 1.0)
    raise ValueError("EDEN supports 1 <= bits <= 2 (the reference's centroid tables, AS:302-306; a rate r below 1 "
                     "is the 1-bit message with dropped coordinates: pass bits 1 and pdrop=1 - r)")


def _pdrop(pdrop) -> float:
    """A message's pdrop as a Python float in [0, 1).  (At 1 the reference divides by zero, AS:423.)"""
    if isinstance(pdrop, (str, bytes)):                  # float() would parse "0.5"; the reference compares numbers
        raise ValueError("EDEN's pdrop must be a number")
    try:
        p = float(pdrop)
    except (TypeError, ValueError):
        raise ValueError("EDEN's pdrop must be a number") from None
    if math.isnan(p) or not 0.0 <= p < 1.0:
        raise ValueError("EDEN's pdrop must be in [0, 1)")
    return p


# AS:302-309: the centroid tables as the reference builds them (f32 of -c reversed, c)
_CENTROIDS = {1: [-0.7978845608028654, 0.7978845608028654],
              2: [-1.5104176087114887, -0.4527800398860679, 0.4527800398860679, 1.5104176087114887]}


def _divided_centroids(nb, p: float):
    """AS:423 `vec /= (1 - pdrop)` on the table instead of the vector: torch's own f32 division of the
    reference's f32 centroids, as host floats for the drop entry points (the kind's table, then the 1-bit
    one at a fractional rate)."""
    t = _CENTROIDS[2] + _CENTROIDS[1] if isinstance(nb, tuple) else _CENTROIDS[nb]
    q = torch.tensor(t, dtype=torch.float32)
    q /= (1 - p)
    return (ctypes.c_float * len(t))(*q.tolist())


def _drop_rows(n: int, D: int, p: float, dev, generator, drop_states):
    """int32 [n, ceil(D / 32)] on the device: the coordinates AS:420-422 drops for each client,
    torch.randperm(D)[:round(D * p)] of the generator's stream (client j from word j (D - 1); the
    generator is left n (D - 1) words on, whatever the count) or of drop_states [n, 626]."""
    k = round(D * p)                                     # AS:421 (Python's round of a float)
    states = randperm.client_states(n, D, generator, drop_states)
    sd = torch.from_numpy(states.view(np.int32)).to(dev)
    return randperm.prefix_from_states(sd, n, D, k, dev, index=False, bits=True)[1]


def _threshold(p_high: float) -> int:
    """torch.bernoulli draws f32(low24(w)) * 2^-24 < f32(p_high) (AS:361: torch.ones(D) * p_high is an
    f32 tensor), i.e. low24(w) < ceil(f32(p_high) * 2^24)."""
    import math
    import struct
    p32 = struct.unpack("f", struct.pack("f", p_high))[0]
    return int(math.ceil(p32 * (1 << 24)))


class _MaskCache(_SignCache):
    """Device mask rows of the fractional rates (uq_eden_mask_bits), kept like the sign tables and
    keyed like them plus the threshold: a mask row is a pure function of (seed, D, threshold).
    `builds` counts the tables built (tests: a warm call builds none)."""

    def __init__(self, budget_bytes: int = 1 << 30):
        super().__init__(budget_bytes)
        self.builds = 0
        self.rank_builds = 0           # rank rows built (uq_eden_mask_ranks: the packed form of these rates)


_masks = _MaskCache()
_count_lock = threading.Lock()         # of _masks.builds (its own: the cached path builds under _cache_lock)


def eden_mask_bits(seeds, D: int, threshold: int, device=None) -> torch.Tensor:
    """int32 [len(seeds), ceil(D / 32)]: bit k of row r set where coordinate k of a client with
    rotation seed seeds[r] takes the 2-bit table (AS:360-361, generator seed 7 * seed + 13)."""
    dev = device or _runtime.device()
    s = torch.as_tensor(seeds, dtype=torch.int64).reshape(-1).to(dev)
    out = torch.empty((s.numel(), (D + 31) // 32), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().uq_eden_mask_bits(ptr(s), s.numel(), D, threshold, ptr(out), stream_ptr(dev)),
               "uq_eden_mask_bits")
    with _count_lock:
        _masks.builds += 1
    return out


def _mask_key(seeds: torch.Tensor, D: int, T: int, dev):
    """(cache key, seeds of the table's rows, whether _masks keeps it) of the mask table of these seeds: the
    layout of _sign_rows' table for the same seeds, so that a client's sign row index is its mask row index
    too: rows of seeds 0..99 when every seed is in that range, the one row of a single other seed, else a
    row per distinct seed in sorted order (kept for up to four)."""
    seeds_cpu = seeds.to("cpu", torch.int64).reshape(-1)
    if bool(((seeds_cpu >= 0) & (seeds_cpu < _SEEDS)).all()):
        return (dev.index, D, T, "ref"), torch.arange(_SEEDS), True
    if seeds_cpu.numel() == 1:
        return (dev.index, D, T, "one", int(seeds_cpu[0])), seeds_cpu, True
    rows = torch.unique(seeds_cpu)
    return (dev.index, D, T, tuple(rows.tolist())), rows, rows.numel() <= 4


def _mask_table(seeds: torch.Tensor, D: int, T: int, dev, ranks: bool = False):
    """The mask rows of these seeds (_mask_key's layout); ranks=True: (mask rows, their rank rows), the rank
    rows kept in _masks beside the mask rows, under the same key and within the same byte budget: both are
    pure functions of the key, so a warm call builds neither."""
    key, rows, keep = _mask_key(seeds, D, T, dev)
    if not keep:
        tab = eden_mask_bits(rows, D, T, dev)
        return (tab, eden_mask_ranks(tab, D)) if ranks else tab
    with _cache_lock:
        tab = _masks.get(key)
        if tab is None:
            tab = eden_mask_bits(rows, D, T, dev)
            _masks.put(key, tab)
        if not ranks:
            return tab
        rk = _masks.get(key + ("ranks",))
        if rk is None:
            rk = eden_mask_ranks(tab, D)
            _masks.put(key + ("ranks",), rk)
        return tab, rk


def eden_mask_ranks(mask_bits: torch.Tensor, D: int) -> torch.Tensor:
    """int32 [rows, ceil(D / 32) + 1]: the set bits before each word of every mask row, and the row's
    count in its last entry (uq_eden_mask_ranks): where the packed form of a fractional message puts
    the low bits of the coordinates that have one."""
    rows = mask_bits.shape[0]
    out = torch.empty((rows, (D + 31) // 32 + 1), dtype=torch.int32, device=mask_bits.device)
    _lib.check(_lib.load().uq_eden_mask_ranks(ptr(mask_bits), rows, D, ptr(out), stream_ptr(mask_bits.device)),
               "uq_eden_mask_ranks")
    with _count_lock:
        _masks.rank_builds += 1
    return out


_KIND_FRAC = 12              # UQ_EDEN_NBITS_FRAC


def _kind(nb) -> int:
    return _KIND_FRAC if isinstance(nb, tuple) else nb


def packed_words(D: int, nb) -> int:
    """Words of a client's payload row (uq_eden_packed_words): ceil(D / 32) at 1 bit, twice that else."""
    P = (D + 31) // 32
    return P if _kind(nb) == 1 else 2 * P


@dataclass
class EdenMessage:
    bins: torch.Tensor      # u8 [n, D], or None for a packed message
    scale: torch.Tensor     # f32 [n]
    seeds: torch.Tensor     # int64 [n] (rotation seeds)
    nbits: object           # 1, 2, or the reference's (1, 2, p_high) for a fractional rate (AS:390)
    dim: int
    payload: torch.Tensor = None          # int32 [n, pitch]: the bins bit-packed (include/uq_dme.h has the layout)
    payload_bits: torch.Tensor = None     # int64 [n]: D, 2 D, or D + the client's mask count
    pdrop: float = 0.0                    # AS:384: the share of coordinates the receiver drops (AS:416-423)

    @property
    def packed(self) -> bool:
        return self.bins is None

    @property
    def nbytes(self) -> int:
        """Bytes of the bins as this message holds them: ceil(payload_bits / 8) per client when packed,
        a byte per coordinate else."""
        if self.bins is None:
            return int(((self.payload_bits + 7) // 8).sum().item())
        return int(self.bins.shape[0] * self.bins.shape[1])


def _prologue(x, bits_per_dimension, seeds, generator):
    """(device, x as f32 [n, d] on it, bits, one seed per row): the senders' argument checks."""
    dev = _runtime.device()
    x = as_batch_f32(x, dev)
    return dev, x, _bits(bits_per_dimension), _seeds(seeds, x.shape[0], generator)


def _call(name, dev, seeds, n, d, D, nb, head, tail):
    """uq_eden_<name>_sb(*head, n, d, nb, signs of D, sign rows, sign bits, *tail, workspace,
    stream); nothing to run for an empty batch."""
    if n and d:
        tab, rows, sb = _sign_rows_bits(seeds, D, dev)
        ws = workspace_for("uq_eden_workspace_bytes", dev, n, d)
        if isinstance(nb, tuple):
            # uq_eden_<name>_frac_f32(*head, n, d, signs, sign rows, sign bits, mask rows of (D, threshold),
            # mask row per client = its sign row, *tail, workspace, stream)
            mb = _mask_table(seeds, D, _threshold(nb[2]), dev)
            fn = "uq_eden_" + {"compress_f32": "compress_frac_f32", "decompress_f32": "decompress_frac_f32",
                               "f32": "frac_f32"}[name]
            _lib.check(getattr(_lib.load(), fn)(*map(ptr, head), n, d, ptr(tab), ptr(rows), ptr(sb), ptr(mb), ptr(rows),
                                                *map(ptr, tail), ptr(ws), ws.numel(), stream_ptr(dev)), fn)
            return
        fn = f"uq_eden_{name}_sb"
        _lib.check(getattr(_lib.load(), fn)(*map(ptr, head), n, d, nb, ptr(tab), ptr(rows), ptr(sb), *map(ptr, tail),
                                            ptr(ws), ws.numel(), stream_ptr(dev)), fn)


def _mask_rows(seeds, D, nb, dev, rows):
    """(mask rows, their rank rows, row per client) of a fractional rate for the packed entry points; three
    nulls at 1 and 2 bits.  The mask row index is the sign row index (_mask_table)."""
    if not isinstance(nb, tuple):
        return None, None, None
    mb, rk = _mask_table(seeds, D, _threshold(nb[2]), dev, ranks=True)
    return mb, rk, rows


def _call_packed(name, dev, seeds, n, d, D, nb, head, tail):
    """uq_eden_<name>_packed_f32(*head, n, d, kind, signs of D, sign rows, sign bits, mask rows, rank rows,
    mask row per client, *tail, workspace, stream); nothing to run for an empty batch."""
    if n and d:
        tab, rows, sb = _sign_rows_bits(seeds, D, dev)
        kind = _kind(nb)
        ws = workspace_for("uq_eden_packed_workspace_bytes", dev, n, d, kind)
        mb, rk, mr = _mask_rows(seeds, D, nb, dev, rows)
        fn = f"uq_eden_{name}_packed_f32"
        _lib.check(getattr(_lib.load(), fn)(*map(ptr, head), n, d, kind, ptr(tab), ptr(rows), ptr(sb), ptr(mb), ptr(rk),
                                            ptr(mr), *map(ptr, tail), ptr(ws), ws.numel(), stream_ptr(dev)), fn)


def _call_drop(fn, dev, seeds, n, d, D, nb, head, tail, drop, cents, ranks: bool = False):
    """uq_eden_decompress_drop_f32 / _packed_drop_f32 / uq_eden_drop_f32(*head, n, d, kind, signs of D, sign rows,
    sign bits, mask rows (, rank rows), mask row per client, drop rows, divided centroids, *tail, workspace, stream)."""
    tab, rows, sb = _sign_rows_bits(seeds, D, dev)
    ws = workspace_for("uq_eden_workspace_bytes", dev, n, d)
    if ranks:
        masks = _mask_rows(seeds, D, nb, dev, rows)
    else:
        frac = isinstance(nb, tuple)
        masks = (_mask_table(seeds, D, _threshold(nb[2]), dev), rows) if frac else (None, None)
    _lib.check(getattr(_lib.load(), fn)(*map(ptr, head), n, d, _kind(nb), ptr(tab), ptr(rows), ptr(sb), *map(ptr, masks),
                                        ptr(drop), cents, *map(ptr, tail), ptr(ws), ws.numel(), stream_ptr(dev)), fn)


def eden_drop_form() -> int:
    """uq_test_last_eden_drop_form: 0 when this thread's last drop call launched nothing, 1 the vector form."""
    f = ctypes.c_int32(0)
    _lib.check(_lib.load().uq_test_last_eden_drop_form(ctypes.byref(f)), "uq_test_last_eden_drop_form")
    return int(f.value)


def eden_with_pdrop(msg: EdenMessage, pdrop: float) -> EdenMessage:
    """The message with its field pdrop set (AS:384: the sender records data['pdrop'] and does not read it; the
    receiver drops, AS:416-423): a copy that shares the tensors.  pdrop must be in [0, 1): at 1 the reference
    divides by zero, and 1, NaN and values outside raise ValueError.  (eden_compress keeps its signature, which
    the packed form's tests pin, so the field is set on its result.)"""
    import dataclasses
    return dataclasses.replace(msg, pdrop=_pdrop(pdrop))


def eden_compress(x, bits_per_dimension=1, seeds=None, *, generator=None, packed: bool = False) -> EdenMessage:
    """EdenSender.compress (AS:355-376) for every row of x [n, d].  packed=True: the message at its rate,
    the bins bit-packed into `payload` rows written by the kernels that compute them (bins is None); the
    same scale, and eden_unpack gives the u8 bins back.  The message's pdrop is 0: eden_with_pdrop sets it."""
    dev, x, nb, s = _prologue(x, bits_per_dimension, seeds, generator)
    n, d = x.shape
    D = padded_dim(d)
    scale = torch.empty(n, dtype=torch.float32, device=dev)
    if packed:
        payload = torch.zeros((n, packed_words(D, nb)), dtype=torch.int32, device=dev) if not d else \
            torch.empty((n, packed_words(D, nb)), dtype=torch.int32, device=dev)
        pbits = torch.zeros(n, dtype=torch.int64, device=dev)
        _call_packed("compress", dev, s, n, d, D, nb, (x,), (payload, pbits, scale))
        return EdenMessage(bins=None, scale=scale, seeds=s, nbits=nb, dim=d, payload=payload, payload_bits=pbits)
    bins = torch.empty((n, D), dtype=torch.uint8, device=dev)
    _call("compress_f32", dev, s, n, d, bins.shape[1], nb, (x,), (bins, scale))
    return EdenMessage(bins=bins, scale=scale, seeds=s, nbits=nb, dim=d)


def eden_decompress(msg: EdenMessage, *, generator=None, drop_states=None) -> torch.Tensor:
    """EdenReceiver.decompress (AS:383-426) for every row, of a u8 or a packed message: the same bits.
    A message with pdrop > 0 has round(D * pdrop) coordinates of each rotated vector (D: the padded
    length) zeroed and the rest divided by 1 - pdrop (AS:419-423): client j's coordinates are
    torch.randperm(D)[:k] of words [j (D - 1), (j + 1)(D - 1)) of `generator` (torch's global CPU
    generator when None), which is n successive EdenReceiver.decompress calls, and the generator is
    left n (D - 1) words on, whatever k; drop_states [n, 626] starts each client's permutation from a
    generator state of its own instead and touches no generator.  pdrop = 0 draws nothing."""
    p = _pdrop(msg.pdrop)
    dev = _runtime.device()
    scale = msg.scale.to(device=dev, dtype=torch.float32).contiguous()
    d = msg.dim
    seeds = torch.as_tensor(msg.seeds)
    if msg.bins is None:
        payload = msg.payload.to(dev).contiguous()
        n, D, nb = payload.shape[0], padded_dim(d), _bits(msg.nbits)
        if payload.shape[1] != packed_words(D, nb) or payload.element_size() != 4:
            raise ValueError("a packed EDEN message's payload is [n, packed_words(D, nbits)] 32-bit words")
        out = torch.empty((n, d), dtype=torch.float32, device=dev)
        if p > 0 and n and d:
            drop = _drop_rows(n, D, p, dev, generator, drop_states)
            _call_drop("uq_eden_decompress_packed_drop_f32", dev, seeds, n, d, D, nb, (payload, scale), (out,), drop,
                       _divided_centroids(nb, p), ranks=True)
            return out
        _call_packed("decompress", dev, seeds, n, d, D, nb, (payload, scale), (out,))
        return out
    bins = msg.bins.to(dev).contiguous()
    n, D, nb = bins.shape[0], bins.shape[1], _bits(msg.nbits)
    out = torch.empty((n, d), dtype=torch.float32, device=dev)
    if p > 0 and n and d:
        drop = _drop_rows(n, D, p, dev, generator, drop_states)
        _call_drop("uq_eden_decompress_drop_f32", dev, seeds, n, d, D, nb, (bins, scale), (out,), drop,
                   _divided_centroids(nb, p))
        return out
    _call("decompress_f32", dev, seeds, n, d, D, nb, (bins, scale), (out,))
    return out


def _convert(fn, dev, msg, n, D, nb, src, dst, extra=()):
    """uq_eden_pack_bins / uq_eden_unpack_bins on the message's rows (the mask and rank rows of its seeds at a
    fractional rate)."""
    if n and D:
        seeds = torch.as_tensor(msg.seeds)
        rows = _sign_rows(seeds, D, dev)[1] if isinstance(nb, tuple) else None
        mb, rk, mr = _mask_rows(seeds, D, nb, dev, rows)
        _lib.check(getattr(_lib.load(), fn)(ptr(src), n, D, _kind(nb), ptr(mb), ptr(rk), ptr(mr), ptr(dst), *map(ptr, extra),
                                            stream_ptr(dev)), fn)


def eden_pack(msg: EdenMessage) -> EdenMessage:
    """The packed form of a u8 message (uq_eden_pack_bins, on the GPU): what eden_compress(..., packed=True)
    returns for the same input.  A packed message comes back as it is."""
    if msg.bins is None:
        return msg
    dev = _runtime.device()
    nb = _bits(msg.nbits)
    bins = msg.bins.to(dev).contiguous()
    n, D = bins.shape
    payload = torch.zeros((n, packed_words(D, nb)), dtype=torch.int32, device=dev)
    pbits = torch.zeros(n, dtype=torch.int64, device=dev)
    _convert("uq_eden_pack_bins", dev, msg, n, D, nb, bins, payload, (pbits,))
    return EdenMessage(bins=None, scale=msg.scale, seeds=msg.seeds, nbits=msg.nbits, dim=msg.dim, payload=payload,
                       payload_bits=pbits, pdrop=msg.pdrop)


def eden_unpack(msg: EdenMessage) -> EdenMessage:
    """The u8 form of a packed message (uq_eden_unpack_bins, on the GPU): bins [n, D] as eden_compress writes
    them.  A u8 message comes back as it is."""
    if msg.bins is not None:
        return msg
    dev = _runtime.device()
    nb = _bits(msg.nbits)
    payload = msg.payload.to(dev).contiguous()
    n, D = payload.shape[0], padded_dim(msg.dim)
    if payload.shape[1] != packed_words(D, nb) or payload.element_size() != 4:
        raise ValueError("a packed EDEN message's payload is [n, packed_words(D, nbits)] 32-bit words")
    bins = torch.zeros((n, D), dtype=torch.uint8, device=dev)
    _convert("uq_eden_unpack_bins", dev, msg, n, D, nb, payload, bins)
    return EdenMessage(bins=bins, scale=msg.scale, seeds=msg.seeds, nbits=msg.nbits, dim=msg.dim, pdrop=msg.pdrop)


def _interleaved_draws(n: int, D: int, generator):
    """n successive reference wrapper calls with a drop on one generator: per client the rotation seed's word
    (AS:800), then the D - 1 words of its torch.randperm(D) (AS:421) -> (seeds int64 [n], the permutations'
    start states uint32 [n, 626]); the generator is left where the n calls leave it.  One host jump-ahead per
    client."""
    gen = torch.default_generator if generator is None else generator
    seeds = torch.empty(n, dtype=torch.int64)
    states = np.empty((n, _mtstate.STATE_WORDS), np.uint32)
    for j in range(n):
        seeds[j] = torch.randint(0, _SEEDS, (1,), generator=gen)[0]
        states[j] = _mtstate.generator_words(gen)[1]
        _mtstate.advance_generator(gen, randperm.words_taken(D))
    return seeds, states


def eden_quantize(x, bits_per_dimension=1, seeds=None, *, return_scale: bool = False, generator=None, pdrop: float = 0.0,
                  drop_states=None):
    """EDEN_quantize_Hadamard for every row of x [n, d] (rotation seed per row).  pdrop in (0, 1): the
    receiver drops round(D * pdrop) coordinates per row (eden_decompress).  With seeds given, the rows'
    permutations take n (D - 1) consecutive words of `generator` (drop_states [n, 626]: explicit starts,
    no generator touched); with seeds=None the call is n successive reference wrapper calls: one seed
    word, then D - 1 permutation words, per row."""
    p = _pdrop(pdrop)                                    # (before any draw)
    if p == 0.0:
        dev, x, nb, s = _prologue(x, bits_per_dimension, seeds, generator)
    else:
        dev = _runtime.device()
        x = as_batch_f32(x, dev)
        nb = _bits(bits_per_dimension)
        if seeds is None and drop_states is not None:
            raise ValueError("drop_states needs seeds: with seeds=None the rows' draws interleave on one generator")
        s = _seeds(seeds, x.shape[0]) if seeds is not None else None
    n, d = x.shape
    D = padded_dim(d)
    out = torch.empty((n, d), dtype=torch.float32, device=dev)
    scale = torch.empty(n, dtype=torch.float32, device=dev)
    if p > 0 and n and d:
        if s is None:
            s, drop_states = _interleaved_draws(n, D, generator)
        drop = _drop_rows(n, D, p, dev, generator, drop_states)
        _call_drop("uq_eden_drop_f32", dev, s, n, d, D, nb, (x, out), (scale,), drop, _divided_centroids(nb, p))
        return (out, scale) if return_scale else out
    if s is None:
        s = _seeds(None, n, generator)
    _call("f32", dev, s, n, d, D, nb, (x, out), (scale,))
    return (out, scale) if return_scale else out


def _rht(x, seeds, inverse: bool):
    dev = _runtime.device()
    x = as_batch_f32(x, dev)
    n, d = x.shape
    D = padded_dim(d)
    if inverse and d != D:
        raise ValueError("the inverse transform takes power-of-two rows (AS:146-153)")
    s = torch.as_tensor(seeds, dtype=torch.int64).reshape(-1)
    if s.numel() != n:
        raise ValueError("one seed per row")
    out = torch.empty((n, D), dtype=torch.float32, device=dev)
    if n and d:
        tab, rows = _sign_rows(s, D, dev)
        ws = workspace_for("uq_eden_workspace_bytes", dev, n, D)
        _lib.check(_lib.load().uq_rht_f32(ptr(x), ptr(out), n, d, int(inverse), ptr(tab), ptr(rows), ptr(ws),
                                          ws.numel(), stream_ptr(dev)), "uq_rht_f32")
    return out


def randomized_hadamard_transform(x, seeds) -> torch.Tensor:
    """HadamardSender.randomized_hadamard_transform (AS:123-141) per row: zero-pad to a
    power of two, multiply by the seeded diagonal, normalized Walsh-Hadamard transform."""
    return _rht(x, seeds, False)


def randomized_inverse_hadamard_transform(x, seeds) -> torch.Tensor:
    """HadamardReceiver.randomized_inverse_hadamard_transform (AS:146-153) per row."""
    return _rht(x, seeds, True)


def EDEN_quantize_Hadamard(input_vector, bits_per_dimension=1, pdrop=0.0):
    """Drop-in for AS:792 (same name for the drivers' result keys).  Draws the rotation
    seed from torch's global CPU generator like the CPU reference (AS:797) and returns a
    NumPy f32 array (AS:811).  pdrop in [0, 1): the receiver's coordinate drop (AS:413-423), which takes
    the D - 1 words of torch.randperm(D) from the global generator after the seed's;
    EDEN_quantize_Hadamard(v, 1, pdrop=1 - r) is the reference's EDEN_quantize_Hadamard(v, r) for a rate
    r below 1, output and generator state alike (the spelling bits_per_dimension < 1 itself raises
    ValueError).  At pdrop = 1 the reference divides by zero; here 1, NaN and values outside [0, 1) raise
    ValueError before any draw."""
    pdrop = _pdrop(pdrop)
    dev = _runtime.device()
    v = as_vector_f32(input_vector, dev)
    _bits(bits_per_dimension)                            # (a rate without a table raises before the draw)
    seed = int(torch.randint(0, _SEEDS, (1,)).item())
    out = eden_quantize(v.view(1, -1), bits_per_dimension, seeds=[seed], pdrop=pdrop)
    # the NumPy result comes back through pinned memory (torch's caching host allocator):
    # a pageable 4 MB copy costs ~1 ms, about twice the whole GPU work at d = 2^20
    host = torch.empty(out.numel(), dtype=torch.float32, pin_memory=True)
    host.copy_(out.view(-1))
    return host.numpy()
