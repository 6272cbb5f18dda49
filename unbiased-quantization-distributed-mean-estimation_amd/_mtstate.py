"""torch's CPU generator (ATen mt19937) as the [626] words the kernels take: (left, next, the 624
state words).  Reading and writing a torch.Generator's state in that form, moving it on by
jump-ahead, and packing the per-client generators of a batch call (states or seeds) for one
host-to-device copy.  Used by every scheme whose randomness is the reference's own draws from a
CPU generator: QUIC-FL's bernoulli(p_X), Scalar's and DRIVE's rand_like, the DME harness.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib

STATE_WORDS = 626                  # UQ_QFL_STATE_WORDS: (left, next, 624 words)


def generator_words(gen: torch.Generator):
    """(get_state() bytes, uint32 [626] = left, next, state words) of a CPU generator."""
    st = gen.get_state().numpy().copy()
    _, left, _, nxt = struct.unpack_from("<QiiQ", st.tobytes(), 0)
    out = np.empty(STATE_WORDS, np.uint32)
    out[0], out[1] = left, nxt
    out[2:] = np.frombuffer(st[24:24 + 624 * 8].tobytes(), dtype=np.uint64).astype(np.uint32)
    return st, out


def set_generator_words(gen: torch.Generator, st: np.ndarray, words: np.ndarray) -> None:
    b = bytearray(st.tobytes())
    struct.pack_into("<i", b, 8, int(words[0]))
    struct.pack_into("<Q", b, 16, int(words[1]))
    b[24:24 + 624 * 8] = np.asarray(words[2:], np.uint32).astype(np.uint64).tobytes()
    gen.set_state(torch.frombuffer(bytearray(b), dtype=torch.uint8).clone())


def advance_words(w: np.ndarray, nwords: int) -> np.ndarray:
    """The [626] words of a generator `nwords` 32-bit draws after the state `w` (a new array), by
    MT19937 jump-ahead (uq_mt_jump_host) instead of drawing them."""
    if nwords < 0:
        raise ValueError("nwords must be >= 0")
    w = np.array(w, np.uint32)
    left, nxt = int(w[0]), int(w[1])
    rem = left - 1                                   # words left in the current block
    if nwords <= rem:
        w[0], w[1] = left - nwords, nxt + nwords
    else:
        after = nwords - rem                         # words read from the following blocks
        k = (after + 623) // 624                     # twists
        r = after - 624 * (k - 1)                    # words read from the last one (1..624)
        out = np.empty(624, np.uint32)
        key = np.ascontiguousarray(w[2:], np.uint32)
        _lib.check(_lib.load().uq_mt_jump_host(key.ctypes.data, k, out.ctypes.data), "uq_mt_jump_host")
        w[2:] = out
        w[0], w[1] = 625 - r, r
    return w


def advance_generator(gen: torch.Generator, nwords: int) -> None:
    """Leave the CPU generator where `nwords` 32-bit draws leave it -- torch.rand(nwords,
    generator=gen) on CPU takes one word per f32 element, so this stands for the D bernoulli(p_X)
    words of AS:489 -- by MT19937 jump-ahead (advance_words) instead of drawing them."""
    if nwords < 0:
        raise ValueError("nwords must be >= 0")
    st, w = generator_words(gen)
    set_generator_words(gen, st, advance_words(w, nwords))


def check_state(words: np.ndarray) -> None:
    left, nxt = int(words[0]), int(words[1])
    if not 1 <= left <= 624 or (left > 1 and nxt != 625 - left):
        raise ValueError("generator state with left/next outside ATen mt19937's invariant")


def pack_generators(n: int, px_states, px_seeds, who: str = "client"):
    """The n generators of a batch call as int32 words for the device -> (words, is_states):
    px_states [n, 626] checked and flattened, else the low 32 bits of the n px_seeds."""
    if px_states is not None:
        w = np.ascontiguousarray(np.asarray(px_states, np.uint32).reshape(n, STATE_WORDS))
        for r in w:
            check_state(r)
        return w.view(np.int32).reshape(-1), True
    if px_seeds is None:
        raise ValueError("px_seeds or px_states is required")
    s = np.asarray(torch.as_tensor(px_seeds, dtype=torch.int64).reshape(-1).numpy(), np.int64)
    if s.size != n:
        raise ValueError(f"one px seed per {who}")
    return (s & 0xFFFFFFFF).astype(np.uint32).view(np.int32), False


def upload_generators(n: int, px_states, px_seeds, dev, who: str = "client", head=None):
    """pack_generators on the device in ONE host-to-device copy, behind the int32 array `head`
    when given (each pageable copy would otherwise wait for the stream on its own)
    -> (head or None, states [n, 626] or None, seeds [n] or None)."""
    tail, is_states = pack_generators(n, px_states, px_seeds, who)
    h = 0 if head is None else head.size
    din = torch.from_numpy(tail if head is None else np.concatenate([head, tail])).to(dev)
    tail_d = din[h:]
    return (None if head is None else din[:h], tail_d.view(n, STATE_WORDS) if is_states else None,
            None if is_states else tail_d)
