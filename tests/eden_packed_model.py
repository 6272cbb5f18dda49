"""Test infrastructure: the bit-packed form of an EDEN message (include/uq_dme.h) in NumPy.

A client's payload is a row of u32 words; coordinate i is bit i % 32 of word i / 32 of a plane, P = ceil(D / 32)
words per plane.  Plane H (words [0, P)): the bin at 1 bit, bin >> 1 at 2 bits, and at a fractional rate bin >> 1
where the client's mask bit is set and the 1-bit bin where it is clear.  Plane L: none at 1 bit; words [P, 2 P) =
bin & 1 at 2 bits; at a fractional rate the low bits of the mask-set coordinates only, compacted in index order.
Every bit that names no coordinate is 0.  kind: 1, 2 or FRAC; mask: bool [D] (FRAC only).
"""
from __future__ import annotations

import numpy as np

FRAC = 12                      # UQ_EDEN_NBITS_FRAC


def words(D: int) -> int:
    return -(-D // 32)


def pitch(D: int, kind: int) -> int:
    return words(D) if kind == 1 else 2 * words(D)


def plane(bits: np.ndarray, nwords: int) -> np.ndarray:
    """bool / 0-1 array -> uint32 [nwords], bit k % 32 of word k / 32, zero past the array"""
    pad = np.zeros(nwords * 32, np.uint8)
    pad[:bits.shape[0]] = bits
    return np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def unplane(w: np.ndarray, count: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(w.astype("<u4")).view(np.uint8), bitorder="little")[:count]


def pack(bins: np.ndarray, kind: int, mask: np.ndarray = None):
    """(payload uint32 [pitch], payload_bits) of one client's bins u8 [D]"""
    bins = np.asarray(bins).astype(np.uint8)
    D = bins.shape[0]
    P = words(D)
    if kind == 1:
        return plane(bins & 1, P), D
    if kind == 2:
        return np.concatenate([plane(bins >> 1, P), plane(bins & 1, P)]), 2 * D
    m = np.asarray(mask, bool)
    assert kind == FRAC and m.shape == (D,)
    high = np.where(m, bins >> 1, bins & 1)
    low = (bins & 1)[m]                                  # the mask-set coordinates in index order
    return np.concatenate([plane(high, P), plane(low, P)]), D + int(m.sum())


def unpack(payload: np.ndarray, D: int, kind: int, mask: np.ndarray = None) -> np.ndarray:
    """bins u8 [D]: 0..3 where the table is the 2-bit one, 0..1 elsewhere"""
    P = words(D)
    payload = np.asarray(payload).view(np.uint32)
    assert payload.shape == (pitch(D, kind),)
    h = unplane(payload[:P], D)
    if kind == 1:
        return h.astype(np.uint8)
    if kind == 2:
        return ((h << 1) | unplane(payload[P:], D)).astype(np.uint8)
    m = np.asarray(mask, bool)
    out = h.astype(np.uint8)
    out[m] = (h[m] << 1) | unplane(payload[P:], int(m.sum()))
    return out


def ranks(mask_row_words: np.ndarray, D: int) -> np.ndarray:
    """uint32 [P + 1]: the set bits of mask[:D] before each word, then their count"""
    m = unplane(np.asarray(mask_row_words).view(np.uint32), D)
    pad = np.zeros(words(D) * 32, np.int64)
    pad[:D] = m
    return np.concatenate([[0], np.cumsum(pad.reshape(-1, 32).sum(axis=1))]).astype(np.uint32)


def unused_bits_zero(payload: np.ndarray, D: int, kind: int, cnt: int = 0) -> bool:
    """every bit that names no coordinate is 0"""
    P = words(D)
    payload = np.asarray(payload).view(np.uint32)
    ok = not unplane(payload[:P], P * 32)[D:].any()
    if kind == 2:
        ok = ok and not unplane(payload[P:], P * 32)[D:].any()
    if kind == FRAC:
        ok = ok and not unplane(payload[P:], P * 32)[cnt:].any()
    return bool(ok)
