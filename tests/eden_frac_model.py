"""Test infrastructure: EDEN at a fractional rate 1 < nbits < 2, restated in NumPy from the
functions oracle/uq_eden.py already has (AS = NMSE_Results/Codes/All_Schemes.py):

  AS:386-390  bits_l = 1, bits_h = 2, p_high = nbits - 1 (a Python double; the message carries
              nbits = (1, 2, p_high)), mask seed = seed * 7 + 13
  AS:352-368  EdenSender.stochastic_quantize: both bucketizes, mask = bernoulli(ones(D) * p_high)
              (an f32 tensor: the draw is f32(low24(w)) * 2^-24 < f32(p_high), one MT19937 word per
              coordinate), bins and centroids mixed by the mask, scale = norm ** 2 / dot(c, vec)
  AS:401-411  EdenReceiver.decompress: the same mask from the message, centroids by it

It stands in for the reference where a batch or an edge input is the subject; tests/golden/
eden_frac_vectors.* (made by the reference itself) pin it.
"""
from __future__ import annotations

import numpy as np

from oracle import uq_eden as E

f32 = np.float32


def p_high(nbits) -> float:
    return float(nbits) - 1.0


def threshold(p: float) -> int:
    """low24(w) < threshold  <=>  f32(low24(w)) * 2^-24 < f32(p)"""
    return int(np.ceil(float(f32(p)) * float(1 << 24)))


def mask(seed: int, D: int, p: float) -> np.ndarray:
    """AS:360-361 / AS:402-406: bool [D], seeded with the low 32 bits of 7 * seed + 13."""
    w = E.mt19937((7 * int(seed) + 13) & 0xFFFFFFFFFFFFFFFF, D)
    return ((w & np.uint32(0xFFFFFF)).astype(f32) * f32(2.0 ** -24)) < f32(p)


def mask_bits(seed: int, D: int, p: float) -> np.ndarray:
    """The mask as the library's rows: uint32 [ceil(D / 32)], bit k % 32 of word k / 32."""
    m = mask(seed, D, p)
    pad = np.zeros(-(-D // 32) * 32, np.uint8)
    pad[:D] = m
    return np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def compress(x: np.ndarray, nbits, seed: int):
    """(bins u8 [D], scale f32, message nbits tuple)"""
    p = p_high(nbits)
    vec = E.rht(np.asarray(x, f32), seed)
    D = vec.shape[0]
    nrm = E.torch_norm2(vec)
    with np.errstate(divide="ignore", invalid="ignore"):
        nv = ((vec * f32(np.sqrt(D))).astype(f32) / nrm).astype(f32)
    nan = np.isnan(nv)
    b_lo = np.where(nan, 1, E.bucketize(nv, E.boundaries(1)))       # NaN: each table's last bin
    b_hi = np.where(nan, 3, E.bucketize(nv, E.boundaries(2)))
    m = mask(seed, D, p)
    bins = np.where(m, b_hi, b_lo)
    c = np.where(m, E.centroids(2)[b_hi], E.centroids(1)[b_lo]).astype(f32)
    dot = E.torch_dot(c, vec)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = f32(f32(nrm * nrm) / dot)
    return bins.astype(np.uint8), scale, (1, 2, p)


def decompress(bins: np.ndarray, scale, nbits_tuple, seed: int, dim: int) -> np.ndarray:
    bins = np.asarray(bins).astype(np.int64)
    m = mask(seed, bins.shape[0], nbits_tuple[2])
    v = np.where(m, E.centroids(2)[bins], E.centroids(1)[np.minimum(bins, 1)]).astype(f32)
    return (f32(scale) * E.inverse_rht(v, seed)).astype(f32)[:dim]


def quantize(x: np.ndarray, nbits, seed: int):
    """(out f32 [d], bins, scale)"""
    x = np.asarray(x, f32)
    bins, scale, t = compress(x, nbits, seed)
    return decompress(bins, scale, t, seed, x.shape[0]), bins, scale
