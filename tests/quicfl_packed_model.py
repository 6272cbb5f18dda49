"""NumPy model of the packed QUIC-FL message (include/uq_dme.h, "QUIC-FL messages at their rate"), one row at a
time: X as nbits planes of P = ceil(D / 32) u32 words (bit i % 32 of word i / 32 of plane b is bit b of X_i, every
other bit 0), the exact coordinates as an ascending int32 index list, payload_bits = nbits D + 64 count."""
import numpy as np


def words(D):
    return (D + 31) // 32


def pitch(D, nbits):
    return nbits * words(D)


def pack(X, nbits, mask=None):
    """X [D] integers in [0, 2^nbits), mask [D] bool or None -> (payload [nbits P] u32, index list int32, bits)"""
    X = np.asarray(X).astype(np.int64)
    D = X.shape[0]
    assert ((X >= 0) & (X < (1 << nbits))).all()
    P = words(D)
    pay = np.zeros(nbits * P, np.uint32)
    for b in range(nbits):
        bits = np.zeros(32 * P, np.uint64)
        bits[:D] = (X >> b) & 1
        pay[b * P:(b + 1) * P] = (bits.reshape(P, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    idx = np.flatnonzero(mask).astype(np.int32) if mask is not None else np.zeros(0, np.int32)
    return pay, idx, nbits * D + 64 * idx.size


def unpack(pay, D, nbits, idx=None):
    """-> (X [D] u8, mask [D] bool)"""
    pay = np.asarray(pay, np.uint32)
    P = words(D)
    assert pay.shape == (nbits * P,)
    X = np.zeros(D, np.uint8)
    i = np.arange(D)
    for b in range(nbits):
        X |= (((pay[b * P + i // 32] >> (i % 32).astype(np.uint32)) & 1) << b).astype(np.uint8)
    mask = np.zeros(D, bool)
    if idx is not None:
        mask[np.asarray(idx, np.int64)] = True
    return X, mask


def unused_bits_zero(pay, D, nbits):
    P = words(D)
    if D % 32 == 0:
        return True
    return all(int(pay[b * P + P - 1]) >> (D % 32) == 0 for b in range(nbits))
