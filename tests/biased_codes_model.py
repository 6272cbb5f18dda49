"""Test infrastructure: a numpy restatement of the type codes' two dequantize forms and of the
recovery of the biased quantizer's codes from its float output.

    code -> q     unbiased  q = +-RN(RN(L1 * k) / f32(m))              (AS:640)
                  biased    q = (L1 * s) * RN(k / f32(m)), s = +-1     (AS:687)
    with k = code for code >= 0 and -code-1 for code < 0 (s = -1).

    (x, q, L1, m) -> codes of the biased form, for a client with finite L1 > 0 and m >= 1:
    k = rint(|q| * m / L1) in fp64, the sign from x, and code 0 where x == 0 (sign 0: the output is
    +0.0 whatever k'' the coordinate had).  The counts are returned unclipped (int64), so a caller
    sees whether they fit an int8 code.
"""
import numpy as np

from oracle import uq_oracle_c as C
from oracle.uq_oracle import rate_to_m
from tests import golden_data as G

f32 = np.float32
UNBIASED, BIASED = 0, 1          # UQ_FORM_*


def counts(codes):
    """(k, negative) of int8-style codes (any integer dtype)."""
    c = np.asarray(codes).astype(np.int64)
    return np.where(c < 0, -c - 1, c), c < 0


def decode(codes, l1, m, form):
    """One client's codes -> q (f32), every product and quotient rounded to f32 on its own."""
    k, neg = counts(codes)
    L, fm, kf = f32(l1), f32(m), k.astype(f32)
    with np.errstate(all="ignore"):
        if form == BIASED:
            mag = (L * (kf / fm)).astype(f32)
        else:
            mag = ((L * kf).astype(f32) / fm).astype(f32)
    bits = mag.view(np.uint32) ^ (neg.astype(np.uint32) << np.uint32(31))
    return bits.view(f32)


def recover_codes(x, q, l1, m):
    """The biased form's codes of one client from its input x and float output q (int64, unclipped)."""
    x = np.asarray(x, f32)
    k = np.rint(np.abs(np.asarray(q, np.float64)) * float(m) / float(l1)).astype(np.int64)
    return np.where(x > 0, k, np.where(x < 0, -k - 1, 0))


def fits(codes):
    """Every count fits the int8 code."""
    k, _ = counts(codes)
    return bool(k.size == 0 or k.max() <= 127)


def qualifying_fixtures():
    """(spec, x, q, L1, m) of the reference fixtures whose output a biased TypeCodes can carry: the
    fixture has an output (the reference did not raise), m >= 1, L1 finite and > 0, and every
    count fits the int8 code."""
    C.build()
    for sp, x, q, _ in G.biased_vectors():
        if sp.get("raises") or q is None:
            continue
        m = rate_to_m(sp["R"], x.shape[0])
        if m < 1:
            continue
        with np.errstate(all="ignore"):
            try:
                _, l1, *_ = C.biased_quantize(x, m, sp["threads"], 0)
            except (ValueError, RuntimeError):
                continue
        if not np.isfinite(l1) or not l1 > 0:
            continue
        if not fits(recover_codes(x, q, l1, m)):
            continue
        yield sp, x, q, f32(l1), m
