"""Test infrastructure: a NumPy f32 model of the client mean taken from type codes (include/uq_dme.h:
uq_codes_mean_form_f32 on int8 codes, uq_nibbles_q_mean_ld_f32 on 4-bit codes), written from the header's
text and not from the kernels' loops, and a generator of synthetic batches that does not run the quantizer.

    est[i] (+)= a_j[i] for clients j in order (f32 adds, from zero or from the given est), where client j adds
      its table entry  t_j[k] = RN(RN(RN(L1_j * k) / f32(m)) / n_div)     unbiased form
                       t_j[k] = RN(RN(L1_j * RN(k / f32(m))) / n_div)     biased form
      for a code of count k, negated for a sign code (byte 255 - k, nibble 15 - k), or
      RN(q_j[i] / n_div) when kmax_j is above the code's range (7 for nibbles, 127 for bytes) and q is given;
      without q (bytes only) such a client adds the entries of its saturated codes, the table built to 127.

Codes are held one per element as uint8 (the raw byte, or the nibble 0 .. 15); pack_nibbles puts element 2i in
the low nibble of byte i.
"""
import numpy as np

f32 = np.float32
UNBIASED, BIASED = 0, 1            # UQ_FORM_*
NIB_MAX, BYTE_MAX = 7, 127         # the largest count a nibble / a byte code carries


def table(l1, km: int, m: int, n_div, form: int) -> np.ndarray:
    """t[k] for k = 0 .. km, every product and quotient rounded to f32 on its own."""
    L, fm, nd = f32(l1), f32(m), f32(n_div)
    k = np.arange(km + 1, dtype=f32)
    with np.errstate(all="ignore"):
        if form == BIASED:
            v = (L * (k / fm).astype(f32)).astype(f32)
        else:
            v = ((L * k).astype(f32) / fm).astype(f32)
        return (v / nd).astype(f32)


def client_adds(codes, l1, kmax, m: int, n_div, form: int = UNBIASED, q=None, nibbles: bool = False) -> np.ndarray:
    """f32 [n, d]: what each client adds to est.  codes uint8 [n, d] (bytes, or nibble values when nibbles),
    q f32 [n, d] or None (rows of clients inside the code's range are never looked at)."""
    codes = np.asarray(codes, np.uint8)
    n, d = codes.shape
    top, cap = (15, NIB_MAX) if nibbles else (255, BYTE_MAX)
    if nibbles and q is None:
        raise ValueError("the mean from 4-bit codes needs q")
    out = np.empty((n, d), f32)
    for j in range(n):
        if int(kmax[j]) > cap and q is not None:
            with np.errstate(all="ignore"):
                out[j] = (np.asarray(q[j], f32) / f32(n_div)).astype(f32)
            continue
        km = min(cap, max(0, int(kmax[j])))
        c = codes[j].astype(np.int64)
        neg = c > top // 2
        k = np.where(neg, top - c, c)
        if int(k.max(initial=0)) > km:
            raise ValueError(f"client {j}: a count above its kmax")
        t = table(l1[j], km, m, n_div, form)
        out[j] = (t[k].view(np.uint32) ^ (neg.astype(np.uint32) << np.uint32(31))).view(f32)
    return out


def fold(adds, est=None) -> np.ndarray:
    """est (+)= the rows of `adds` in order, one f32 add each; from zero when est is None."""
    adds = np.asarray(adds, f32)
    e = np.zeros(adds.shape[1], f32) if est is None else np.array(est, f32)
    with np.errstate(all="ignore"):
        for a in adds:
            e = (e + a).astype(f32)
    return e


def mean(codes, l1, kmax, m: int, n_div, form: int = UNBIASED, q=None, est=None, nibbles: bool = False) -> np.ndarray:
    return fold(client_adds(codes, l1, kmax, m, n_div, form, q, nibbles), est)


def pack_nibbles(nib) -> np.ndarray:
    """uint8 [n, d] nibble values -> uint8 [n, d / 2]: element 2i in the low nibble of byte i."""
    nib = np.asarray(nib, np.uint8)
    assert nib.shape[1] % 2 == 0 and int(nib.max(initial=0)) <= 15
    return (nib[:, 0::2] | (nib[:, 1::2] << np.uint8(4))).astype(np.uint8)


def synthetic(rng, n: int, d: int, kmax_set, nibbles: bool = False, binades=(-6, 10)):
    """-> (codes uint8 [n, d], l1 f32 [n], kmax int32 [n]): per client kmax drawn from kmax_set (all inside the
    code's range), counts uniform in 0 .. kmax with at least one equal to kmax, random signs (negative zeros
    among them), L1 log-uniform over the binades, so that a table row taken from the wrong client shows."""
    top, cap = (15, NIB_MAX) if nibbles else (255, BYTE_MAX)
    kmax = rng.choice(np.asarray(kmax_set, np.int64), n)
    assert int(kmax.max()) <= cap and int(kmax.min()) >= 0
    k = np.floor(rng.random((n, d)) * (kmax[:, None] + 1)).astype(np.int64)
    k = np.minimum(k, kmax[:, None])
    k[np.arange(n), rng.integers(0, d, n)] = kmax
    neg = rng.random((n, d)) < 0.5
    codes = np.where(neg, top - k, k).astype(np.uint8)
    l1 = np.exp2(rng.uniform(binades[0], binades[1], n)).astype(f32)
    return codes, l1, kmax.astype(np.int32)


def overflowed(rng, rows: int, d: int, nibbles: bool = False, binades=(-20, 20)):
    """-> (q f32 [rows, d], codes uint8 [rows, d]) of clients above the code's range: arbitrary finite q (zeros of
    both signs among them) and random bytes (nibble values) as their codes."""
    q = (rng.standard_normal((rows, d)) * np.exp2(rng.uniform(binades[0], binades[1], (rows, d)))).astype(f32)
    z = rng.random((rows, d))
    q[z < 0.02] = f32(0.0)
    q[z < 0.01] = f32(-0.0)
    assert np.isfinite(q).all()
    codes = rng.integers(0, 16 if nibbles else 256, (rows, d)).astype(np.uint8)
    return q, codes
