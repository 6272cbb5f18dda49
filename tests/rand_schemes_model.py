"""NumPy restatement of the reference's Scalar_quantize (AS:755-790) and DRIVE_quantize_Hadamard
(AS:707-752) on torch CPU, from the oracle's blocks: the MT19937 stream (uq_quicfl.mt_draw),
torch's CPU sum (uq_oracle.torch_sum) and norm (uq_eden.torch_norm2).  Every step is one f32
operation.  tests/test_rand_schemes_oracle.py and tests/test_rand_edges_oracle.py pin it to the
reference's own outputs (tests/golden/rand_schemes_vectors.*, rand_schemes_edges.*); the GPU
tests compare the kernels with both.

A generator state is the oracle's (left, next, words[624]).
"""
from __future__ import annotations

import json
import os

import numpy as np

from oracle.uq_eden import torch_norm2
from oracle.uq_oracle import torch_sum
from oracle.uq_quicfl import mt_draw, seeded_state, torch_state_pack, torch_state_unpack  # noqa: F401

f32 = np.float32
CHUNK = 2048                                   # AS:712 batch_size
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def uniforms(words: np.ndarray) -> np.ndarray:
    """torch.rand_like on CPU: one word per element, u = f32(w & 0xFFFFFF) * 2^-24 (exact)."""
    return (words & np.uint32(0xFFFFFF)).astype(f32) * f32(2.0 ** -24)


def pow2ceil(L: int) -> int:
    p = 1
    while p < L:
        p <<= 1
    return p


def drive_words(d: int) -> int:
    """Generator words one DRIVE call takes: 2048 per whole chunk, the padded length of the last."""
    full, rem = divmod(int(d), CHUNK)
    return full * CHUNK + (pow2ceil(rem) if rem else 0)


def scalar_quantize(x, bits, state):
    """-> (out f32 [d], state after, words taken, constant).  `constant`: den == 0 (AS:763)."""
    x = np.asarray(x, f32)
    d = x.shape[0]
    with np.errstate(all="ignore"):
        nan = bool(np.isnan(x).any())
        mn = f32(np.nan) if nan else x.min()
        mx = f32(np.nan) if nan else x.max()
        den = f32(mx - mn)
        if den == 0:
            return x.copy(), state, 0, True
        nl = 2 ** bits - 1
        if nl < 1:                             # AS:772
            return x.copy(), state, 0, False
        nl = f32(nl)
        q = ((x - mn).astype(f32) / den).astype(f32)
        q = np.where(np.isnan(q), q, np.minimum(np.maximum(q, f32(0)), f32(1))).astype(f32)
        t = (q * nl).astype(f32)
        fl = np.floor(t).astype(f32)
        fr = (t - fl).astype(f32)
        words, state = mt_draw(state, d)
        b = (fl + (uniforms(words) < fr).astype(f32)).astype(f32)
        out = (((b / nl).astype(f32) * den).astype(f32) + mn).astype(f32)
    return out, state, d, False


def pair_steps(v: np.ndarray, k: int) -> np.ndarray:
    """AS:37-59 as it runs: its views alias, so each of its k stages maps every adjacent pair
    (a, b) to (s, s - b) with s = a + b; nothing crosses a pair."""
    v = np.asarray(v, f32).copy()
    for _ in range(k):
        s = (v[0::2] + v[1::2]).astype(f32)
        v[1::2] = (s - v[1::2]).astype(f32)
        v[0::2] = s
    return v


def drive_quantize(x, state, norm=torch_norm2):
    """-> (out f32 [d], state after, words taken, S f32 [chunks]).  `norm`: the chunk norm
    (AS:741), torch's order unless a test asks what another order would give."""
    x = np.asarray(x, f32)
    d = x.shape[0]
    out = np.empty(d, f32)
    S_all = []
    taken = 0
    with np.errstate(all="ignore"):
        for c0 in range(0, d, CHUNK):
            v = x[c0:c0 + CHUNK]
            L = v.shape[0]
            P = pow2ceil(L)
            k = P.bit_length() - 1
            vp = np.zeros(P, f32)
            vp[:L] = v
            words, state = mt_draw(state, P)
            taken += P
            D = np.where(uniforms(words) > f32(0.5), f32(1), f32(-1)).astype(f32)
            Rx = pair_steps((D * vp).astype(f32), k)
            nrm = norm(v)
            S = f32(f32(nrm * nrm) / f32(torch_sum(np.abs(Rx)) + f32(1e-12)))
            sg = (Rx > 0).astype(f32) - (Rx < 0).astype(f32)          # torch.sign: +0 at +-0
            Rh = (S * sg).astype(f32)
            o = (pair_steps(Rh, k) * D).astype(f32)
            out[c0:c0 + L] = o[:L]
            S_all.append(S)
    return out, state, taken, np.asarray(S_all, f32)


# ---- the fixture (tests/golden/make_golden_rand_schemes.py) -----------------------------------
def gen_input(c) -> np.ndarray:
    """A case's input: legacy RandomState draws (stable across numpy versions), then its edit."""
    rs = np.random.RandomState(c["vseed"])
    d, kind = c["d"], c["kind"]
    if kind == "normal":
        v = rs.normal(0, 1, d)
    elif kind == "lognormal":
        v = rs.lognormal(1, 2, d)
    elif kind == "constant":
        v = np.full(d, 1.25)
    elif kind == "zeros":
        v = np.zeros(d)
    elif kind == "nan":
        v = rs.normal(0, 1, d)
        v[d // 2] = np.nan
    elif kind == "inf":
        v = rs.normal(0, 1, d)
        v[d // 3] = np.inf
    elif kind == "zero_pairs":                 # zero pairs inside a live chunk
        v = rs.normal(0, 1, d)
        v[(np.arange(d) // 2) % 3 == 1] = 0.0
    # ---- the edge fixture's kinds (tests/golden/make_golden_rand_edges.py) ----
    elif kind == "nan_at":                     # one NaN at c["at"]
        v = rs.normal(0, 1, d)
        v[c["at"]] = np.nan
    elif kind == "ninf_at":                    # one -inf at c["at"]
        v = rs.normal(0, 1, d)
        v[c["at"]] = -np.inf
    elif kind == "pm_inf":                     # +inf and -inf together: max - min = inf
        v = rs.normal(0, 1, d)
        v[d // 3] = np.inf
        v[2 * d // 3] = -np.inf
    elif kind == "huge_span":                  # finite, max - min overflows
        v = rs.normal(0, 1, d)
        v[d // 4] = 3e38
        v[3 * d // 4] = -3e38
    elif kind == "subnormal":                  # every element subnormal in f32
        v = rs.normal(0, 1, d) * 1e-41
    elif kind == "normal_1e19":                # nrm * nrm overflows
        v = rs.normal(0, 1, d) * 1e19
    elif kind == "few_ulps":                   # a span of a few ulps of 1
        v = 1 + np.abs(rs.normal(0, 1, d)) * 1e-7
    elif kind == "neg_zero_third":             # -0.0 at every third element
        v = rs.normal(0, 1, d)
        v[::3] = -0.0
    else:
        raise ValueError(kind)
    return v.astype(f32)


def load_fixture(name="rand_schemes_vectors"):
    """(meta, npz) of rand_schemes_vectors, or of rand_schemes_edges (make_golden_rand_edges.py)."""
    meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return meta, z


def start_state(c):
    """The generator state a case starts from: manual_seed(gseed), then `pre` one-word draws
    (the fixture's torch.randint(0, 100, (1,)) calls)."""
    _, st = mt_draw(seeded_state(c["gseed"]), c["pre"])
    return st


def state_words(state) -> np.ndarray:
    """(left, next, words) as the [626] u32 the C entry points take."""
    w = np.empty(626, np.uint32)
    w[0], w[1] = state[0], state[1]
    w[2:] = state[2]
    return w
