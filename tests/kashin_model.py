"""NumPy f32 model of the reference's Kashin_quantize (AS = NMSE_Results/Codes/All_Schemes.py:
834-854 with 62-91, 95-156, 191-274), assembled from the oracle's pieces: the RHT and its
seeded diagonal (oracle/uq_eden.py), torch's norm order (oracle/uq_oracle_c.torch_norm2) and
xxh64 / ATen's mt19937 (oracle/uq_quicfl.py).  Test infrastructure only.

    kashin(x, bits, seed) -> dict(out, bins, mn, step, iters, raises)
        seed: the torch.randint(0, 100, (1,)) draw of the call; iters: forward transforms run.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import uq_eden as E
from oracle import uq_oracle_c as OC
from oracle import uq_quicfl as Q
from tests import golden_data as G

f32 = np.float32
ROTATION_SEED = 123            # AS:843
PAD_THRESHOLD = 0.85           # AS:245


def kashin_padded_dim(dim: int, pad_threshold: float = PAD_THRESHOLD) -> int:
    """AS:202-210."""
    if dim & (dim - 1) == 0:
        return 2 * dim
    D = 1 << (dim - 1).bit_length()
    return 2 * D if dim / D > pad_threshold else D


@functools.lru_cache(maxsize=8)
def _diag(D: int, seed: int) -> np.ndarray:
    return E.random_diagonal(D, seed)


def rht(v: np.ndarray, seed: int = ROTATION_SEED) -> np.ndarray:
    """uq_eden.rht of a row that is a power of two long already (the diagonal cached)."""
    return E.hadamard((v * _diag(v.shape[0], seed)).astype(f32))


def inverse_rht(v: np.ndarray, seed: int = ROTATION_SEED) -> np.ndarray:
    return (E.hadamard(v) * _diag(v.shape[0], seed)).astype(f32)


@functools.lru_cache(maxsize=4)
def normal_batch(seed: int, n: int, d: int) -> np.ndarray:
    """RandomState(seed).normal(size=(n, d)).astype(f32), read-only (shared between tests)."""
    x = np.random.RandomState(seed).normal(size=(n, d)).astype(f32)
    x.setflags(write=False)
    return x


def gen_input(c) -> np.ndarray:
    """A fixture case's input from its spec.  "normal" is RandomState(seed).normal(size=d).astype(f32)
    (golden_data.spec_gen's); "normal_f32" names that draw itself and "normal_row" row c["row"] of
    RandomState(seed).normal(size=(c["n"], d)).astype(f32) (tests/golden/kashin_edges.*)."""
    d, kind = c["d"], c["dist"]
    if kind == "normal_f32":
        return np.random.RandomState(c["seed"]).normal(size=d).astype(f32)
    if kind == "normal_row":
        return normal_batch(c["seed"], c["n"], d)[c["row"]].copy()
    if kind == "onehot":
        v = np.zeros(d, f32)
        v[c["seed"] % d] = f32(2.5)
        return v
    if kind == "constant":
        return np.full(d, f32(0.75), f32)
    if kind == "zeros":
        return np.zeros(d, f32)
    if kind in ("nan", "inf"):
        v = G.spec_gen({"seed": c["seed"], "d": d, "dist": "normal"})
        v[d // 3] = np.nan if kind == "nan" else np.inf
        return v
    return G.spec_gen(c)


def sample_positions(k: int, d: int, count: int = 4096) -> np.ndarray:
    """The positions at which tests/golden/kashin_edges.* keeps case k's long output."""
    return np.sort(np.random.RandomState(k).choice(d, count, replace=False))


def edge_fixture():
    """(cases, npz) of tests/golden/kashin_edges.* (make_golden_kashin_edges.py)."""
    import json
    import os
    cases = json.load(open(os.path.join(G.GOLDEN, "kashin_edges.json")))["cases"]
    return cases, np.load(os.path.join(G.GOLDEN, "kashin_edges.npz"))


def edge_expected(c, Z) -> dict:
    """A kashin_edges case's recorded results: ms = (min, step) and either out and bins (u16) in
    full or out_s at sample_positions with the sha256s in the case (`same_as` followed)."""
    k = c.get("same_as", c["idx"])
    e = {"ms": Z[f"ms{k}"]}
    if f"out{k}" in Z.files:
        e["out"], e["bins"] = Z[f"out{k}"], Z[f"bins{k}"]
    else:
        e["out_s"], e["pos"] = Z[f"out{k}_s"], sample_positions(k, c["x"]["d"])
    return e


def kashin(x, bits: int, seed: int, niters: int = 3, eta: float = 0.9, delta: float = 1.0, err: float = 1e-6):
    x = np.asarray(x, f32).reshape(-1)
    dim = x.shape[0]
    D = kashin_padded_dim(dim)
    nl = 2 ** bits
    c = np.zeros(D, f32)
    r = x.copy()
    with np.errstate(all="ignore"):
        M = f32(OC.torch_norm2(x) / f32(np.sqrt(delta * D)))                 # AS:220, one f32 division
        iters = 0
        for i in range(niters):
            p = np.zeros(D, f32)
            p[:dim] = r
            b = rht(p)                                                       # AS:222-224
            iters += 1
            b_hat = np.minimum(np.maximum(b, -M), M).astype(f32)             # AS:227 (NaN propagates)
            c = (c + b_hat).astype(f32)                                      # AS:228
            if i < niters - 1:
                r = (r - inverse_rht(b_hat)[:dim]).astype(f32)               # AS:231-232
                M = f32(M * f32(eta))                                        # AS:233
            u = inverse_rht(c)[:dim]
            e = f32(OC.torch_norm2((x - u).astype(f32)) / OC.torch_norm2(r))  # AS:235
            if e < f32(err):                                                 # AS:236, compared in f32
                break
        mn, mx = c.min(), c.max()                                            # NaN propagates
        step = f32((mx - mn) / f32(nl - 1))                                  # AS:73
        q = ((c - mn) / step).astype(f32)                                    # AS:79
        fl = np.floor(q).astype(f32)
        pr = (q - fl).astype(f32)
        res = {"iters": iters, "mn": f32(mn), "step": step, "raises": False, "D": D}
        if not np.all((pr >= 0) & (pr <= 1)):                                # torch.bernoulli's check
            res["raises"] = True
            return res
        words, _ = Q.mt_draw(Q.seeded_state(Q.prng_seed(seed)), D)           # AS:68
        bins = (fl + ((words & 0xFFFFFF).astype(f32) * f32(2.0 ** -24) < pr).astype(f32)).astype(f32)   # AS:80
        deq = (mn + (bins * step).astype(f32)).astype(f32)                   # AS:91: multiply, then add
        res["bins"] = bins
        res["out"] = inverse_rht(deq)[:dim]                                  # AS:274
    return res
