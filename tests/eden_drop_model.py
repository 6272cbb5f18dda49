"""NumPy model of EDEN with the receiver's coordinate drop (AS:398-426), from pieces that are pinned
elsewhere: the EDEN oracle (oracle/uq_eden.py) and its fractional-rate model (tests/eden_frac_model.py), the
MT19937 stream (oracle/uq_quicfl.mt_draw), the permutation prefix (tests/randperm_model.py) and torch's own
f32 division for AS:423.  tests/test_eden_drop_model.py pins it to the reference's outputs
(tests/golden/eden_drop.*); the GPU tests compare the kernels with those fixtures.

A generator state is the oracle's (left, next, words[624])."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import torch

from oracle import uq_eden as E
from tests import eden_frac_model as F
from tests import randperm_model as R

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NSAMPLE = 4096


def load():
    with open(os.path.join(GOLDEN, "eden_drop.json")) as f:
        meta = json.load(f)
    z = dict(np.load(os.path.join(GOLDEN, "eden_drop.npz")))
    for d in sorted({c["d"] for c in meta["cases"] if c["d"] >= 65536}):
        z.update(np.load(os.path.join(GOLDEN, f"eden_drop_outs_d{d}.npz")))
    return meta["cases"], z


def sample_pos(idx, dim):
    return np.random.default_rng(idx).choice(dim, NSAMPLE, replace=False).astype(np.int64)


def spelled(c):
    """(bits, pdrop) of the case in the library's spelling: a rate r below 1 is bits 1 with the total drop
    share the reference computes (AS:413-417), in the same double operations."""
    nbits, pdrop = c["nbits"], c["pdrop"]
    if nbits >= 1:
        return nbits, pdrop
    p = 1 - nbits
    if pdrop > 0:
        p += (1 - p) * pdrop
    return 1, p


def start_state(c):
    """The global generator when the call begins: manual_seed(gseed), then `pre` one-word draws."""
    return R.mt_draw(R.seeded_state(c["gseed"]), c["pre"])[1]


def state_sha(gseed: int, state) -> str:
    """sha256 of torch's get_state() bytes of a CPU generator seeded with gseed that stands at `state`."""
    g = torch.Generator()
    g.manual_seed(gseed)
    packed = R.torch_state_pack(g.get_state().numpy(), state)
    return hashlib.sha256(packed.tobytes()).hexdigest()


def rotated(bins, nb, seed):
    """take(centroids, bins) as the receiver reads a message (AS:399-411)."""
    bins = np.asarray(bins).astype(np.int64)
    if isinstance(nb, tuple):
        m = F.mask(seed, bins.shape[0], nb[2])
        return np.where(m, E.centroids(2)[bins], E.centroids(1)[np.minimum(bins, 1)]).astype(f32)
    return E.centroids(nb)[bins].astype(f32)


def decompress(bins, scale, nb, seed, dim, p, state):
    """AS:398-426 -> (out f32 [dim], the generator state after, the dropped coordinates)."""
    vec = rotated(bins, nb, seed)
    idx = np.zeros(0, np.int64)
    if p > 0:
        D = vec.shape[0]
        idx, state = R.randperm_prefix(state, D, round(D * p))             # AS:420-421
        vec[idx] = 0
        t = torch.from_numpy(vec)
        t /= (1 - p)                                                       # AS:423, torch's own division
        vec = t.numpy()
    return (f32(scale) * E.inverse_rht(vec, seed)).astype(f32)[:dim], state, idx


def wrapper_call(x, bits, pdrop, state):
    """One reference wrapper call with a drop from `state` -> (out, state after, seed, bins, scale)."""
    w, state = R.mt_draw(state, 1)
    seed = int(w[0]) % 100                                                 # AS:800 torch.randint(0, 100)
    if isinstance(bits, float) and 1 < bits < 2:
        bins, scale, nb = F.compress(x, bits, seed)
    else:
        nb = int(bits)
        bins, scale, _, _ = E.eden_compress(x, nb, seed)
    out, state, _ = decompress(bins, scale, nb, seed, x.shape[0], pdrop, state)
    return out, state, seed, np.asarray(bins).astype(np.uint8), scale
