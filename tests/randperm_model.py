"""NumPy models of torch.randperm(D)[:k] on the CPU generator, for D < 2^32 / 20.

torch's CPU randperm is a forward Fisher-Yates shuffle: step i = 0 .. D - 2 swaps r[i] with
r[i + w_i % (D - i)], w_i the i-th 32-bit word of the generator; it takes D - 1 words whatever
the prefix.  The first k entries are final after the first K = min(k, D - 1) steps.

  serial(words, D, k)     the shuffle itself, the first K steps
  parallel(words, D, k)   the same prefix without the serial chain, the form the GPU kernels take:
        h_i      = i + w_i % (D - i), the position step i swaps with (h_{D-1} = D - 1 when k = D)
        W(p, i)  = the largest step j < i with h_j = p, or none
        par(j)   = W(j, j);  root(j) follows par until there is none (par(j) < j: it ends)
        r[i]     = root(i) if h_i = i, else with q = W(h_i, i): h_i if q is none, else root(q)
     root(j) is the value at position j when step j begins: j itself unless an earlier step wrote
     there, and the last such step q wrote what position q held when it began, root(q).

A generator state is the oracle's (left, next, words[624]) (oracle/uq_quicfl.py).
"""
from __future__ import annotations

import numpy as np

from oracle.uq_quicfl import mt_draw, seeded_state, torch_state_pack, torch_state_unpack  # noqa: F401

MAX_D = (1 << 32) // 20            # torch switches to another algorithm from here on


def steps(D: int, k: int) -> int:
    """Shuffle steps (= generator words) that the prefix of length k depends on."""
    return max(0, min(int(k), int(D) - 1))


def words_taken(D: int) -> int:
    """Generator words one torch.randperm(D) takes."""
    return max(0, int(D) - 1)


def targets(words, D: int, k: int) -> np.ndarray:
    """h_i for i < k as int64 (the virtual step D - 1 hits itself)."""
    K = steps(D, k)
    i = np.arange(K, dtype=np.int64)
    h = i + np.asarray(words[:K], np.uint32).astype(np.int64) % (D - i)
    if k == D and D >= 1:
        h = np.concatenate([h, np.array([D - 1], np.int64)])
    return h


def serial(words, D: int, k: int) -> np.ndarray:
    K = steps(D, k)
    r = np.arange(D, dtype=np.int64)
    w = np.asarray(words[:K], np.uint32).astype(np.int64)
    for i in range(K):
        j = i + int(w[i]) % (D - i)
        r[i], r[j] = r[j], r[i]
    return r[:k].copy()


def parallel(words, D: int, k: int) -> np.ndarray:
    h = targets(words, D, k)
    n = h.shape[0]                                   # = k
    if n == 0:
        return np.zeros(0, np.int64)
    idx = np.arange(n, dtype=np.int64)
    # the writers of each position in ascending step order: a stable sort by target
    order = np.lexsort((idx, h))
    hs = h[order]
    same = np.concatenate([[False], hs[1:] == hs[:-1]])
    q = np.full(n, -1, np.int64)                     # q[i] = W(h_i, i): the previous step with the same target
    q[order[same]] = order[np.flatnonzero(same) - 1]
    # par(j) = W(j, j): the last step below j that hit position j (a self-hit is step j itself: never below)
    last = np.full(n, -1, np.int64)
    hit = (h < n) & (h != idx)
    np.maximum.at(last, h[hit], idx[hit])
    root = np.where(last >= 0, last, idx)
    for _ in range(max(1, int(n).bit_length())):     # pointer doubling: at most ceil(log2 n) rounds
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    out = np.where(h == idx, root, np.where(q < 0, h, root[np.maximum(q, 0)]))
    return out.astype(np.int64)


def randperm_prefix(state, D: int, k: int):
    """-> (torch.randperm(D)[:k] from `state`, the state after its D - 1 words)."""
    w, after = mt_draw(state, words_taken(D))
    return parallel(w, D, k), after


def drop_bits(index, D: int) -> np.ndarray:
    """The index set as uint32 [ceil(D / 32)]: bit i % 32 of word i // 32 (uq_rht_sign_bits' numbering)."""
    bits = np.zeros((D + 31) // 32, np.uint32)
    index = np.asarray(index, np.int64)
    np.bitwise_or.at(bits, index >> 5, (np.uint32(1) << (index & 31).astype(np.uint32)))
    return bits


WALK, JUMP = 1, 2                 # UQ_RANDPERM_FORM_*
WALK_BLOCKS = 16                   # streams of up to this many MT19937 blocks: one wave per client walks them
RUN_BLOCKS = 16                    # jump form: blocks per run at least
MAX_RUNS = 1024                    # ... and runs per client at most
RUN_WAVES = 4096                   # ... and about this many run waves per call
WORKSPACE_CAP = 1 << 30            # uq_randperm_prefix_workspace_bytes asks for no more (one client aside)
MAX_GROUP = 65535                  # one grid row per client of a group
JUMP_X = 33 * 624                  # stream words the jump kernel keeps per client
JUMP_PARTS = 4                     # partial windows per jumped block


def plan(n: int, D: int, k: int):
    """-> (form, runs, run_blocks, K) of the words stage of uq_randperm_prefix(n, D, k) from generator states:
    the K = min(k, D - 1) words of a stream that may start anywhere in its first block touch B blocks at
    most; up to 16 blocks one wave walks them (one run of B blocks), else runs of L blocks from jumped
    states, L = max(16, ceil(B / 1024), min(ceil(n B / 4096), B)).  (0, 0, 0, 0) when nothing runs."""
    n, D, k = int(n), int(D), int(k)
    if n < 1 or k < 1:
        return 0, 0, 0, 0
    K = min(k, D - 1)
    B = (624 + K - 1) // 624 + 1
    if B <= WALK_BLOCKS:
        return WALK, 1, B, K
    per = -(-n * B // RUN_WAVES)
    L = max(RUN_BLOCKS, -(-B // MAX_RUNS), min(per, B))
    return JUMP, -(-B // L), L, K


def workspace_bytes(n: int, D: int, k: int, G: int) -> int:
    """Bytes of the workspace of a group of G clients under plan(n, D, k): 512 bytes of control block and round
    flags, then h [G, K], next [G, k], a [G, k], head [G, D] (4-byte entries) and, in the jump form, the stream
    words [G, 33 * 624] and the partial windows [G, runs, 4, 624]; every array rounded up to 256 bytes."""
    form, R, _, K = plan(n, D, k)
    up = lambda b: -(-b // 256) * 256                                 # noqa: E731
    jump = form == JUMP
    return 512 + up(G * K * 4) + 2 * up(G * k * 4) + up(G * D * 4) + up(G * JUMP_X * 4 if jump else 0) \
        + up(G * R * JUMP_PARTS * 624 * 4 if jump else 0)


def group(n: int, D: int, k: int, nbytes: int) -> int:
    """Clients per group of a call with a workspace of `nbytes`: the most whose workspace fits (0: not one)."""
    lo, hi = 0, min(int(n), MAX_GROUP)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if workspace_bytes(n, D, k, mid) <= nbytes:
            lo = mid
        else:
            hi = mid - 1
    return lo


def adversarial(kind: str, D: int, K: int) -> np.ndarray:
    """K words whose targets are the hard cases: 'zero' z = 0 (every step hits itself), 'last' every step
    hits position D - 1 (one writer list of length K), 'chain' z_i = 1 but z_{K-1} = 0 (K - 1 links)."""
    i = np.arange(K, dtype=np.int64)
    if kind == "zero":
        z = np.zeros(K, np.int64)
    elif kind == "last":
        z = D - 1 - i
    elif kind == "chain":
        z = np.ones(K, np.int64)
        z[K - 1:] = 0
        z = np.minimum(z, D - 1 - i)
    else:
        raise ValueError(kind)
    # a word with w % (D - i) = z: z itself (z < D - i <= D < 2^32 / 20), plus a multiple of the modulus so
    # that the words are not small numbers
    m = D - i
    mult = ((1 << 32) - 1 - z) // m
    return (z + (mult // 2) * m).astype(np.uint64).astype(np.uint32)
