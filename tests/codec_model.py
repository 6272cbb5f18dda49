"""A plain numpy model of the UQR1 type-message format, written from the format text at the
top of oracle/uq_codec.c (not from the HIP kernels, and not from the C functions below that
text).  Test infrastructure: tests/test_codec_model.py pins it to the C oracle byte for
byte, tests/test_gpu_codec_stress.py uses it as the third voice between the GPU codec and
the oracle, to write messages with tables the project's own encoder never chooses, and to
prove (words_per_group) that a synthetic input reaches the load a test claims.

All chunks advance together: x is [nchunks, W], one numpy step per coder step (<= 1024),
whatever d is.
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"UQR1"
PROB_BITS = 12
M = 1 << PROB_BITS
L = 1 << 16
STEPS = 1024
GROUP = 4                     # steps per group of the GPU kernels' full-chunk paths


def lanes(d: int) -> int:
    return min(64, max(1, -(-d // STEPS)))


def nchunks(d: int) -> int:
    return -(-d // (lanes(d) * STEPS)) if d > 0 else 0


def _align4(x: int) -> int:
    return (x + 3) & ~3


def header_bytes(nsym: int, nch: int, W: int) -> int:
    return _align4(40 + 2 * nsym) + 4 * nch + 4 * nch * W


def code_sym(codes, exact: bool) -> np.ndarray:
    """s = 2k + neg; in value mode the sign of a zero count is dropped."""
    c = np.asarray(codes, np.int8).astype(np.int64)
    k = np.where(c < 0, -c - 1, c)
    neg = c < 0
    return 2 * k + (neg if exact else (neg & (k > 0)))


def sym_code(syms) -> np.ndarray:
    s = np.asarray(syms, np.int64)
    return np.where(s & 1, -(s >> 1) - 1, s >> 1).astype(np.int8)


def normalize(cnt, total: int):
    """Quantized frequencies (sum M) and the number of adjustment rounds: f = max(1,
    cnt * M // total) for present symbols; a shortfall goes to the most frequent symbol
    (lowest index on ties); an excess is taken from the most frequent symbols in turn,
    never below 1."""
    cnt = np.asarray(cnt, np.int64)
    f = np.where(cnt > 0, np.maximum(1, cnt * M // max(1, total)), 0)
    rounds = 0
    if f.sum() == 0:
        return f, rounds
    while f.sum() != M:
        best = int(np.argmax(f))                       # first of the largest
        over = int(f.sum()) - M
        f[best] -= min(over, int(f[best]) - 1) if over > 0 else over
        rounds += 1
    return f, rounds


def _table(codes, exact, freqs, nsym):
    sy = code_sym(codes, exact)
    d = sy.shape[0]
    if freqs is None:
        kmax = int((sy >> 1).max()) if d else 0
        nsym = 2 * kmax + 2 if d else 0
        f, rounds = normalize(np.bincount(sy, minlength=nsym)[:nsym], d)
    else:
        f = np.asarray(freqs, np.int64)
        assert nsym is not None and f.shape[0] == nsym and 0 <= nsym <= 256
        assert d == 0 or (int(f.sum()) == M and sy.max() < nsym and (f[sy] >= 1).all())
        rounds = 0
    return sy, f, int(nsym), rounds


def _chunks(sy, f):
    """rANS over all chunks at once.  Returns (need [nch, steps, W] bool, low [nch, steps, W]
    u16, states [nch, W]): lane l of chunk c emits low[c, j, l] at step j where need is set."""
    d = sy.shape[0]
    W, nch = lanes(d), nchunks(d)
    csz = W * STEPS
    pad = np.zeros(nch * csz, np.int64)
    pad[:d] = sy
    act = np.zeros(nch * csz, bool)
    act[:d] = True
    pad = pad.reshape(nch, STEPS, W)                   # symbol i: step i // W, lane i % W
    act = act.reshape(nch, STEPS, W)
    cum = np.concatenate([[0], np.cumsum(f)]).astype(np.int64)
    fq = f.astype(np.int64)
    x = np.full((nch, W), L, np.int64)
    need = np.zeros((nch, STEPS, W), bool)
    low = np.zeros((nch, STEPS, W), np.uint16)
    for j in range(STEPS - 1, -1, -1):                 # the encoder runs the steps in reverse
        a = act[:, j]
        if not a.any():
            continue
        fs = np.where(a, fq[pad[:, j]], 1)
        nd = a & (x >= (fs << 20))                     # x_max = (L >> 12 << 16) * f
        need[:, j] = nd
        low[:, j] = (x & 0xFFFF).astype(np.uint16)
        x = np.where(nd, x >> 16, x)
        x = np.where(a, ((x // fs) << PROB_BITS) + (x % fs) + cum[pad[:, j]], x)
    return need, low, x


def encode(codes, m: int, l1, exact: bool, freqs=None, nsym=None) -> bytes:
    """One client's int8 codes -> a UQR1 message.  freqs=None: the normalisation rule;
    otherwise the caller's table (sum 4096, every used symbol >= 1) and nsym (may be odd)."""
    sy, f, nsym, _ = _table(codes, exact, freqs, nsym)
    d = sy.shape[0]
    W, nch = lanes(d), nchunks(d)
    need, low, x = _chunks(sy, f)
    words = low[need]                                  # chunk, then step, then lane
    wend = np.cumsum(need.sum(axis=(1, 2))).astype("<u4")
    nw = int(words.shape[0])
    hdr = (struct.pack("<4sHHQQ", MAGIC, 1, 1 if exact else 0, d, int(m)) + np.float32(l1).astype("<f4").tobytes() +
           struct.pack("<HBBII", nsym, PROB_BITS, W, nch, header_bytes(nsym, nch, W) + _align4(2 * nw)))
    tab = f.astype("<u2").tobytes()
    tab += bytes(_align4(40 + 2 * nsym) - 40 - 2 * nsym)
    body = wend.tobytes() + x.astype("<u4").tobytes() + words.astype("<u2").tobytes()
    return hdr + tab + body + bytes(_align4(2 * nw) - 2 * nw)


def words_per_group(codes, exact: bool, freqs=None, nsym=None) -> np.ndarray:
    """[nchunks, 1024 / 4]: renormalisation words of each group of 4 steps, per chunk."""
    sy, f, _, _ = _table(codes, exact, freqs, nsym)
    need, _, _ = _chunks(sy, f)
    return need.reshape(need.shape[0], STEPS // GROUP, -1).sum(axis=2)


def table_of(codes, exact: bool):
    """(f [nsym], nsym, normalisation rounds) the encoder chooses for these codes."""
    _, f, nsym, rounds = _table(codes, exact, None, None)
    return f, nsym, rounds


def parse(msg: bytes) -> dict:
    """Section offsets and fields of a well-formed message (for tests that corrupt one)."""
    magic, ver, flags, d, m, _, nsym, pb, W, nch, total = struct.unpack_from("<4sHHQQfHBBII", msg, 0)
    l1 = np.frombuffer(msg, "<f4", 1, 24)[0]
    wend = _align4(40 + 2 * nsym)
    return dict(d=d, m=m, l1=np.float32(l1), flags=flags, nsym=nsym, W=W, nch=nch, total=total, table=40, wend=wend,
                states=wend + 4 * nch, words=header_bytes(nsym, nch, W),
                f=np.frombuffer(msg, "<u2", nsym, 40).astype(np.int64),
                words_end=np.frombuffer(msg, "<u4", nch, wend).astype(np.int64))


def decode(msg: bytes, d: int):
    """UQR1 message -> (codes int8 [d], l1 f32, m); ValueError where the oracle refuses."""
    size = len(msg)
    if size < 40:
        raise ValueError("short header")
    magic, ver, _, dd, m, _, nsym, pb, W, nch, total = struct.unpack_from("<4sHHQQfHBBII", msg, 0)
    l1 = np.frombuffer(msg, "<f4", 1, 24)[0]
    if magic != MAGIC or ver != 1 or pb != PROB_BITS or dd != d or total != size:
        raise ValueError("bad header")
    if W != lanes(d) or nch != nchunks(d) or nsym > 256 or (d > 0 and nsym < 2) or header_bytes(nsym, nch, W) > size:
        raise ValueError("bad header")
    f = np.frombuffer(msg, "<u2", nsym, 40).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(f)]).astype(np.int64)
    if d > 0 and int(cum[-1]) != M:
        raise ValueError("bad table")
    if d == 0:
        return np.zeros(0, np.int8), np.float32(l1), int(m)
    lut = np.repeat(np.arange(nsym), f.astype(np.int64))           # slot -> symbol
    off = _align4(40 + 2 * nsym)
    wend = np.frombuffer(msg, "<u4", nch, off).astype(np.int64)
    x = np.frombuffer(msg, "<u4", nch * W, off + 4 * nch).astype(np.int64).reshape(nch, W)
    words = np.frombuffer(msg, "<u2", (size - header_bytes(nsym, nch, W)) // 2, header_bytes(nsym, nch, W))
    if (wend > words.shape[0]).any():
        raise ValueError("words_end past the message")
    words = np.concatenate([words.astype(np.int64), np.zeros(1, np.int64)])
    csz = W * STEPS
    act = np.zeros(nch * csz, bool)
    act[:d] = True
    act = act.reshape(nch, STEPS, W)
    out = np.zeros((nch, STEPS, W), np.int64)
    r = np.concatenate([[0], wend[:-1]])
    for j in range(STEPS):
        a = act[:, j]
        if not a.any():
            break
        slot = x & (M - 1)
        s = lut[slot]
        out[:, j] = s
        x = np.where(a, f[s] * (x >> PROB_BITS) + slot - cum[s], x)
        nd = a & (x < L)
        k = nd.sum(axis=1)
        if (r + k > wend).any():
            raise ValueError("words overrun")
        idx = np.clip(r[:, None] + np.cumsum(nd, axis=1) - 1, 0, words.shape[0] - 1)
        x = np.where(nd, (x << 16) | words[idx], x)
        r = r + k
    if (r != wend).any():
        raise ValueError("words underrun")
    if (x != L).any():
        raise ValueError("final state")
    return sym_code(out.reshape(-1)[:d]), np.float32(l1), int(m)
