"""Synthetic int8 code batches for the UQR1 codec's stress tests (not a test file): the inputs
shared by tests/test_codec_model.py (model against the C oracle, on the CPU) and
tests/test_gpu_codec_stress.py (GPU codec against both).  Every batch comes from a seed;
natural quantizer output (80 % zeros, codes in -4..3) never looks like any of them.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import codec_model as M

CHUNK = 64 * M.STEPS          # symbols of a full chunk


def _i8(a):
    return np.ascontiguousarray(np.asarray(a, np.int64).astype(np.int8))


def uniform256(n, d, seed):
    """Every code equally likely: 8 bits per symbol, nsym = 256."""
    return _i8(np.random.default_rng(seed).integers(-128, 128, (n, d)))


def burst(n, d, at, seed):
    """All 0 but one run of the 254 codes other than 0 and -1, 31 times each, shuffled inside
    the run: each of them gets f = 1 (12 bits), the dominant symbol the rest."""
    rng = np.random.default_rng(seed)
    run = np.repeat(np.concatenate([np.arange(-128, -1), np.arange(1, 128)]), 31)
    c = np.zeros((n, d), np.int64)
    for j in range(n):
        c[j, at:at + run.shape[0]] = rng.permutation(run)
    return _i8(c)


def constant_rows(d):
    """Rows of one code each: 127, -128, -1 and 0 (f = 4096, no words)."""
    return _i8(np.repeat(np.array([127, -128, -1, 0])[:, None], d, axis=1))


def one_rare(n, d, seed):
    """All 0 but one coordinate 5 per row: f = 1 against 4095."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, d), np.int64)
    c[np.arange(n), rng.integers(0, d, n)] = 5
    return _i8(c)


FREQUENT = np.arange(-32, 32)                                    # 64 frequent codes (0 and -1 among them)
RARE = np.setdiff1d(np.arange(-128, 128), FREQUENT)              # 192 codes, once each


def multi_round(n, d, equal, seed):
    """192 codes once each and 64 codes sharing the rest (exactly equally if `equal`): the
    quantized frequencies overshoot 4096 by more than the largest one can give back."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        rest = d - RARE.shape[0]
        fill = (np.repeat(FREQUENT, rest // 64) if equal else rng.choice(FREQUENT, rest))
        assert fill.shape[0] == rest
        rows.append(rng.permutation(np.concatenate([RARE, fill])))
    return _i8(np.stack(rows))


def natural(n, d, seed):
    """The skew of quantizer output at R = 1: codes -4..3, P(0) = 0.8."""
    p = np.array([0.01, 0.02, 0.03, 0.05, 0.8, 0.05, 0.03, 0.01])
    return _i8(np.random.default_rng(seed).choice(np.arange(-4, 4), (n, d), p=p))


# name -> builder of the [n, d] batch.  n >= 2 with an odd d wherever the case allows it, so
# the second row is not 16-byte aligned.
STRESS = {}
for _d in (1, 63, 64, 65, 1023, 1024, 1025, 65535, 65536, 65537, 2 * CHUNK + 1000):
    STRESS[f"uniform256-{_d}"] = functools.partial(uniform256, 3 if _d < 1000 else 2, _d, 100 + _d)
for _name, _at in (("start", 0), ("end", CHUNK - 254 * 31), ("mid", 30000)):
    STRESS[f"burst-{_name}"] = functools.partial(burst, 2, CHUNK, _at, 200 + _at)
STRESS["single-65536"] = functools.partial(constant_rows, CHUNK)
STRESS["single-70001"] = functools.partial(constant_rows, 70001)
STRESS["one-rare-2^20"] = functools.partial(one_rare, 2, 1 << 20, 300)
STRESS["one-rare-3*2^18+1"] = functools.partial(one_rare, 2, 3 * (1 << 18) + 1, 301)
STRESS["multi-round-random"] = functools.partial(multi_round, 2, CHUNK, False, 400)
STRESS["multi-round-equal"] = functools.partial(multi_round, 2, CHUNK, True, 401)
STRESS["chunks-65+"] = functools.partial(natural, 1, 65 * CHUNK + 17, 500)


@functools.lru_cache(maxsize=None)
def stress(name):
    c = STRESS[name]()
    c.setflags(write=False)
    return c


def side(name, n):
    """(l1 [n] f32, m) sent along with a batch: arbitrary, only carried."""
    rng = np.random.default_rng(sum(map(ord, name)))
    return (rng.random(n) * 7 + 0.01).astype(np.float32), int(rng.integers(1, 1 << 40))


# Tables the project's encoder never writes: name -> (d, n, freqs, nsym, symbols used)
def _table_cases():
    t = {}
    f12 = np.ones(256, np.int64)
    f12[255] = 3841                                                # unused: every symbol costs 12 bits
    t["12bit-65536"] = (CHUNK, 2, f12, 256, np.arange(255))
    t["12bit-2*65536+5"] = (2 * CHUNK + 5, 2, f12, 256, np.arange(255))
    t["nsym3"] = (CHUNK + 1001, 2, np.array([1000, 96, 3000]), 3, np.arange(3))
    rng = np.random.default_rng(7)
    f255 = np.ones(255, np.int64) + np.bincount(rng.integers(0, 255, 4096 - 255), minlength=255)
    t["nsym255"] = (CHUNK + 1001, 2, f255, 255, np.arange(255))
    gap = np.zeros(40, np.int64)
    gap[[0, 7, 8, 30, 39]] = [5, 2000, 1, 90, 2000]
    t["gaps"] = (CHUNK + 1001, 2, gap, 40, np.array([0, 7, 8, 30, 39]))
    one = np.zeros(12, np.int64)
    one[9] = 4096
    t["f4096-at-9"] = (CHUNK + 1001, 2, one, 12, np.array([9]))
    return t


TABLES = _table_cases()


@functools.lru_cache(maxsize=None)
def table_case(name):
    """(codes [n, d], freqs, nsym, messages): symbols uniform over the used ones, written by
    the model with the exact-signs flag (every symbol index is then a code)."""
    d, n, f, nsym, used = TABLES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    codes = M.sym_code(rng.choice(used, (n, d)))
    l1, m = side(name, n)
    msgs = tuple(M.encode(codes[j], m, l1[j], True, freqs=f, nsym=nsym) for j in range(n))
    codes.setflags(write=False)
    return codes, f, nsym, msgs
