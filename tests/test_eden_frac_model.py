"""EDEN at fractional rates, without a GPU: the NumPy model (tests/eden_frac_model.py) against the
reference's own outputs (tests/golden/eden_frac_vectors.*), the dispatch plan of a fractional call
on both sides of every threshold it crosses, and the new entry points' declarations."""
import ctypes
import json
import os

import numpy as np
import pytest

import uqdme
from tests import eden_frac_model as M
from tests import eden_plan_hook as H
from tests import golden_data as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAC = 12                      # UQ_EDEN_NBITS_FRAC
NFIELDS = 25                   # UQ_EDEN_PLAN_FIELDS


def load_fixture():
    with open(os.path.join(GOLD, "eden_frac_vectors.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLD, "eden_frac_vectors.npz"))


META, Z = load_fixture()
_OUTS = {}


def sampled(c):
    """(positions, the reference's outputs there) of a case longer than 1024, else None"""
    if c["d"] <= 1024:
        return None
    if c["d"] not in _OUTS:
        _OUTS[c["d"]] = np.load(os.path.join(GOLD, f"eden_frac_outs_d{c['d']}.npz"))
    return np.random.default_rng(c["idx"]).choice(c["d"], 4096, replace=False).astype(np.int64), _OUTS[c["d"]][f"outs{c['idx']}"]
DIMS = sorted({c["d"] for c in META["cases"]})


def bits_of(x):
    return int(np.float32(x).view(np.uint32))


def test_fixture_holds_the_cases():
    cases = META["cases"]
    assert {c["d"] for c in cases} == {1, 3, 5, 31, 33, 333, 623, 625, 1000, 1024, 4096, 5000, 8192, 16384, 65536,
                                       172554, 1 << 20}
    assert {c["nbits"] for c in cases} == {1.5, 1.25, 1.3, 1.999, 1.0000001}
    assert {c["rseed"] for c in cases} >= {0, 42, 99} and max(c["rseed"] for c in cases) > 99
    assert len(cases) == 17 * 5 * 4
    assert {e["name"] for e in META["edges"]} == {"zeros", "nan", "onehot"} and len(META["dropin"]) == 3
    for c in cases:
        assert c["pdrop"] == 0 and c["msg_nbits"][:2] == [1, 2]
        assert c["msg_nbits"][2] == c["nbits"] - 1.0                       # the Python double of AS:388


@pytest.mark.parametrize("dim", DIMS)
def test_model_equals_the_reference(dim):
    """bins, scale bits, output bits and the message tuple of every stored case of this length"""
    for c in (c for c in META["cases"] if c["d"] == dim):
        x = G.spec_gen(c)
        bins, scale, t = M.compress(x, c["nbits"], c["rseed"])
        tag = (c["idx"], dim, c["nbits"], c["rseed"])
        assert bins.shape[0] == c["D"] and G.sha(bins) == c["bins_sha"], tag
        assert bits_of(scale) == c["scale_bits"], tag
        assert list(t) == c["msg_nbits"], tag
        out = M.decompress(bins, scale, t, c["rseed"], dim)
        assert G.sha(out) == c["out_sha"], tag
        if f"out{c['idx']}" in Z.files:
            assert np.array_equal(bins, Z[f"bins{c['idx']}"]) and G.bits_equal(out, Z[f"out{c['idx']}"]), tag
        else:
            pos, want = sampled(c)
            assert G.bits_equal(out[pos], want), tag


def edge_input(e):
    d = e["d"]
    x = np.zeros(d, np.float32) if e["name"] != "nan" else G.spec_gen({"dist": "normal", "d": d, "seed": 77})
    if e["name"] == "nan":
        x[d // 3] = np.nan
    if e["name"] == "onehot":
        x[d // 2] = 3.5
    return x


def test_model_equals_the_reference_on_edge_rows():
    """an all-zero row (NaN quotients: last bins, NaN scale), a row with one NaN, a one-hot row"""
    for e in META["edges"]:
        out, bins, scale = M.quantize(edge_input(e), e["nbits"], e["rseed"])
        assert np.array_equal(bins, Z[f"ebins{e['k']}"]), e
        assert bits_of(scale) == e["scale_bits"] or (np.isnan(scale) and np.isnan(np.uint32(e["scale_bits"]).view(np.float32))), e
        assert G.bits_equal(out, Z[f"eout{e['k']}"]), e
        if e["name"] == "zeros":
            m = M.mask(e["rseed"], bins.shape[0], e["nbits"] - 1.0)
            assert np.isnan(scale) and np.array_equal(bins, np.where(m, 3, 1))


def test_mask_rule_and_rows():
    """f32(low24) * 2^-24 < f32(p) is low24 < ceil(f32(p) * 2^24); the packed rows hold bit k of word k / 32"""
    from oracle import uq_eden as E
    for p in (0.5, 0.25, 0.30000000000000004, 0.9990000000000001, 1.0000001 - 1.0):
        T = M.threshold(p)
        for seed, D in ((0, 1), (5, 31), (42, 33), (99, 1248), (123456789, 5000)):
            w = E.mt19937((7 * seed + 13) & 0xFFFFFFFF, D)
            m = M.mask(seed, D, p)
            assert np.array_equal(m, (w & 0xFFFFFF) < T)
            rows = M.mask_bits(seed, D, p)
            assert rows.shape[0] == -(-D // 32)
            assert np.array_equal(m, [(int(rows[k >> 5]) >> (k & 31)) & 1 for k in range(D)])
    assert M.threshold(0.5) == 1 << 23 and M.threshold(1.0000001 - 1.0) == 2


# ---- the plan of a fractional call (host only) ---------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return uqdme.load_library()


def plan(lib, op, n, dim, nbits=FRAC):
    buf = (ctypes.c_int64 * NFIELDS)()
    assert lib.uq_test_eden_plan(op, n, dim, nbits, 0, buf, NFIELDS) == 0
    return dict(H._as_dict(buf), frac=int(buf[24]))


ROWS = [      # (n, dim, norm, dot): derived by hand from DESIGN 4.3's rules for 2 bits
    (128, 1 << 14, H.SEG_NORM, H.SEG_DOT),            # few clients of a long vector: both segmented
    (129, 1 << 14, H.SEG_NORM, H.ONE_WAVE),           # the dot's one wave per client from 129 clients on
    (256, 1 << 14, H.SEG_NORM, H.ONE_WAVE),
    (257, 1 << 14, H.CHAINS_WHOLE, H.ONE_WAVE),       # the norm's chains from 257 clients on; never KE2+4
    (1, 1 << 13, H.CHAINS_WHOLE, H.ONE_WAVE),         # below 2^14 nothing is segmented
    (128, 1 << 13, H.CHAINS_WHOLE, H.ONE_WAVE),
    (1, 1 << 14, H.SEG_NORM, H.SEG_DOT),
    (2, (1 << 13) + 1, H.SEG_NORM, H.SEG_DOT),        # the padded D decides
    (257, 2048, H.CHAINS_WHOLE, H.ONE_WAVE),          # D a multiple of the 2048-float chunk ...
    (257, 1024, H.CHAINS_GENERIC, H.ONE_WAVE),        # ... or not
    (3, 5000, H.CHAINS_WHOLE, H.ONE_WAVE),
    (3, 1000, H.CHAINS_GENERIC, H.ONE_WAVE),
    (1, 5, H.CHAINS_GENERIC, H.ONE_WAVE),
    (1024, 1 << 20, H.CHAINS_WHOLE, H.ONE_WAVE),
]


@pytest.mark.parametrize("n,dim,norm,dot", ROWS)
def test_fractional_plan_rows(lib, n, dim, norm, dot):
    p = plan(lib, H.COMPRESS, n, dim)
    assert (p["norm"], p["dot"], p["frac"]) == (norm, dot, 1), p
    two = plan(lib, H.COMPRESS, n, dim, 2)
    assert two["frac"] == 0 and {k: v for k, v in p.items() if k != "frac"} == {k: v for k, v in two.items() if k != "frac"}
    d = plan(lib, H.DECOMPRESS, n, dim)
    d2 = plan(lib, H.DECOMPRESS, n, dim, 2)
    assert d["frac"] == 1 and d2["frac"] == 0 and d["passes"] == d2["passes"] and (d["norm"], d["dot"]) == (0, 0)


def test_integer_plans_and_other_ops_are_not_fractional(lib):
    for n, dim, *_ in ROWS:
        for nbits in (1, 2):
            assert plan(lib, H.COMPRESS, n, dim, nbits)["frac"] == 0
        for op in (H.RHT_FORWARD, H.RHT_INVERSE, H.NORM, H.QFL_FRONT, H.QFL_INVERSE):
            assert plan(lib, op, n, dim)["frac"] == 0
    assert plan(lib, H.COMPRESS, 0, 4096)["frac"] == 0 and plan(lib, H.COMPRESS, 4, 0)["frac"] == 0


def test_new_symbols_declared_and_bound(lib):
    from uqdme_amd import _lib as L
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "uq_dme.h")).read()
    for name in ("uq_eden_mask_bits", "uq_eden_compress_frac_f32", "uq_eden_decompress_frac_f32", "uq_eden_frac_f32"):
        assert name + "(" in header and name in L.SIGNATURES and hasattr(lib, name)
    assert "#define UQ_EDEN_NBITS_FRAC 12" in header and "#define UQ_EDEN_PLAN_FIELDS 25" in header
    # host-side argument checks: nothing is launched
    assert lib.uq_eden_mask_bits(None, -1, 16, 5, None, None) == -1
    assert lib.uq_eden_mask_bits(None, 0, 16, 5, None, None) == 0
    assert lib.uq_eden_mask_bits(None, 1, 16, (1 << 24) + 1, None, None) == -1 and b"threshold" in lib.uq_last_error()
    assert lib.uq_eden_frac_f32(None, None, 0, 16, None, None, None, None, None, None, None, 0, None) == 0
    p = ctypes.c_void_p(256)
    assert lib.uq_eden_compress_frac_f32(p, 1, 16, p, None, None, None, None, p, p, p, 1 << 20, None) == -1
    assert b"mask_bits" in lib.uq_last_error()
    # the integer entry points still refuse every other nbits, the hook's constant included
    for nb in (3, 0, FRAC):
        assert lib.uq_eden_compress_f32(None, 1, 16, nb, None, None, None, None, None, 0, None) == -1
        assert b"nbits" in lib.uq_last_error()


def test_bits_argument_rules():
    """what eden._bits takes: 1, 2 (ints, floats), anything strictly between, the message tuple"""
    import torch
    from uqdme_amd import eden as ED
    assert ED._bits(1) == 1 and ED._bits(2.0) == 2 and type(ED._bits(1.0)) is int
    for b in (1.5, np.float64(1.5), np.float32(1.5), torch.tensor(1.5)):
        assert ED._bits(b) == (1, 2, 0.5)
    assert ED._bits(1.3) == (1, 2, 1.3 - 1.0) and ED._bits((1, 2, 0.25)) == (1, 2, 0.25)
    assert ED._bits([1, 2, 0.5]) == (1, 2, 0.5)                                  # a tuple that went through JSON
    for b in (0.5, 2.5, 3, 0, -1, float("nan"), (1, 2, 1.0), (2, 3, 0.5), [1, 2], [1, 2, "x"], "1", "1.5", b"2", None):
        with pytest.raises(ValueError):
            ED._bits(b)
    assert ED._threshold(0.5) == 1 << 23 and ED._threshold(1.3 - 1.0) == M.threshold(1.3 - 1.0)
