"""Kashin_quantize on the host: the NumPy model (tests/kashin_model.py) against the reference's
own outputs (tests/golden/kashin_vectors.* and kashin_edges.*), and the host pieces of the GPU path -- the padded
dimension, the prng seeds, the run tables, the harness's draws, the C argument checks."""
import ctypes
import hashlib
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests import golden_data as G
from tests import kashin_model as M
from oracle import uq_quicfl as Q

META = json.load(open(os.path.join(G.GOLDEN, "kashin_vectors.json")))["cases"]
EDGES, _ = M.edge_fixture()
PADDED = {1: 2, 2: 4, 3: 4, 5: 8, 7: 16, 13: 16, 14: 32, 27: 32, 28: 64, 1740: 2048, 1741: 4096, 2048: 4096,
          3481: 4096, 3482: 8192}


@pytest.fixture(scope="module")
def Z():
    return np.load(os.path.join(G.GOLDEN, "kashin_vectors.npz"))


def test_fixture_covers_the_issue():
    cs = [c for c in META if c["d"] > 0]
    for dist in ("normal", "lognormal"):
        for d in (2, 3, 5, 7, 13, 14, 27, 28, 1000, 1740, 1741, 2048, 2049, 3481, 3482, 5000):
            for bits in (1, 2, 4):
                assert any(c["dist"] == dist and c["d"] == d and c["bits"] == bits for c in cs)
    assert {c["d"] for c in cs} >= {70001, 1 << 20}
    raising = [(c["dist"], c["d"]) for c in cs if c["raises"]]
    assert ("zeros", 8) in raising and ("nan", 100) in raising and ("inf", 100) in raising
    assert any(d == 1 for _, d in raising)
    early = [c for c in cs if c["iters"] == 2]
    assert len(early) >= 4
    assert any(c["dist"] == "normal" and c["d"] in (3, 4) for c in early)
    assert any(c["dist"] == "smallint" and c["d"] >= 5 for c in early)
    assert {c["pre"] for c in cs} == {0, 1, 300}
    assert all(c["iters"] == 3 for c in cs if c["dist"] in ("onehot", "constant"))


@pytest.mark.parametrize("c", [c for c in META if c["d"] > 0], ids=lambda c: f"{c['idx']}-{c['dist']}-d{c['d']}-b{c['bits']}")
def test_model_equals_reference(c, Z):
    r = M.kashin(M.gen_input(c), c["bits"], c.get("seed_drawn", 0))
    assert r["raises"] == c["raises"]
    assert r["iters"] == c["iters"]
    if c["raises"]:
        return
    k = c["idx"]
    assert G.bits_equal([r["mn"], r["step"]], Z[f"ms{k}"])
    bins = r["bins"].astype(np.uint8)
    if f"out{k}" in Z.files:
        assert np.array_equal(bins, Z[f"bins{k}"])
        assert G.bits_equal(r["out"], Z[f"out{k}"])
    else:
        assert hashlib.sha256(bins.tobytes()).hexdigest() == c["bins_sha"]
        assert hashlib.sha256(r["out"].tobytes()).hexdigest() == c["sha"]
        assert G.bits_equal(r["out"][Z[f"out{k}_pos"]], Z[f"out{k}_s"])


@pytest.fixture(scope="module")
def ZE():
    return M.edge_fixture()[1]


def test_edge_fixture_covers_the_issue(ZE):
    def has(group, d=None, dist="normal", **kw):
        return any(c["group"] == group and (d is None or c["x"]["d"] == d) and c["x"]["dist"] == dist and
                   all(c[k] == v for k, v in kw.items()) for c in EDGES)
    defaults = dict(niters=3, err=1e-6, eta=0.9, delta=1.0)
    for bits in (3, 5, 6, 7, 8):
        for d in (13, 1741, 5000):
            assert has("rates", d, bits=bits, **defaults)
        assert has("rates", dist="lognormal", bits=bits, **defaults)
    top = [c for c in EDGES if c["group"] == "top_bin"]
    assert len(top) == 1 and top[0]["x"] == {"dist": "normal_f32", "d": 2048, "seed": 5238}
    assert (top[0]["bits"], top[0]["seed"], top[0]["bins_max"]) == (8, 37, 256)
    tb = M.edge_expected(top[0], ZE)["bins"]
    assert tb.dtype == np.uint16 and np.flatnonzero(tb == 256).tolist() == [1399] and tb.max() == 256
    assert all(c["bins_max"] == 2 ** c["bits"] - 1 for c in EDGES if c["group"] != "top_bin")
    for d in (4, 6, 8, 12, 15, 16, 2047, 2055, 2056, 4100, 4103, 6147, 6150):
        assert has("norm_edges", d, bits=1, **defaults)
    for d in (100, 5000):
        for niters in (1, 2, 4, 5):
            assert has("niters", d, **dict(defaults, niters=niters))
        assert has("eta", d, **dict(defaults, eta=0.75))
        assert has("delta", d, **dict(defaults, delta=0.5)) and has("delta", d, **dict(defaults, delta=2.0))
    for niters in (4, 5):
        rows = [c for c in EDGES if c["group"] == "err1" and c["x"]["d"] == 5000 and c["niters"] == niters]
        assert [c["x"]["row"] for c in rows] == list(range(8))
        assert all(c["x"] == {"dist": "normal_row", "n": 24, "d": 5000, "seed": 11, "row": c["x"]["row"]} and c["err"] == 1.0
                   for c in rows)
        if niters == 4:
            assert [c["iters"] for c in rows] == [2, 4, 3, 4, 2, 4, 2, 3]
        assert max(c["iters"] for c in rows) == niters and min(c["iters"] for c in rows) == 2
    assert all(c["iters"] == c["niters"] for c in EDGES if c["group"] == "niters" and c["niters"] <= 2)
    assert has("large", 1 << 21, bits=1, **defaults)
    for c in EDGES:                                      # in full below 8192 coordinates, else sha256s and samples
        e = M.edge_expected(c, ZE)
        assert e["ms"].dtype == np.float32 and e["ms"].shape == (2,)
        if c["x"]["d"] < 8192:
            assert e["out"].shape == (c["x"]["d"],) and e["bins"].shape == (c["D"],) and e["bins"].dtype == np.uint16
        else:
            assert e["out_s"].shape == e["pos"].shape == (4096,) and len(c["sha"]) == len(c["bins_sha"]) == 64
        assert c["D"] == M.kashin_padded_dim(c["x"]["d"])
        if "same_as" in c:                               # only a client that left the loop early repeats a result
            o = EDGES[c["same_as"]]
            assert o["x"] == c["x"] and (o["bits"], o["seed"], o["err"]) == (c["bits"], c["seed"], c["err"])
    size = [os.path.getsize(os.path.join(G.GOLDEN, f)) for f in ("kashin_edges.npz", "kashin_vectors.npz")]
    assert size[0] <= size[1]


@pytest.mark.parametrize("c", EDGES, ids=lambda c: f"{c['idx']}-{c['group']}-d{c['x']['d']}-b{c['bits']}")
def test_model_equals_reference_edges(c, ZE):
    """The model with the loop's parameters, 8 bits and its bin 256 included, against the reference."""
    r = M.kashin(M.gen_input(c["x"]), c["bits"], c["seed"], c["niters"], c["eta"], c["delta"], c["err"])
    e = M.edge_expected(c, ZE)
    assert not r["raises"]
    assert r["iters"] == c["iters"]
    assert G.bits_equal([r["mn"], r["step"]], e["ms"])
    assert r["bins"].max() == c["bins_max"] and r["bins"].min() >= 0
    bins = r["bins"].astype(np.uint16)
    if "out" in e:
        assert np.array_equal(bins, e["bins"])
        assert G.bits_equal(r["out"], e["out"])
    else:
        assert hashlib.sha256(bins.tobytes()).hexdigest() == c["bins_sha"]
        assert hashlib.sha256(r["out"].tobytes()).hexdigest() == c["sha"]
        assert G.bits_equal(r["out"][e["pos"]], e["out_s"])


def test_model_exits_after_one_transform_above_err_1():
    """AS:236 at i = 0 compares 1.0 with the bound: a bound above 1 ends the loop there (the
    reference with data['err'] = 1.5 does; the library refuses such a bound)."""
    x = M.gen_input({"dist": "normal", "d": 100, "seed": 3})
    assert M.kashin(x, 1, 0, niters=4, err=1.5)["iters"] == 1
    assert M.kashin(x, 1, 0, niters=4, err=1.0)["iters"] >= 2


def test_the_seed_drawn_is_one_randint_word():
    for c in META:
        if "seed_drawn" not in c:
            continue
        torch.manual_seed(c["gseed"])
        for _ in range(c["pre"]):
            torch.randint(0, 100, (1,))
        assert int(torch.randint(0, 100, (1,))) == c["seed_drawn"]
        assert hashlib.sha256(torch.default_generator.get_state().numpy().tobytes()).hexdigest() == c["state_sha"]


def test_padded_dim():
    import uqdme
    lib = uqdme.load_library()
    for d, D in PADDED.items():
        assert M.kashin_padded_dim(d) == D
        assert uqdme.kashin_padded_dim(d) == D
        out = ctypes.c_int64(0)
        assert lib.uq_kashin_padded_dim(d, ctypes.byref(out)) == 0 and out.value == D
    for d in list(range(1, 300)) + [70001, 1 << 20, (1 << 20) + 1, 3565158, 3565159]:
        assert uqdme.kashin_padded_dim(d) == M.kashin_padded_dim(d)
    assert lib.uq_kashin_padded_dim(-1, ctypes.byref(out)) != 0
    assert lib.uq_kashin_padded_dim(5, None) != 0


def test_prng_seeds():
    from uqdme_amd import kashin
    for s in list(range(100)) + [123, -3, 10 ** 12]:
        assert kashin.prng_seed(s) == Q.xxh64(str(s).encode()) % 65536


@pytest.mark.parametrize("run_words", [1000, 624, 9984])
def test_run_table_reproduces_the_stream(run_words):
    from uqdme_amd import kashin
    D, prng = 8192, Q.prng_seed(17)
    tab = kashin.run_table(prng, D, run_words)
    R = -(-D // run_words)
    assert tab.shape == (R, 626) and tab.dtype == np.uint32
    straight, _ = Q.mt_draw(Q.seeded_state(prng), D)
    for r in range(R):
        n = min(run_words, D - r * run_words)
        got, _ = Q.mt_draw((int(tab[r, 0]), int(tab[r, 1]), tab[r, 2:]), n)
        assert np.array_equal(got, straight[r * run_words:r * run_words + n])
    assert kashin.run_table(prng, D, run_words) is tab           # cached


def test_run_table_cache_is_bounded():
    from uqdme_amd import kashin
    lru = kashin._LRU(3000)
    for k in range(4):
        lru.put(k, np.zeros(250, np.uint32), 1000)
    assert lru.get(0) is None and lru.get(3) is not None and lru.bytes <= 3000
    lru.put("big", np.zeros(2500, np.uint32), 10000)             # the newest entry always stays
    assert lru.get("big") is not None and len(lru.items) == 1


def test_client_draws_with_kashin():
    from uqdme_amd import dme
    assert dme.SCHEME_ORDER.index("kashin") == dme.SCHEME_ORDER.index("quicfl") + 1
    order, rates, n = ["eden", "unbiased", "kashin"], (1, 2), 5
    g = torch.Generator().manual_seed(9)
    want = {(sc, r): [] for sc in order for r in rates}
    for _ in range(n):
        for sc in order:
            for r in rates:
                want[(sc, r)].append(float(torch.rand(1, generator=g)) if sc == "unbiased"
                                     else int(torch.randint(0, 100, (1,), generator=g)))
    end = g.get_state()
    assert dme._client_words(order, rates, None) == 6
    for fn in (lambda gen: dme._client_draws(gen, n, order, rates, None),
               lambda gen: dme._client_draws_parallel(gen, n, order, rates, None, None)):
        gen = torch.Generator().manual_seed(9)
        assert fn(gen) == want
        assert torch.equal(gen.get_state(), end)


def test_c_argument_checks_launch_nothing():
    """Refused before any launch: this test runs without a GPU."""
    import uqdme
    lib = uqdme.load_library()
    one = ctypes.c_void_p(16)          # non-null, never dereferenced: every call below is refused first
    null = ctypes.c_void_p(0)
    E_INVALID = -1                     # UQ_E_INVALID

    def compress(n=1, dim=5, D=8, niters=3, nlevels=2, x=one, signs=one, runs=one, run_words=1000, bins=one, ws=one,
                 err=1e-6):
        return lib.uq_kashin_compress_f32(x, n, dim, D, niters, 0.9, 1.0, err, nlevels, signs, null, runs, null,
                                          run_words, bins, one, one, one, one, ws, 1 << 40, null)

    def fused(n=1, dim=5, D=8, niters=3, nlevels=2, x=one, out=one, info=one, err=1e-6):
        return lib.uq_kashin_f32(x, out, n, dim, D, niters, 0.9, 1.0, err, nlevels, one, null, one, null, 1000, null,
                                 null, info, null, one, 1 << 40, null)

    def decompress(n=1, dim=5, D=8, bins=one, out=one):
        return lib.uq_kashin_decompress_f32(bins, one, one, n, dim, D, one, null, out, one, 1 << 40, null)

    for f in (compress, fused):
        assert f(n=0) == 0 and f(dim=0) == 0                     # no-ops
        assert f(x=null) != 0
        assert f(D=6) != 0 and f(D=4) != 0 and f(dim=1, D=1) != 0
        assert f(niters=0) != 0
        assert f(nlevels=1) != 0 and f(nlevels=257) != 0
        assert f(n=-1) != 0
        # f32(err) > 1: the reference leaves the loop after its first transform, the device loop cannot
        for err in (1.5, 1.0000001, float("inf")):
            assert f(err=err) == E_INVALID and f(err=err, n=0) == E_INVALID
            msg = lib.uq_last_error()
            assert b"err must be <= 1" in msg and b"first transform" in msg
        # err = 1.0 (and a double that rounds to f32 1.0) passes that check: refused by the next one, or a no-op
        for err in (1.0, 1.0 + 1e-12):
            assert f(err=err, n=0) == 0
            assert f(err=err, D=6) == E_INVALID and b"power of two" in lib.uq_last_error()
            assert f(err=err, x=null) == E_INVALID and b"null pointer" in lib.uq_last_error()
    assert compress(signs=null) != 0 and compress(runs=null) != 0 and compress(bins=null) != 0
    assert compress(run_words=0) != 0 and compress(ws=null) != 0
    assert fused(out=null) != 0 and fused(info=null) != 0
    assert decompress(n=0) == 0 and decompress(bins=null) != 0 and decompress(out=null) != 0 and decompress(D=6) != 0
    assert b"kashin" in lib.uq_last_error()
    sz = ctypes.c_size_t(0)
    assert lib.uq_kashin_workspace_bytes(3, 8192, ctypes.byref(sz)) == 0 and sz.value >= 4 * 3 * 8192 * 4
    assert lib.uq_kashin_workspace_bytes(3, 8192, None) != 0


def test_dropin_signature():
    import uqdme
    sig = inspect.signature(uqdme.Kashin_quantize)
    assert list(sig.parameters) == ["input_vector", "bits_per_dimension"]
    assert sig.parameters["bits_per_dimension"].default == 1
    assert "Kashin_quantize" in uqdme.__all__ and "kashin_quantize" in uqdme.__all__
    from uqdme_amd import kashin
    assert {"Kashin_quantize", "kashin_quantize", "kashin_compress", "kashin_decompress", "kashin_padded_dim",
            "KashinMessage"} <= set(kashin.__all__)
