"""GPU: the corners of Kashin_quantize that tests/test_gpu_kashin.py leaves out, bit for bit against
the reference's own outputs on torch CPU (tests/golden/kashin_edges.*: rates 3, 5, 6, 7 and 8, the
8-bit input whose top coordinate the reference puts in bin 256, torch.norm's chunk and tail edges,
niters, err, eta and delta, d = 2^21) and against the NumPy model (tests/kashin_model.py, pinned to
that fixture with the same parameters by tests/test_kashin_oracle.py): clients that leave the loop
at different iterations in batches that take the SMALL high pass and more than one pass pair,
niters = 1 and 2, err > 1 refused.  Everything is compared as u32 bit patterns
(golden_data.bits_equal); nothing here takes a tolerance."""
import functools
import hashlib

import numpy as np
import pytest
import torch

from tests import eden_plan_hook as EH
from tests import golden_data as G
from tests import kashin_model as M

pytestmark = pytest.mark.gpu

EDGES, _ = M.edge_fixture()
GROUPS = sorted({c["group"] for c in EDGES})


@pytest.fixture(scope="module")
def ZE(gpu_ready):
    return M.edge_fixture()[1]


def loop(c):
    return dict(niters=c["niters"], eta=c["eta"], delta=c["delta"], err=c["err"])


def check_out(c, e, out):
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == (c["x"]["d"],)
    if "out" in e:
        assert G.bits_equal(out, e["out"]), (c, G.n_mismatch(out, e["out"]))
    else:
        assert G.bits_equal(out[e["pos"]], e["out_s"]), c
        assert G.sha(out) == c["sha"], c


@pytest.mark.parametrize("group", GROUPS)
def test_fixture_cases_fused(ZE, group):
    """kashin_quantize (uq_kashin_f32: the quantizer's bins never leave f32, so bin 256 is exact)."""
    import uqdme
    for c in (c for c in EDGES if c["group"] == group):
        x = torch.from_numpy(M.gen_input(c["x"]))
        out, info, iters = uqdme.kashin_quantize(x[None], c["bits"], seeds=[c["seed"]], return_info=True, **loop(c))
        assert iters.tolist() == [c["iters"]], c
        assert info.tolist() == [0], c
        check_out(c, M.edge_expected(c, ZE), out[0].cpu().numpy())
        if group == "large":                                     # D = 2^22: 14 + 8 bits, forward and inverse
            for op in (EH.QFL_FRONT, EH.QFL_INVERSE):
                p = EH.last_plan(uqdme.load_library(), op)
                assert p["D"] == 1 << 22 and EH.kernels(p) == [EH.LOW16K, EH.HIGH256], p


@pytest.mark.parametrize("group", GROUPS)
def test_fixture_cases_compress_and_decompress(ZE, group):
    """The sender's message of every case; the receiver on the fixture's own message where its bins
    are stored and fit a byte.  The top-bin case saturates at 255 and says so."""
    import uqdme
    from uqdme_amd.kashin import KASHIN_BIN_RANGE
    for c in (c for c in EDGES if c["group"] == group):
        e = M.edge_expected(c, ZE)
        top = c["bins_max"] > 255
        x = torch.from_numpy(M.gen_input(c["x"]))
        msg = uqdme.kashin_compress(x[None], c["bits"], seeds=[c["seed"]], **loop(c))
        assert msg.bins.shape == (1, c["D"]) and msg.bins.dtype == torch.uint8 and msg.dim == c["x"]["d"]
        assert msg.iters.tolist() == [c["iters"]], c
        assert msg.info.tolist() == [KASHIN_BIN_RANGE if top else 0], c
        assert G.bits_equal([float(msg.mn[0]), float(msg.step[0])], e["ms"]), c
        bins = msg.bins[0].cpu().numpy().astype(np.uint16)
        if "bins" in e:
            want = np.minimum(e["bins"], 255)
            assert np.array_equal(bins, want), (c, int((bins != want).sum()))
        else:
            assert hashlib.sha256(bins.tobytes()).hexdigest() == c["bins_sha"], c
        if "bins" in e and not top:
            fix = uqdme.KashinMessage(bins=torch.from_numpy(e["bins"].astype(np.uint8)).view(1, -1),
                                      mn=torch.tensor([e["ms"][0]]), step=torch.tensor([e["ms"][1]]),
                                      seeds=torch.tensor([0]), nbits=c["bits"], dim=c["x"]["d"])
            check_out(c, e, uqdme.kashin_decompress(fix)[0].cpu().numpy())


def test_top_bin_alone_and_inside_a_batch(ZE):
    """8 bits: step = (mx - mn) / f32(255) rounds down, q_max = 255 + 2^-16 and the reference's
    bernoulli fires: bin 256.0 at coordinate 1399.  The fused path reproduces it (info 0); a u8
    message flags KASHIN_BIN_RANGE for that row alone and stores 255."""
    import uqdme
    from uqdme_amd.kashin import KASHIN_BAD_P, KASHIN_BIN_RANGE
    c = next(c for c in EDGES if c["group"] == "top_bin")
    e = M.edge_expected(c, ZE)
    assert e["bins"].max() == 256 and int((e["bins"] == 256).sum()) == 1
    x1 = M.gen_input(c["x"])
    out, info, iters = uqdme.kashin_quantize(torch.from_numpy(x1)[None], 8, seeds=[c["seed"]], return_info=True)
    assert info.tolist() == [0] and iters.tolist() == [c["iters"]]
    assert G.bits_equal(out[0].cpu().numpy(), e["out"])
    msg = uqdme.kashin_compress(torch.from_numpy(x1)[None], 8, seeds=[c["seed"]])
    assert msg.info.tolist() == [KASHIN_BIN_RANGE] and not int(msg.info[0]) & KASHIN_BAD_P
    assert np.array_equal(msg.bins[0].cpu().numpy(), np.minimum(e["bins"], 255).astype(np.uint8))
    assert G.bits_equal([float(msg.mn[0]), float(msg.step[0])], e["ms"])

    x = np.stack([M.gen_input({"dist": "normal", "d": 2048, "seed": 71}), x1,
                  M.gen_input({"dist": "normal", "d": 2048, "seed": 72})])
    seeds = [5, c["seed"], 9]
    want = [M.kashin(x[j], 8, seeds[j]) for j in range(3)]
    assert [int(w["bins"].max()) for w in want] == [255, 256, 255]
    assert G.bits_equal(want[1]["out"], e["out"])
    out, info, iters = uqdme.kashin_quantize(torch.from_numpy(x), 8, seeds=seeds, return_info=True)
    assert info.tolist() == [0, 0, 0] and iters.tolist() == [w["iters"] for w in want]
    msg = uqdme.kashin_compress(torch.from_numpy(x), 8, seeds=seeds)
    assert msg.info.tolist() == [0, KASHIN_BIN_RANGE, 0]
    for j in range(3):
        assert G.bits_equal(out[j].cpu().numpy(), want[j]["out"]), (j, G.n_mismatch(out[j].cpu().numpy(), want[j]["out"]))
        assert np.array_equal(msg.bins[j].cpu().numpy(), np.minimum(want[j]["bins"], 255).astype(np.uint8)), j
        assert G.bits_equal([float(msg.mn[j]), float(msg.step[j])], [want[j]["mn"], want[j]["step"]]), j


# ---- clients that are done while the batch goes on ------------------------------------------

def check_batch(x, bits, seeds, want, **kw):
    """kashin_quantize and kashin_compress of the batch against the model's rows `want`: iters of
    every row, KASHIN_BAD_P on exactly the rows the reference raises on, the other rows' bits."""
    import uqdme
    from uqdme_amd.kashin import KASHIN_BAD_P
    n = x.shape[0]
    bad = [w["raises"] for w in want]
    out, info, iters = uqdme.kashin_quantize(torch.tensor(x), bits, seeds=seeds, return_info=True, **kw)
    plans = [EH.last_plan(uqdme.load_library(), op) for op in (EH.QFL_FRONT, EH.QFL_INVERSE)]
    msg = uqdme.kashin_compress(torch.tensor(x), bits, seeds=seeds, **kw)
    out, bins, mn, step = out.cpu().numpy(), msg.bins.cpu().numpy(), msg.mn.cpu().numpy(), msg.step.cpu().numpy()
    assert iters.tolist() == msg.iters.tolist() == [w["iters"] for w in want]
    for flags in (info.tolist(), msg.info.tolist()):
        assert [bool(v & KASHIN_BAD_P) for v in flags] == bad
        assert all(v == 0 for v, b in zip(flags, bad) if not b)
    for j in range(n):
        if bad[j]:
            continue
        assert G.bits_equal(out[j], want[j]["out"]), (j, want[j]["iters"], G.n_mismatch(out[j], want[j]["out"]))
        assert np.array_equal(bins[j], want[j]["bins"].astype(np.uint8)), (j, want[j]["iters"])
        assert G.bits_equal([mn[j], step[j]], [want[j]["mn"], want[j]["step"]]), (j, want[j]["iters"])
    return plans


SMALL_N, SMALL_D, SMALL_BITS, SMALL_NITERS = 64, 5000, 3, 4
BAD_ROWS = {9: "zeros", 13: "nan", 21: "inf"}                  # all inside the first 24 rows


@functools.lru_cache(maxsize=None)
def small_batch():
    """(x [64, 5000], seeds, the model's rows): computed once, shared by both batch sizes, read-only."""
    x = np.random.RandomState(11).normal(size=(SMALL_N, SMALL_D)).astype(np.float32)
    assert G.bits_equal(x[:24], M.normal_batch(11, 24, SMALL_D))          # the fixture's err1 rows are this batch's first
    for j, kind in BAD_ROWS.items():
        if kind == "zeros":
            x[j] = 0
        else:
            x[j, SMALL_D // 3] = np.nan if kind == "nan" else np.inf
    x.setflags(write=False)
    seeds = [j % 100 for j in range(SMALL_N)]
    want = [M.kashin(x[j], SMALL_BITS, seeds[j], niters=SMALL_NITERS, err=1.0) for j in range(SMALL_N)]
    return x, seeds, want


def test_done_rows_with_the_small_high_pass():
    """err = 1.0 splits the rows by themselves (1.0 < 1.0 is false, so the skipped test at i = 0
    stays right): 64 clients of D = 8192 take UQ_EDEN_PASS_SMALL for the 13th bit, forward and
    inverse, while clients done after 2 and 3 transforms keep c, r and M."""
    import uqdme
    x, seeds, want = small_batch()
    lib = uqdme.load_library()
    assert [j for j, w in enumerate(want) if w["raises"]] == sorted(BAD_ROWS)
    its = [w["iters"] for w in want if not w["raises"]]
    assert all(its.count(k) >= 4 for k in (2, 3, 4)) and set(its) == {2, 3, 4}, its
    assert [w["iters"] for w in want[:8]] == [2, 4, 3, 4, 2, 4, 2, 3]
    D = M.kashin_padded_dim(SMALL_D)
    for op in (EH.QFL_FRONT, EH.QFL_INVERSE):
        assert EH.kernels(EH.plan(lib, op, SMALL_N, D)) == [EH.LOW4096, EH.SMALL]
    plans = check_batch(x, SMALL_BITS, seeds, want, niters=SMALL_NITERS, err=1.0)
    assert [EH.kernels(p) for p in plans] == [[EH.LOW4096, EH.SMALL]] * 2, plans
    assert [p["D"] for p in plans] == [D, D]


def test_done_rows_with_the_generic_high_pass():
    """The first 24 of the same rows: the same bits per row from the generic second pass."""
    x, seeds, want = small_batch()
    assert len({w["iters"] for w in want[:24]}) == 3
    plans = check_batch(x[:24], SMALL_BITS, seeds[:24], want[:24], niters=SMALL_NITERS, err=1.0)
    assert [EH.kernels(p) for p in plans] == [[EH.LOW4096, EH.GENERIC]] * 2, plans


def test_done_rows_above_one_pass_pair():
    """d = 70001, D = 2^17: the transforms' ping-pong buffers, KK1's chunk loop and the element-wise
    kernels' grids at a size where the rows of a done client are many tiles."""
    n, d, bits, niters = 6, 70001, 2, 5
    x = M.normal_batch(11, n, d)
    seeds = list(range(n))
    want = [M.kashin(x[j], bits, seeds[j], niters=niters, err=1.0) for j in range(n)]
    its = [w["iters"] for w in want]
    assert its == [4, 5, 4, 2, 4, 2]
    assert len(set(its)) >= 2 and niters in its and not any(w["raises"] for w in want)
    plans = check_batch(np.asarray(x), bits, seeds, want, niters=niters, err=1.0)
    assert all(len(p["passes"]) == 2 and p["D"] == 1 << 17 for p in plans)


@pytest.mark.parametrize("niters", [1, 2])
def test_niters_1_and_2(niters):
    """niters = 1: one transform, no inverse, no exit test; niters = 2: one residual update, the
    exit test skipped at i = 0 and moot at i = 1.  (d = 2056: the norm's last chunk is one step.)"""
    n, d, bits = 5, 2056, 2
    x = M.normal_batch(23, n, d)
    seeds = [7, 99, 0, 7, 50]
    want = [M.kashin(x[j], bits, seeds[j], niters=niters) for j in range(n)]
    assert [w["iters"] for w in want] == [niters] * n
    check_batch(np.asarray(x), bits, seeds, want, niters=niters)


def test_err_above_1_is_refused_before_any_draw():
    import uqdme
    x = torch.from_numpy(M.normal_batch(23, 5, 2056).copy())
    for fn in (uqdme.kashin_quantize, uqdme.kashin_compress):
        g = torch.Generator().manual_seed(31)
        before = g.get_state().clone()
        torch.manual_seed(31)
        glob = torch.default_generator.get_state().clone()
        for kw in (dict(generator=g), dict()):
            with pytest.raises(ValueError, match="err must be <= 1"):
                fn(x, 1, err=1.5, niters=4, **kw)
        assert torch.equal(g.get_state(), before) and torch.equal(torch.default_generator.get_state(), glob)
        g1 = torch.Generator().manual_seed(31)
        fn(x, 1, err=1.0, niters=4, generator=g1)                # the bound itself is taken, and draws
        assert not torch.equal(g1.get_state(), before)
