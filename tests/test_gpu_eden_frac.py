"""EDEN at fractional rates 1 < bits < 2 on the GPU: compress, decompress and the fused quantize
bit for bit against the reference's own outputs (tests/golden/eden_frac_vectors.*), batches against
the NumPy model (tests/eden_frac_model.py) at the smallest shapes that reach each dispatch form,
the drop-in, the argument checks and the NMSE loop at rate 1.5."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import eden_frac_model as M
from tests import eden_plan_hook as H
from tests import golden_data as G
from tests.test_eden_frac_model import META, Z, bits_of, edge_input, sampled

pytestmark = pytest.mark.gpu
DIMS = sorted({c["d"] for c in META["cases"]})


def last(lib, op):
    buf = (ctypes.c_int64 * 25)()
    assert lib.uq_test_last_eden_plan(op, buf, 25) == 0
    return dict(H._as_dict(buf), frac=int(buf[24]))


def forms(n, D):
    """(norm, dot) a fractional compress of n clients of padded length D runs"""
    seg = n <= 256 and D >= 16384
    norm = H.SEG_NORM if seg else H.CHAINS_WHOLE if D % 2048 == 0 else H.CHAINS_GENERIC
    return norm, H.SEG_DOT if seg and n <= 128 else H.ONE_WAVE


def assert_plans(lib, n, D, fused):
    c = last(lib, H.COMPRESS)
    assert (c["norm"], c["dot"], c["frac"], c["D"]) == (*forms(n, D), 1, D), c
    if fused:
        d = last(lib, H.DECOMPRESS)
        assert d["frac"] == 1 and d["D"] == D and len(d["passes"]) >= 1, d


@pytest.mark.parametrize("dim", DIMS)
def test_fixture_cases(gpu_ready, dim):
    """every stored case of this length: the message, the receiver on it, and the fused call"""
    import uqdme
    lib = uqdme.load_library()
    for c in (c for c in META["cases"] if c["d"] == dim):
        tag = (c["idx"], dim, c["nbits"], c["rseed"])
        x = torch.from_numpy(G.spec_gen(c)).cuda().view(1, -1)
        msg = uqdme.eden_compress(x, c["nbits"], seeds=[c["rseed"]])
        assert_plans(lib, 1, c["D"], False)
        bins = msg.bins.cpu().numpy()[0]
        assert bins.shape[0] == c["D"] and G.sha(bins) == c["bins_sha"], tag
        assert bits_of(msg.scale.cpu().numpy()[0]) == c["scale_bits"], tag
        assert isinstance(msg.nbits, tuple) and list(msg.nbits) == c["msg_nbits"] and msg.dim == dim, tag
        out = uqdme.eden_decompress(msg).cpu().numpy()[0]
        d = last(lib, H.DECOMPRESS)
        assert d["frac"] == 1 and d["D"] == c["D"], tag
        assert G.sha(out) == c["out_sha"], tag
        q, sc = uqdme.eden_quantize(x, c["nbits"], seeds=[c["rseed"]], return_scale=True)
        assert_plans(lib, 1, c["D"], True)
        assert G.sha(q.cpu().numpy()[0]) == c["out_sha"] and bits_of(sc.cpu().numpy()[0]) == c["scale_bits"], tag
        if f"out{c['idx']}" in Z.files:
            assert np.array_equal(bins, Z[f"bins{c['idx']}"]) and G.bits_equal(out, Z[f"out{c['idx']}"]), tag
        else:
            pos, want = sampled(c)
            assert G.bits_equal(out[pos], want), tag


def test_edge_rows_against_the_reference(gpu_ready):
    import uqdme
    for e in META["edges"]:
        x = torch.from_numpy(edge_input(e)).cuda().view(1, -1)
        msg = uqdme.eden_compress(x, e["nbits"], seeds=[e["rseed"]])
        assert np.array_equal(msg.bins.cpu().numpy()[0], Z[f"ebins{e['k']}"]), e
        s = msg.scale.cpu().numpy()[0]
        assert bits_of(s) == e["scale_bits"] or (np.isnan(s) and np.isnan(np.uint32(e["scale_bits"]).view(np.float32))), e
        assert G.bits_equal(uqdme.eden_decompress(msg).cpu().numpy()[0], Z[f"eout{e['k']}"]), e
        assert G.bits_equal(uqdme.eden_quantize(x, e["nbits"], seeds=[e["rseed"]]).cpu().numpy()[0], Z[f"eout{e['k']}"]), e


def model_rows(xs, nbits, seeds):
    return [M.quantize(x, nbits, s) for x, s in zip(xs, seeds)]


def check_batch(uqdme, lib, x, nbits, seeds, want, period=None):
    """compress + decompress and the fused call on the batch; row j against want[j % period]"""
    n, d = x.shape
    D = M.E.padded_dim(d)
    xd = torch.from_numpy(x).cuda()
    msg = uqdme.eden_compress(xd, nbits, seeds=seeds)
    assert_plans(lib, n, D, False)
    out = uqdme.eden_decompress(msg)
    q, sc = uqdme.eden_quantize(xd, nbits, seeds=seeds, return_scale=True)
    assert_plans(lib, n, D, True)
    assert torch.equal(q.view(torch.int32), out.view(torch.int32))               # separate == fused, bit for bit
    assert torch.equal(sc.view(torch.int32), msg.scale.view(torch.int32))
    bins, scale, o = msg.bins.cpu().numpy(), msg.scale.cpu().numpy(), out.cpu().numpy()
    for j in range(n):
        wo, wb, ws = want[j % (period or n)]
        assert np.array_equal(bins[j], wb), j
        assert bits_of(scale[j]) == bits_of(ws) or (np.isnan(scale[j]) and np.isnan(ws)), j
        assert G.bits_equal(o[j], wo), j


def tiled(n, d, period, seeds, seed0):
    base = np.stack([G.spec_gen({"dist": "lognormal" if j % 2 else "normal", "d": d, "seed": seed0 + j})
                     for j in range(period)])
    return base[np.arange(n) % period].copy(), [seeds[j % period] for j in range(n)]


def test_batch_mixed_and_repeated_seeds(gpu_ready):
    """3 x 5000: two rows share a seed (one mask row), one seed outside 0..99"""
    import uqdme
    x, _ = tiled(3, 5000, 3, [0, 0, 0], 2100)
    for seeds in ([7, 123456789, 7], [5, 99, 5]):
        check_batch(uqdme, uqdme.load_library(), x, 1.3, seeds, model_rows(x, 1.3, seeds))


@pytest.mark.parametrize("n,d,nbits", [(129, 1 << 14, 1.5),      # segmented norm, one-wave dot
                                       (257, 1 << 14, 1.25),     # whole-chunk chains
                                       (257, 1024, 1.3),         # generic chains
                                       (2, 1 << 14, 1.999),      # segmented dot
                                       (5, 16400, 1.5)])         # padded to 2^15: segmented, ragged input rows
def test_batch_forms(gpu_ready, n, d, nbits):
    """rows j and j + 8 hold the same vector and seed, so eight model rows check every row"""
    import uqdme
    x, seeds = tiled(n, d, min(n, 8), [3, 42, 99, 0, 17, 42, 64, 5], 2200 + d % 100)
    check_batch(uqdme, uqdme.load_library(), x, nbits, seeds, model_rows(x[:8], nbits, seeds[:8]), min(n, 8))


@pytest.mark.parametrize("d", [1, 2, 5, 17, 31])
def test_short_rows_partial_mask_word(gpu_ready, d):
    import uqdme
    rng = np.random.default_rng(d)
    x = rng.standard_normal((6, d)).astype(np.float32)
    seeds = [0, 42, 99, 100, 42, 7]
    for nbits in (1.5, 1.0000001, 1.999):
        check_batch(uqdme, uqdme.load_library(), x, nbits, seeds, model_rows(x, nbits, seeds))


@pytest.mark.parametrize("d", [1000, 1 << 14])
def test_nan_and_zero_rows_leave_their_neighbours(gpu_ready, d):
    import uqdme
    x, seeds = tiled(6, d, 6, [1, 2, 3, 4, 5, 6], 2300)
    x[1] = 0.0
    x[3, d // 2] = np.nan
    x[4] = 0.0
    x[4, 5] = -2.0
    check_batch(uqdme, uqdme.load_library(), x, 1.5, seeds, model_rows(x, 1.5, seeds))


def test_drop_in(gpu_ready):
    """a NumPy f32 array of the input's shape with the reference's bits, one randint word taken,
    and no mask row built by a second call with the same seed"""
    import uqdme
    from uqdme_amd import eden as ED
    for c in META["dropin"]:
        x = G.spec_gen({"dist": "normal", "d": c["d"], "seed": c["spec_seed"]})
        for arg in (torch.from_numpy(x.copy()), x):
            torch.manual_seed(c["tseed"])
            out = uqdme.EDEN_quantize_Hadamard(arg, c["nbits"])
            assert int(torch.randint(0, 1 << 30, (1,)).item()) == c["next_word"], c      # exactly one word
            assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == x.shape
            assert G.bits_equal(out, Z[f"dout{c['tseed']}"]), c
        builds = ED._masks.builds
        torch.manual_seed(c["tseed"])
        again = uqdme.EDEN_quantize_Hadamard(x, np.float64(c["nbits"]))
        assert ED._masks.builds == builds and G.bits_equal(again, out)
    # a new (D, threshold) builds its rows once
    builds = ED._masks.builds
    v = G.spec_gen({"dist": "normal", "d": 77, "seed": 1})
    torch.manual_seed(3)
    a = uqdme.EDEN_quantize_Hadamard(v, 1.7)
    assert ED._masks.builds == builds + 1
    torch.manual_seed(3)
    assert G.bits_equal(uqdme.EDEN_quantize_Hadamard(v, torch.tensor(1.7, dtype=torch.float64)), a) and ED._masks.builds == builds + 1


def test_mask_rows_against_the_model(gpu_ready):
    from uqdme_amd import eden as ED
    for D, p in ((1, 0.5), (16, 0.25), (32, 0.5), (1024, 0.3), (1248, 0.999), (4096, 1e-7), (1 << 15, 0.5)):
        seeds = [0, 42, 99, 123456789, -3]
        T = M.threshold(p)
        rows = ED.eden_mask_bits(seeds, D, T).cpu().numpy().view(np.uint32)
        for j, s in enumerate(seeds):
            assert np.array_equal(rows[j], M.mask_bits(s, D, p)), (D, p, s)


def test_rates_without_a_table_raise_before_any_draw(gpu_ready):
    import uqdme
    x = torch.randn(64)
    torch.manual_seed(11)
    state = torch.get_rng_state()
    for b in (0.5, 2.5, 3, 0, float("nan")):
        for f in (uqdme.EDEN_quantize_Hadamard, lambda v, r: uqdme.eden_quantize(v.view(1, -1), r),
                  lambda v, r: uqdme.eden_compress(v.view(1, -1), r)):
            with pytest.raises(ValueError):
                f(x, b)
            assert torch.equal(torch.get_rng_state(), state)
    assert uqdme.eden_compress(x.view(1, -1), 2.0, seeds=[1]).nbits == 2        # 1.0 and 2.0 stay the integer paths
    assert uqdme.eden_compress(x.view(1, -1), 1.0, seeds=[1]).nbits == 1


def test_nmse_loop_at_rate_one_and_a_half(gpu_ready):
    """EDEN and the unbiased quantizer at R = 1.5 in the driver's call order against the reference's
    own loop (tests/golden/nd_nmse_eden_frac.json, made by make_golden_nmse_eden_frac.py): every
    EDEN scale bit for bit, every NMSE within 1e-6 relative (north_star's bound for the loop)."""
    import uqdme
    ref = json.load(open(os.path.join(G.GOLDEN, "nd_nmse_eden_frac.json")))
    r = ref["rate"]
    for dist, rows in ref["rows"].items():
        mine = {}
        res = uqdme.nmse_simulation(dist, dim=ref["dim"], users=(1, 6), num_instances=2, rates=(r,),
                                    schemes=("eden", "unbiased"), torch_threads=1, eden_scales_out=mine)
        theirs = {}
        for n, inst, client, bits, seed, sbits in ref["eden_scales"][dist]:
            theirs.setdefault((n, inst, bits), []).append(np.uint32(sbits))
        for key, sc_ref in theirs.items():
            assert np.array_equal(mine[key].view(np.uint32), np.asarray(sc_ref, np.uint32)), (dist, key)
        for row in rows:
            ui = (1, 6).index(row["n"])
            for sc in ("eden", "unbiased"):
                got, exp = float(res[(sc, r)]["script"][ui, row["inst"]]), row[sc]
                assert abs(got - exp) <= 1e-6 * exp, (dist, row["n"], row["inst"], sc, got, exp)
