"""GPU: Kashin_quantize (AS:834-854) through the drop-in, the batch forms and the DME harness, bit
for bit against the reference's own outputs on torch CPU (tests/golden/kashin_vectors.*) and
against the NumPy model (tests/kashin_model.py, pinned to that fixture by
tests/test_kashin_oracle.py).  Outputs are compared as u32 bit patterns (golden_data.bits_equal),
the generator by the sha256 of its state."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import golden_data as G
from tests import kashin_model as M

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(G.GOLDEN, "kashin_vectors.json")))["cases"]
CASES = [c for c in META if c["d"] > 0]


@pytest.fixture(scope="module")
def Z(gpu_ready):
    return np.load(os.path.join(G.GOLDEN, "kashin_vectors.npz"))


def set_global(c):
    torch.manual_seed(c["gseed"])
    for _ in range(c["pre"]):
        torch.randint(0, 100, (1,))


def global_sha(gen=None):
    return hashlib.sha256((gen or torch.default_generator).get_state().numpy().tobytes()).hexdigest()


def check_out(c, Z, out):
    k = c["idx"]
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == (c["d"],)
    if "sha" in c:
        assert G.bits_equal(out[Z[f"out{k}_pos"]], Z[f"out{k}_s"]), c
        assert G.sha(out) == c["sha"], c
    else:
        assert G.bits_equal(out, Z[f"out{k}"]), (c, G.n_mismatch(out, Z[f"out{k}"]))


def test_dropin_matches_the_reference(Z):
    """Every fixture case through Kashin_quantize after torch.manual_seed and 0, 1 or 300 pre-draws:
    the reference's output bits, its generator state afterwards, RuntimeError where it raises (the
    generator one word on all the same)."""
    import uqdme
    for c in CASES:
        x = M.gen_input(c)
        set_global(c)
        if c["raises"]:
            with pytest.raises(RuntimeError):
                uqdme.Kashin_quantize(x.copy(), c["bits"])
        else:
            out = uqdme.Kashin_quantize(x.copy(), c["bits"])
            assert isinstance(out, np.ndarray)
            check_out(c, Z, out)
        assert global_sha() == c["state_sha"], c


def test_dropin_inputs_and_empty_vector(Z):
    import uqdme
    c = next(c for c in CASES if c["d"] == 1000 and c["bits"] == 2 and c["dist"] == "normal")
    x = M.gen_input(c)
    for v in (x.tolist(), torch.from_numpy(x.copy()), torch.from_numpy(x.copy()).cuda(), x.astype(np.float64)):
        set_global(c)
        check_out(c, Z, uqdme.Kashin_quantize(v, c["bits"]))
    e = META[-1]
    assert e["d"] == 0 and e["draws_one_word"]           # what the reference does with an empty vector
    set_global(e)
    out = uqdme.Kashin_quantize(np.zeros(0, np.float32))
    assert out.shape == (0,) and out.dtype == np.float32
    assert global_sha() == e["state_sha"]


def test_compress_matches_the_reference(Z):
    """The sender's message (bins, min, step), the iteration count and the flag of every case."""
    import uqdme
    from uqdme_amd.kashin import KASHIN_BAD_P
    for c in CASES:
        k = c["idx"]
        x = M.gen_input(c)
        seed = c.get("seed_drawn", 0)
        msg = uqdme.kashin_compress(torch.from_numpy(x.copy()).view(1, -1), c["bits"], seeds=[seed])
        D = M.kashin_padded_dim(c["d"])
        assert msg.bins.shape == (1, D) and msg.bins.dtype == torch.uint8 and msg.dim == c["d"] and msg.nbits == c["bits"]
        assert int(msg.iters[0]) == c["iters"], c
        assert bool(int(msg.info[0]) & KASHIN_BAD_P) == c["raises"], c
        if c["raises"]:
            continue
        assert int(msg.info[0]) == 0
        assert G.bits_equal([float(msg.mn[0]), float(msg.step[0])], Z[f"ms{k}"]), c
        bins = msg.bins[0].cpu().numpy()
        if "bins_sha" in c:
            assert hashlib.sha256(bins.tobytes()).hexdigest() == c["bins_sha"], c
        else:
            assert np.array_equal(bins, Z[f"bins{k}"]), (c, int((bins != Z[f"bins{k}"]).sum()))


def test_decompress_of_the_fixtures_messages(Z):
    import uqdme
    n = 0
    for c in CASES:
        k = c["idx"]
        if f"bins{k}" not in Z.files:
            continue
        ms = Z[f"ms{k}"]
        msg = uqdme.KashinMessage(bins=torch.from_numpy(Z[f"bins{k}"]).view(1, -1), mn=torch.tensor([ms[0]]),
                                  step=torch.tensor([ms[1]]), seeds=torch.tensor([0]), nbits=c["bits"], dim=c["d"])
        check_out(c, Z, uqdme.kashin_decompress(msg)[0].cpu().numpy())
        n += 1
    assert n >= 96


def test_batch_with_an_early_exit_and_a_zero_row():
    """Three rows, one of which exits after two transforms and one is all zeros (flagged): info and
    iters per row, the other rows as if alone."""
    import uqdme
    from uqdme_amd.kashin import KASHIN_BAD_P
    for d in (4, 8):
        early = next(c for c in CASES if c["iters"] == 2 and c["d"] == d)
        x = np.stack([M.gen_input({"dist": "normal", "d": d, "seed": 77}), M.gen_input(early), np.zeros(d, np.float32)])
        bits, seeds = early["bits"], [5, early["seed_drawn"], 9]
        want = [M.kashin(x[j], bits, seeds[j]) for j in range(3)]
        assert [w["iters"] for w in want] == [3, 2, 3] and [w["raises"] for w in want] == [False, False, True]
        out, info, iters = uqdme.kashin_quantize(torch.from_numpy(x), bits, seeds=seeds, return_info=True)
        assert iters.tolist() == [3, 2, 3]
        assert [bool(v & KASHIN_BAD_P) for v in info.tolist()] == [False, False, True]
        for j in (0, 1):
            assert G.bits_equal(out[j].cpu().numpy(), want[j]["out"]), (d, j)
        with pytest.raises(RuntimeError):
            uqdme.kashin_quantize(torch.from_numpy(x), bits, seeds=seeds)
        msg = uqdme.kashin_compress(torch.from_numpy(x), bits, seeds=seeds)
        assert msg.iters.tolist() == [3, 2, 3]
        for j in (0, 1):
            assert np.array_equal(msg.bins[j].cpu().numpy(), want[j]["bins"].astype(np.uint8))
            assert G.bits_equal([float(msg.mn[j]), float(msg.step[j])], [want[j]["mn"], want[j]["step"]])


def test_batch_of_300_against_the_model():
    import uqdme
    n, d = 300, 2048
    rs = np.random.RandomState(5)
    x = rs.normal(size=(n, d)).astype(np.float32)
    x[7] = np.round(x[7] * 2)
    x[11] *= np.float32(1e-20)
    seeds = rs.randint(0, 100, size=n).astype(np.int64)
    seeds[:5] = [0, 99, 123, -3, 10 ** 12]
    out, info, iters = uqdme.kashin_quantize(torch.from_numpy(x), 2, seeds=seeds, return_info=True)
    out = out.cpu().numpy()
    assert not info.any()
    it = iters.tolist()
    for j in range(n):
        w = M.kashin(x[j], 2, int(seeds[j]))
        assert not w["raises"] and w["iters"] == it[j]
        assert G.bits_equal(out[j], w["out"]), (j, G.n_mismatch(out[j], w["out"]))


def test_run_words_do_not_change_the_bits():
    import uqdme
    x = torch.from_numpy(np.random.RandomState(8).normal(size=(2, 5000)).astype(np.float32))
    ref = uqdme.kashin_compress(x, 1, seeds=[3, 42])
    assert ref.bins.shape == (2, 8192)
    want = M.kashin(x[1].numpy(), 1, 42)
    assert np.array_equal(ref.bins[1].cpu().numpy(), want["bins"].astype(np.uint8))
    for rw in (1000, 624, 8192, 100000):
        got = uqdme.kashin_compress(x, 1, seeds=[3, 42], run_words=rw)
        assert torch.equal(got.bins, ref.bins) and torch.equal(got.mn, ref.mn) and torch.equal(got.step, ref.step)
        q = uqdme.kashin_quantize(x, 1, seeds=[3, 42], run_words=rw)
        assert torch.equal(q.view(torch.int32), uqdme.kashin_decompress(ref).view(torch.int32))


def test_generator_draws_the_seeds_in_client_order():
    import uqdme
    n = 7
    x = torch.from_numpy(np.random.RandomState(2).normal(size=(n, 100)).astype(np.float32))
    g = torch.Generator().manual_seed(31)
    seeds = [int(torch.randint(0, 100, (1,), generator=g)) for _ in range(n)]
    end = global_sha(g)
    g2 = torch.Generator().manual_seed(31)
    msg = uqdme.kashin_compress(x, 2, generator=g2)
    assert msg.seeds.tolist() == seeds and global_sha(g2) == end
    g3 = torch.Generator().manual_seed(31)
    q = uqdme.kashin_quantize(x, 2, generator=g3)
    assert global_sha(g3) == end
    assert torch.equal(q.view(torch.int32), uqdme.kashin_quantize(x, 2, seeds=seeds).view(torch.int32))
    assert torch.equal(q.view(torch.int32), uqdme.kashin_decompress(msg).view(torch.int32))


def test_two_dropin_calls_back_to_back():
    import uqdme
    x = M.gen_input({"dist": "lognormal", "d": 1741, "seed": 12})
    torch.manual_seed(4)
    a, b = uqdme.Kashin_quantize(x, 1), uqdme.Kashin_quantize(x, 2)
    end = global_sha()
    torch.manual_seed(4)
    s1, s2 = int(torch.randint(0, 100, (1,))), int(torch.randint(0, 100, (1,)))
    assert global_sha() == end
    assert G.bits_equal(a, M.kashin(x, 1, s1)["out"]) and G.bits_equal(b, M.kashin(x, 2, s2)["out"])


def test_nmse_simulation_equals_dropin_calls():
    """The harness with schemes=("kashin",) against the drivers' loop (ND:88-95, 143-144, 151-157)
    made of drop-in calls on the same generators."""
    import uqdme
    from uqdme_amd import dme
    dim, users, inst, trials, rates, seed = 100, (1, 3), 2, 50, (1, 2), 42
    got = uqdme.nmse_simulation(dim=dim, users=users, num_instances=inst, num_trials=trials, rates=rates, seed=seed,
                                schemes=("kashin",))
    rs = np.random.RandomState(seed)
    saved = torch.get_rng_state()
    torch.manual_seed(seed)
    try:
        for ui, n in enumerate(users):
            for i in range(inst):
                vecs, vns = dme.draw_vectors("normal", n, dim, rs)
                xs = [torch.tensor(v, dtype=torch.float32) for v in vecs]
                emp = torch.stack(xs).sum(dim=0) / n
                est = {r: torch.zeros(dim) for r in rates}
                for v in xs:
                    for r in rates:
                        est[r] += torch.from_numpy(uqdme.Kashin_quantize(v, r)) / n
                for r in rates:
                    want = np.float32(float(torch.norm(est[r] - emp).pow(2) / (trials * vns * n)))
                    assert got[("kashin", r)]["script"][ui, i] == want, (n, i, r)
        end = global_sha()
        torch.manual_seed(seed)
        for _ in range(sum(users) * inst * len(rates)):
            torch.randint(0, 100, (1,))
        assert global_sha() == end
    finally:
        torch.set_rng_state(saved)


def test_flagged_client_raises_in_the_harness(monkeypatch):
    import uqdme
    from uqdme_amd import dme
    monkeypatch.setitem(dme.DISTRIBUTIONS, "normal", lambda rs, d: np.zeros(d))
    monkeypatch.setitem(dme.LEGACY, "normal", (5, 0.0, 0.0))     # uniform on [0, 0): all zeros
    with pytest.raises(RuntimeError):
        uqdme.nmse_simulation(dim=64, users=(2,), num_instances=1, schemes=("kashin",))
