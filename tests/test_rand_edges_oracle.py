"""CPU: the NumPy restatement of Scalar_quantize and DRIVE_quantize_Hadamard
(tests/rand_schemes_model.py) against the reference's own outputs on the edge fixture
(tests/golden/make_golden_rand_edges.py): ragged last chunks of DRIVE (torch.norm's tail), NaN,
Inf, subnormal and overflowing inputs, 3 to 32 bits, several min / max slices, generator starts
at a block's edges; and the model's word stream against torch.rand itself."""
import numpy as np
import pytest
import torch

from tests import golden_data as G
from tests import rand_schemes_model as M
from tests.test_rand_schemes_oracle import run_model, state_sha

f32 = np.float32
PRE_SWEEP = (0, 1, 2, 63, 64, 65, 300, 575, 576, 577, 622, 623, 624, 625, 1247, 1248, 1249)
SCALAR_SWEEP_D = (1, 2, 63, 64, 65, 100, 623, 624, 625, 1249)
DRIVE_SWEEP_D = (1, 2, 3, 33, 64, 65, 1000, 2047, 2049, 4097)


@pytest.fixture(scope="module")
def fx():
    return M.load_fixture("rand_schemes_edges")


def old_tail_norm2(v):
    """The tail rule this fixture was made to catch: after the 8 fma lanes every remaining
    element by mul + add (torch takes 4 that way when 4 remain, and the last 1 to 3 by fma)."""
    v = np.asarray(v, f32)
    if v.shape[0] <= 2:
        return M.torch_norm2(v)
    n = v.shape[0] - v.shape[0] % 8
    acc = np.zeros(8, f32)
    for r in v[:n].reshape(-1, 8).astype(np.float64):
        acc = (acc.astype(np.float64) + r * r).astype(f32)
    s = acc[0]
    for j in range(1, 8):
        s = f32(s + acc[j])
    for t in v[n:]:
        s = f32(s + f32(t * t))
    return f32(np.sqrt(s))


def test_model_matches_every_edge_case(fx):
    meta, z = fx
    assert len(meta["cases"]) == 34
    for c in meta["cases"]:
        k = c["idx"]
        out, st = run_model(c, M.gen_input(c), M.start_state(c))
        if "sha" in c:
            assert G.sha(out) == c["sha"], c
            assert G.bits_equal(out[z[f"out{k}_pos"]], z[f"out{k}_s"]), c
        else:
            assert G.bits_equal(out, z[f"out{k}"]), (c, G.n_mismatch(out, z[f"out{k}"]))
        assert state_sha(c["gseed"], st) == c["state_sha"], c


def test_edge_fixture_sees_the_old_norm_tail(fx):
    """Every ragged "normal" DRIVE case of the fixture has a last chunk whose output bits change
    when the norm's tail is taken by mul + add throughout: the fixture tells the two orders
    apart (at least 8 cases are asked for; the seeds were chosen so that all 13 do)."""
    meta, z = fx
    differ = []
    for c in meta["cases"]:
        if c["scheme"] != "drive" or c["kind"] != "normal":
            continue
        assert c["d"] % 2048 % 4 != 0
        x, st = M.gen_input(c), M.start_state(c)
        old, st_old, _, S_old = M.drive_quantize(x, st, norm=old_tail_norm2)
        new, _, _, S_new = M.drive_quantize(x, st)
        assert G.bits_equal(new, z[f"out{c['idx']}"])
        # only the last chunk's S, and with it only the last chunk's outputs
        assert np.array_equal(S_old[:-1].view(np.uint32), S_new[:-1].view(np.uint32))
        last = c["d"] - c["d"] % 2048
        assert G.bits_equal(old[:last], new[:last])
        if not G.bits_equal(old, z[f"out{c['idx']}"]):
            assert S_old[-1] != S_new[-1]
            differ.append(c["d"])
    assert len(differ) >= 8, differ
    assert set(differ) == {3, 5, 6, 7, 9, 11, 13, 15, 2051, 2053, 2055, 4099, 6147}, differ


def test_edge_fixture_holds_what_the_gpu_tests_rely_on(fx):
    meta, z = fx
    cs = meta["cases"]
    dr = [c for c in cs if c["scheme"] == "drive"]
    sc = [c for c in cs if c["scheme"] == "scalar"]
    assert {c["pre"] for c in dr} >= {0, 1, 63, 575, 577, 623, 624}
    assert {c["pre"] for c in sc} >= {0, 623, 624}
    assert {c["bits"] for c in sc} >= {3, 8, 16, 24, 25, 32}
    assert {c["kind"] for c in cs} >= {"nan", "nan_at", "ninf_at", "pm_inf", "huge_span", "subnormal", "normal_1e19",
                                       "few_ulps", "neg_zero_third", "lognormal", "normal"}
    assert any(c["d"] == 266241 and "sha" in c for c in sc)
    # a NaN at d = 1: den is NaN, not 0, so the call takes one word
    ones = [c for c in sc if c["d"] == 1]
    assert {c["pre"] for c in ones} == {0, 624}
    for c in ones:
        assert np.isnan(M.gen_input(c)).all() and np.isnan(z[f"out{c['idx']}"]).all()
        assert state_sha(c["gseed"], M.mt_draw(M.start_state(c), 1)[1]) == c["state_sha"], c
        assert state_sha(c["gseed"], M.start_state(c)) != c["state_sha"], c
    # the NaN in the middle chunk of three poisons that chunk alone
    (c,) = [c for c in dr if c["kind"] == "nan_at"]
    out, clean = z[f"out{c['idx']}"], z[f"out{c['clean']}"]
    assert c["d"] == 6147 and 2048 <= c["at"] < 4096
    assert np.isnan(out[2048:4096]).all() and not np.isnan(clean).any()
    assert np.array_equal(out[:2048].view(np.uint32), clean[:2048].view(np.uint32))
    assert np.array_equal(out[4096:].view(np.uint32), clean[4096:].view(np.uint32))
    # -inf in the last chunk of d = 4099: the whole chunks before it are finite
    (c,) = [c for c in dr if c["kind"] == "ninf_at"]
    assert c["d"] == 4099 and c["at"] >= 4096 and np.isfinite(z[f"out{c['idx']}"][:4096]).all()
    # what the inputs are meant to be
    for c in cs:
        x = M.gen_input(c)
        if c["kind"] == "subnormal":
            assert (np.abs(x) < np.finfo(f32).tiny).all() and x.any()
        if c["kind"] == "huge_span":
            with np.errstate(over="ignore"):
                assert np.isfinite(x).all() and np.isinf(x.max() - x.min())
        if c["kind"] == "few_ulps":
            assert 1 < len(np.unique(x)) <= 64
        if c["kind"] == "neg_zero_third":
            assert np.signbit(x[::3]).all() and not x[::3].any()


# ---- the batch of tests/test_gpu_rand_edges.py's ragged DRIVE test -----------------------------------
RAGGED_D = (3, 5, 6, 7, 11, 13, 2051, 2055, 4099)
RAGGED_STATES = [(31, 0), (32, 577), (33, 624)]                 # (seed, pre draws) of rows 0, 1, 2
# input seeds of rows 1 (lognormal) and 2 (normal * 3e-4) at which, from those states, the old
# tail rule changes the output (row 0 takes the fixture's seed); found by scanning seeds upwards
RAGGED_ROW_SEEDS = {3: (22, 5), 5: (15, 1), 6: (15, 1), 7: (15, 2), 11: (6, 25), 13: (202, 37), 2051: (2, 8),
                    2055: (29, 1), 4099: (10, 1)}


def ragged_rows(d, vseed0):
    v1, v2 = RAGGED_ROW_SEEDS[d]
    return np.stack([M.gen_input({"vseed": vseed0, "d": d, "kind": "normal"}),
                     M.gen_input({"vseed": v1, "d": d, "kind": "lognormal"}),
                     M.gen_input({"vseed": v2, "d": d, "kind": "normal"}) * f32(3e-4)])


def ragged_vseeds(meta):
    return {c["d"]: c["vseed"] for c in meta["cases"] if c["scheme"] == "drive" and c["kind"] == "normal"}


def test_every_row_of_the_ragged_gpu_batch_sees_the_old_norm_tail(fx):
    """All 27 (d, row) pairs the GPU test compares with the model would differ, in S and in the
    output, from a kernel that took the whole tail by mul + add."""
    vs = ragged_vseeds(fx[0])
    for d in RAGGED_D:
        x = ragged_rows(d, vs[d])
        for j, (seed, pre) in enumerate(RAGGED_STATES):
            st = M.mt_draw(M.seeded_state(seed), pre)[1]
            old, _, _, S_old = M.drive_quantize(x[j], st, norm=old_tail_norm2)
            new, _, _, S_new = M.drive_quantize(x[j], st)
            assert S_old[-1].view(np.uint32) != S_new[-1].view(np.uint32), (d, j)
            assert not G.bits_equal(old, new), (d, j)


def _torch_stream(pre, n):
    """torch.rand(n) after manual_seed(9) and `pre` one-word draws -> (u f32 [n], state after)."""
    g = torch.Generator()
    g.manual_seed(9)
    for _ in range(pre):
        torch.randint(0, 100, (1,), generator=g)
    u = torch.rand(n, generator=g).numpy()
    return u, M.torch_state_unpack(g.get_state().numpy())


def test_model_stream_is_torch_rand_at_every_sweep_start():
    """The words the GPU sweep (tests/test_gpu_rand_edges.py) is checked against: after `pre`
    draws of seed 9, the model's next n words are torch.rand(n)'s and the end state is torch's,
    for Scalar's n = d and DRIVE's n = drive_words(d)."""
    lengths = sorted(set(SCALAR_SWEEP_D) | {M.drive_words(d) for d in DRIVE_SWEEP_D})
    for pre in PRE_SWEEP:
        st0 = M.mt_draw(M.seeded_state(9), pre)[1]
        for n in lengths:
            words, st1 = M.mt_draw(st0, n)
            u, (left, nxt, tw) = _torch_stream(pre, n)
            assert np.array_equal(M.uniforms(words).view(np.uint32), u.view(np.uint32)), (pre, n)
            assert (int(st1[0]), int(st1[1])) == (int(left), int(nxt)), (pre, n)
            assert np.array_equal(np.asarray(st1[2], np.uint32), np.asarray(tw, np.uint32)), (pre, n)
