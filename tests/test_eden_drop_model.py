"""CPU: the NumPy model of EDEN with the coordinate drop (tests/eden_drop_model.py) against every case the
reference produced (tests/golden/eden_drop.*, made by make_golden_eden_drop.py): the drawn seed, the bins, the
scale, the output bit for bit, its count of exact zeros and the global generator's state afterwards.  So the
fixtures the GPU tests compare with are verified here, and with them the reading of AS:413-423 the kernels
implement: Python's round, torch.randperm's prefix, a true f32 division by f32(1 - p)."""
import numpy as np
import pytest

from tests import eden_drop_model as M
from tests import golden_data as G
from tests import randperm_model as R

CASES, Z = M.load()


def test_fixture_covers_the_issue():
    small = [c for c in CASES if c["nbits"] >= 1]
    for bits in (1, 2, 1.5, 1.3):
        assert {c["pdrop"] for c in small if c["nbits"] == bits} >= {0.5, 1 - 0.3, 0.25, 0.999, 1e-7}
        assert {c["d"] for c in small if c["nbits"] == bits} >= {1, 2, 5, 64, 1000, 2048, 4099}
    assert {c["d"] for c in CASES} == {1, 2, 5, 64, 1000, 2048, 4099, 65536, 172554, 1 << 20}
    sub = [c for c in CASES if c["nbits"] < 1]
    assert {(c["nbits"], c["pdrop"]) for c in sub} == {(r, q) for r in (0.5, 0.3, 0.75) for q in (0, 0.5)}
    assert all(c["wrapper"] for c in sub if c["pdrop"] == 0)
    assert any(c["k"] == 0 and c["p"] > 0 for c in CASES) and any(c["k"] == c["D"] for c in CASES)
    assert {c["pre"] for c in CASES} == {0, 1, 3, 700}


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"{c['idx']}-d{c['d']}-b{c['nbits']}-p{c['pdrop']}")
def test_model_matches_the_reference(c):
    bits, pdrop = M.spelled(c)
    assert pdrop == c["p"] and round(c["D"] * pdrop) == c["k"]
    x = G.spec_gen(c)
    out, state, seed, bins, scale = M.wrapper_call(x, bits, pdrop, M.start_state(c))
    assert seed == c["rseed"]
    assert G.sha(bins) == c["bins_sha"] and int(np.float32(scale).view(np.uint32)) == c["scale_bits"]
    if f"out{c['idx']}" in Z:
        assert G.bits_equal(out, Z[f"out{c['idx']}"]), G.n_mismatch(out, Z[f"out{c['idx']}"])
    else:
        assert G.bits_equal(out[M.sample_pos(c["idx"], c["d"])], Z[f"outs{c['idx']}"])
    assert G.sha(out) == c["out_sha"]
    assert int((out == 0).sum()) == c["nzero"]
    assert M.state_sha(c["gseed"], state) == c["state_sha"]
    # the generator took one seed word and D - 1 permutation words
    _, want = R.mt_draw(M.start_state(c), 1 + R.words_taken(c["D"]))
    assert want[0] == state[0] and np.array_equal(want[2], state[2])
