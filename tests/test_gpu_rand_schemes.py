"""GPU: Scalar_quantize (AS:755-790) and DRIVE_quantize_Hadamard (AS:707-752) through the C ABI
(uq_scalar_quantize_f32, uq_drive_hadamard_f32), bit for bit against the reference's own outputs
on torch CPU (tests/golden/rand_schemes_vectors.*) and against the NumPy restatement
(tests/rand_schemes_model.py, pinned to that fixture by tests/test_rand_schemes_oracle.py).

Outputs are compared as u32 bit patterns (tests/golden_data.bits_equal; a NaN matches a NaN at
the same place whatever its sign and payload, which x86 and the GPU choose differently), and the
generator by the sha256 of torch.default_generator.get_state() or by its 626 state words."""
import hashlib

import numpy as np
import pytest
import torch

from tests import golden_data as G
from tests import rand_schemes_model as M

pytestmark = pytest.mark.gpu

SCALAR_D = (1, 2, 5, 623, 624, 625, 1251, 2048, 5000, 65553)
DRIVE_D = (1, 2, 3, 5, 1000, 2048, 2049, 3073, 4096, 5000, 6768)


@pytest.fixture(scope="module")
def fx(gpu_ready):
    return M.load_fixture()


def set_global(c):
    torch.manual_seed(c["gseed"])
    for _ in range(c["pre"]):
        torch.randint(0, 100, (1,))


def global_sha():
    return hashlib.sha256(torch.default_generator.get_state().numpy().tobytes()).hexdigest()


def states_of(specs):
    """[(seed, pre draws)] -> (oracle states, [n, 626] uint32)."""
    sts = [M.mt_draw(M.seeded_state(s), pre)[1] for s, pre in specs]
    return sts, np.stack([M.state_words(s) for s in sts])


def check_fixture(c, z, key, out):
    assert out.dtype == torch.float32 and out.is_cuda and out.shape == (c["d"],)
    out = out.cpu().numpy()
    if "sha" in c:
        assert G.bits_equal(out[z[key + "_pos"]], z[key + "_s"]), c
        assert G.sha(out) == c["sha"], c
    else:
        assert G.bits_equal(out, z[key]), (c, G.n_mismatch(out, z[key]))


def dropin(c):
    import uqdme
    return uqdme.Scalar_quantize if c["scheme"] == "scalar" else uqdme.DRIVE_quantize_Hadamard


def test_dropins_match_the_reference(fx):
    """Every fixture case through the drop-ins after torch.manual_seed and 0, 1 or 300 pre-draws:
    the reference's output and the reference's generator state afterwards.  Scalar at every d
    around a block's `left` and at 1, 2 and 4 bits, lognormal inputs, a constant vector, bits = 0,
    a NaN and an inf; DRIVE at P = 1, padded last chunks, chunk starts that are not block starts,
    an all-zero vector and zero pairs."""
    meta, z = fx
    seen = set()
    for c in meta["cases"]:
        x = M.gen_input(c)
        set_global(c)
        before = global_sha()
        xt = torch.from_numpy(x.copy())
        out = dropin(c)(xt, c["bits"])
        check_fixture(c, z, f"out{c['idx']}", out)
        assert global_sha() == c["state_sha"], c
        assert G.bits_equal(xt.numpy(), x)                                  # the input is only read
        if c["kind"] == "constant" or c["bits"] == 0:
            assert G.bits_equal(out.cpu().numpy(), x) and global_sha() == before, c
        if c["kind"] in ("nan", "inf"):
            assert np.isnan(out.cpu().numpy()).all(), c
        seen.add((c["scheme"], c["d"], c["bits"], c["pre"], c["kind"]))
    for d in SCALAR_D:
        for bits in (1, 2, 4):
            assert any(s[:3] == ("scalar", d, bits) for s in seen)
    for d in DRIVE_D:
        assert any(s[:2] == ("drive", d) for s in seen)
    for scheme in ("scalar", "drive"):
        assert {s[3] for s in seen if s[0] == scheme} >= {0, 1, 300}


def test_two_dropin_calls_back_to_back(fx):
    meta, z = fx
    for c in meta["pairs"]:
        x = M.gen_input(c)
        set_global(c)
        for t in range(2):
            check_fixture(c, z, f"pair{c['idx']}_{t}", dropin(c)(x, c["bits"]))
        assert global_sha() == c["state_sha"], c


def test_dropin_shapes():
    import uqdme
    for f in (uqdme.Scalar_quantize, uqdme.DRIVE_quantize_Hadamard):
        torch.manual_seed(5)
        before = global_sha()
        e = f(np.zeros(0, np.float32))
        assert e.shape == (0,) and e.is_cuda and e.dtype == torch.float32 and global_sha() == before
        with pytest.raises(RuntimeError):
            f(np.zeros((2, 3), np.float32))
        assert global_sha() == before
    x = torch.tensor([3.0, 1.0, 2.0], device="cuda")
    q = uqdme.Scalar_quantize(x, 1)
    assert q.data_ptr() != x.data_ptr() and set(q.cpu().tolist()) <= {1.0, 3.0}
    torch.manual_seed(9)
    one = uqdme.DRIVE_quantize_Hadamard(np.array([-2.5], np.float32))      # d = 1 comes back unchanged
    assert one.cpu().tolist() == [-2.5]


# ---- the batch forms against the model -----------------------------------------------------------
def scalar_rows(n, d, seed, kind="normal"):
    return np.stack([M.gen_input({"vseed": seed + j, "d": d, "kind": kind}) for j in range(n)])


def check_scalar_batch(x, bits, sts, q, new, info):
    q = q.cpu().numpy()
    for j in range(x.shape[0]):
        exp, st1, taken, const = M.scalar_quantize(x[j], bits, sts[j])
        assert G.bits_equal(q[j], exp), (j, G.n_mismatch(q[j], exp))
        assert np.array_equal(new[j], M.state_words(st1)), j
        assert int(info[j]) == (1 if const else 0), j
        assert taken == (0 if const else x.shape[1])


def test_scalar_batch_of_three_states():
    """Three clients from three generator states (fresh: left = 1; after one draw: left = 623;
    mid-block), one of them constant: its output is its input, its info bit is set and its state
    comes back unchanged."""
    import uqdme
    for d in (5, 625, 1251):
        x = scalar_rows(3, d, 40 + d, "lognormal")
        x[1] = -0.75
        sts, words = states_of([(11, 0), (12, 1), (13, 300)])
        for bits in (1, 2, 4):
            q, new, info = uqdme.scalar_quantize(torch.from_numpy(x), bits, px_states=words)
            check_scalar_batch(x, bits, sts, q, new, info)
            assert list(info) == [0, 1, 0] and np.array_equal(new[1], words[1])
            assert G.bits_equal(q[1].cpu().numpy(), x[1])


def test_scalar_batch_300_from_seeds():
    import uqdme
    n, d = 300, 2048
    x = scalar_rows(n, d, 7000)
    x[17] = 2.0
    seeds = np.arange(n) * 31 + 5
    q, new, info = uqdme.scalar_quantize(torch.from_numpy(x), 2, px_seeds=seeds)
    check_scalar_batch(x, 2, [M.seeded_state(int(s)) for s in seeds], q, new, info)
    assert int(info.sum()) == 1


def test_scalar_generator_form_runs_clients_in_order():
    """generator=: client j starts where clients 0..j-1 leave the stream (a constant one leaves
    it where it was), and the generator ends where the last one leaves it."""
    import uqdme
    from uqdme_amd.quicfl import generator_words
    x = scalar_rows(4, 1000, 8100)
    x[2] = 0.0
    g = torch.Generator()
    g.manual_seed(321)
    st = M.seeded_state(321)
    q, new, info = uqdme.scalar_quantize(torch.from_numpy(x), 4, generator=g)
    q = q.cpu().numpy()
    for j in range(4):
        exp, st, _, const = M.scalar_quantize(x[j], 4, st)
        assert G.bits_equal(q[j], exp) and np.array_equal(new[j], M.state_words(st)) and int(info[j]) == int(const)
    assert np.array_equal(generator_words(g)[1], M.state_words(st))
    assert int(st[1]) == (3 * 1000) % 624                    # three clients' words, not four


def check_drive_batch(x, sts, q, new, S):
    q, new, S = q.cpu().numpy(), new.cpu().numpy().view(np.uint32), S.cpu().numpy()
    for j in range(x.shape[0]):
        exp, st1, taken, eS = M.drive_quantize(x[j], sts[j])
        # S first: it tells the two reductions (torch's norm and sum orders) apart from the rest
        assert np.array_equal(S[j].view(np.uint32), eS.view(np.uint32)), (j, S[j], eS)
        assert G.bits_equal(q[j], exp), (j, G.n_mismatch(q[j], exp))
        assert np.array_equal(q[j].view(np.uint32), exp.view(np.uint32))     # signed zeros included
        assert np.array_equal(new[j], M.state_words(st1)), j
        assert taken == M.drive_words(x.shape[1])


@pytest.mark.parametrize("d", DRIVE_D)
def test_drive_scale_per_chunk_and_three_states(d):
    """n = 3 from three generator states at every d: S per chunk, outputs and end states against
    the model.  Row 1 is all zero (the signed zeros come from D), row 2 has zero pairs inside
    live chunks."""
    import uqdme
    x = np.stack([M.gen_input({"vseed": 50 + d, "d": d, "kind": "lognormal"}),
                  np.zeros(d, np.float32),
                  M.gen_input({"vseed": 51 + d, "d": d, "kind": "zero_pairs"})])
    sts, words = states_of([(21, 0), (22, 1), (23, 300)])
    q, new, S = uqdme.drive_quantize(torch.from_numpy(x), px_states=words, return_scale=True)
    assert S.shape == (3, (d + 2047) // 2048)
    check_drive_batch(x, sts, q, new, S)
    assert not q[1].cpu().numpy().any()                                      # +-0 only
    if d >= 1000:                                                            # both signs of D among that many
        assert np.signbit(q[1].cpu().numpy()).any() and not np.signbit(q[1].cpu().numpy()).all()


def test_drive_batch_300_from_seeds():
    import uqdme
    n, d = 300, 2048
    x = scalar_rows(n, d, 9000)
    seeds = np.arange(n) * 17 + 3
    q, new, S = uqdme.drive_quantize(torch.from_numpy(x), px_seeds=seeds, return_scale=True)
    check_drive_batch(x, [M.seeded_state(int(s)) for s in seeds], q, new, S)


def test_drive_generator_form_places_every_client():
    import uqdme
    from uqdme_amd.quicfl import generator_words
    x = scalar_rows(3, 3073, 9500)
    g = torch.Generator()
    g.manual_seed(77)
    torch.randint(0, 100, (1,), generator=g)
    st = M.mt_draw(M.seeded_state(77), 1)[1]
    q, new = uqdme.drive_quantize(torch.from_numpy(x), generator=g)
    q, new = q.cpu().numpy(), new.cpu().numpy().view(np.uint32)
    for j in range(3):
        exp, st, _, _ = M.drive_quantize(x[j], st)
        assert G.bits_equal(q[j], exp) and np.array_equal(new[j], M.state_words(st)), j
    assert np.array_equal(generator_words(g)[1], M.state_words(st))
