"""GPU: EDEN's receiver-side coordinate drop (AS:413-423) through every public path, bit for bit against the
reference's own outputs (tests/golden/eden_drop.*, pinned to the NumPy model by tests/test_eden_drop_model.py):
the drop-in with the global generator's state afterwards, the fused eden_quantize, eden_decompress on the u8 and
on the packed message; the rates below 1 bit through bits = 1, pdrop = 1 - r; batches against single calls in
the reference's word order; an independent cross-check that drops and divides with torch on the CPU; and
pdrop = 0, which runs what ran before."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from tests import eden_drop_model as M
from tests import eden_frac_model as F
from tests import golden_data as G

pytestmark = pytest.mark.gpu

OP_DECOMPRESS, NFIELDS, DROP_VECTOR = 1, 25, 1


@pytest.fixture(scope="module")
def fx(gpu_ready):
    return M.load()


@pytest.fixture(scope="module")
def U(gpu_ready):
    import uqdme
    return uqdme


def generator(gseed, draws):
    g = torch.Generator()
    g.manual_seed(gseed)
    for _ in range(draws):
        torch.randint(0, 100, (1,), generator=g)
    return g


def sha_of(g):
    return hashlib.sha256(g.get_state().numpy().tobytes()).hexdigest()


def check_out(c, z, out):
    out = np.asarray(out, np.float32).reshape(-1)
    assert out.shape == (c["d"],)
    if f"out{c['idx']}" in z:
        assert G.bits_equal(out, z[f"out{c['idx']}"]), (c, G.n_mismatch(out, z[f"out{c['idx']}"]))
    else:
        assert G.bits_equal(out[M.sample_pos(c["idx"], c["d"])], z[f"outs{c['idx']}"]), c
    assert G.sha(out) == c["out_sha"], c
    assert int((out == 0).sum()) == c["nzero"], c


def eden_plan(U):
    f = (ctypes.c_int64 * NFIELDS)()
    assert U.load_library().uq_test_last_eden_plan(OP_DECOMPRESS, f, NFIELDS) == 0
    return list(f)


def test_dropin_matches_the_reference(fx, U):
    """Every fixture case (bits 1, 2, 1.5, 1.3 with pdrop 0.5, 0.7, 0.25, 0.999 and 1e-7; the rates 0.5, 0.3
    and 0.75 as bits = 1 with the total drop share) through EDEN_quantize_Hadamard after torch.manual_seed and
    0, 1, 3 or 700 pre-draws: the reference's output and its generator state afterwards, by the vector form."""
    from uqdme_amd import eden, randperm
    cases, z = fx
    for c in cases:
        bits, pdrop = M.spelled(c)
        x = G.spec_gen(c)
        torch.manual_seed(c["gseed"])
        for _ in range(c["pre"]):
            torch.randint(0, 100, (1,))
        out = U.EDEN_quantize_Hadamard(torch.from_numpy(x.copy()), bits, pdrop=pdrop)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32
        check_out(c, z, out)
        assert sha_of(torch.default_generator) == c["state_sha"], c
        assert eden.eden_drop_form() == DROP_VECTOR
        if c["k"]:
            assert randperm.last_plan()["K"] == min(c["k"], c["D"] - 1), c


def test_fused_and_message_paths_match_the_reference(fx, U):
    """The same cases with the seed given and the generator standing behind the seed's word: the fused
    eden_quantize, eden_decompress of the u8 message and of the packed one.  Each leaves the generator
    D - 1 words on, where the reference's call leaves the global one."""
    cases, z = fx
    for c in cases:
        bits, pdrop = M.spelled(c)
        x = torch.from_numpy(G.spec_gen(c).copy()).view(1, -1)
        g = generator(c["gseed"], c["pre"] + 1)
        out, scale = U.eden_quantize(x, bits, seeds=[c["rseed"]], pdrop=pdrop, generator=g, return_scale=True)
        check_out(c, z, out.cpu().numpy())
        assert int(scale.cpu().numpy().view(np.uint32)[0]) == c["scale_bits"] and sha_of(g) == c["state_sha"], c
        msg = U.eden_with_pdrop(U.eden_compress(x, bits, seeds=[c["rseed"]]), pdrop)
        assert msg.pdrop == pdrop and G.sha(msg.bins.cpu().numpy().reshape(-1)) == c["bins_sha"]
        g = generator(c["gseed"], c["pre"] + 1)
        check_out(c, z, U.eden_decompress(msg, generator=g).cpu().numpy())
        assert sha_of(g) == c["state_sha"], c
        packed = U.eden_pack(msg)
        assert packed.pdrop == pdrop and packed.packed and U.eden_unpack(packed).pdrop == pdrop
        g = generator(c["gseed"], c["pre"] + 1)
        check_out(c, z, U.eden_decompress(packed, generator=g).cpu().numpy())
        assert sha_of(g) == c["state_sha"], c
        if c["d"] <= 4099:                               # a message packed by the sender's own kernels
            sent = U.eden_with_pdrop(U.eden_compress(x, bits, seeds=[c["rseed"]], packed=True), pdrop)
            g = generator(c["gseed"], c["pre"] + 1)
            check_out(c, z, U.eden_decompress(sent, generator=g).cpu().numpy())


@pytest.mark.parametrize("d,bits,pdrop", ((1000, 1, 0.5), (5000, 1.5, 0.25), (20000, 2, 1 - 0.3), (3, 1, 0.5)))
def test_batch_equals_single_calls_in_the_reference_word_order(U, d, bits, pdrop):
    x = torch.from_numpy(np.stack([G.spec_gen({"dist": "normal", "d": d, "seed": 900 + j}) for j in range(3)]))
    seeds = [7, 99, 7]
    # seeds given: the permutations take 3 (D - 1) consecutive words
    g, t = generator(21, 5), generator(21, 5)
    batch = U.eden_quantize(x, bits, seeds=seeds, pdrop=pdrop, generator=g)
    for j in range(3):
        one = U.eden_quantize(x[j:j + 1], bits, seeds=seeds[j:j + 1], pdrop=pdrop, generator=t)
        assert torch.equal(batch[j].view(torch.int32), one[0].view(torch.int32)), j
    assert torch.equal(g.get_state(), t.get_state())
    # ... and the message path takes the same words
    t = generator(21, 5)
    out = U.eden_decompress(U.eden_with_pdrop(U.eden_compress(x, bits, seeds=seeds), pdrop), generator=t)
    assert torch.equal(out.view(torch.int32), batch.view(torch.int32)) and torch.equal(g.get_state(), t.get_state())
    # seeds=None: per row one seed word, then D - 1 permutation words -- three wrapper calls, and the model's
    g, t = generator(22, 2), generator(22, 2)
    batch = U.eden_quantize(x, bits, pdrop=pdrop, generator=g)
    state = M.R.mt_draw(M.R.seeded_state(22), 2)[1]
    for j in range(3):
        one = U.eden_quantize(x[j:j + 1], bits, pdrop=pdrop, generator=t)
        assert torch.equal(batch[j].view(torch.int32), one[0].view(torch.int32)), j
        if d <= 5000:
            want, state, _, _, _ = M.wrapper_call(x[j].numpy(), bits, pdrop, state)
            assert G.bits_equal(batch[j].cpu().numpy(), want), j
    assert torch.equal(g.get_state(), t.get_state())
    # explicit start states: the rows of the first call again, no generator touched
    from uqdme_amd import _mtstate
    t = generator(21, 5)
    starts = []
    D = 1 << (d - 1).bit_length()
    for _ in range(3):
        starts.append(_mtstate.generator_words(t)[1])
        torch.randperm(D, generator=t)
    before = torch.default_generator.get_state()
    again = U.eden_quantize(x, bits, seeds=seeds, pdrop=pdrop, drop_states=np.stack(starts))
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))
    assert torch.equal(torch.default_generator.get_state(), before)


@pytest.mark.parametrize("d,bits,pdrop", ((1000, 1, 0.5), (4099, 2, 0.25), (4099, 1.3, 0.999), (70000, 1.5, 1 - 0.3),
                                          (64, 1, 1e-7)))
def test_receiver_against_torch_drop_and_the_plain_inverse(U, d, bits, pdrop):
    """Independent of the drop kernels: take the centroids, drop with torch.randperm and divide with torch on
    the CPU (AS:419-423 verbatim), then the GPU's plain inverse transform and scale * vec."""
    from oracle import uq_eden as E
    x = torch.from_numpy(G.spec_gen({"dist": "lognormal", "d": d, "seed": 31})).view(1, -1)
    seed = 42
    msg = U.eden_with_pdrop(U.eden_compress(x, bits, seeds=[seed]), pdrop)
    bins = msg.bins.cpu().numpy()[0].astype(np.int64)
    D = bins.shape[0]
    if isinstance(msg.nbits, tuple):
        m = F.mask(seed, D, msg.nbits[2])
        vec = np.where(m, E.centroids(2)[bins], E.centroids(1)[np.minimum(bins, 1)]).astype(np.float32)
    else:
        vec = E.centroids(msg.nbits)[bins].astype(np.float32)
    vec = torch.from_numpy(vec)
    g, t = generator(8, 9), generator(8, 9)
    ri = torch.randperm(D, generator=t)[:round(D * pdrop)]
    vec[ri] = 0
    vec /= (1 - pdrop)
    inv = U.randomized_inverse_hadamard_transform(vec.view(1, -1), [seed])
    want = (msg.scale.to(inv.device).view(1, 1) * inv)[:, :d]
    got = U.eden_decompress(msg, generator=g)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(g.get_state(), t.get_state())


@pytest.mark.parametrize("d,bits", ((1000, 1), (5000, 2), (5000, 1.5), (70000, 1)))
def test_pdrop_zero_runs_what_ran_before(U, d, bits):
    x = torch.from_numpy(np.stack([G.spec_gen({"dist": "normal", "d": d, "seed": 40 + j}) for j in range(2)]))
    g = generator(1, 0)
    before = g.get_state()
    torch.manual_seed(2)
    gbefore = torch.default_generator.get_state()
    plain = U.eden_quantize(x, bits, seeds=[3, 4])
    plan = eden_plan(U)
    zero = U.eden_quantize(x, bits, seeds=[3, 4], pdrop=0.0, generator=g)
    assert eden_plan(U) == plan and torch.equal(zero.view(torch.int32), plain.view(torch.int32))
    msg = U.eden_compress(x, bits, seeds=[3, 4])
    assert msg.pdrop == 0.0
    out = U.eden_decompress(msg, generator=g)
    assert eden_plan(U) == plan and torch.equal(out.view(torch.int32), plain.view(torch.int32))
    out = U.eden_decompress(U.eden_pack(msg), generator=g)
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))
    assert torch.equal(g.get_state(), before) and torch.equal(torch.default_generator.get_state(), gbefore)
    # the drop-in at pdrop = 0 takes the seed's word alone
    torch.manual_seed(5)
    a = U.EDEN_quantize_Hadamard(x[0], bits)
    sa = torch.default_generator.get_state()
    torch.manual_seed(5)
    b = U.EDEN_quantize_Hadamard(x[0], bits, 0.0)
    assert G.bits_equal(a, b) and torch.equal(torch.default_generator.get_state(), sa)


def test_sub_1_bit_spelling_still_raises(U):
    torch.manual_seed(1)
    before = torch.default_generator.get_state()
    with pytest.raises(ValueError, match="pdrop=1 - r"):
        U.EDEN_quantize_Hadamard(np.ones(8, np.float32), 0.5)
    assert torch.equal(torch.default_generator.get_state(), before)


DROP_STARTS = ((101, 0), (202, 300), (303, 623), (404, 1000))      # freshly seeded, mid-block, next = 623, second block


@pytest.mark.parametrize("bits", (1, 1.5))
def test_batch_whose_permutation_runs_are_set_by_the_batch(U, bits):
    """n = 3200, d = 16384, pdrop = 0.75: k = 12288 words touch B = 21 blocks and n B / 4096 asks for runs of 17
    blocks (two runs, the second of 4), where every other test of the drop has runs of 16.  All rows against the
    same rows in calls of 64 (runs of 16), and sampled rows against the torch path of
    test_receiver_against_torch_drop_and_the_plain_inverse: centroids from the bins, torch.randperm and the
    division on the CPU, the GPU's plain inverse.  drop_states tile 4 generator states; seeds are given."""
    from oracle import uq_eden as E
    from tests import randperm_model as RM
    from uqdme_amd import _mtstate, randperm
    n, d, pdrop = 3200, 16384, 0.75
    k = round(d * pdrop)
    rng = np.random.default_rng(16384)
    x = torch.from_numpy(rng.lognormal(0, 1, (64, d)).astype(np.float32) * rng.choice([-1, 1], (64, d)).astype(np.float32))
    x = x.cuda().repeat(n // 64, 1)
    seeds = [int(v) for v in rng.integers(0, 1 << 31, n)]
    four = np.stack([_mtstate.generator_words(generator(*a))[1] for a in DROP_STARTS])
    states = four[np.arange(n) % 4]
    before = torch.default_generator.get_state()
    big = U.eden_quantize(x, bits, seeds=seeds, pdrop=pdrop, drop_states=states)
    plan = randperm.last_plan()
    assert (plan["form"], plan["runs"], plan["run_blocks"], plan["K"]) == RM.plan(n, d, k) == (RM.JUMP, 2, 17, 12288), plan
    assert plan["group"] * plan["groups"] >= n and plan["group"] == RM.group(n, d, k, RM.WORKSPACE_CAP), plan
    for c0 in range(0, n, 64):
        part = U.eden_quantize(x[c0:c0 + 64], bits, seeds=seeds[c0:c0 + 64], pdrop=pdrop, drop_states=states[c0:c0 + 64])
        assert randperm.last_plan()["run_blocks"] == 16 and randperm.last_plan()["runs"] == 2
        assert torch.equal(part.view(torch.int32), big[c0:c0 + 64].view(torch.int32)), c0
    assert torch.equal(torch.default_generator.get_state(), before)
    rows = {0, 1, 2, 3, 1601, 2046, n - 2, n - 1}                  # every start state among them
    G0 = plan["group"]
    if plan["groups"] > 1:                                         # either side of each group boundary
        rows |= {G0 - 1, G0, (plan["groups"] - 1) * G0 - 1, (plan["groups"] - 1) * G0}
    for j in sorted(rows):
        msg = U.eden_with_pdrop(U.eden_compress(x[j:j + 1], bits, seeds=[seeds[j]]), pdrop)
        bins = msg.bins.cpu().numpy()[0].astype(np.int64)
        if isinstance(msg.nbits, tuple):
            m = F.mask(seeds[j], d, msg.nbits[2])
            vec = np.where(m, E.centroids(2)[bins], E.centroids(1)[np.minimum(bins, 1)]).astype(np.float32)
        else:
            vec = E.centroids(msg.nbits)[bins].astype(np.float32)
        vec = torch.from_numpy(vec)
        ri = torch.randperm(d, generator=generator(*DROP_STARTS[j % 4]))[:round(d * pdrop)]
        vec[ri] = 0
        vec /= (1 - pdrop)
        inv = U.randomized_inverse_hadamard_transform(vec.view(1, -1), [seeds[j]])
        want = (msg.scale.to(inv.device).view(1, 1) * inv)[:, :d]
        assert torch.equal(big[j:j + 1].view(torch.int32), want.view(torch.int32)), j
