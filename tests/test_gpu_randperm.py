"""GPU: randperm_prefix (uq_randperm_prefix) against live torch.randperm on a CPU generator, bit for bit, with
the generator's state afterwards, at every form of the words stage the plan hook names (one wave walks the
stream up to K = 9360 words, runs of 16 blocks from jumped states above), and the later stages on word
patterns no generator draws (uq_test_randperm_from_words) against the serial NumPy model."""
import ctypes

import numpy as np
import pytest
import torch

from tests import randperm_model as M

pytestmark = pytest.mark.gpu

WALK, JUMP, WORDS = 1, 2, 3
WALK_MAX_K = 9360                   # (624 + K - 1) // 624 + 1 <= 16 blocks


@pytest.fixture(scope="module")
def rp(gpu_ready):
    import uqdme  # noqa: F401
    from uqdme_amd import randperm
    return randperm


def generator(seed, pre):
    g = torch.Generator()
    g.manual_seed(seed)
    for _ in range(pre):
        torch.randint(0, 100, (1,), generator=g)
    return g


def ks(D):
    return sorted({0, min(1, D), D // 2, max(D - 2, 0), max(D - 1, 0), D})


def check(rp, D, k, pre, form=None, seed=77):
    g, t = generator(seed + D, pre), generator(seed + D, pre)
    ref = torch.randperm(D, generator=t)[:k]
    got = rp.randperm_prefix(D, k, generator=g)
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == (1, k)
    assert torch.equal(got.cpu()[0], ref), (D, k, pre)
    assert torch.equal(g.get_state(), t.get_state()), (D, k, pre)
    if form is not None and k:
        plan = rp.last_plan()
        assert plan["form"] == form and plan["K"] == min(k, D - 1), plan
        return plan


@pytest.mark.parametrize("D", (1, 2, 3, 8, 33, 624, 625, 1000, 4096))
def test_walk_form_every_k_and_start(rp, D):
    for pre in (0, 1, 623, 624, 1000):
        for k in ks(D):
            check(rp, D, k, pre, WALK if D > 1 else None)


def test_form_threshold(rp):
    """K one below, at and one above the last stream one wave walks; above it two runs of 16 blocks."""
    for K, form in ((WALK_MAX_K - 1, WALK), (WALK_MAX_K, WALK), (WALK_MAX_K + 1, JUMP)):
        for pre in (0, 623):
            plan = check(rp, K + 1, K + 1, pre, form)
            assert (plan["runs"], plan["run_blocks"]) == ((1, 16) if form == WALK else (2, 16)), plan
    # the same K as a short prefix of a long permutation: the plan follows K, not D
    plan = check(rp, 65536, WALK_MAX_K, 5, WALK)
    plan = check(rp, 65536, WALK_MAX_K + 1, 5, JUMP)
    assert plan["runs"] == 2


@pytest.mark.parametrize("pre", (0, 1, 623, 624, 1000))
def test_jump_form_run_boundaries(rp, pre):
    """Runs start at blocks 16, 32, ... of the stream, wherever in its first block the generator stands:
    K ending one word before, at and after the second run's first word, and several runs."""
    vG = 624 if pre % 624 == 0 else pre % 624                 # the stream's word 0 in its first block
    first = 16 * 624 - vG                                     # index of the second run's first word
    for K in (first, first + 1, first + 2):
        if K > WALK_MAX_K:
            check(rp, K + 1, K, pre, JUMP)
    plan = check(rp, 65536, 65536, pre, JUMP)
    assert plan["runs"] == 7 and plan["run_blocks"] == 16     # 107 blocks
    check(rp, 65536, 32768, pre, JUMP)


def test_large_permutation(rp):
    D = 1 << 20
    plan = check(rp, D, D // 2, 3, JUMP)
    assert plan["runs"] > 1
    check(rp, D, D, 700, JUMP)


def test_batch_consecutive_streams_and_explicit_states(rp):
    from uqdme_amd import _mtstate
    for D, k in ((1000, 500), (20000, 20000), (2, 2), (1, 1)):
        g, t = generator(5, 17), generator(5, 17)
        starts = []
        refs = []
        for _ in range(3):
            starts.append(_mtstate.generator_words(t)[1])
            refs.append(torch.randperm(D, generator=t)[:k])
        got = rp.randperm_prefix(D, k, 3, generator=g)
        assert torch.equal(got.cpu(), torch.stack(refs)), (D, k)
        assert torch.equal(g.get_state(), t.get_state())
        # the same rows from explicit states, in another order; no generator is touched
        before = torch.default_generator.get_state()
        got = rp.randperm_prefix(D, k, 3, px_states=np.stack(starts[::-1]))
        assert torch.equal(got.cpu(), torch.stack(refs[::-1])), (D, k)
        assert torch.equal(torch.default_generator.get_state(), before)


def test_default_generator_is_the_global_one(rp):
    torch.manual_seed(11)
    ref = torch.randperm(300)[:7]
    after = torch.default_generator.get_state()
    torch.manual_seed(11)
    got = rp.randperm_prefix(300, 7)
    assert torch.equal(got.cpu()[0], ref) and torch.equal(torch.default_generator.get_state(), after)


@pytest.mark.parametrize("D", (1, 2, 31, 32, 33, 1000, 20000))
def test_drop_bits_are_the_index_set(rp, D):
    for k in ks(D):
        g = generator(9, 2)
        idx, bits = rp.randperm_prefix(D, k, 2, generator=g, return_bits=True)
        assert bits.dtype == torch.int32 and bits.shape == (2, (D + 31) // 32)
        for j in range(2):
            want = M.drop_bits(idx[j].cpu().numpy(), D)
            assert np.array_equal(bits[j].cpu().numpy().view(np.uint32), want), (D, k, j)
            assert int(np.unpackbits(want.view(np.uint8)).sum()) == k          # k distinct coordinates below D


def test_small_workspace_splits_the_batch(rp):
    import uqdme
    lib = uqdme.load_library()
    for D, k in ((1000, 1000), (20000, 10000)):
        one = ctypes.c_size_t(0)
        assert lib.uq_randperm_prefix_workspace_bytes(1, D, k, ctypes.byref(one)) == 0
        g, t = generator(3, 0), generator(3, 0)
        refs = torch.stack([torch.randperm(D, generator=t)[:k] for _ in range(5)])
        whole = rp.randperm_prefix(D, k, 5, generator=generator(3, 0))
        assert rp.last_plan()["groups"] == 1
        # room for two clients, not three: groups of 2, 2 and 1
        got = rp.randperm_prefix(D, k, 5, generator=g, workspace_bytes=2 * one.value)
        plan = rp.last_plan()
        assert (plan["group"], plan["groups"]) == (2, 3), plan
        assert torch.equal(got.cpu(), refs) and torch.equal(whole.cpu(), refs)
        with pytest.raises(uqdme.UQError, match="workspace too small"):
            rp.randperm_prefix(D, k, 5, generator=g, workspace_bytes=one.value - 256)


@pytest.mark.parametrize("kind", ("zero", "last", "chain"))
def test_adversarial_words(rp, kind):
    """z = 0 (every step hits itself), every step hitting position D - 1 (one list of K writers), and
    z = 1 with a last 0 (a chain of K - 1 links, the most doubling rounds), against the serial model."""
    import uqdme
    from uqdme_amd._runtime import device, ptr, stream_ptr
    lib = uqdme.load_library()
    dev = device()
    for D, K in ((2, 1), (33, 32), (1000, 999), (4097, 4096), (5000, 4096), (5000, 257)):
        for k in sorted({K, K + 1 if K + 1 == D else K}):
            w = M.adversarial(kind, D, K)
            ref = M.serial(w, D, k)
            wd = torch.from_numpy(np.stack([w, w]).view(np.int32)).to(dev)
            idx = torch.empty((2, k), dtype=torch.int64, device=dev)
            bits = torch.empty((2, (D + 31) // 32), dtype=torch.int32, device=dev)
            ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
            rc = lib.uq_test_randperm_from_words(ptr(wd), 2, D, k, ptr(idx), ptr(bits), ptr(ws), ws.numel(), stream_ptr(dev))
            assert rc == 0, lib.uq_last_error()
            assert rp.last_plan()["form"] == WORDS
            for j in range(2):
                assert np.array_equal(idx[j].cpu().numpy(), ref), (kind, D, K, k)
                assert np.array_equal(bits[j].cpu().numpy().view(np.uint32), M.drop_bits(ref, D))


def test_random_words_through_the_test_entry(rp):
    import uqdme
    from uqdme_amd._runtime import device, ptr, stream_ptr
    lib = uqdme.load_library()
    dev = device()
    rng = np.random.default_rng(8)
    D, k = 3000, 3000
    w = rng.integers(0, 1 << 32, size=(1, D - 1), dtype=np.uint64).astype(np.uint32)
    idx = torch.empty((1, k), dtype=torch.int64, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    wd = torch.from_numpy(w.view(np.int32)).to(dev)
    assert lib.uq_test_randperm_from_words(ptr(wd), 1, D, k, ptr(idx), None, ptr(ws), ws.numel(), stream_ptr(dev)) == 0
    assert np.array_equal(idx[0].cpu().numpy(), M.serial(w[0], D, k))


def test_argument_checks(rp):
    g = generator(1, 0)
    before = g.get_state()
    for D, k in ((5, 6), (-1, 0), (5, -1), (rp.MAX_D, 1)):
        with pytest.raises(ValueError):
            rp.randperm_prefix(D, k, generator=g)
    assert torch.equal(g.get_state(), before)
