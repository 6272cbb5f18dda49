"""CPU: the serial and the parallel model of torch.randperm(D)[:k] (tests/randperm_model.py) against live
torch.randperm on a CPU generator, bit for bit, with the generator's state afterwards; and the parallel
model against the serial one on word arrays no generator would draw."""
import numpy as np
import pytest
import torch

from tests import randperm_model as M

DS = (1, 2, 3, 8, 33, 624, 625, 1000, 4096, 65536)
PRE = (0, 1, 623, 624, 1000)


def ks(D):
    return sorted({0, min(1, D), D // 2, max(D - 2, 0), max(D - 1, 0), D})


def generator(seed, pre):
    g = torch.Generator()
    g.manual_seed(seed)
    for _ in range(pre):
        torch.randint(0, 100, (1,), generator=g)                      # one word each
    return g


def state_of(g):
    return M.torch_state_unpack(g.get_state().numpy())


@pytest.mark.parametrize("D", DS)
def test_models_match_torch_randperm(D):
    for pre in PRE:
        g = generator(1234 + D, pre)
        st = state_of(g)
        ref = torch.randperm(D, generator=g).numpy()
        words, after = M.mt_draw(st, M.words_taken(D))
        left, nxt, mt = state_of(g)
        if D > 1:                                                     # D <= 1 takes no word: the state is untouched
            assert (after[0], after[1]) == (left, nxt) and np.array_equal(after[2], mt), (D, pre)
        else:
            assert st[0] == left and st[1] == nxt and np.array_equal(st[2], mt)
        for k in ks(D):
            assert np.array_equal(M.parallel(words, D, k), ref[:k]), (D, pre, k)
            if D <= 4096:
                assert np.array_equal(M.serial(words, D, k), ref[:k]), (D, pre, k)
            got, after2 = M.randperm_prefix(st, D, k)
            assert np.array_equal(got, ref[:k]) and after2[0] == after[0] and np.array_equal(after2[2], after[2])


def test_state_after_is_rand_of_d_minus_1():
    """randperm(D) leaves the generator where torch.rand(D - 1) leaves it: D - 1 words."""
    for D in (2, 625, 1000):
        a, b = generator(7, 3), generator(7, 3)
        torch.randperm(D, generator=a)
        torch.rand(D - 1, generator=b)
        assert torch.equal(a.get_state(), b.get_state())


@pytest.mark.parametrize("kind", ("zero", "last", "chain"))
def test_parallel_model_on_adversarial_words(kind):
    for D in (2, 3, 8, 33, 257, 2000):
        for K in sorted({1, 2, D // 2, D - 2, D - 1} - {0, -1}):
            if K < 1:
                continue
            w = M.adversarial(kind, D, K)
            h = M.targets(w, D, K)
            i = np.arange(K)
            if kind == "zero":
                assert np.array_equal(h, i)
            elif kind == "last":
                assert (h == D - 1).all()
            else:
                assert np.array_equal(h[:K - 1], i[:K - 1] + 1) and h[K - 1] == K - 1
            for k in sorted({K, K + 1 if K + 1 == D else K}):          # k = D adds the virtual step
                ww = w if k == K else np.concatenate([w, np.zeros(1, np.uint32)])
                assert np.array_equal(M.parallel(ww, D, k), M.serial(ww, D, k)), (kind, D, K, k)


def test_parallel_model_on_random_words():
    rng = np.random.default_rng(5)
    for D in (2, 5, 64, 1000, 2000):
        for k in ks(D):
            w = rng.integers(0, 1 << 32, size=max(D - 1, 1), dtype=np.uint64).astype(np.uint32)
            assert np.array_equal(M.parallel(w, D, k), M.serial(w, D, k)), (D, k)


def test_drop_bits_numbering():
    bits = M.drop_bits([0, 31, 32, 70], 71)
    assert bits.tolist() == [0x80000001, 1, 1 << 6]


PLAN_TABLE = (
    # n, D, k -> form, runs R, run blocks L
    ((3, 20000, 20000), (M.JUMP, 3, 16)),
    ((2500, 20000, 20000), (M.JUMP, 2, 21)),            # L set by the batch, a last run of 13 blocks
    ((4096, 20000, 20000), (M.JUMP, 1, 34)),            # L = B: one run, no jump taken
    ((5000, 20000, 10000), (M.JUMP, 1, 18)),
    ((1300, 65536, 32768), (M.JUMP, 3, 18)),
    ((128, 1 << 20, 1 << 19), (M.JUMP, 32, 27)),
    ((128, 1 << 20, 1 << 20), (M.JUMP, 32, 53)),
    ((1, 10_223_000, 10_223_000), (M.JUMP, 964, 17)),   # B = 16385: L set by the 1024 runs a client may have
    ((1, 10_222_000, 10_222_000), (M.JUMP, 1024, 16)),  # B = 16383: 1024 runs of 16, the last of 15 blocks
)


@pytest.mark.parametrize("args,want", PLAN_TABLE)
def test_plan_table(args, want):
    n, D, k = args
    form, R, L, K = M.plan(n, D, k)
    assert (form, R, L) == want and K == min(k, D - 1)
    B = (624 + K - 1) // 624 + 1
    assert (R - 1) * L < B <= R * L                                   # the runs cover the blocks, none is empty


def test_plan_walk_form_and_empty_calls():
    assert M.plan(1, 9361, 9361) == (M.WALK, 1, 16, 9360)
    assert M.plan(7, 9362, 9362) == (M.JUMP, 2, 16, 9361)
    assert M.plan(5000, 65536, 9360) == (M.WALK, 1, 16, 9360)         # the walk form whatever the batch
    assert M.plan(1, 2, 2) == (M.WALK, 1, 2, 1) and M.plan(1, 1, 1) == (M.WALK, 1, 1, 0)
    assert M.plan(0, 100, 10) == (0, 0, 0, 0) and M.plan(3, 100, 0) == (0, 0, 0, 0)
    # the 1024-run limit takes over between B = 16384 and 16385 blocks: K = 10 222 992 and 10 222 993 words
    assert M.plan(1, 10_222_993, 10_222_993)[:3] == (M.JUMP, 1024, 16)
    assert M.plan(1, 10_222_994, 10_222_994)[:3] == (M.JUMP, 964, 17)


def test_workspace_model_matches_the_library():
    """tests/randperm_model.py's workspace_bytes and group against uq_randperm_prefix_workspace_bytes (host code):
    a batch below the 1 GiB cap asks for its n clients' worth, one above for its largest group's."""
    import ctypes

    import uqdme
    lib = uqdme.load_library()
    b = ctypes.c_size_t(0)
    for (n, D, k), _ in PLAN_TABLE + (((5, 1000, 1000), None), ((40, 20000, 20000), None), ((128, 1 << 22, 1 << 22), None)):
        assert lib.uq_randperm_prefix_workspace_bytes(n, D, k, ctypes.byref(b)) == 0
        G = max(1, M.group(n, D, k, M.WORKSPACE_CAP))
        assert b.value == M.workspace_bytes(n, D, k, G), (n, D, k)
        assert G == n or M.workspace_bytes(n, D, k, G + 1) > M.WORKSPACE_CAP
        assert M.group(n, D, k, b.value) == G and M.group(n, D, k, M.workspace_bytes(n, D, k, 1) - 1) == 0
