"""Host-only: torch's CPU generator as (left, next, 624 words) and the packing of a batch call's
per-client generators (_mtstate.py), which QUIC-FL's sender and the Scalar / DRIVE batch forms
share.  No GPU: the uploader is run with the CPU as its device."""
import numpy as np
import pytest
import torch

import uqdme  # noqa: F401  (registers the uqdme_amd package alias)
from uqdme_amd import _mtstate as M
from uqdme_amd import quicfl


def gen_after(seed, draws):
    g = torch.Generator().manual_seed(seed)
    if draws:
        torch.rand(draws, generator=g)
    return g


def states(specs):
    return np.stack([M.generator_words(gen_after(s, k))[1] for s, k in specs])


def test_quicfl_reexports_the_generator_helpers():
    for name in ("STATE_WORDS", "generator_words", "set_generator_words", "advance_generator"):
        assert getattr(quicfl, name) is getattr(M, name)


def test_pack_states_layout():
    w = states([(1, 0), (2, 1), (3, 700)])
    assert w.shape == (3, M.STATE_WORDS) and w.dtype == np.uint32
    packed, is_states = M.pack_generators(3, w, None)
    assert is_states and packed.dtype == np.int32 and packed.shape == (3 * 626,)
    assert np.array_equal(packed.view(np.uint32), w.reshape(-1))
    # nested lists and a torch tensor of the same words pack to the same bytes
    for form in (w.tolist(), torch.from_numpy(w.astype(np.int64))):
        assert M.pack_generators(3, form, None)[0].tobytes() == packed.tobytes()


def test_pack_seeds_keeps_the_low_32_bits():
    for seeds in ([-1, 2**32 + 5, 7], torch.tensor([-1, 2**32 + 5, 7]), np.array([-1, 2**32 + 5, 7])):
        packed, is_states = M.pack_generators(3, None, seeds)
        assert not is_states and packed.dtype == np.int32
        assert packed.view(np.uint32).tolist() == [0xFFFFFFFF, 5, 7]


def with_left_next(left, nxt):
    w = states([(5, 3)])
    w[0, 0], w[0, 1] = left, nxt
    return w


def test_pack_refuses_bad_input():
    w = states([(1, 0), (2, 1), (3, 2)])
    with pytest.raises(ValueError):
        M.pack_generators(2, w, None)                                # three states for two clients
    with pytest.raises(ValueError, match="one px seed per client"):
        M.pack_generators(2, None, [1, 2, 3])
    with pytest.raises(ValueError, match="one px seed per message"):
        M.pack_generators(2, None, [1, 2, 3], "message")
    with pytest.raises(ValueError, match="required"):
        M.pack_generators(2, None, None)
    for left, nxt in ((0, 0), (625, 0), (5, 619)):
        with pytest.raises(ValueError, match="invariant"):
            M.pack_generators(1, with_left_next(left, nxt), None)
        with pytest.raises(ValueError, match="invariant"):
            M.check_state(with_left_next(left, nxt)[0])


def test_pack_accepts_every_state_torch_can_be_in():
    for nxt in (0, 1, 624, 12345):                                   # left = 1: the next draw twists, next is unused
        M.pack_generators(1, with_left_next(1, nxt), None)
    for left in (2, 5, 624):
        M.pack_generators(1, with_left_next(left, 625 - left), None)


def test_quicfl_and_the_rand_schemes_pack_the_same_bytes():
    """The two routines this one replaced, restated: QUIC-FL's sender put `tail` behind its prng
    seeds, the Scalar / DRIVE batch forms sent `alone`; for the same generators they are the same
    bytes, and both are what pack_generators returns."""
    n = 4
    w = states([(11, 0), (12, 1), (13, 623), (14, 624)])
    seeds = [-(2**40) - 3, -1, 2**31, 2**32 + 5]
    ps = np.array([7, 65535, 0, 12], np.int32)
    for px_states, px_seeds in ((w, None), (None, seeds)):
        if px_states is not None:
            tail = np.asarray(px_states, np.uint32).reshape(n, 626).view(np.int32).reshape(-1)
            alone = np.ascontiguousarray(np.asarray(px_states, np.uint32).reshape(n, 626)).view(np.int32)
        else:
            s = np.asarray(torch.as_tensor(px_seeds, dtype=torch.int64).reshape(-1).numpy(), np.int64)
            tail = alone = (s & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        assert tail.tobytes() == alone.tobytes()
        for who in ("client", "message"):
            assert M.pack_generators(n, px_states, px_seeds, who)[0].tobytes() == tail.tobytes()
        # the uploader: one tensor, the head in front (QUIC-FL) or none (Scalar, DRIVE)
        head, st, sd = M.upload_generators(n, px_states, px_seeds, "cpu", "message", head=ps)
        got = st if px_states is not None else sd
        assert (st is None) != (sd is None) and got.dtype == torch.int32
        assert got.shape == ((n, 626) if px_states is not None else (n,))
        assert head.numpy().tobytes() == ps.tobytes() and got.numpy().tobytes() == tail.tobytes()
        assert got.data_ptr() == head.data_ptr() + 4 * n                      # one buffer, one copy
        head, st, sd = M.upload_generators(n, px_states, px_seeds, "cpu")
        got = st if px_states is not None else sd
        assert head is None and got.numpy().tobytes() == alone.tobytes()


@pytest.mark.parametrize("draws,left,nxt", [(0, 1, None), (1, 624, 1), (624, 1, None)])
def test_generator_words_round_trip(draws, left, nxt):
    g = gen_after(4242, draws)
    st, w = M.generator_words(g)
    assert w.shape == (626,) and w.dtype == np.uint32 and int(w[0]) == left
    if nxt is not None:
        assert int(w[1]) == nxt
    M.check_state(w)
    assert np.array_equal(st, g.get_state().numpy())
    h = torch.Generator().manual_seed(1)
    M.set_generator_words(h, st, w)
    assert torch.equal(h.get_state(), g.get_state())
    st2, w2 = M.generator_words(h)
    assert np.array_equal(w2, w) and np.array_equal(st2, st)
    assert torch.equal(torch.rand(1000, generator=h), torch.rand(1000, generator=g))
