"""CPU: the host rules of EDEN's coordinate drop and of randperm_prefix's C entry points -- argument checks
that raise before any draw, the message field, the divided centroid tables, the new symbols' ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import uqdme
from uqdme_amd import eden, randperm
from uqdme_amd._lib import SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_PDROP = (1, 1.0, 1.5, -0.1, -1e-9, float("nan"), float("inf"), "0.5", None)


@pytest.fixture(scope="module")
def lib():
    return uqdme.load_library()


@pytest.mark.parametrize("bad", BAD_PDROP)
def test_pdrop_outside_0_1_raises_before_any_draw(bad):
    torch.manual_seed(3)
    before = torch.default_generator.get_state()
    g = torch.Generator()
    g.manual_seed(4)
    gb = g.get_state()
    x = np.ones((2, 8), np.float32)
    with pytest.raises(ValueError, match="pdrop"):
        uqdme.EDEN_quantize_Hadamard(x[0], 1, pdrop=bad)
    with pytest.raises(ValueError, match="pdrop"):
        uqdme.eden_quantize(x, 1, pdrop=bad, generator=g)
    good = uqdme.EdenMessage(torch.zeros((2, 8), dtype=torch.uint8), torch.ones(2), torch.zeros(2, dtype=torch.int64), 1, 8)
    with pytest.raises(ValueError, match="pdrop"):
        uqdme.eden_with_pdrop(good, bad)
    msg = uqdme.EdenMessage(torch.zeros((2, 8), dtype=torch.uint8), torch.ones(2), torch.zeros(2, dtype=torch.int64), 1, 8,
                            pdrop=bad)
    with pytest.raises(ValueError, match="pdrop"):
        uqdme.eden_decompress(msg, generator=g)
    assert torch.equal(torch.default_generator.get_state(), before) and torch.equal(g.get_state(), gb)


def test_pdrop_accepts_the_half_open_interval():
    for ok in (0, 0.0, 1e-7, 0.5, np.float32(0.25), torch.tensor(0.75), 1 - 2 ** -53):
        assert 0.0 <= eden._pdrop(ok) < 1.0


def test_message_field_is_last_and_defaults_to_zero():
    b, s, r = torch.zeros((1, 4), dtype=torch.uint8), torch.ones(1), torch.zeros(1, dtype=torch.int64)
    old = uqdme.EdenMessage(b, s, r, 1, 4)                                 # the positional arguments of before
    assert old.pdrop == 0.0 and old.payload is None and not old.packed
    packed = uqdme.EdenMessage(None, s, r, 2, 4, torch.zeros((1, 2), dtype=torch.int32), torch.tensor([8]))
    assert packed.pdrop == 0.0 and packed.packed
    import dataclasses
    assert [f.name for f in dataclasses.fields(uqdme.EdenMessage)][-1] == "pdrop"
    with_p = uqdme.eden_with_pdrop(old, 0.25)
    assert with_p.pdrop == 0.25 and old.pdrop == 0.0 and with_p.bins is old.bins and with_p.dim == 4


def test_sub_1_bit_spelling_points_to_pdrop():
    with pytest.raises(ValueError, match=r"pdrop=1 - r"):
        eden._bits(0.5)


@pytest.mark.parametrize("p", (0.5, 1 - 0.3, 0.25, 0.999, 1e-7, 0.75, 0.85))
def test_divided_centroids_are_the_vector_division(p):
    """AS:423 divides the whole rotated vector; the binding divides the tables.  Both are torch's f32
    division of the same f32 values by the same Python float: equal element by element, and a true division
    (not a product with the reciprocal, which differs at 0.25 and 0.999)."""
    for nb in (1, 2, (1, 2, 0.3)):
        got = np.array(list(eden._divided_centroids(nb, p)), np.float32)
        tabs = eden._CENTROIDS[2] + eden._CENTROIDS[1] if isinstance(nb, tuple) else eden._CENTROIDS[nb]
        vec = torch.tensor(tabs, dtype=torch.float32).repeat(1000)         # long enough for torch's vector path
        vec /= (1 - p)
        assert np.array_equal(vec.numpy()[:len(tabs)].view(np.uint32), got.view(np.uint32))
        assert np.array_equal(vec.numpy().reshape(1000, -1).view(np.uint32), np.tile(got.view(np.uint32), (1000, 1)))
        true = (np.array(tabs, np.float32).astype(np.float64) / np.float64(np.float32(1 - p))).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), true.view(np.uint32))
        assert np.array_equal(got[:len(got) // 2], -got[len(got) // 2:][::-1]) or isinstance(nb, tuple)


def test_new_symbols_match_the_header(lib):
    header = open(os.path.join(ROOT, "include", "uq_dme.h")).read()
    for name in ("uq_randperm_prefix_workspace_bytes", "uq_randperm_prefix", "uq_test_randperm_from_words",
                 "uq_test_last_randperm_plan", "uq_test_last_eden_drop_form", "uq_eden_decompress_drop_f32",
                 "uq_eden_decompress_packed_drop_f32", "uq_eden_drop_f32"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    for define in ("UQ_RANDPERM_PLAN_FIELDS 6", "UQ_RANDPERM_FORM_WALK 1", "UQ_RANDPERM_FORM_JUMP 2",
                   "UQ_RANDPERM_FORM_WORDS 3", "UQ_EDEN_DROP_VECTOR 1"):
        assert "#define " + define in header


def test_randperm_argument_checks_launch_nothing(lib):
    b = ctypes.c_size_t(7)
    assert lib.uq_randperm_prefix_workspace_bytes(3, 1000, 500, ctypes.byref(b)) == 0 and b.value > 3 * 4 * 2500
    assert lib.uq_randperm_prefix_workspace_bytes(3, 1000, 0, ctypes.byref(b)) == 0 and b.value == 0
    assert lib.uq_randperm_prefix_workspace_bytes(0, 1000, 10, ctypes.byref(b)) == 0 and b.value == 0
    for n, D, k in ((1, 5, 6), (-1, 5, 1), (1, -5, 0), (1, 5, -1), (1, randperm.MAX_D, 1), (1, 1 << 40, 1)):
        assert lib.uq_randperm_prefix_workspace_bytes(n, D, k, ctypes.byref(b)) == -1, (n, D, k)
        assert lib.uq_randperm_prefix(None, n, D, k, None, None, None, 0, None) == -1, (n, D, k)
    assert lib.uq_randperm_prefix_workspace_bytes(1, randperm.MAX_D - 1, 1, ctypes.byref(b)) == 0
    assert lib.uq_randperm_prefix(None, 0, 100, 10, None, None, None, 0, None) == 0          # an empty batch
    assert lib.uq_randperm_prefix(None, 2, 100, 0, None, None, None, 0, None) == 0           # k = 0, no outputs
    plan = (ctypes.c_int64 * 6)(*[9] * 6)
    assert lib.uq_test_last_randperm_plan(plan, 6) == 0 and list(plan) == [0] * 6
    # a workspace that holds one client is the least; one byte less is refused before any launch
    one = ctypes.c_size_t(0)
    assert lib.uq_randperm_prefix_workspace_bytes(1, 64, 64, ctypes.byref(one)) == 0
    fake = ctypes.c_void_p(256)                                            # (never dereferenced: the call fails first)
    assert lib.uq_randperm_prefix(fake, 4, 64, 64, None, None, fake, one.value - 1, None) == -3
    assert b"workspace too small" in lib.uq_last_error()


def test_workspace_request_is_bounded(lib):
    """A large batch asks for about a GiB at most; the call processes it in groups of clients."""
    b = ctypes.c_size_t(0)
    D = 1 << 22
    assert lib.uq_randperm_prefix_workspace_bytes(128, D, D, ctypes.byref(b)) == 0
    one = ctypes.c_size_t(0)
    assert lib.uq_randperm_prefix_workspace_bytes(1, D, D, ctypes.byref(one)) == 0
    assert one.value <= b.value <= (1 << 30) and b.value < 128 * (one.value // 2)


def test_generator_advance_matches_torch():
    from uqdme_amd import _mtstate
    for D, pre in ((2, 0), (625, 3), (70000, 700)):
        g, t = torch.Generator(), torch.Generator()
        for x in (g, t):
            x.manual_seed(12)
            for _ in range(pre):
                torch.randint(0, 100, (1,), generator=x)
        st = randperm.client_states(3, D, generator=g)
        for j in range(3):
            assert np.array_equal(st[j], _mtstate.generator_words(t)[1]), (D, j)
            torch.randperm(D, generator=t)
        assert torch.equal(g.get_state(), t.get_state())
