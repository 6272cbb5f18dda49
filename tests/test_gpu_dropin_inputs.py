"""GPU: what the seven drop-ins do with their input before any kernel runs -- Type_unbiased_quantize,
Type_biased_quantize, EDEN_quantize_Hadamard, QUICFL_quantize, Scalar_quantize,
DRIVE_quantize_Hadamard and Kashin_quantize.  The kernels are not under test here, only what reaches them: every
form an input may take gives the bits of the contiguous f32 GPU tensor and leaves torch's
global CPU generator where that form leaves it; the input is only read; rank-2, empty and
unknown-rate calls end the way each scheme ends them.

d = 33 is odd and unaligned (the scalar-tail instances); d = 2050 leaves DRIVE a ragged second
chunk and does not fit one tile.  The values are multiples of 1/64 below 8 in magnitude, exact
in f32, so the f64 forms hold the same numbers."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests import golden_data as G

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from quicfl_tables import write_tables  # noqa: E402

SEED = 7
DIMS = (33, 2050)
RANK1_ONLY = ("Type_unbiased_quantize", "Type_biased_quantize", "Scalar_quantize", "DRIVE_quantize_Hadamard")
# Kashin_quantize (AS:834-854) takes [1, d] through numel() and broadcasting: the 1-D call's bits and draw on torch CPU
FLATTENING = ("EDEN_quantize_Hadamard", "QUICFL_quantize", "Kashin_quantize")
SCHEMES = RANK1_ONLY + FLATTENING
FORMS = ("list", "numpy_f64", "cpu_f32", "gpu_f64", "gpu_strided", "requires_grad")


@pytest.fixture(scope="module")
def dropins(gpu_ready, tmp_path_factory):
    """The package with QUICFL_quantize's tables in place (synthetic sender tables, the
    reference's receiver tables: tests/golden/quicfl_tables.py)."""
    import uqdme
    uqdme.set_tables_prefix(write_tables(str(tmp_path_factory.mktemp("qfl_tabs") / "t")))
    yield uqdme
    uqdme.set_tables_prefix(None)


def values(d) -> np.ndarray:
    v = np.round(np.random.RandomState(1000 + d).standard_normal(d) * 64.0) / 64.0
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v) and v.min() != v.max()
    return v


def make_input(form, d):
    """(the input in that form, check() that it is still what it was)."""
    x = values(d)
    f32 = torch.from_numpy(x.astype(np.float32))
    if form == "list":
        v = x.tolist()
        was = list(v)
        return v, lambda: v == was
    if form == "numpy_f64":
        v = x.copy()
        return v, lambda: v.dtype == np.float64 and np.array_equal(v, x)
    if form == "gpu_strided":
        base = torch.full((2 * d,), 1.0e9, dtype=torch.float32, device="cuda")
        base[::2] = f32.cuda()
        v = base[::2]
        assert not v.is_contiguous()
        holder = base
    else:
        v = {"cpu_f32": lambda: f32.clone(), "gpu_f32": lambda: f32.cuda(), "gpu_f64": lambda: torch.from_numpy(x).cuda(),
             "requires_grad": lambda: f32.cuda().requires_grad_(True)}[form]()
        holder = v
    was = holder.detach().clone()
    meta = (v.dtype, v.device, v.shape, v.stride(), v.requires_grad)
    return v, lambda: (v.dtype, v.device, v.shape, v.stride(), v.requires_grad) == meta and torch.equal(holder.detach(), was)


def state():
    return torch.default_generator.get_state().clone()


def state_after(draw=None):
    """The global generator's state after manual_seed(SEED) and `draw`."""
    torch.manual_seed(SEED)
    if draw is not None:
        draw()
    return state()


def call(uqdme, name, v, bits=1):
    """-> (the result's kind, its f32 values on the host, the generator's state after the call)."""
    torch.manual_seed(SEED)
    out = getattr(uqdme, name)(v, bits)
    st = state()
    if isinstance(out, np.ndarray):
        assert out.dtype == np.float32 and out.ndim == 1
        return "numpy", out.copy(), st
    assert torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 1
    assert not out.requires_grad
    return "gpu", out.cpu().numpy(), st


@functools.lru_cache(maxsize=None)
def reference(uqdme, name, d):
    """The call on the contiguous f32 GPU tensor: computed once per (scheme, d), never changed."""
    v, unchanged = make_input("gpu_f32", d)
    kind, out, st = call(uqdme, name, v)
    assert unchanged() and out.shape == (d,)
    assert kind == ("numpy" if name in FLATTENING else "gpu")
    out.setflags(write=False)
    return kind, out, st


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", SCHEMES)
def test_every_input_form_gives_the_same_bits(dropins, name, d):
    kind, ref, st_ref = reference(dropins, name, d)
    for form in FORMS:
        v, unchanged = make_input(form, d)
        k, out, st = call(dropins, name, v)
        assert k == kind, (form, k)
        assert G.bits_equal(out, ref), (form, G.n_mismatch(out, ref))
        assert torch.equal(st, st_ref), form
        assert unchanged(), form


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", RANK1_ONLY)
def test_rank_2_raises(dropins, name, d):
    """[1, d] is refused before any draw (the reference fails on other ranks as well)."""
    x = values(d)
    before = state_after()
    for v in (torch.from_numpy(x.astype(np.float32)).cuda().view(1, d), [x.tolist()], x.reshape(1, d)):
        torch.manual_seed(SEED)
        with pytest.raises(RuntimeError, match=f"{name} expects a 1-D vector") as e:
            getattr(dropins, name)(v, 1)
        assert torch.equal(state(), before)
        if name == "Type_unbiased_quantize":
            assert "torch.cat" in str(e.value)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", FLATTENING)
def test_rank_2_is_flattened(dropins, name, d):
    kind, ref, st_ref = reference(dropins, name, d)
    x = values(d)
    for v in (torch.from_numpy(x.astype(np.float32)).cuda().view(1, d), [x.tolist()], x.reshape(1, d)):
        k, out, st = call(dropins, name, v)
        assert k == kind and G.bits_equal(out, ref) and torch.equal(st, st_ref)


def empty_inputs():
    return (torch.empty(0, dtype=torch.float32, device="cuda"), torch.empty(0, dtype=torch.float64), [],
            np.zeros(0, np.float64))


@pytest.mark.parametrize("name,draw", [("Type_unbiased_quantize", lambda: torch.rand(1)),       # AS:634 is still taken
                                       ("Type_biased_quantize", None), ("Scalar_quantize", None),
                                       ("DRIVE_quantize_Hadamard", None)])
def test_empty_input_returns_an_empty_gpu_tensor(dropins, name, draw):
    after = state_after(draw)
    for v in empty_inputs():
        kind, out, st = call(dropins, name, v)
        assert kind == "gpu" and out.shape == (0,)
        assert torch.equal(st, after)


def test_empty_input_eden_returns_an_empty_array_after_the_seed_draw(dropins):
    after = state_after(lambda: torch.randint(0, 100, (1,)))                 # AS:797 is still taken
    for v in empty_inputs():
        kind, out, st = call(dropins, "EDEN_quantize_Hadamard", v)
        assert kind == "numpy" and out.shape == (0,)
        assert torch.equal(st, after)


def test_empty_input_kashin_returns_an_empty_array_after_the_seed_draw(dropins):
    after = state_after(lambda: torch.randint(0, 100, (1,)))                 # AS:841 is still taken
    for v in empty_inputs():
        kind, out, st = call(dropins, "Kashin_quantize", v)
        assert kind == "numpy" and out.shape == (0,)
        assert torch.equal(st, after)


def test_empty_input_quicfl_raises_after_the_seed_draw(dropins):
    """QUICFL_quantize draws its message seed (AS:820) and then refuses the empty vector."""
    after = state_after(lambda: torch.randint(0, 100, (1,)))
    for v in empty_inputs():
        torch.manual_seed(SEED)
        with pytest.raises(ValueError, match="empty vector"):
            dropins.QUICFL_quantize(v, 1)
        assert torch.equal(state(), after)


@pytest.mark.parametrize("name", ["Type_unbiased_quantize", "Type_biased_quantize"])
def test_unknown_rate_raises_before_the_input_is_looked_at(dropins, name):
    before = state_after()
    for v in (make_input("gpu_f32", 33)[0], [[1.0, 2.0]], "not a vector"):
        torch.manual_seed(SEED)
        with pytest.raises(KeyError):
            getattr(dropins, name)(v, 99)
        assert torch.equal(state(), before)
