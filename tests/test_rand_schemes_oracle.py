"""CPU: the NumPy restatement of Scalar_quantize (AS:755-790) and DRIVE_quantize_Hadamard
(AS:707-752) in tests/rand_schemes_model.py against the reference's own outputs on torch CPU
(tests/golden/make_golden_rand_schemes.py), bit for bit, the words taken included (the sha256 of
torch's generator state after each call); and the host side of the new C entry points."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from tests import golden_data as G
from tests import rand_schemes_model as M


@pytest.fixture(scope="module")
def fx():
    return M.load_fixture()


def state_sha(gseed, state):
    """sha256 of torch.default_generator.get_state() with (left, next, words) replaced."""
    torch.manual_seed(gseed)
    tpl = torch.default_generator.get_state().numpy()
    return hashlib.sha256(M.torch_state_pack(tpl, state).tobytes()).hexdigest()


def run_model(c, x, st):
    if c["scheme"] == "scalar":
        out, st, taken, const = M.scalar_quantize(x, c["bits"], st)
        expect = 0 if (const or 2 ** c["bits"] - 1 < 1) else c["d"]
    else:
        out, st, taken, _ = M.drive_quantize(x, st)
        expect = M.drive_words(c["d"])
    assert taken == expect, c
    return out, st


def test_model_matches_every_fixture_case(fx):
    meta, z = fx
    assert len(meta["cases"]) >= 60
    for c in meta["cases"]:
        k = c["idx"]
        out, st = run_model(c, M.gen_input(c), M.start_state(c))
        if "sha" in c:
            assert G.sha(out) == c["sha"], c
            assert G.bits_equal(out[z[f"out{k}_pos"]], z[f"out{k}_s"]), c
        else:
            assert G.bits_equal(out, z[f"out{k}"]), (c, G.n_mismatch(out, z[f"out{k}"]))
        assert state_sha(c["gseed"], st) == c["state_sha"], c


def test_model_matches_back_to_back_calls(fx):
    meta, z = fx
    for c in meta["pairs"]:
        x, st = M.gen_input(c), M.start_state(c)
        for t in range(2):
            out, st = run_model(c, x, st)
            assert G.bits_equal(out, z[f"pair{c['idx']}_{t}"]), (c, t)
        assert state_sha(c["gseed"], st) == c["state_sha"], c


def test_fixture_covers_the_edges(fx):
    """What the GPU tests rely on being in the fixture."""
    meta, _ = fx
    cs = meta["cases"]
    assert {c["d"] for c in cs if c["scheme"] == "scalar"} >= {1, 2, 5, 623, 624, 625, 1251, 2048, 5000, 65553}
    assert {c["bits"] for c in cs if c["scheme"] == "scalar"} >= {0, 1, 2, 4}
    assert {c["d"] for c in cs if c["scheme"] == "drive"} >= {1, 2, 3, 5, 1000, 2048, 2049, 3073, 4096, 5000, 6768}
    for scheme in ("scalar", "drive"):
        assert {c["pre"] for c in cs if c["scheme"] == scheme} >= {0, 1, 300}
    assert {c["kind"] for c in cs} >= {"normal", "lognormal", "constant", "nan", "inf", "zeros", "zero_pairs"}
    # a constant vector and bits = 0 leave the generator where the pre-draws left it
    for c in cs:
        if c["kind"] == "constant" or c["bits"] == 0:
            assert state_sha(c["gseed"], M.start_state(c)) == c["state_sha"], c


def test_pair_steps_are_not_a_transform():
    """AS:37-59 through its aliasing views: (a, b) -> (a + b, (a + b) - b) per adjacent pair."""
    v = np.array([1, 2, 3, 5, -7, 0.5, 0, 0], np.float32)
    assert np.array_equal(M.pair_steps(v, 1), np.array([3, 1, 8, 3, -6.5, -7, 0, 0], np.float32))
    assert np.array_equal(M.pair_steps(v, 3), M.pair_steps(M.pair_steps(M.pair_steps(v, 1), 1), 1))


# ---- the C entry points' host side (no kernel launched) ------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import uqdme
    return uqdme.load_library()


def test_version_minor_bumped(lib):
    assert lib.uq_version() >= 103


def test_drive_words(lib):
    w = ctypes.c_int64(-1)
    for d, want in ((0, 0), (1, 1), (3, 4), (2048, 2048), (2049, 2049), (5000, 5120), (2047, 2048), (3073, 4096),
                    (70001, 34 * 2048 + 512), (1 << 28, 1 << 28)):
        assert lib.uq_drive_words(d, ctypes.byref(w)) == 0
        assert w.value == want == M.drive_words(d), d
    assert lib.uq_drive_words(-1, ctypes.byref(w)) == -1
    assert lib.uq_drive_words((1 << 28) + 1, ctypes.byref(w)) == -1
    assert lib.uq_drive_words(5, None) == -1
    assert b"words_out" in lib.uq_last_error()


def test_workspace_bytes(lib):
    b = ctypes.c_size_t()
    assert lib.uq_rand_workspace_bytes(0, 0, ctypes.byref(b)) == 0
    assert lib.uq_rand_workspace_bytes(4, 5000, ctypes.byref(b)) == 0
    assert b.value >= 4 * 5120 // 8                           # DRIVE's sign bits: 1/8 byte per word
    small = b.value
    assert lib.uq_rand_workspace_bytes(1024, 1 << 20, ctypes.byref(b)) == 0
    assert small < b.value and 1024 * (1 << 20) // 8 <= b.value < 1024 * (1 << 20) // 4
    assert lib.uq_rand_workspace_bytes(-1, 16, ctypes.byref(b)) == -1
    assert lib.uq_rand_workspace_bytes(1, (1 << 28) + 1, ctypes.byref(b)) == -1
    assert lib.uq_rand_workspace_bytes(1, 16, None) == -1


def test_scalar_and_drive_argument_errors(lib):
    p = ctypes.c_void_p(256)
    big = 1 << 30
    # empty batches are no-ops that touch no pointer
    assert lib.uq_scalar_quantize_f32(None, None, 0, 100, 1.0, None, None, None, None, None, 0, None) == 0
    assert lib.uq_scalar_quantize_f32(None, None, 3, 0, 3.0, None, None, None, None, None, 0, None) == 0
    assert lib.uq_drive_hadamard_f32(None, None, 0, 100, None, None, None, None, None, 0, None) == 0
    assert lib.uq_drive_hadamard_f32(None, None, 3, 0, None, None, None, None, None, 0, None) == 0
    # Scalar: nlevels below 1 (the Python side returns early), NaN and inf are refused
    for nl in (0.0, 0.5, -1.0, float("nan"), float("inf")):
        assert lib.uq_scalar_quantize_f32(p, p, 1, 10, nl, p, None, p, p, p, big, None) == -1
        assert b"nlevels" in lib.uq_last_error()
    # bad shapes, null pointers, no generator, a short workspace: all before any launch
    assert lib.uq_scalar_quantize_f32(p, p, -1, 10, 1.0, p, None, p, p, p, big, None) == -1
    assert lib.uq_scalar_quantize_f32(p, p, 1, (1 << 28) + 1, 1.0, p, None, p, p, p, big, None) == -1
    assert lib.uq_scalar_quantize_f32(None, p, 1, 10, 1.0, p, None, p, p, p, big, None) == -1
    assert lib.uq_scalar_quantize_f32(p, None, 1, 10, 1.0, p, None, p, p, p, big, None) == -1
    assert lib.uq_scalar_quantize_f32(p, p, 1, 10, 1.0, None, None, p, p, p, big, None) == -1
    assert b"px_state or px_seeds" in lib.uq_last_error()
    assert lib.uq_scalar_quantize_f32(p, p, 1, 10, 1.0, p, None, p, None, p, big, None) == -1
    assert b"info" in lib.uq_last_error()
    assert lib.uq_scalar_quantize_f32(p, p, 1, 10, 1.0, p, None, p, p, None, big, None) == -1
    assert lib.uq_scalar_quantize_f32(p, p, 1, 10, 1.0, p, None, p, p, p, 8, None) == -3
    assert lib.uq_drive_hadamard_f32(p, p, 1, -5, p, None, p, None, p, big, None) == -1
    assert lib.uq_drive_hadamard_f32(p, p, 1, (1 << 28) + 1, p, None, p, None, p, big, None) == -1
    assert lib.uq_drive_hadamard_f32(None, p, 1, 10, p, None, p, None, p, big, None) == -1
    assert lib.uq_drive_hadamard_f32(p, None, 1, 10, p, None, p, None, p, big, None) == -1
    assert lib.uq_drive_hadamard_f32(p, p, 1, 10, None, None, p, None, p, big, None) == -1
    assert lib.uq_drive_hadamard_f32(p, p, 1, 10, p, None, p, None, None, big, None) == -1
    assert lib.uq_drive_hadamard_f32(p, p, 1, 10, p, None, p, None, p, 8, None) == -3
    assert b"workspace" in lib.uq_last_error()


def test_drop_in_names_and_signatures():
    import inspect

    import uqdme
    for f, name in ((uqdme.Scalar_quantize, "Scalar_quantize"), (uqdme.DRIVE_quantize_Hadamard, "DRIVE_quantize_Hadamard")):
        assert f.__name__ == name and name in uqdme.__all__
        sig = inspect.signature(f)
        assert list(sig.parameters) == ["input_vector", "bits_per_dimension"]
        assert sig.parameters["bits_per_dimension"].default == 1
    for name in ("scalar_quantize", "drive_quantize", "drive_words"):
        assert name in uqdme.__all__ and callable(getattr(uqdme, name))


def test_advance_generator_places_drive_clients(fx):
    """The drop-in moves torch's generator on by uq_drive_words(d) words on the host: where the
    reference's DRIVE call leaves it (the fixture's state sha)."""
    from uqdme_amd.quicfl import advance_generator
    from uqdme_amd.rand_schemes import drive_words
    meta, _ = fx
    g = torch.Generator()
    for c in meta["cases"]:
        if c["scheme"] != "drive" or c["d"] > 6768:
            continue
        g.manual_seed(c["gseed"])
        for _ in range(c["pre"]):
            torch.randint(0, 100, (1,), generator=g)
        advance_generator(g, drive_words(c["d"]))
        assert hashlib.sha256(g.get_state().numpy().tobytes()).hexdigest() == c["state_sha"], c
