"""The bit-packed EDEN message form without a GPU: the NumPy model of the layout (tests/eden_packed_model.py)
against itself, the host-only entry points against the model, the dispatch of the packed form, and the argument
checks of every new entry point (no kernel is launched here)."""
import ctypes

import numpy as np
import pytest

import uqdme
from tests import eden_packed_model as PM
from tests import eden_plan_hook as H

FRAC = PM.FRAC
NONE, FUSED, CONVERTER = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    return uqdme.load_library()


def packed_plan(lib, op, n, dim, kind):
    buf = (ctypes.c_int64 * 4)()
    assert lib.uq_test_eden_packed_plan(op, n, dim, kind, buf, 4) == 0
    return dict(kind=int(buf[0]), form=int(buf[1]), P=int(buf[2]), pitch=int(buf[3]))


@pytest.mark.parametrize("D", [1, 2, 16, 32, 64, 4096])
@pytest.mark.parametrize("kind", [1, 2])
def test_model_round_trip_integer_rates(D, kind):
    rng = np.random.default_rng(100 * D + kind)
    for _ in range(3):
        b = rng.integers(0, 1 << kind, D).astype(np.uint8)
        pay, nbits = PM.pack(b, kind)
        assert pay.dtype == np.uint32 and pay.shape == (PM.pitch(D, kind),) and nbits == kind * D
        assert PM.unused_bits_zero(pay, D, kind)
        assert np.array_equal(PM.unpack(pay, D, kind), b)
        # bit i % 32 of word i / 32, plane H then plane L
        i = int(rng.integers(0, D))
        hi = (int(pay[i // 32]) >> (i % 32)) & 1
        assert hi == (b[i] if kind == 1 else b[i] >> 1)
        if kind == 2:
            assert (int(pay[PM.words(D) + i // 32]) >> (i % 32)) & 1 == b[i] & 1


def frac_masks(D, rng):
    """masks with cnt = 0, cnt = D and cnt % 32 in {0, 1, 31} where D allows them, and a random one"""
    out = [np.zeros(D, bool), np.ones(D, bool), rng.random(D) < 0.4]
    for cnt in (32, 33, 63, 1, 31):
        if cnt <= D:
            m = np.zeros(D, bool)
            m[rng.choice(D, cnt, replace=False)] = True
            out.append(m)
    return out


@pytest.mark.parametrize("D", [1, 2, 16, 32, 64, 4096])
def test_model_round_trip_fractional(D):
    rng = np.random.default_rng(D)
    seen = set()
    for m in frac_masks(D, rng):
        cnt = int(m.sum())
        seen.add(cnt % 32 if 0 < cnt < D else -cnt)
        b = np.where(m, rng.integers(0, 4, D), rng.integers(0, 2, D)).astype(np.uint8)
        pay, nbits = PM.pack(b, FRAC, m)
        assert pay.shape == (2 * PM.words(D),) and nbits == D + cnt
        assert PM.unused_bits_zero(pay, D, FRAC, cnt)
        assert np.array_equal(PM.unpack(pay, D, FRAC, m), b)
        # the r-th set bit of the mask owns bit r % 32 of word P + r / 32
        pos = np.flatnonzero(m)
        for r in (0, cnt - 1, cnt // 2) if cnt else ():
            assert (int(pay[PM.words(D) + r // 32]) >> (r % 32)) & 1 == b[pos[r]] & 1
        # and the rank rows are the cumulative popcounts of the mask words
        rk = PM.ranks(PM.plane(m, PM.words(D)), D)
        assert rk[0] == 0 and rk[-1] == cnt and rk.shape == (PM.words(D) + 1,)
        assert all(rk[w] == m[:32 * w].sum() for w in range(PM.words(D) + 1))
    if D == 4096:
        assert seen >= {0, -D, 1, 31}


def test_packed_words_against_the_model(lib):
    w = ctypes.c_int64()
    for D in (0, 1, 5, 31, 32, 33, 64, 2048, 4096, 1 << 20, 1 << 28):
        for kind in (1, 2, FRAC):
            assert lib.uq_eden_packed_words(D, kind, ctypes.byref(w)) == 0
            assert w.value == PM.pitch(D, kind), (D, kind)
    assert lib.uq_eden_packed_words(64, 3, ctypes.byref(w)) == -1
    assert b"kind" in lib.uq_last_error()
    assert lib.uq_eden_packed_words(-1, 1, ctypes.byref(w)) == -1
    assert lib.uq_eden_packed_words(64, 1, None) == -1
    assert b"pitch_words" in lib.uq_last_error()


def test_workspace_is_the_u8_calls(lib):
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    for n, d in ((1, 5), (12, 3000), (257, 2048), (1, 32768), (1024, 1 << 20)):
        assert lib.uq_eden_workspace_bytes(n, d, ctypes.byref(a)) == 0
        for kind in (1, 2, FRAC):
            assert lib.uq_eden_packed_workspace_bytes(n, d, kind, ctypes.byref(b)) == 0
            # the u8 layout holds a region of n * D bins (the fused round trip's), which the converter path uses
            assert b.value == a.value >= n * H.plan(lib, H.COMPRESS, n, d)["D"] * 5
    assert lib.uq_eden_packed_workspace_bytes(1, 16, 7, ctypes.byref(b)) == -1
    assert b"kind" in lib.uq_last_error()
    assert lib.uq_eden_packed_workspace_bytes(-1, 16, 1, ctypes.byref(b)) == -1
    assert lib.uq_eden_packed_workspace_bytes(1, 16, 1, None) == -1


# (n, dim, kind) -> (sender's form, receiver's form): DESIGN 4.3's dispatch rule
FORMS = {
    (12, 3000, 1): (FUSED, FUSED), (12, 3000, 2): (FUSED, FUSED),                    # D = 4096
    (257, 1024, 1): (FUSED, CONVERTER), (257, 1024, 2): (FUSED, CONVERTER),          # generic first pass
    (257, 2048, 1): (FUSED, CONVERTER), (257, 2048, 2): (FUSED, CONVERTER),          # KE2+4 / KE4
    (300, 16384, 1): (FUSED, FUSED),
    (1, 32768, 1): (CONVERTER, FUSED), (1, 32768, 2): (CONVERTER, FUSED),            # segmented dot
    (129, 16384, 1): (FUSED, FUSED), (129, 16384, 2): (FUSED, FUSED),                # segmented norm, one-wave dot
    (5, 48, 1): (FUSED, CONVERTER), (2, 5, 2): (FUSED, CONVERTER),
    (1024, 1 << 20, 1): (FUSED, FUSED), (1024, 1 << 20, 2): (FUSED, FUSED),
    (4, 1 << 22, 1): (CONVERTER, CONVERTER),                                         # 16k first pass
    (7, 3000, FRAC): (CONVERTER, CONVERTER), (1024, 1 << 20, FRAC): (CONVERTER, CONVERTER),
}


def test_packed_dispatch(lib):
    for (n, dim, kind), (snd, rcv) in FORMS.items():
        D = H.plan(lib, H.COMPRESS, n, dim, kind)["D"]
        for op, want in ((H.COMPRESS, snd), (H.DECOMPRESS, rcv)):
            p = packed_plan(lib, op, n, dim, kind)
            assert p == dict(kind=kind, form=want, P=PM.words(D), pitch=PM.pitch(D, kind)), (n, dim, kind, op)
    # the sender is fused exactly where one wave per client or KE2+4 writes the bins, the receiver where the
    # 4096-element kernel is its first pass
    for n in (1, 128, 129, 256, 257, 1024):
        for p2 in range(0, 23):
            for kind in (1, 2):
                e = H.plan(lib, H.COMPRESS, n, 1 << p2, kind)
                assert (packed_plan(lib, H.COMPRESS, n, 1 << p2, kind)["form"] == FUSED) == (e["dot"] in (H.ONE_WAVE, H.FUSED_REDO))
                r = H.plan(lib, H.DECOMPRESS, n, 1 << p2, kind)
                assert (packed_plan(lib, H.DECOMPRESS, n, 1 << p2, kind)["form"] == FUSED) == (H.kernels(r)[:1] == [H.LOW4096])
    assert packed_plan(lib, H.COMPRESS, 0, 16, 1) == dict(kind=0, form=NONE, P=0, pitch=0)
    buf = (ctypes.c_int64 * 4)()
    assert lib.uq_test_eden_packed_plan(H.NORM, 1, 16, 1, buf, 4) == -1
    assert lib.uq_test_eden_packed_plan(H.COMPRESS, 1, 16, 5, buf, 4) == -1
    assert lib.uq_test_last_eden_packed_plan(H.RHT_FORWARD, buf, 4) == -1


def test_hook_sends_every_call_to_the_converter(lib):
    prev = lib.uq_test_set_eden_hooks(1)
    try:
        assert prev == 0
        for (n, dim, kind) in FORMS:
            for op in (H.COMPRESS, H.DECOMPRESS):
                assert packed_plan(lib, op, n, dim, kind)["form"] == CONVERTER
    finally:
        assert lib.uq_test_set_eden_hooks(prev) == 1
    assert packed_plan(lib, H.COMPRESS, 12, 3000, 1)["form"] == FUSED


def test_argument_errors(lib):
    from uqdme_amd import _lib as L
    for name in ("uq_eden_compress_packed_f32", "uq_eden_decompress_packed_f32", "uq_eden_pack_bins", "uq_eden_unpack_bins",
                 "uq_eden_mask_ranks"):
        res, args = L.SIGNATURES[name]
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    p = ctypes.c_void_p(16)
    big = 1 << 40

    def compress(n=4, dim=100, kind=1, payload=p, ranks=None, mask=None, ws=p, ws_bytes=big):
        return lib.uq_eden_compress_packed_f32(p, n, dim, kind, p, p, None, mask, ranks, None, payload, None, p, ws, ws_bytes, None)

    def decompress(n=4, dim=100, kind=1, payload=p, ranks=None, mask=None, ws=p, ws_bytes=big):
        return lib.uq_eden_decompress_packed_f32(payload, p, n, dim, kind, p, p, None, mask, ranks, None, p, ws, ws_bytes, None)

    for f in (compress, decompress):
        assert f(payload=None) == -1 and b"null pointer" in lib.uq_last_error()          # NULL payload, n and d > 0
        assert f(kind=3) == -1 and b"kind must be 1, 2 or UQ_EDEN_NBITS_FRAC" in lib.uq_last_error()
        assert f(kind=0) == -1
        assert f(ws_bytes=1000) == -3 and b"workspace too small" in lib.uq_last_error()
        assert f(ws=None) == -3
        assert f(n=-1) == -1 and b"n and dim must be >= 0" in lib.uq_last_error()
        assert f(kind=FRAC) == -1 and b"null mask_bits" in lib.uq_last_error()
        assert f(kind=FRAC, mask=p) == -1 and b"null pointer" in lib.uq_last_error()       # no rank rows
        assert f(n=0, payload=None, ws=None, ws_bytes=0) == 0                             # no-ops
        assert f(dim=0, payload=None, ws=None, ws_bytes=0) == 0
        assert f(n=0, kind=FRAC, payload=None, ws=None, ws_bytes=0) == 0
    # a call that launched nothing leaves no packed plan behind
    buf = (ctypes.c_int64 * 4)()
    for op in (H.COMPRESS, H.DECOMPRESS):
        assert lib.uq_test_last_eden_packed_plan(op, buf, 4) == 0 and list(buf) == [0, 0, 0, 0]

    def pack(n=4, D=100, kind=2, a=p, b=p, mask=None, ranks=None):
        return lib.uq_eden_pack_bins(a, n, D, kind, mask, ranks, None, b, None, None)

    def unpack(n=4, D=100, kind=2, a=p, b=p, mask=None, ranks=None):
        return lib.uq_eden_unpack_bins(a, n, D, kind, mask, ranks, None, b, None)

    for f in (pack, unpack):
        assert f(a=None) == -1 and b"null pointer" in lib.uq_last_error()
        assert f(b=None) == -1
        assert f(kind=4) == -1 and b"kind" in lib.uq_last_error()
        assert f(n=-1) == -1 and f(D=-1) == -1 and b"n and D must be >= 0" in lib.uq_last_error()
        assert f(n=70000) == -1 and b"65535" in lib.uq_last_error()
        assert f(kind=FRAC) == -1 and b"null mask_bits or mask_ranks" in lib.uq_last_error()
        assert f(kind=FRAC, mask=p) == -1
        assert f(n=0, a=None, b=None) == 0 and f(D=0, a=None, b=None) == 0
    assert lib.uq_eden_mask_ranks(None, 3, 64, p, None) == -1 and b"null pointer" in lib.uq_last_error()
    assert lib.uq_eden_mask_ranks(p, 3, 64, None, None) == -1
    assert lib.uq_eden_mask_ranks(p, -1, 64, p, None) == -1
    assert lib.uq_eden_mask_ranks(None, 0, 64, None, None) == 0


def test_python_surface_without_a_gpu():
    """the keyword, the new fields' defaults and nbytes (no device work: the message is built by hand)"""
    import inspect
    import torch
    from uqdme_amd import eden as ED
    sig = inspect.signature(uqdme.eden_compress)
    assert list(sig.parameters) == ["x", "bits_per_dimension", "seeds", "generator", "packed"]
    assert sig.parameters["packed"].default is False and sig.parameters["packed"].kind is inspect.Parameter.KEYWORD_ONLY
    old = uqdme.EdenMessage(torch.zeros((3, 64), dtype=torch.uint8), torch.ones(3), torch.arange(3), 1, 50)
    assert old.payload is None and old.payload_bits is None and not old.packed and old.nbytes == 3 * 64
    new = uqdme.EdenMessage(None, torch.ones(3), torch.arange(3), (1, 2, 0.5), 50, payload=torch.zeros((3, 4), dtype=torch.int32),
                            payload_bits=torch.tensor([64, 65, 64 + 33]))
    assert new.packed and new.nbytes == 8 + 9 + 13
    assert ED.packed_words(64, 1) == 2 and ED.packed_words(64, 2) == 4 and ED.packed_words(5, (1, 2, 0.5)) == 2
    assert callable(uqdme.eden_pack) and callable(uqdme.eden_unpack)


def test_the_two_normdot1_kernels_stay_in_step():
    """eden_normdot1_packed_kernel is a copy of eden_normdot1_kernel's text (a shared body moved the u8 kernel's
    instructions): the two may differ only where the bins are staged and stored, so an edit of the loaders, the
    chains, the dot or the redo rule made in one of them alone fails here."""
    import difflib
    import os
    src = open(os.path.join(uqdme.PACKAGE_DIR, "csrc", "uq_eden_kernels.h")).read()

    def body(name):
        j = src.index("{", src.index("\n" + name + "("))
        return [ln.strip() for ln in src[j:src.index("\n}\n", j)].split("\n") if ln.strip() and not ln.strip().startswith("//")]
    u8, pk = body("eden_normdot1_kernel"), body("eden_normdot1_packed_kernel")
    assert len(u8) > 100
    staging = ("lb", "sbins", "w |=", "u32x4b", "squeeze", "a = (a", "return (a", "for (int r", "const int w0", "#pragma unroll", "}", "};")
    changed = [ln[1:] for ln in difflib.unified_diff(u8, pk, lineterm="", n=0) if ln[:1] in "+-" and ln[:2] not in ("--", "++")]
    assert 0 < len(changed) <= 24, changed
    for ln in changed:
        assert any(t in ln for t in staging), ln
