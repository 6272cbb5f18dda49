"""The packed QUIC-FL message without a GPU: the NumPy model of the layout (tests/quicfl_packed_model.py) against
itself and a hand-written row, the host-only entry points against the model, the argument checks of every new entry
point (no kernel is launched here), and the Python surface."""
import ctypes

import numpy as np
import pytest

import uqdme
from tests import quicfl_packed_model as PM

NONE, FUSED, CONVERTER = 0, 1, 2
INVALID, WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    L = uqdme.load_library()
    from uqdme_amd import _lib
    for name in ("uq_quicfl_compress_packed_f32", "uq_quicfl_receive_packed_f32", "uq_quicfl_pack_x", "uq_quicfl_unpack_x",
                 "uq_quicfl_packed_words", "uq_quicfl_packed_workspace_bytes", "uq_quicfl_receive_packed_workspace_bytes",
                 "uq_test_set_quicfl_packed_hooks", "uq_test_last_quicfl_packed_plan"):
        res, args = _lib.SIGNATURES[name]
        getattr(L, name).restype = res
        getattr(L, name).argtypes = args
    return L


@pytest.mark.parametrize("D", [1, 2, 16, 32, 64, 1024, 4096])
@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
def test_model_round_trip(D, nbits):
    rng = np.random.default_rng(100 * D + nbits)
    for mask in (np.zeros(D, bool), np.ones(D, bool), rng.random(D) < 0.01, None):
        X = rng.integers(0, 1 << nbits, D).astype(np.uint8)
        pay, idx, bits = PM.pack(X, nbits, mask)
        cnt = 0 if mask is None else int(mask.sum())
        assert pay.dtype == np.uint32 and pay.shape == (PM.pitch(D, nbits),) and idx.dtype == np.int32
        assert bits == nbits * D + 64 * cnt and idx.size == cnt and (np.diff(idx) > 0).all()
        assert PM.unused_bits_zero(pay, D, nbits)
        X2, m2 = PM.unpack(pay, D, nbits, idx)
        assert np.array_equal(X2, X) and np.array_equal(m2, np.zeros(D, bool) if mask is None else mask)
        i = int(rng.integers(0, D))                                  # bit i % 32 of word i / 32 of plane b is bit b of X_i
        for b in range(nbits):
            assert (int(pay[b * PM.words(D) + i // 32]) >> (i % 32)) & 1 == (int(X[i]) >> b) & 1


def test_model_against_a_hand_written_row():
    """64 coordinates at 2 bits: X_0 = 3, X_31 = 1, X_32 = 2, X_63 = 3, the others 0; exact coordinates 5 and 40"""
    X = np.zeros(64, np.uint8)
    X[[0, 31, 32, 63]] = [3, 1, 2, 3]
    mask = np.zeros(64, bool)
    mask[[40, 5]] = True
    pay, idx, bits = PM.pack(X, 2, mask)
    assert pay.tolist() == [0x80000001, 0x80000000, 0x00000001, 0x80000001]        # plane 0 (low bits), then plane 1
    assert idx.tolist() == [5, 40] and bits == 2 * 64 + 64 * 2
    X2, m2 = PM.unpack(np.array([0x80000001, 0x80000000, 1, 0x80000001], np.uint32), 64, 2, [5, 40])
    assert np.array_equal(X2, X) and np.array_equal(m2, mask)


def test_packed_words(lib):
    w = ctypes.c_int64()
    for D in (1, 16, 32, 64, 1 << 28):
        for nbits in (1, 2, 3, 4):
            assert lib.uq_quicfl_packed_words(D, nbits, ctypes.byref(w)) == 0
            assert w.value == PM.pitch(D, nbits) == nbits * ((D + 31) // 32), (D, nbits)
    for nbits in (1, 2, 3, 4):
        assert lib.uq_quicfl_packed_words(33, nbits, ctypes.byref(w)) == INVALID
        assert b"power of two" in lib.uq_last_error()
        assert lib.uq_quicfl_packed_words(1 << 29, nbits, ctypes.byref(w)) == INVALID
        assert b"2^28" in lib.uq_last_error()
    for nbits in (0, 5, -1):
        assert lib.uq_quicfl_packed_words(64, nbits, ctypes.byref(w)) == INVALID
        assert b"nbits must be 1..4" in lib.uq_last_error()
    assert lib.uq_quicfl_packed_words(0, 1, ctypes.byref(w)) == INVALID
    assert lib.uq_quicfl_packed_words(64, 1, None) == INVALID
    assert b"pitch_words" in lib.uq_last_error()


def test_workspaces_hold_the_u8_calls_and_the_converter_rows(lib):
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    for n, d, D in ((1, 5, 8), (3, 5000, 8192), (257, 1 << 18, 1 << 18), (1024, 1 << 20, 1 << 20)):
        assert lib.uq_quicfl_workspace_bytes(n, d, ctypes.byref(a)) == 0
        assert lib.uq_quicfl_packed_workspace_bytes(n, d, ctypes.byref(b)) == 0
        assert a.value + 2 * n * D <= b.value <= a.value + 2 * n * D + 4 * n + 1024
        assert lib.uq_quicfl_receive_workspace_bytes(n, D, ctypes.byref(a)) == 0
        assert lib.uq_quicfl_receive_packed_workspace_bytes(n, D, ctypes.byref(b)) == 0
        assert a.value + 2 * n * D <= b.value <= a.value + 2 * n * D + 4 * n + 1024
    assert lib.uq_quicfl_packed_workspace_bytes(-1, 16, ctypes.byref(b)) == INVALID
    assert lib.uq_quicfl_packed_workspace_bytes(1, 16, None) == INVALID
    assert lib.uq_quicfl_receive_packed_workspace_bytes(1, -16, ctypes.byref(b)) == INVALID
    assert lib.uq_quicfl_receive_packed_workspace_bytes(1, 16, None) == INVALID


def test_argument_errors(lib):
    p = ctypes.c_void_p(16)
    big = 1 << 40

    def compress(n=4, dim=100, nbits=1, payload=p, eidx=p, ev=p, cnt=p, pbits=p, x=p, ws=p, ws_bytes=1000):
        return lib.uq_quicfl_compress_packed_f32(x, n, dim, p, p, p, None, 512, 256, 0.5, p, None, p, None, payload, nbits, eidx, ev,
                                                 cnt, pbits, p, p, ws, ws_bytes, None)

    for nbits in (0, 5):
        assert compress(nbits=nbits) == INVALID and b"nbits must be 1..4" in lib.uq_last_error()
    assert compress(dim=(1 << 28) + 1) == INVALID and b"2^28" in lib.uq_last_error()
    for kw in ("payload", "eidx", "ev", "cnt", "pbits", "x"):
        assert compress(**{kw: None}) == INVALID and b"null pointer" in lib.uq_last_error(), kw
    assert compress() == WORKSPACE and b"workspace too small" in lib.uq_last_error()      # (all else valid: no launch)
    assert compress(ws=None, ws_bytes=big) == WORKSPACE
    need = ctypes.c_size_t()
    assert lib.uq_quicfl_packed_workspace_bytes(4, 100, ctypes.byref(need)) == 0
    assert compress(ws_bytes=need.value - 1) == WORKSPACE
    assert compress(n=-1) == INVALID and compress(n=70000) == INVALID
    assert compress(n=0, payload=None, ws=None, ws_bytes=0) == 0 and compress(dim=0, payload=None, ws=None, ws_bytes=0) == 0

    def receive(n=4, D=128, nbits=1, payload=p, eidx=p, ev=p, cnt=p, out=p, ws=p, ws_bytes=10):
        return lib.uq_quicfl_receive_packed_f32(payload, nbits, n, D, p, 2, 256, p, eidx, ev, cnt, p, out, p, ws, ws_bytes, None)

    for nbits in (0, 5):
        assert receive(nbits=nbits) == INVALID and b"nbits must be 1..4" in lib.uq_last_error()
    assert receive(D=100) == INVALID and b"power of two" in lib.uq_last_error()
    assert receive(D=1 << 29) == INVALID and b"2^28" in lib.uq_last_error()
    assert receive(payload=None) == INVALID and b"null pointer" in lib.uq_last_error()
    assert receive(out=None) == INVALID and b"null pointer" in lib.uq_last_error()
    assert receive(eidx=None) == INVALID and b"go together" in lib.uq_last_error()
    assert receive(cnt=None) == INVALID and receive(ev=None) == INVALID
    assert receive() == WORKSPACE and receive(ws=None, ws_bytes=big) == WORKSPACE
    assert receive(n=-1) == INVALID and receive(n=70000) == INVALID
    assert receive(n=0, payload=None, ws=None, ws_bytes=0) == 0
    # a call that launched nothing leaves no packed plan behind
    buf = (ctypes.c_int64 * 4)()
    for side in (0, 1):
        assert lib.uq_test_last_quicfl_packed_plan(side, buf, 4) == 0 and list(buf) == [0, 0, 0, 0]
    assert lib.uq_test_last_quicfl_packed_plan(2, buf, 4) == INVALID
    assert lib.uq_test_last_quicfl_packed_plan(0, None, 4) == INVALID

    def pack(n=4, D=128, nbits=2, kind=1, X=p, payload=p, eidx=p, cnt=p):
        return lib.uq_quicfl_pack_x(X, kind, n, D, nbits, p, payload, eidx, cnt, None, None, None)

    def unpack(n=4, D=128, nbits=2, payload=p, X=p, mask=p, eidx=p, cnt=p):
        return lib.uq_quicfl_unpack_x(payload, n, D, nbits, eidx, cnt, X, mask, None, None)

    for f in (pack, unpack):
        for nbits in (0, 5):
            assert f(nbits=nbits) == INVALID and b"nbits must be 1..4" in lib.uq_last_error()
        assert f(D=33) == INVALID and b"power of two" in lib.uq_last_error()
        assert f(D=1 << 29) == INVALID and b"2^28" in lib.uq_last_error()
        assert f(D=0) == INVALID
        assert f(payload=None) == INVALID and b"null pointer" in lib.uq_last_error()
        assert f(X=None) == INVALID and b"null pointer" in lib.uq_last_error()
        assert f(n=-1) == INVALID and f(n=70000) == INVALID and b"65535" in lib.uq_last_error()
        assert f(n=0, X=None, payload=None) == 0
    assert pack(kind=3) == INVALID and b"x_kind" in lib.uq_last_error()
    assert pack(eidx=None) == INVALID and pack(cnt=None) == INVALID
    assert unpack(mask=None) == INVALID
    assert unpack(eidx=None) == INVALID and b"go together" in lib.uq_last_error()


def test_packed_hooks_round_trip(lib):
    prev = lib.uq_test_set_quicfl_packed_hooks(1)
    try:
        assert prev == 0
    finally:
        assert lib.uq_test_set_quicfl_packed_hooks(prev) == 1
    assert lib.uq_test_set_quicfl_packed_hooks(0) == 0


def test_python_surface_without_a_gpu():
    """the keyword, the new fields' defaults, packed and nbytes (no device work: the messages are built by hand)"""
    import inspect
    import torch
    sig = inspect.signature(uqdme.quicfl_compress)
    assert sig.parameters["packed"].default is False and sig.parameters["packed"].kind is inspect.Parameter.KEYWORD_ONLY
    # the old ten positional arguments still build a message
    old = uqdme.QuicFLMessages(torch.zeros((3, 64), dtype=torch.uint8), torch.zeros((3, 64), dtype=torch.bool),
                               torch.zeros((3, 64)), torch.tensor([0, 2, 1], dtype=torch.int32), torch.ones(3), torch.arange(3),
                               torch.arange(3), 50, 2, 256)
    assert old.payload is None and old.exact_index is None and old.payload_bits is None and not old.packed
    assert (old.dim, old.nbits, old.h_len) == (50, 2, 256)
    assert old.nbytes == 3 * 64 * 2 + 4 * 3
    new = uqdme.QuicFLMessages(None, None, torch.zeros((3, 64)), torch.tensor([0, 2, 1], dtype=torch.int32), torch.ones(3),
                               torch.arange(3), torch.arange(3), 50, 2, 256, payload=torch.zeros((3, 4), dtype=torch.int32),
                               exact_index=torch.zeros((3, 64), dtype=torch.int32),
                               payload_bits=torch.tensor([128, 128 + 128, 128 + 64]))
    assert new.packed and new.nbytes == 16 + 32 + 24
    assert uqdme.quicfl_pack(new) is new and uqdme.quicfl_unpack(old) is old
    with pytest.raises(ValueError, match="int64"):
        uqdme.quicfl_compress(torch.zeros((1, 8)), 1, [1], [2], sender=None, x_dtype=torch.int64, packed=True)
    assert callable(uqdme.quicfl_pack) and callable(uqdme.quicfl_unpack)
