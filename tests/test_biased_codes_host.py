"""Type codes of the biased type quantizer, host side (no GPU: no kernel is launched here): the
library's new entry points and their argument checks, the numpy model of the biased dequantize
form against the reference's fixtures, and the UQT1 serialisation of both forms."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import uqdme
from oracle import uq_oracle_c as C
from tests import biased_codes_model as M
from tests import golden_data as G

f32 = np.float32
NEW_SYMBOLS = ("uq_type_biased_codes_f32", "uq_biased_codes_workspace_bytes", "uq_codes_decode_form_f32",
               "uq_codes_mean_form_f32")
UQ_E_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return uqdme.load_library()


def test_library_exports_the_new_symbols(lib):
    from uqdme_amd import _lib as L
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in L.SIGNATURES, n
    for n in ("biased_quantize_encode", "biased_quantize_mean"):
        assert callable(getattr(uqdme, n)), n


def test_noop_and_error_cases(lib):
    buf = (ctypes.c_char * 64)()                      # never dereferenced: every call ends in its checks
    p = ctypes.cast(buf, ctypes.c_void_p)
    enc = lib.uq_type_biased_codes_f32
    # n == 0 or d == 0: a no-op that never touches the device
    assert enc(None, None, None, None, 0, 100, 10, 1, 0, None, None, None, 0, None) == 0
    assert enc(None, None, None, None, 4, 0, 10, 1, 0, None, None, None, 0, None) == 0
    # m < 1
    assert enc(p, None, p, p, 2, 8, 0, 1, 0, p, None, p, 64, None) == UQ_E_INVALID
    assert b"m must be >= 1" in lib.uq_last_error()
    # codes, kmax or l1_out NULL with n, d > 0
    assert enc(p, None, None, p, 2, 8, 4, 1, 0, p, None, p, 64, None) == UQ_E_INVALID
    assert b"codes" in lib.uq_last_error()
    assert enc(p, None, p, None, 2, 8, 4, 1, 0, p, None, p, 64, None) == UQ_E_INVALID
    assert b"kmax" in lib.uq_last_error()
    assert enc(p, None, p, p, 2, 8, 4, 1, 0, None, None, p, 64, None) == UQ_E_INVALID
    assert b"l1_out" in lib.uq_last_error()
    # the tie policy is checked as in uq_type_biased_f32
    assert enc(p, None, p, p, 2, 8, 4, 1, 3, p, None, p, 64, None) == UQ_E_INVALID
    assert b"tie_policy" in lib.uq_last_error()
    # the codes call's workspace: the plain call's plus one int32 per output tile and client
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    for n, d in ((1, 1), (3, 4097), (1024, 1 << 20)):
        assert lib.uq_biased_workspace_bytes(n, d, 1, ctypes.byref(a)) == 0
        assert lib.uq_biased_codes_workspace_bytes(n, d, 1, ctypes.byref(b)) == 0
        assert a.value + 4 * n * -(-d // 4096) <= b.value <= a.value + 4 * n * -(-d // 4096) + 256, (n, d)
    assert lib.uq_biased_codes_workspace_bytes(-1, 8, 1, ctypes.byref(b)) == UQ_E_INVALID
    assert lib.uq_biased_codes_workspace_bytes(1, 8, 1, None) == UQ_E_INVALID
    dec, mean = lib.uq_codes_decode_form_f32, lib.uq_codes_mean_form_f32
    for form in (0, 1):
        assert dec(None, None, 0, 16, 4, form, None, None) == 0
        assert dec(None, None, 3, 0, 4, form, None, None) == 0
        assert mean(None, 0, None, 0, None, None, 3, 0, 4, form, 3.0, 0, None, None) == 0
    for form in (2, -1, 7):
        assert dec(p, p, 1, 16, 4, form, p, None) == UQ_E_INVALID
        assert b"form" in lib.uq_last_error()
        assert mean(p, 16, None, 16, p, p, 1, 16, 4, form, 1.0, 0, p, None) == UQ_E_INVALID
        assert b"form" in lib.uq_last_error()
    # the biased form divides by m
    assert dec(p, p, 1, 16, 0, 1, p, None) == UQ_E_INVALID
    assert mean(p, 16, None, 16, p, p, 1, 16, 0, 1, 1.0, 0, p, None) == UQ_E_INVALID
    # the new UQR1 flag is accepted, unknown ones are not (n == 0: only the offsets would be written)
    assert lib.uq_tc_encode(None, None, 0, 8, 4, 4, None, 0, None, None, 0, None) == UQ_E_INVALID
    assert b"flags" in lib.uq_last_error()


def test_model_reproduces_reference_fixtures():
    """code -> q of the biased form, on codes recovered from the reference's own outputs: bit for
    bit on every qualifying fixture (98 when this was written)."""
    n, bad, kbig = 0, [], 0
    for sp, x, q, l1, m in M.qualifying_fixtures():
        codes = M.recover_codes(x, q, l1, m)
        k, _ = M.counts(codes)
        kbig = max(kbig, int(k.max()))
        assert int(k.sum()) <= m, sp["idx"]
        if not np.any(x == 0):
            assert int(k.sum()) == m, sp["idx"]
        if not G.bits_equal(M.decode(codes, l1, m, M.BIASED), q):
            bad.append(sp["idx"])
        n += 1
    assert n >= 90, n
    assert not bad, f"model differs from the reference on fixtures {bad}"
    assert kbig > 1


def test_forms_differ_in_low_bits():
    """The two forms group their products differently: the unbiased table is wrong for biased codes."""
    codes = np.arange(0, 128, dtype=np.int64)
    a = M.decode(codes, f32(797.8845), 1000003, M.UNBIASED)
    b = M.decode(codes, f32(797.8845), 1000003, M.BIASED)
    assert np.allclose(a, b, rtol=1e-6) and not G.bits_equal(a, b)


def _tc(form):
    rng = np.random.default_rng(5)
    codes = rng.integers(-6, 6, (3, 17)).astype(np.int8)
    k, _ = M.counts(codes)
    return uqdme.TypeCodes(codes=torch.from_numpy(codes), l1=torch.tensor([1.5, 0.0, 3e7]), m=23,
                           overflow=torch.from_numpy(k.max(axis=1).astype(np.int32)), form=form)


@pytest.mark.parametrize("form", ["unbiased", "biased"])
def test_typecodes_bytes_round_trip(form):
    tc = _tc(form)
    buf = tc.to_bytes()
    assert struct.unpack_from("<I", buf, 4)[0] == (2 if form == "biased" else 1)
    back = uqdme.TypeCodes.from_bytes(buf)
    assert back.form == form and back.m == 23 and (back.n, back.d) == (3, 17)
    assert torch.equal(back.codes, tc.codes) and torch.equal(back.l1, tc.l1) and torch.equal(back.overflow, tc.overflow)
    with pytest.raises(ValueError):
        uqdme.TypeCodes.from_bytes(buf[:-1])


def test_version_1_buffer_loads_as_unbiased():
    tc = _tc("unbiased")
    codes = tc.codes.numpy()
    v1 = (struct.pack("<4sIqqq", b"UQT1", 1, 3, 17, 23) + tc.l1.numpy().astype("<f4").tobytes()
          + codes.astype(np.int8).tobytes())
    assert v1 == tc.to_bytes()                       # unbiased codes keep the version-1 layout
    back = uqdme.TypeCodes.from_bytes(v1)
    assert back.form == "unbiased" and torch.equal(back.codes, tc.codes)
    with pytest.raises(ValueError):                  # an unknown form
        uqdme.TypeCodes.from_bytes(struct.pack("<4sIqqqI", b"UQT1", 2, 0, 0, 1, 9))
    with pytest.raises(ValueError):
        uqdme.TypeCodes(codes=tc.codes, l1=tc.l1, m=23, overflow=tc.overflow, form="other").to_bytes()


def test_from_messages_reads_the_form_and_refuses_a_mix():
    C.build()
    codes = np.array([3, -1, 0, 2, -4, 0, 1, 0], np.int8)
    plain = C.codec_encode(codes, 10, 2.5, True)
    biased = bytearray(plain)
    biased[6] |= 2                                   # UQ_TC_BIASED_FORM beside bit 0
    biased = bytes(biased)
    assert uqdme.TypeMessages.from_messages([plain, plain], 8, device="cpu").form == "unbiased"
    tm = uqdme.TypeMessages.from_messages([biased, biased], 8, device="cpu")
    assert tm.form == "biased" and tm.exact_zero_signs and tm.m == 10
    with pytest.raises(ValueError, match="form"):
        uqdme.TypeMessages.from_messages([plain, biased], 8, device="cpu")
