"""GPU: the UQR1 codec (csrc/uq_codec_kernels.h, KC1-KC7) away from quantizer output.

The other codec tests feed natural codes at R <= 2: 80 % zeros, a handful of renormalisation
words per step, tables from the project's own normalisation.  Here the codes are synthetic
(tests/codec_cases.py) and three voices must agree byte for byte: the GPU, the C oracle
(oracle/uq_codec.c) and the numpy model of the format (tests/codec_model.py, pinned to the
oracle in test_codec_model.py).  Each case first proves from the model that it reaches what
it claims:

* all 256 codes (nsym = 256, code -128; KC1's LDS-atomic path as the common one; ~128 words
  per 4-step group in the full-chunk rings) at every d where W or the path changes;
* a burst of 254 symbols with f = 1: 192 words in one group, the most the coder can emit (12
  bits per step, 16 per word), at the start, the end and the middle of a full chunk;
* one symbol (f = 4096, x_max = 2^32 - 1, no words, total_words = 0, KC1's SWAR path on one
  bin) and one rare symbol against f = 4095;
* KC2's normalisation loop running 2 and 3 rounds, with ties on every round;
* 66 chunks (KC4's carry into a second block of 64);
* decoder tables the encoder never writes: 12 bits for every symbol of a chunk (192 words per
  group, sustained: the refill logic's worst load), odd nsym, zero-frequency gaps, f = 4096 at
  a non-zero index;
* each decoder status bit alone, the good messages beside the bad one still decoded.
"""
import struct

import numpy as np
import pytest
import torch

from oracle import uq_oracle_c as C
from tests import codec_cases as K
from tests import codec_model as M

pytestmark = pytest.mark.gpu


def _value_codes(c):
    return np.where(c == -1, 0, c).astype(np.int8)


def _type_codes(codes, l1, m):
    import uqdme
    k = np.where(codes < 0, -codes.astype(np.int32) - 1, codes.astype(np.int32))
    kmax = k.max(axis=1) if codes.shape[1] else np.zeros(codes.shape[0], np.int32)
    return uqdme.TypeCodes(codes=torch.from_numpy(codes.copy()).cuda(), l1=torch.from_numpy(l1.copy()).cuda(), m=m,
                           overflow=torch.from_numpy(kmax.astype(np.int32)).cuda())


UNIFORM_REACH = {1: (1, 0, 1), 63: (1, 0, 63), 64: (1, 0, 64), 65: (1, 0, 65), 1023: (1, 0, 1023), 1024: (1, 0, 1024),
                 1025: (2, 0, 1025), 65535: (64, 0, 65535), 65536: (64, 1, 0), 65537: (64, 1, 1),
                 2 * 65536 + 1000: (64, 2, 1000)}


def _precondition(name, row, exact):
    """What the case claims, from the model (never from the code under test)."""
    d = row.shape[0]
    f, nsym, rounds = M.table_of(row, exact)
    wpg = M.words_per_group(row, exact)
    kind = name.split("-")[0]
    if kind == "uniform256":
        # what each d reaches: (lanes W, chunks on the full-chunk path, symbols of a generic-path chunk)
        fast = d // K.CHUNK if M.lanes(d) == 64 else 0
        assert (M.lanes(d), fast, d - fast * K.CHUNK) == UNIFORM_REACH[d], d
        if d == 1:
            assert f.max() == 4096 and wpg.sum() == 0      # one symbol: a state, no words
        else:
            assert wpg.sum() > 0                           # the states renormalise at all
        if d >= 1023:                                      # ~8 bits = half a word per symbol (a little less for
            assert nsym == 256                             # a small sample, a little more for quantized f)
            assert 0.45 * d <= wpg.sum() <= 0.52 * d
        if d >= K.CHUNK - 1:
            assert wpg[0].max() >= 128                     # 8 bits per symbol = 128 words per group
    elif kind == "burst":
        assert nsym == 256 and (f == 1).sum() == 254 and f.max() == 3842
        assert wpg.max() == 192
    elif kind == "single":
        assert (f == 4096).sum() == 1 and f.sum() == 4096 and wpg.sum() == 0
    elif kind == "one":
        assert sorted(f[f > 0].tolist()) == [1, 4095] and M.nchunks(d) >= 12
    elif kind == "multi":
        assert rounds >= 2 and nsym == 256
        if name.endswith("equal"):                         # every round chooses among equal frequencies
            assert (f == np.sort(f)[-2]).sum() >= 32
    elif kind == "chunks":
        assert M.nchunks(d) > 64 and d % K.CHUNK not in (0, 1)
    return nsym


@pytest.mark.parametrize("name", list(K.STRESS))
def test_synthetic_codes_three_way(gpu_ready, name):
    import uqdme
    codes = K.stress(name)
    n, d = codes.shape
    l1, m = K.side(name, n)
    if name.startswith("single"):
        l1[:] = l1[0]                                      # rows comparable byte for byte
    tc = _type_codes(codes, l1, m)
    for exact in (False, True):
        nsym = [_precondition(name, codes[j], exact) for j in range(n)]
        want = codes if exact else _value_codes(codes)
        msgs = uqdme.encode_messages(tc, exact_zero_signs=exact)
        gpu = msgs.messages()
        ref = [C.codec_encode(codes[j], m, l1[j], exact) for j in range(n)]
        for j in range(n):
            assert gpu[j] == ref[j], (name, exact, j, len(gpu[j]), len(ref[j]))
            assert gpu[j] == M.encode(codes[j], m, l1[j], exact), (name, exact, j)
            c2, L2, m2 = C.codec_decode(gpu[j], d)                         # the CPU decodes the GPU's message
            assert np.array_equal(c2, want[j]) and L2.view(np.uint32) == l1[j].view(np.uint32) and m2 == m
        if name.startswith("single"):
            for j in range(n):                             # header, table, one words_end and states per chunk: no words, no padding
                assert len(gpu[j]) == M.header_bytes(nsym[j], M.nchunks(d), 64), (name, j)
                assert M.parse(gpu[j])["words_end"].tolist() == [0] * M.nchunks(d)
            if not exact:
                assert gpu[2] == gpu[3]                    # all -1 is all 0 in value mode
        for src in (msgs, uqdme.TypeMessages.from_messages(ref, d)):       # the GPU decodes its own and the CPU's
            back = uqdme.decode_messages(src)
            assert np.array_equal(back.codes.cpu().numpy(), want), (name, exact)
            assert np.array_equal(back.l1.cpu().numpy().view(np.uint32), l1.view(np.uint32)) and back.m == m
            assert back.overflow.cpu().tolist() == [(s - 2) // 2 for s in nsym]


@pytest.mark.parametrize("name", list(K.TABLES))
def test_decoder_on_tables_the_encoder_never_writes(gpu_ready, name):
    import uqdme
    codes, f, nsym, msgs = K.table_case(name)
    n, d = codes.shape
    l1, m = K.side(name, n)
    if name.startswith("12bit"):
        full = d // K.CHUNK
        for j in range(n):
            wpg = M.words_per_group(codes[j], True, f, nsym)
            assert (wpg[:full] == 192).all() and (wpg[:full].sum(axis=1) == 49152).all()
    if name.startswith("f4096"):
        assert all(M.parse(b)["words_end"][-1] == 0 for b in msgs) and np.flatnonzero(f).tolist() == [9]
    for j in range(n):
        assert np.array_equal(C.codec_decode(msgs[j], d)[0], codes[j])
    back = uqdme.decode_messages(uqdme.TypeMessages.from_messages(list(msgs), d))
    assert np.array_equal(back.codes.cpu().numpy(), codes), name
    assert np.array_equal(back.l1.cpu().numpy().view(np.uint32), l1.view(np.uint32)) and back.m == m
    assert back.overflow.cpu().tolist() == [(nsym - 2) // 2] * n


# ---- each status bit alone --------------------------------------------------------------------
# Every corruption keeps the decoder's reads inside the message: the header size is checked
# before words_end and the states are read, a chunk's word count is clamped (`bad`), the slot
# table is indexed with x & 4095 and the rings modulo their size.

D_ST = 70001                  # one full chunk and one ragged chunk
M_ST = 4242


@pytest.fixture(scope="module")
def good():
    codes = K.natural(4, D_ST, 600)
    msgs = [C.codec_encode(codes[j], M_ST, np.float32(1.25 + j), False) for j in range(4)]
    return _value_codes(codes), msgs


def _u32(b, off, v=None):
    if v is None:
        return struct.unpack_from("<I", b, off)[0]
    struct.pack_into("<I", b, off, v & 0xFFFFFFFF)


def _table_sum_4097(b, p):
    a = int(np.argmax(p["f"]))
    struct.pack_into("<H", b, 40 + 2 * a, int(p["f"][a]) + 1)


def _table_shifted(b, p):                                  # the sum stays 4096
    a = int(np.argmax(p["f"]))
    o = int(np.flatnonzero(p["f"])[-1])
    assert o != a
    struct.pack_into("<H", b, 40 + 2 * a, int(p["f"][a]) - 1)
    struct.pack_into("<H", b, 40 + 2 * o, int(p["f"][o]) + 1)


def _words_present(b, p):
    return (len(b) - p["words"]) // 2


TABLE, WORDS, WORDS_OR_STATE, HEADER = 2, 4, 12, 1
CORRUPTIONS = {
    "table-sum-4097": (_table_sum_4097, TABLE),
    "table-shifted": (_table_shifted, WORDS_OR_STATE),
    "words_end0-minus-1": (lambda b, p: _u32(b, p["wend"], _u32(b, p["wend"]) - 1), WORDS),
    "words_end-decreasing": (lambda b, p: _u32(b, p["wend"] + 4, _u32(b, p["wend"]) - 1), WORDS),
    "words_end-past-words": (lambda b, p: _u32(b, p["wend"] + 4, _words_present(b, p) + 1), WORDS),
    "state-low-bit": (lambda b, p: _u32(b, p["states"] + 4 * 5, _u32(b, p["states"] + 4 * 5) ^ 1), WORDS_OR_STATE),
    "state-high-bit": (lambda b, p: _u32(b, p["states"] + 4 * 70, _u32(b, p["states"] + 4 * 70) ^ (1 << 21)), WORDS_OR_STATE),
    "word-bit": (lambda b, p: b.__setitem__(p["words"] + 2 * (int(p["words_end"][0]) // 2),
                                            b[p["words"] + 2 * (int(p["words_end"][0]) // 2)] ^ 0x10), WORDS_OR_STATE),
    "nsym-1": (lambda b, p: struct.pack_into("<H", b, 28, 1), HEADER),
    "nsym-257": (lambda b, p: struct.pack_into("<H", b, 28, 257), HEADER),
    "size-plus-4": (lambda b, p: _u32(b, 36, len(b) + 4), HEADER),
    "size-minus-4": (lambda b, p: _u32(b, 36, len(b) - 4), HEADER),
}


@pytest.mark.parametrize("k,name", list(enumerate(CORRUPTIONS)))
def test_each_status_bit_alone(gpu_ready, good, k, name):
    import uqdme
    from uqdme_amd import _lib
    lib = _lib.load()
    want, msgs = good
    n, victim = 4, k % 4
    spoil, expect = CORRUPTIONS[name]
    b = bytearray(msgs[victim])
    p = M.parse(msgs[victim])
    assert p["nch"] == 2 and p["words_end"][0] > 256 and len(b) == p["total"]
    spoil(b, p)
    assert bytes(b) != msgs[victim] and len(b) == len(msgs[victim])
    batch = list(msgs)
    batch[victim] = bytes(b)
    tm = uqdme.TypeMessages.from_messages(batch, D_ST)
    codes = torch.zeros((n, D_ST), dtype=torch.int8, device="cuda")
    l1 = torch.zeros(n, device="cuda")
    km = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    _lib.check(lib.uq_tc_decode(tm.data.data_ptr(), tm.data.numel(), tm.offsets.data_ptr(), n, D_ST, M_ST,
                                codes.data_ptr(), l1.data_ptr(), km.data_ptr(), st.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), "decode")
    torch.cuda.synchronize()
    st = st.cpu().tolist()
    got = codes.cpu().numpy()
    for j in range(n):
        if j != victim:
            assert st[j] == 0 and np.array_equal(got[j], want[j]), (name, j, st)
            assert l1[j].item() == 1.25 + j and km[j].item() == (M.parse(msgs[j])["nsym"] - 2) // 2
    s = st[victim]
    if name == "table-shifted":                            # a valid table, the wrong one
        assert s != 0 and (s & 12 or not np.array_equal(got[victim], want[victim])), (name, s)
        assert (s & ~12) == 0, (name, s)
    elif expect == WORDS_OR_STATE:
        assert (s & 12) != 0 and (s & ~12) == 0, (name, s)
    elif name == "words_end0-minus-1":                     # chunk 0 overruns (4); chunk 1 starts a word early: 4 or 8
        assert (s & 4) != 0 and (s & ~12) == 0, (name, s)
    elif expect == WORDS:                                  # only chunk 1 is touched, and refused before it decodes
        assert s == 4, (name, s)
    else:
        assert s == expect, (name, s)
    # the oracle's verdict on the same bytes
    try:
        c2, _, _ = C.codec_decode(bytes(b), D_ST)
    except ValueError:
        return
    assert name == "table-shifted" and not np.array_equal(c2, want[victim])
