"""CPU: the numpy model of the UQR1 format (tests/codec_model.py) against the C oracle
(oracle/uq_codec.c).  The two were written separately from the same format text; here they
must agree byte for byte on every input of test_codec_oracle.py and on every synthetic
batch of tests/codec_cases.py, and the oracle must decode the model's messages with tables
its own encoder never chooses.  The GPU stress tests then lean on both."""
import numpy as np
import pytest

from oracle import uq_oracle as O
from oracle import uq_oracle_c as C
from tests import codec_cases as K
from tests import codec_model as M


def _value_codes(c):
    return np.where(c == -1, 0, c).astype(np.int8)


def _agree(c, m, l1, d):
    for exact in (False, True):
        ref = C.codec_encode(c, m, l1, exact)
        got = M.encode(c, m, l1, exact)
        assert got == ref, (d, exact, len(got), len(ref))
        c2, L2, m2 = M.decode(ref, d)
        assert np.array_equal(c2, c if exact else _value_codes(c))
        assert np.float32(L2).view(np.uint32) == np.float32(l1).view(np.uint32) and m2 == m


# the cases of test_codec_oracle.py::test_roundtrip_exact_and_value, same draws
@pytest.mark.parametrize("d,R,dist", [(1024, 1, "normal"), (4099, 2, "laplace"), (65536, 0.5, "normal"),
                                      (65537, 1, "normal"), (172554, 1, "normal"), (100003, 4, "normal"),
                                      (3000, 5, "laplace"), (1, 1, "normal"), (63, 2, "normal"), (70000, 6, "normal")])
def test_model_matches_oracle_on_quantizer_output(d, R, dist):
    rng = np.random.default_rng(d)
    x = (rng.standard_normal(d) if dist == "normal" else rng.laplace(1, 2, d)).astype(np.float32)
    m = O.rate_to_m(R, d)
    c, L, ovf = O.type_codes(x, m, np.float32(0.37))
    assert not ovf
    _agree(c, m, L, d)


def test_model_matches_oracle_on_rate_inputs():
    """test_codec_oracle.py::test_rate_near_nominal's inputs: d = 2^20 at R = 1, 2 and 0.5."""
    x = np.random.default_rng(1).standard_normal(1 << 20).astype(np.float32)
    for R in (1, 2, 0.5):
        m = O.rate_to_m(R, x.shape[0])
        c, L, ovf = O.type_codes(x, m, np.float32(0.37))
        assert not ovf
        _agree(c, m, L, x.shape[0])


def test_model_matches_oracle_on_degenerate_inputs():
    """test_codec_oracle.py's degenerate and corruption inputs."""
    _agree(np.zeros(5000, np.int8), 10, np.float32(3.0), 5000)
    for exact in (False, True):
        msg = M.encode(np.zeros(0, np.int8), 0, np.float32(0.0), exact)
        assert msg == C.codec_encode(np.zeros(0, np.int8), 0, np.float32(0.0), exact) and len(msg) == 40
        assert M.decode(msg, 0)[0].shape == (0,)
    c = np.arange(-128, 128, dtype=np.int64).astype(np.int8).repeat(7)
    np.random.default_rng(0).shuffle(c)
    _agree(c, 999, np.float32(1.5), c.shape[0])
    rng = np.random.default_rng(2)
    m = O.rate_to_m(1, 20000)
    c, L, _ = O.type_codes(rng.standard_normal(20000).astype(np.float32), m, np.float32(0.37))
    _agree(c, m, L, 20000)
    msg = bytearray(C.codec_encode(c, m, L, True))
    for pos in (0, 8, 30, len(msg) - 1):                              # the same verdicts on corrupted bytes
        bad = bytearray(msg)
        bad[pos] ^= 0x5A
        verdict = []
        for dec in (C.codec_decode, M.decode):
            try:
                verdict.append(dec(bytes(bad), 20000)[0].tobytes())
            except ValueError:
                verdict.append(None)
        assert verdict[0] == verdict[1], pos
    for dec in (C.codec_decode, M.decode):                            # wrong d
        with pytest.raises(ValueError):
            dec(bytes(msg), 20001)


@pytest.mark.parametrize("name", list(K.STRESS))
def test_model_matches_oracle_on_stress_inputs(name):
    codes = K.stress(name)
    l1, m = K.side(name, codes.shape[0])
    for j in range(codes.shape[0]):
        _agree(codes[j], m, l1[j], codes.shape[1])


def test_normalisation_matches_oracle_rule():
    """normalize() against uqc_normalize on count vectors that need several rounds, ties and
    a shortfall; the model also reports the rounds."""
    rng = np.random.default_rng(3)
    cases = [np.r_[np.ones(192, np.int64), np.full(64, 1021)], np.r_[5, np.ones(255, np.int64)],
             np.array([1, 0, 65535]), np.array([0, 7]), np.full(256, 3)]
    cases += [rng.integers(0, 2000, 256) * (rng.random(256) < 0.7) for _ in range(20)]
    cases += [np.r_[np.ones(200, np.int64), rng.integers(900, 1100, 56)] for _ in range(5)]
    rounds = []
    for cnt in cases:
        cnt = np.ascontiguousarray(cnt, np.uint32)
        if cnt.sum() == 0:
            continue
        f = C.codec_normalize(cnt, int(cnt.sum()))
        got, r = M.normalize(cnt, int(cnt.sum()))
        assert np.array_equal(got, f) and got.sum() == M.M and (got[cnt > 0] >= 1).all()
        rounds.append(r)
    assert rounds[0] == 3 and max(rounds) >= 3


@pytest.mark.parametrize("name", list(K.TABLES))
def test_oracle_decodes_model_messages_with_foreign_tables(name):
    codes, f, nsym, msgs = K.table_case(name)
    n, d = codes.shape
    l1, m = K.side(name, n)
    for j in range(n):
        p = M.parse(msgs[j])
        assert p["nsym"] == nsym and np.array_equal(p["f"], f) and len(msgs[j]) % 4 == 0
        for dec in (C.codec_decode, M.decode):
            c2, L2, m2 = dec(msgs[j], d)
            assert np.array_equal(c2, codes[j]), (name, j, dec)
            assert np.float32(L2).view(np.uint32) == l1[j].view(np.uint32) and m2 == m


def test_oracle_refuses_what_it_cannot_bound():
    """A header longer than the message, a chunk count that is not d's, and words_end past the
    words present are refused (before: read past the buffer)."""
    import struct
    c = K.natural(1, 70001, 9)[0]
    msg = C.codec_encode(c, 77, np.float32(1.0), False)
    p = M.parse(msg)
    assert np.array_equal(C.codec_decode(msg, 70001)[0], _value_codes(c))
    words_present = (len(msg) - p["words"]) // 2

    def put(off, fmt, v):
        b = bytearray(msg)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)

    bad = [put(p["wend"] + 4, "<I", words_present + 1),              # words_end[last] past the words
           put(p["wend"] + 4, "<I", 0xFFFFFFFF),
           put(p["wend"], "<I", words_present + 1),
           put(32, "<I", p["nch"] + 1), put(32, "<I", 1 << 30),      # chunk count
           put(28, "<H", 1)]                                         # nsym < 2 with d > 0
    short = bytearray(msg[:p["states"]])                             # the header no longer fits
    struct.pack_into("<I", short, 36, len(short))
    bad.append(bytes(short))
    for b in bad:
        for dec in (C.codec_decode, M.decode):
            with pytest.raises(ValueError):
                dec(b, 70001)
