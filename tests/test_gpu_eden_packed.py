"""EDEN messages at their rate on the GPU: the converters against the NumPy model of the layout
(tests/eden_packed_model.py), the packed sender and receiver against the u8 entry points at the smallest shapes that
reach each dispatch form (fused KE4 / KE2+4 / redo KE4 / 4096-element first pass, and the converter path), fused
against fallback through the test hook, the fractional rates, the reference's own fixtures, and the Python surface."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import uq_eden as E
from tests import eden_frac_model as M
from tests import eden_packed_model as PM
from tests import eden_plan_hook as H
from tests import golden_data as G
from tests.test_eden_frac_model import META, Z, bits_of, sampled
from tests.test_eden_packed_host import CONVERTER, FRAC, FUSED

pytestmark = pytest.mark.gpu
FRAC_DIMS = sorted({c["d"] for c in META["cases"]})


@pytest.fixture(scope="module")
def uq(gpu_ready):
    import uqdme
    return uqdme


@pytest.fixture(scope="module")
def lib(uq):
    return uq.load_library()


def packed_form(lib, op):
    buf = (ctypes.c_int64 * 4)()
    assert lib.uq_test_last_eden_packed_plan(op, buf, 4) == 0
    return int(buf[1])


def words(t):
    """an int32 payload tensor as uint32 NumPy words"""
    return t.cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def model_rows(bins, kind, masks=None):
    rows = [PM.pack(bins[j], kind, None if masks is None else masks[j]) for j in range(bins.shape[0])]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.int64)


def convert(lib, name, src, n, D, kind, dst, mask=None, ranks=None, rows=None, pbits=None):
    from uqdme_amd._runtime import ptr, stream_ptr
    extra = (ptr(pbits),) if name == "uq_eden_pack_bins" else ()
    rc = getattr(lib, name)(ptr(src), n, D, kind, ptr(mask), ptr(ranks), ptr(rows), ptr(dst), *extra, stream_ptr(src.device))
    assert rc == 0, lib.uq_last_error()


# ---- converters ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 16, 32, 64, 2048, 4096, 32768])
@pytest.mark.parametrize("kind", [1, 2])
def test_converters_against_the_model(lib, D, kind):
    n = 3
    bins = np.stack([np.random.default_rng(s).integers(0, 1 << kind, D) for s in (11, 12, 13 + D)]).astype(np.uint8)
    want, wbits = model_rows(bins, kind)
    bd = torch.from_numpy(bins).cuda()
    pay = torch.full((n, PM.pitch(D, kind)), -1, dtype=torch.int32, device="cuda")            # prefilled with 0xFF
    pbits = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    convert(lib, "uq_eden_pack_bins", bd, n, D, kind, pay, pbits=pbits)
    assert np.array_equal(words(pay), want)                                                    # whole rows, the pitch included
    assert np.array_equal(pbits.cpu().numpy(), wbits) and wbits[0] == kind * D
    back = torch.full((n, D), 255, dtype=torch.uint8, device="cuda")
    convert(lib, "uq_eden_unpack_bins", pay, n, D, kind, back)
    assert torch.equal(back, bd)


@pytest.mark.parametrize("D", [1, 16, 32, 64, 2048, 4096, 32768])
@pytest.mark.parametrize("p_high", [0.25, 0.5, 0.999, 1e-7])
def test_converters_fractional_against_the_model(lib, D, p_high):
    from uqdme_amd import eden as ED
    seeds = [5, 123456789, 99]
    n = 3
    mask_rows = ED.eden_mask_bits(seeds, D, M.threshold(p_high))
    ranks = ED.eden_mask_ranks(mask_rows, D)
    mw = mask_rows.cpu().numpy().view(np.uint32)
    assert np.array_equal(words(ranks), np.stack([PM.ranks(mw[r], D) for r in range(n)]))       # cumulative popcounts
    rows = [2, 0, 1]                                                                           # client j reads mask row rows[j]
    masks = [PM.unplane(mw[r], D).astype(bool) for r in rows]
    if p_high == 1e-7:
        assert M.threshold(p_high) == 2 and sum(int(m.sum()) for m in masks) <= 1
    rng = np.random.default_rng(D)
    bins = np.stack([np.where(m, rng.integers(0, 4, D), rng.integers(0, 2, D)) for m in masks]).astype(np.uint8)
    want, wbits = model_rows(bins, FRAC, masks)
    assert all(wbits[j] == D + int(masks[j].sum()) for j in range(n))
    bd, rd = torch.from_numpy(bins).cuda(), torch.tensor(rows, dtype=torch.int32, device="cuda")
    pay = torch.full((n, PM.pitch(D, FRAC)), -1, dtype=torch.int32, device="cuda")
    pbits = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    convert(lib, "uq_eden_pack_bins", bd, n, D, FRAC, pay, mask_rows, ranks, rd, pbits)
    assert np.array_equal(words(pay), want)
    assert np.array_equal(pbits.cpu().numpy(), wbits)
    back = torch.full((n, D), 255, dtype=torch.uint8, device="cuda")
    convert(lib, "uq_eden_unpack_bins", pay, n, D, FRAC, back, mask_rows, ranks, rd)
    assert torch.equal(back, bd)


# ---- sender, receiver, fused == fallback ------------------------------------------------------
# (n, d, bits) -> (sender's packed form, receiver's, the u8 sender's norm and dot)
SHAPES = {
    (12, 3000, 1): (FUSED, FUSED, H.FUSED_NORM, H.FUSED_REDO),              # D = 4096: KE2+4, two chunks
    (12, 3000, 2): (FUSED, FUSED, H.CHAINS_WHOLE, H.ONE_WAVE),              # KE4, one pipelined pair of sets
    (257, 1024, 1): (FUSED, CONVERTER, H.CHAINS_GENERIC, H.ONE_WAVE),       # KE4's generic steps
    (257, 1024, 2): (FUSED, CONVERTER, H.CHAINS_GENERIC, H.ONE_WAVE),
    (257, 2048, 1): (FUSED, CONVERTER, H.FUSED_NORM, H.FUSED_REDO),         # KE2+4, smallest case
    (257, 2048, 2): (FUSED, CONVERTER, H.CHAINS_WHOLE, H.ONE_WAVE),         # KE4 pipelined, the half-size set
    (300, 16384, 1): (FUSED, FUSED, H.FUSED_NORM, H.FUSED_REDO),            # KE2+4 over 8 chunks
    (1, 32768, 1): (CONVERTER, FUSED, H.SEG_NORM, H.SEG_DOT),               # segmented dot -> converter
    (1, 32768, 2): (CONVERTER, FUSED, H.SEG_NORM, H.SEG_DOT),
    (129, 16384, 1): (FUSED, FUSED, H.SEG_NORM, H.ONE_WAVE),                # segmented norm + one-wave dot
    (129, 16384, 2): (FUSED, FUSED, H.SEG_NORM, H.ONE_WAVE),
    (5, 48, 1): (FUSED, CONVERTER, H.CHAINS_GENERIC, H.ONE_WAVE),           # D = 64: a single step
    (5, 48, 2): (FUSED, CONVERTER, H.CHAINS_GENERIC, H.ONE_WAVE),
    (2, 5, 1): (FUSED, CONVERTER, H.CHAINS_GENERIC, H.ONE_WAVE),            # D = 8 < 32
    (2, 5, 2): (FUSED, CONVERTER, H.CHAINS_GENERIC, H.ONE_WAVE),
}


def check_packed_against_u8(uq, lib, x, bits, seeds, snd, rcv):
    """The packed sender and receiver on x against the u8 ones, then both again as the fallback (test hook bit 0).
    Returns (u8 message, packed message)."""
    D = E.padded_dim(x.shape[1])
    xd = torch.from_numpy(x).cuda()
    u8 = uq.eden_compress(xd, bits, seeds=seeds)
    plan_u8 = H.last_plan(lib, H.COMPRESS)
    pk = uq.eden_compress(xd, bits, seeds=seeds, packed=True)
    assert packed_form(lib, H.COMPRESS) == snd
    assert H.last_plan(lib, H.COMPRESS) == plan_u8                       # the same norm / dot / passes as the u8 call
    want, wbits = model_rows(u8.bins.cpu().numpy(), bits)
    assert pk.bins is None and np.array_equal(words(pk.payload), want)
    assert np.array_equal(pk.payload_bits.cpu().numpy(), wbits) and wbits[0] == bits * D
    assert same_bits(pk.scale, u8.scale)
    out_u8 = uq.eden_decompress(u8)
    plan_d = H.last_plan(lib, H.DECOMPRESS)
    assert packed_form(lib, H.DECOMPRESS) == 0                           # (a u8 call leaves no packed plan)
    out_pk = uq.eden_decompress(pk)
    assert packed_form(lib, H.DECOMPRESS) == rcv and H.last_plan(lib, H.DECOMPRESS) == plan_d
    assert out_pk.shape == (x.shape[0], x.shape[1]) and same_bits(out_pk, out_u8)
    prev = lib.uq_test_set_eden_hooks(1)
    try:
        fb = uq.eden_compress(xd, bits, seeds=seeds, packed=True)
        assert packed_form(lib, H.COMPRESS) == CONVERTER and H.last_plan(lib, H.COMPRESS) == plan_u8
        out_fb = uq.eden_decompress(pk)
        assert packed_form(lib, H.DECOMPRESS) == CONVERTER
    finally:
        lib.uq_test_set_eden_hooks(prev)
    assert torch.equal(fb.payload, pk.payload) and same_bits(fb.scale, pk.scale) and torch.equal(fb.payload_bits, pk.payload_bits)
    assert same_bits(out_fb, out_pk)
    return u8, pk


@pytest.mark.parametrize("n,d,bits", list(SHAPES))
def test_sender_and_receiver_against_u8(uq, lib, n, d, bits):
    snd, rcv, norm, dot = SHAPES[(n, d, bits)]
    rng = np.random.default_rng(1000 * bits + d + n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    seeds = [int(s) for s in rng.integers(0, 100, n)]
    if n > 2:
        seeds[1] = 123456                                                # one seed outside 0..99
    if (n, d, bits) == (257, 2048, 1):
        # two rows KE2+4 flags (a zero vector, a norm that overflows to inf): its redo is the packed KE4 with the
        # half-size register set (D = 2048), which no other case runs at 1 bit
        x[7] = 0.0
        x[100] *= np.float32(1e25)
    check_packed_against_u8(uq, lib, x, bits, seeds, snd, rcv)
    p = H.last_plan(lib, H.COMPRESS)
    assert (p["norm"], p["dot"]) == (norm, dot), p
    assert (H.kernels(H.last_plan(lib, H.DECOMPRESS))[0] == H.LOW4096) == (rcv == FUSED)


def test_redo_clients_in_the_fused_batch(uq, lib):
    """260 x 4096 at 1 bit runs KE2+4; the rows with norms outside the sign rule's range (tiny, huge, underflowing
    quotients, a zero vector) are flagged and rewritten by KE4's packed redo instance: payload and scale are the u8
    path's, which for those rows are the oracle's, and a zero vector's coordinates all sit in the last bin."""
    rng = np.random.default_rng(12)
    n, d = 260, 4096
    x = rng.standard_normal((n, d)).astype(np.float32)
    special = {3: 1e-13, 64: 1e9, 65: 1e-15, 130: 1e15, 200: 3e-30, 259: 0.0}
    for j, s in special.items():
        x[j] = (rng.standard_normal(d) * s).astype(np.float32) if s else 0.0
    seeds = [int(s) for s in rng.integers(0, 100, n)]
    u8, pk = check_packed_against_u8(uq, lib, x, 1, seeds, FUSED, FUSED)
    p = H.last_plan(lib, H.COMPRESS)
    assert (p["norm"], p["dot"]) == (H.FUSED_NORM, H.FUSED_REDO)
    pay, sc = words(pk.payload), pk.scale.cpu().numpy()
    for j in list(special) + [0]:
        with np.errstate(invalid="ignore", divide="ignore"):
            bins, s, _, _ = E.eden_compress(x[j], 1, seeds[j])
        assert np.array_equal(pay[j], PM.pack(bins, 1)[0]), j
        assert bits_of(sc[j]) == bits_of(s) or (np.isnan(sc[j]) and np.isnan(s)), j
    assert (pay[259] == 0xFFFFFFFF).all()                                # 0 / 0 -> NaN -> the last bin


# ---- the reference's fixtures -------------------------------------------------------------------
def test_reference_fixtures_integer_rates(uq):
    meta, z = G.eden()
    for case in meta["cases"]:
        i = case["idx"]
        x = torch.as_tensor(G.eden_input(case, z)).cuda().view(1, -1)
        msg = uq.eden_compress(x, case["nbits"], seeds=[case["rseed"]], packed=True)
        assert msg.bins is None and int(msg.payload_bits[0]) == case["nbits"] * case["D"], i
        bins = uq.eden_unpack(msg).bins.cpu().numpy()[0]
        assert bins.shape[0] == case["D"] and G.sha(bins) == case["bins_sha"], i
        s = np.float32(msg.scale.cpu().numpy()[0])
        assert bits_of(s) == bits_of(np.float32(case["scale"])) or (np.isnan(s) and np.isnan(case["scale"])), i
        out = uq.eden_decompress(msg).cpu().numpy()[0]
        assert G.sha(out) == case["out_sha"], i
        if f"out{i}" in z.files:
            assert G.bits_equal(out, z[f"out{i}"]), i
        else:
            assert G.bits_equal(out[z[f"pos{i}"]], z[f"outs{i}"]), i


@pytest.mark.parametrize("dim", FRAC_DIMS)
def test_reference_fixtures_fractional_rates(uq, dim):
    for c in (c for c in META["cases"] if c["d"] == dim):
        tag = (c["idx"], dim, c["nbits"], c["rseed"])
        x = torch.from_numpy(G.spec_gen(c)).cuda().view(1, -1)
        msg = uq.eden_compress(x, c["nbits"], seeds=[c["rseed"]], packed=True)
        assert msg.bins is None and list(msg.nbits) == c["msg_nbits"], tag
        bins = uq.eden_unpack(msg).bins.cpu().numpy()[0]
        assert bins.shape[0] == c["D"] and G.sha(bins) == c["bins_sha"], tag
        assert bits_of(msg.scale.cpu().numpy()[0]) == c["scale_bits"], tag
        out = uq.eden_decompress(msg).cpu().numpy()[0]
        assert G.sha(out) == c["out_sha"], tag
        if f"out{c['idx']}" in Z.files:
            assert G.bits_equal(out, Z[f"out{c['idx']}"]), tag
        else:
            pos, want = sampled(c)
            assert G.bits_equal(out[pos], want), tag


# ---- fractional rates ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(7, 3000), (1, 32768)])
@pytest.mark.parametrize("rate", [1.25, 1.5])
def test_fractional_against_the_model(uq, lib, n, d, rate):
    from uqdme_amd import eden as ED
    D = E.padded_dim(d)
    rng = np.random.default_rng(d + int(100 * rate))
    x = rng.standard_normal((n, d)).astype(np.float32)
    # seeds 0..99 (the shared rows); a set the cache keeps with seeds outside that range (<= 4 distinct, one of them
    # negative); and, for the batch, six distinct seeds, which the cache does not keep
    for seeds in ([7, 99, 0, 42, 7, 13, 64][:n], [123456789, 5, -3, 5, 1000003, 123456789, -3][:n],
                  [123456789, 5, 5, 100, 99, 1000003, -3][:n]):
        xd = torch.from_numpy(x).cuda()
        u8 = uq.eden_compress(xd, rate, seeds=seeds)
        pk = uq.eden_compress(xd, rate, seeds=seeds, packed=True)
        assert packed_form(lib, H.COMPRESS) == CONVERTER
        masks = [M.mask(s, D, M.p_high(rate)) for s in seeds]
        want, wbits = model_rows(u8.bins.cpu().numpy(), FRAC, masks)
        assert np.array_equal(words(pk.payload), want)
        assert np.array_equal(pk.payload_bits.cpu().numpy(), np.array([D + int(m.sum()) for m in masks])) and (wbits == pk.payload_bits.cpu().numpy()).all()
        assert same_bits(pk.scale, u8.scale) and pk.nbits == u8.nbits
        assert pk.nbytes == sum(-(-int(b) // 8) for b in wbits) < u8.nbytes // 4
        out = uq.eden_decompress(pk)
        assert packed_form(lib, H.DECOMPRESS) == CONVERTER
        assert same_bits(out, uq.eden_decompress(u8))
        # warm: no mask row and no rank row built (the cache keeps seeds 0..99, single seeds and sets of <= 4)
        builds, rank_builds = ED._masks.builds, ED._masks.rank_builds
        again = uq.eden_compress(xd, rate, seeds=seeds, packed=True)
        assert same_bits(uq.eden_decompress(again), out)
        kept = all(0 <= s < 100 for s in seeds) or len(set(seeds)) <= 4
        assert kept == ((ED._masks.builds, ED._masks.rank_builds) == (builds, rank_builds)), seeds
        assert torch.equal(again.payload, pk.payload)
        assert torch.equal(uq.eden_unpack(pk).bins, u8.bins)


# ---- the Python surface ---------------------------------------------------------------------------
def test_python_surface(uq):
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((6, 100)).astype(np.float32)).cuda()
    seeds = [1, 2, 3, 101, 2, 99]
    for b in (1, 2, 1.5):
        u8 = uq.eden_compress(x, b, seeds=seeds)
        pk = uq.eden_compress(x, b, seeds=seeds, packed=True)
        assert pk.bins is None and pk.packed and not u8.packed and u8.payload is None and u8.payload_bits is None
        assert pk.payload.dtype == torch.int32 and pk.payload_bits.dtype == torch.int64 and pk.payload.shape[0] == 6
        packed = uq.eden_pack(u8)                                           # field for field
        assert packed.bins is None and torch.equal(packed.payload, pk.payload) and torch.equal(packed.payload_bits, pk.payload_bits)
        assert same_bits(packed.scale, pk.scale) and torch.equal(packed.seeds, pk.seeds)
        assert packed.nbits == pk.nbits and packed.dim == pk.dim == 100 and packed.nbytes == pk.nbytes
        back = uq.eden_unpack(pk)
        assert back.payload is None and torch.equal(back.bins, u8.bins) and back.nbytes == u8.nbytes == 6 * 128
        assert uq.eden_pack(pk) is pk and uq.eden_unpack(u8) is u8
        assert same_bits(uq.eden_decompress(pk), uq.eden_decompress(u8))
    one = uq.eden_compress(x, 1, seeds=seeds, packed=True)
    assert one.nbytes == 128 // 8 * 6                                       # D / 8 bytes per client at 1 bit
    # a message built the old way, positional fields and nothing else, still decompresses
    u8 = uq.eden_compress(x, 2, seeds=seeds)
    old = uq.EdenMessage(u8.bins, u8.scale, u8.seeds, 2, 100)
    assert same_bits(uq.eden_decompress(old), uq.eden_decompress(u8))
    with pytest.raises(ValueError):
        uq.eden_decompress(uq.EdenMessage(None, u8.scale, u8.seeds, 2, 100, payload=one.payload, payload_bits=one.payload_bits))
    empty = uq.eden_compress(torch.zeros((0, 16)), 1, packed=True)
    assert empty.payload.shape == (0, 1) and empty.nbytes == 0 and uq.eden_decompress(empty).shape == (0, 16)
