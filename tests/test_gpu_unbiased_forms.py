"""GPU: every K2 form of the unbiased quantizer, and the template instances inside each, against
the oracle -- with the form a call took asserted through uq_test_last_unbiased_plan, so that a
case cannot drift onto another kernel unnoticed.

Each case calls the C API with its own workspace and checks: the plan (form, V / Q / C / CV, l1
supplied, chunks, prefix launch); q bit-equal to oracle.uq_oracle_c for every row; l1_out
bit-equal to the oracle's L1 (or to the supplied l1); the codes equal to oracle.uq_oracle.type_codes
on every codable row and kmax equal to the oracle's largest count (128 on the other rows); the
pads between pitched rows untouched; and the mean from the codes (or nibbles) bit-equal to the
oracle's client mean of the oracle's q.

Inputs are the division-guard rows of tests/guard_batches.py (NaN, inf, subnormal, huge-L1,
all-zero, tiny-quotient, -0.0, tiny negative and heavy-tailed rows) with X = 0 and the largest
f32 below 1 among the draws, at R = 1 (codes fit) and R = 6.5 (counts >= 256 on the sparse and
huge-element rows: the arithmetic output path; their codes overflow).  A supplied l1 is 1.5 x the
true one, so a kernel that recomputed it would not match.  Shapes are the smallest that reach
each form (thresholds: tests/test_unbiased_plan.py)."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import uq_oracle as O
from oracle import uq_oracle_c as C
from tests import golden_data as G
from tests import guard_batches as GB
from tests import plan_hook as H

pytestmark = pytest.mark.gpu
f32 = np.float32

SENT_F = -12345.5      # sentinels in the pads
SENT_C = 77
SENT_N = 0xA5


@pytest.fixture(scope="module")
def api(gpu_ready):
    from uqdme_amd import _lib as L
    return L.load(), L


def guard_rows(n, d, seed):
    """n rows of the guard batch; fewer than 16 clients get a spread of its kinds (row 0 carries
    the -0.0 / tiny negative extras, row 8 of a 16-row batch is the all-zero row)."""
    rng = np.random.default_rng(seed)
    if n >= 16:
        return GB.division_guard_batch(n, d, rng, extras=True), GB.guard_draws(n, rng)
    x = GB.division_guard_batch(16, d, rng, extras=True)[[0, 7, 2, 8, 6, 1, 3, 4, 5][:n]]
    return np.ascontiguousarray(x), GB.guard_draws(n, rng)


def make_ref(x, X, R, T, l1_mode, code_rows=None):
    """The oracle's q, L1, codes and kmax for a batch (code_rows: the rows whose codes the numpy
    oracle restates; all by default)."""
    n, d = x.shape
    m = O.rate_to_m(R, d)
    q, l1 = C.quantize_batch(x, m, X, T)
    l1_in = None
    if l1_mode == "given":
        with np.errstate(all="ignore"):
            l1_in = (l1 * f32(1.5)).astype(f32)
        q = np.stack([C.quantize_with_l1(x[j], m, X[j], l1_in[j]) for j in range(n)])
        l1 = l1_in
    rows = np.arange(n) if code_rows is None else np.asarray(code_rows)
    codes = np.zeros((rows.size, d), np.int8)
    kmax = np.empty(rows.size, np.int32)
    for i, j in enumerate(rows):
        c, _, ovf = O.type_codes(x[j], m, X[j], l1=l1[j])
        codes[i] = c
        k = np.where(c < 0, -c.astype(np.int32) - 1, c.astype(np.int32))
        kmax[i] = 128 if ovf else int(k.max())
    return SimpleNamespace(x=x, X=X, m=m, T=T, q=q, l1=l1, l1_in=l1_in, rows=rows, codes=codes, kmax=kmax,
                           mean=C.client_mean(q, float(n)))


@functools.lru_cache(maxsize=2)
def guard_ref(n, d, R, T, l1_mode):
    x, X = guard_rows(n, d, n * 31 + d)
    return make_ref(x, X, R, T, l1_mode)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def workspace(lib, L, n, d, T):
    b = ctypes.c_size_t()
    L.check(lib.uq_workspace_bytes(n, d, T, ctypes.byref(b)), "ws")
    return torch.zeros(max(b.value, 1 << 16), dtype=torch.uint8, device="cuda")


def ptr(t):
    return None if t is None else t.data_ptr()


def run(api, ref, xd, Xd, kind, pq=0, pc=0, code_offset=0):
    """One call of uq_type_unbiased_codes_ld_f32; code_offset moves the codes' base off 16 bytes."""
    lib, L = api
    n, d = ref.x.shape
    ldq, ldc = d + pq, d + pc
    ws = workspace(lib, L, n, d, ref.T)
    qs = torch.full((n, ldq), SENT_F, device="cuda") if "Q" in kind else None
    cbuf = torch.full((n * ldc + 16,), SENT_C, dtype=torch.int8, device="cuda") if "C" in kind else None
    cs = cbuf[code_offset:code_offset + n * ldc].view(n, ldc) if "C" in kind else None
    km = torch.full((n,), 99, dtype=torch.int32, device="cuda") if "C" in kind else None
    l1o = torch.full((n,), -1.0, device="cuda")
    l1d = dev(ref.l1_in) if ref.l1_in is not None else None
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.uq_type_unbiased_codes_ld_f32(xd.data_ptr(), ptr(qs), ldq, ptr(cs), ldc, ptr(km), n, d, ref.m,
                                              Xd.data_ptr(), ptr(l1d), l1o.data_ptr(), ref.T, ws.data_ptr(), ws.numel(),
                                              st), "uq_type_unbiased_codes_ld_f32")
    torch.cuda.synchronize()
    return SimpleNamespace(q=qs, codes=cs, kmax=km, l1=l1o, ws=ws, plan=H.last_plan(lib), kind=kind, ldq=ldq, ldc=ldc)


def check_plan(p, form, kind, **want):
    assert H.FORM_NAMES[p["form"]] == form, p
    assert (p["Q"], p["C"]) == ("Q" in kind, "C" in kind), p
    for k, v in want.items():
        assert p[k] == v, (k, p)


def check_outputs(api, ref, r, min_codable=0.0):
    lib, L = api
    n, d = ref.x.shape
    assert G.bits_equal(r.l1.cpu().numpy(), ref.l1), "l1_out"
    if r.q is not None:
        got = r.q[:, :d].cpu().numpy()
        bad = [j for j in range(n) if G.n_mismatch(got[j], ref.q[j])]
        assert not bad, ("q rows differ", bad[:16], G.n_mismatch(got, ref.q))
        assert bool((r.q[:, d:] == SENT_F).all()), "q pad written"
    if r.codes is None:
        return
    codable = ref.kmax <= 127
    assert codable.mean() >= min_codable, ("too few codable rows", int(codable.sum()), n)
    km = r.kmax.cpu().numpy()
    assert np.array_equal(km[ref.rows], ref.kmax), ("kmax", np.nonzero(km[ref.rows] != ref.kmax)[0][:16])
    codes = r.codes[:, :d].cpu().numpy()
    badc = [int(j) for i, j in enumerate(ref.rows) if codable[i] and not np.array_equal(codes[j], ref.codes[i])]
    assert not badc, ("code rows differ", badc[:16])
    assert bool((r.codes[:, d:] == SENT_C).all()), "codes pad written"
    # ND:137-138 from the codes; overflowed clients are read from q (the oracle's, when the call wrote none)
    q, ldq = (r.q, r.ldq) if r.q is not None else (dev(ref.q), d)
    est = torch.empty(d, device="cuda")
    L.check(lib.uq_codes_q_mean_ld_f32(r.codes.data_ptr(), r.ldc, q.data_ptr(), ldq, r.l1.data_ptr(), r.kmax.data_ptr(),
                                       n, d, ref.m, float(n), 0, est.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "codes mean")
    torch.cuda.synchronize()
    assert G.bits_equal(est.cpu().numpy(), ref.mean), ("codes mean", G.n_mismatch(est.cpu().numpy(), ref.mean))
    # ... and over the clients with a finite L1 alone (a NaN / inf client makes the mean above NaN everywhere)
    fin = np.isfinite(ref.l1)
    if not fin.all() and fin.any():
        sel = dev(np.nonzero(fin)[0])
        cg, qg = r.codes[:, :d][sel].contiguous(), q[:, :d][sel].contiguous()
        lg, kg = r.l1[sel].contiguous(), r.kmax[sel].contiguous()
        L.check(lib.uq_codes_q_mean_ld_f32(cg.data_ptr(), d, qg.data_ptr(), d, lg.data_ptr(), kg.data_ptr(), int(fin.sum()),
                                           d, ref.m, float(n), 0, est.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "codes mean (finite clients)")
        torch.cuda.synchronize()
        want = C.client_mean(ref.q[fin], float(n))
        assert G.bits_equal(est.cpu().numpy(), want), ("codes mean (finite clients)", G.n_mismatch(est.cpu().numpy(), want))


VARIANTS = (("Q", 0, 0, 0), ("QC", 0, 0, 0), ("C", 0, 0, 0), ("QC", 64, 256, 0), ("C", 64, 256, 0), ("QC", 0, 7, 0),
            ("QC", 0, 0, 1))


def run_variants(api, ref, form, variants=VARIANTS, min_codable=0.0, **want):
    """Output kinds x pitches of one batch: (kind, ldq - d, ldc - d, offset of the codes' base)."""
    n, d = ref.x.shape
    xd, Xd = dev(ref.x), dev(ref.X)
    for kind, pq, pc, off in variants:
        r = run(api, ref, xd, Xd, kind, pq, pc, off)
        cv = "C" not in kind or (d % 16 == 0 and (pc % 16 == 0 or n == 1) and off == 0)
        check_plan(r.plan, form, kind, CV=cv, l1_given=ref.l1_in is not None, tiles=-(-d // 4096), **want)
        check_outputs(api, ref, r, min_codable)
    return r


# (d, R, T, l1): 32772 has a ragged 4-element last tile and d % 16 != 0 (no 16-byte code rows); T = 3 there
# splits |x|.sum() into two chunks
STREAM = [(32768, 1, 1, "computed"), (32768, 6.5, 3, "given"), (32772, 1, 3, "computed"), (32772, 6.5, 1, "computed"),
          (32772, 1, 1, "given"), (36880, 1, 1, "computed"), (36880, 6.5, 3, "computed"), (36880, 1, 3, "given")]


@pytest.mark.parametrize("d,R,T,l1", STREAM)
def test_stream_form(api, d, R, T, l1):
    """quantize_stream_kernel over whole clients (n >= 256, d >= 32768): <Q>, <Q, C>, <C> with
    and without 16-byte code rows."""
    ref = guard_ref(256, d, R, T, l1)
    run_variants(api, ref, "stream", min_codable=0.75 if R == 1 else 0.0, V=True, chunks=1)


@pytest.mark.parametrize("n,d,l1", [(1, 1, "computed"), (1, 5, "computed"), (1, 4096, "given"), (1, 4100, "computed"),
                                    (1, 32764, "given"), (300, 4096, "computed"), (300, 4100, "given"),
                                    (300, 32764, "computed")])
def test_small_form(api, n, d, l1):
    """quantize_small_kernel (aligned rows of d < 32768, L1 and the scan in one launch)."""
    for R in (1, 6.5):
        ref = guard_ref(n, d, R, 1, l1)
        run_variants(api, ref, "small", min_codable=0.75 if (R == 1 and n > 1) else 0.0, V=True, chunks=1)


@pytest.mark.parametrize("n,d,prefixed", [(128, 36864, True), (4, 1 << 20, True), (3, 1 << 21, False)])
def test_segments_form(api, n, d, prefixed):
    """Segmented stream: each client's kmax is an atomicMax across its segments."""
    for R in (1, 6.5) if n == 128 else (1,):
        ref = guard_ref(n, d, R, 1, "computed")
        r = run_variants(api, ref, "segments", variants=VARIANTS[:4], min_codable=0.75 if R == 1 else 0.0, V=True,
                         prefixed=prefixed, chunks=1, nj=n)
        assert r.plan["nseg"] > 1 and r.plan["R"] * r.plan["nseg"] >= r.plan["tiles"], r.plan


@pytest.mark.parametrize("n,d,V,prefixed", [(1, 32768, True, False), (4, 32768, True, True), (5, 32769, False, True),
                                            (300, 1, False, True)])
def test_phased_form(api, n, d, V, prefixed):
    """One workgroup per tile (tile_out_kernel), float4 and scalar lanes."""
    for R, l1 in ((1, "computed"), (6.5, "given")):
        ref = guard_ref(n, d, R, 1, l1)
        run_variants(api, ref, "phased", V=V, prefixed=prefixed, chunks=1, nj=n)


def test_phased_clients_past_the_record_clients(api):
    """(257, 2^17 + 1): clients at index >= 256 (no event records) with 33 tiles each.  The rows
    repeat four guard rows (the oracle runs once per distinct row), each with its own place."""
    n, d = 257, (1 << 17) + 1
    xb, Xb = guard_rows(4, d, 5)
    base = make_ref(xb, Xb, 1, 1, "computed")
    sel = np.arange(n) % 4
    ref = SimpleNamespace(x=xb[sel], X=Xb[sel], m=base.m, T=1, q=base.q[sel], l1=base.l1[sel], l1_in=None,
                          rows=np.arange(n), codes=base.codes[sel], kmax=base.kmax[sel],
                          mean=C.client_mean(base.q[sel], float(n)))
    run_variants(api, ref, "phased", variants=VARIANTS[1:2], V=False, prefixed=True, chunks=1, nj=n)


@functools.lru_cache(maxsize=1)
def two_chunk_ref():
    n, d = 65537, 5
    rng = np.random.default_rng(65537)
    x = np.tile(GB.division_guard_batch(512, d, rng, extras=True), (129, 1))[:n].copy()
    x[65535:] = rng.standard_normal((2, d)).astype(f32)          # the second chunk: ordinary, codable rows
    X = GB.guard_draws(n, rng)
    rows = np.concatenate([np.arange(256), np.arange(n - 130, n)])
    return make_ref(x, X, 4, 1, "computed", code_rows=rows)


def test_phased_two_chunks_of_clients(api):
    """(65537, 5): the grid's 65535-client chunks, every row of both chunks compared (codes
    against the numpy oracle on the first 256 and the last 130 rows; all rows through the mean)."""
    ref = two_chunk_ref()
    r = run_variants(api, ref, "phased", variants=(("Q", 0, 0, 0), ("QC", 3, 11, 0)), V=False, chunks=2, nj=2,
                     prefixed=False)
    assert r.plan["tiles"] == 1


def test_codec_two_chunks_of_clients(gpu_ready):
    """The same batch (its non-finite coordinates set to 1: the codec takes codable clients only)
    through uq_tc_encode / uq_tc_decode, whose launches chunk the clients the same way: messages
    of both chunks against the CPU restatement, and all of them back."""
    import uqdme
    big = two_chunk_ref()
    n, d = big.x.shape
    rows = np.array([0, 1, 6, 65533, 65534, 65535, 65536])
    ref = make_ref(np.where(np.isfinite(big.x), big.x, f32(1.0)), big.X, 4, 1, "computed", code_rows=rows)
    assert (ref.kmax <= 127).all()
    tc = uqdme.quantize_encode(dev(ref.x), m=ref.m, X=ref.X, torch_threads=1)
    codes = tc.codes.cpu().numpy()
    l1 = tc.l1.cpu().numpy()
    assert G.bits_equal(l1, ref.l1)
    msgs = uqdme.encode_messages(tc, exact_zero_signs=True)
    got = msgs.messages()
    assert len(got) == n
    for i, j in enumerate(rows):
        assert np.array_equal(codes[j], ref.codes[i]), j
        assert got[j] == C.codec_encode(ref.codes[i], ref.m, ref.l1[j], True), j
    back = uqdme.decode_messages(msgs)
    assert np.array_equal(back.codes.cpu().numpy(), codes)
    assert G.bits_equal(back.l1.cpu().numpy(), l1)


def unpack_nibbles(nib):
    """uint8 [n, d/2] 4-bit fields (element 2b in the low nibble of byte b) -> int8 [n, d] codes."""
    v = np.stack([nib & 0xF, nib >> 4], axis=-1).reshape(nib.shape[0], -1).astype(np.int16)
    return np.where(v >= 8, v - 16, v).astype(np.int8)


@pytest.mark.parametrize("d,pad", [(4096, 0), (4096, 16), (36864, 0), (36864, 16)])
def test_stream_nibbles_form(api, d, pad):
    """uq_type_unbiased_nibbles_ld_f32: the stream kernel with 4-bit codes; clients with kmax <= 7
    are codable in 4 bits, and uq_nibbles_q_mean_ld_f32 reads the others from q."""
    lib, L = api
    n, ldn = 256, d // 2 + pad
    for l1_mode in ("computed", "given"):
        ref = guard_ref(n, d, 1, 1, l1_mode)
        ws = workspace(lib, L, n, d, 1)
        xd, Xd = dev(ref.x), dev(ref.X)
        qs = torch.full((n, d + 4), SENT_F, device="cuda")
        nb = torch.full((n, ldn), SENT_N, dtype=torch.uint8, device="cuda")
        km = torch.full((n,), 99, dtype=torch.int32, device="cuda")
        l1o = torch.full((n,), -1.0, device="cuda")
        l1d = dev(ref.l1_in) if ref.l1_in is not None else None
        st = torch.cuda.current_stream().cuda_stream
        L.check(lib.uq_type_unbiased_nibbles_ld_f32(xd.data_ptr(), qs.data_ptr(), d + 4, nb.data_ptr(), ldn, km.data_ptr(),
                                                    n, d, ref.m, Xd.data_ptr(), ptr(l1d), l1o.data_ptr(), 1,
                                                    ws.data_ptr(), ws.numel(), st), "nibbles")
        torch.cuda.synchronize()
        check_plan(H.last_plan(lib), "stream-nibbles", "QC", V=True, CV=True, l1_given=l1d is not None, chunks=1,
                   tiles=d // 4096)
        assert G.bits_equal(l1o.cpu().numpy(), ref.l1)
        assert G.n_mismatch(qs[:, :d].cpu().numpy(), ref.q) == 0
        assert bool((qs[:, d:] == SENT_F).all()) and bool((nb[:, d // 2:] == SENT_N).all()), "pad written"
        assert np.array_equal(km.cpu().numpy(), ref.kmax)
        fits = ref.kmax <= 7
        assert fits.mean() >= 0.5, int(fits.sum())
        assert np.array_equal(unpack_nibbles(nb[:, :d // 2].cpu().numpy())[fits], ref.codes[fits])
        est = torch.empty(d, device="cuda")
        L.check(lib.uq_nibbles_q_mean_ld_f32(nb.data_ptr(), ldn, qs.data_ptr(), d + 4, l1o.data_ptr(), km.data_ptr(), n,
                                             d, ref.m, float(n), 0, est.data_ptr(), st), "nibbles mean")
        torch.cuda.synchronize()
        assert G.bits_equal(est.cpu().numpy(), ref.mean), G.n_mismatch(est.cpu().numpy(), ref.mean)
        fin = np.isfinite(ref.l1)                 # the clients with a finite L1 alone (the mean above is all NaN)
        sel = dev(np.nonzero(fin)[0])
        ng, qg = nb[:, :d // 2][sel].contiguous(), qs[:, :d][sel].contiguous()
        lg, kg = l1o[sel].contiguous(), km[sel].contiguous()
        L.check(lib.uq_nibbles_q_mean_ld_f32(ng.data_ptr(), d // 2, qg.data_ptr(), d, lg.data_ptr(), kg.data_ptr(),
                                             int(fin.sum()), d, ref.m, float(n), 0, est.data_ptr(), st), "nibbles mean")
        torch.cuda.synchronize()
        want = C.client_mean(ref.q[fin], float(n))
        assert G.bits_equal(est.cpu().numpy(), want), G.n_mismatch(est.cpu().numpy(), want)
