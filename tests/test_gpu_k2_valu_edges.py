"""GPU: the edges of K2's leaner per-element arithmetic (tile_pass1 / tile_pass2, shared by the
stream, per-tile and small kernels), bit for bit against oracle.uq_oracle_c.quantize_batch: q,
the codes implied by the oracle's counts and signs (nibble = low nibble of the int8 code), kmax,
and est against the client-ordered mean of the oracle's q.

What changed and so what is planted (each plant is first checked on the oracle's own output, so a
case cannot quietly stop being the case it names):
  * pass 1 folds sign(v) into one product fm * v.  x = -0.0 and a negative subnormal beside
    large coordinates (the quotient underflows to -0) must stay "not negative": q = +0.0, code 0;
    negative coordinates with floor 0 and r = 0 must stay q = -0.0, code -1 (nibble 15).
  * pass 2 keeps the count k as an integer and re-derives the float count only for a group of
    four with a k >= 256: one client's largest k is exactly 255 (the table's last entry) and
    another's exactly 256 (the arithmetic path), each from one outlier inside a group, at a high
    rate; likewise 7 and 8, the last count a 4-bit code holds and the first it does not.
  * an all-zero client, a client holding +inf and one holding NaN.

Shapes: the stream form's three tiles at n = 256, d = 12288 (tile 0 irregular, then regular
tiles at R = 1), pipelines "codes4" (R = 1 and 2, where codes4_fits), "codes" and "q" (R = 1 and
6.5); a partial last tile at d = 8192 + 20; the per-tile form at n = 1, d = 40004; the small
kernel at d = 2048 and d = 4097.

A floor difference of 2 between neighbouring prefix sums (r must stay 0) needs a prefix sum of
at least 2^24, hence a vector of more than 2^24 coordinates (each adds less than 1): an oracle
pass of seconds and hundreds of megabytes per case.  tests/test_gpu_large.py runs those sizes
(2^27 and more coordinates, m > 2^24) against the same oracle."""
import functools

import numpy as np
import pytest
import torch

from oracle import uq_oracle as O
from oracle import uq_oracle_c as C
from tests import golden_data as G
from tests import plan_hook as H
from tests import test_gpu_unbiased_forms as F
from tests.test_gpu_unbiased_forms import api  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 256
ROW_NEG0, ROW_SUB, ROW_K_LO, ROW_K_HI, ROW_ZERO, ROW_INF, ROW_NAN = 3, 17, 40, 41, 100, 254, 255
POS = (5, 4096 + 1001, 8192 + 2222)        # one planted coordinate per tile of d = 12288


def counts(x, m, X, l1):
    """The oracle's k = fl + r and sign(v) < 0 per coordinate (oracle.uq_oracle.type_codes without
    the int8 clamp)."""
    v, fl, fr = O.fractional_parts(x, m, f32(l1))
    c = O.prefix_c(fr)
    with np.errstate(all="ignore"):
        diff = np.floor((c[1:] - f32(X)).astype(f32)) - np.floor((c[:-1] - f32(X)).astype(f32))
        k = (fl + (diff == 1).astype(f32)).astype(f32)
    return k, v < 0


def plant_count(x, m, X, pos, target):
    """Set x[pos] (negative) so that its count is exactly `target`, the row's largest, with every
    other count below target - 1."""
    x = x.copy()
    x[pos] = 0
    l0 = float(C.l1_torch_order(x, 1))
    for f in np.arange(target - 0.95, target + 1.0, 0.05):
        x[pos] = f32(-f * l0 / (m - f))             # m * a / (l0 + a) = f
        k, neg = counts(x, m, X, C.l1_torch_order(x, 1))
        rest = np.delete(k, pos)
        if k[pos] == target and neg[pos] and rest.max() < target - 1:
            return x
    raise AssertionError(("no magnitude gives the count", target))


@functools.lru_cache(maxsize=8)
def batch(d, R, k_lo, nonfinite):
    """(x, X, m, q, l1, codes, kmax, est), read-only.  Rows ROW_K_LO / ROW_K_HI: largest count
    exactly k_lo / k_lo + 1 at POS[1] (or the last coordinate's tile when d is smaller)."""
    C.build()
    m = O.rate_to_m(R, d)
    rng = np.random.default_rng(d * 7 + int(R * 2))
    x = rng.standard_normal((N, d)).astype(f32)
    X = rng.random(N).astype(f32)
    pos = [p for p in POS if p < d]
    for p in pos:
        x[ROW_NEG0, p] = f32(-0.0)
        x[ROW_SUB, p] = f32(-1e-45)
    x[ROW_ZERO] = 0
    x[ROW_K_LO] = plant_count(x[ROW_K_LO], m, X[ROW_K_LO], pos[-1] if len(pos) < 3 else POS[1], k_lo)
    x[ROW_K_HI] = plant_count(x[ROW_K_HI], m, X[ROW_K_HI], pos[-1] if len(pos) < 3 else POS[1], k_lo + 1)
    if nonfinite:
        x[ROW_INF, POS[0]] = f32(np.inf)
        x[ROW_NAN, d - 3] = f32(np.nan)
    q, l1 = C.quantize_batch(x, m, X, 1)
    codes = np.zeros((N, d), np.int8)
    kmax = np.empty(N, np.int32)
    for j in range(N):
        k, neg = counts(x[j], m, X[j], l1[j])
        ok = bool(np.isfinite(l1[j])) and bool((k <= 127).all())
        kmax[j] = int(k.max()) if ok else 128
        if ok:
            codes[j] = np.where(neg, -k.astype(np.int32) - 1, k.astype(np.int32)).astype(np.int8)
    # the plants are what they are said to be, on the oracle's side
    zero = np.zeros(1, f32).view(np.uint32)[0]
    for p in pos:
        for row in (ROW_NEG0, ROW_SUB):
            assert q[row, p].view(np.uint32) == zero and codes[row, p] == 0, (row, p, q[row, p])
    assert (l1[ROW_SUB] > 1.0) and np.all(q[ROW_ZERO].view(np.uint32) == zero) and kmax[ROW_ZERO] == 0
    negzero = (q.view(np.uint32) == np.uint32(0x80000000))
    if R == 1:
        assert negzero[:ROW_INF].any(axis=1).sum() >= N - 3        # floor 0, r = 0, v < 0: in nearly every row
        assert np.all(codes[:ROW_INF][negzero[:ROW_INF]] == -1)
    if k_lo + 1 <= 127:
        assert (kmax[ROW_K_LO], kmax[ROW_K_HI]) == (k_lo, k_lo + 1)
    else:
        assert counts(x[ROW_K_LO], m, X[ROW_K_LO], l1[ROW_K_LO])[0].max() == k_lo
        assert counts(x[ROW_K_HI], m, X[ROW_K_HI], l1[ROW_K_HI])[0].max() == k_lo + 1
    if nonfinite:
        assert np.isinf(l1[ROW_INF]) and np.isnan(l1[ROW_NAN]) and np.isnan(q[ROW_NAN]).all()
    est = C.client_mean(q, f32(N))
    for a in (x, X, q, l1, codes, kmax, est):
        a.setflags(write=False)
    return x, X, m, q, l1, codes, kmax, est


def run_pipeline(d, R, k_lo, nonfinite, pl, form=None):
    import uqdme
    x, X, m, q_ref, l1, codes, kmax, est_ref = batch(d, R, k_lo, nonfinite)
    p = uqdme.DMEPipeline(N, d, R, torch_threads=1, pipeline=pl)
    assert p.m == m
    est = p.step(torch.tensor(x).cuda(), torch.tensor(X).cuda())
    torch.cuda.synchronize()
    if form is not None:
        assert H.FORM_NAMES[H.last_plan(p.lib)["form"]] == form
    qn = p.q.cpu().numpy()
    bad = [j for j in range(N) if G.n_mismatch(qn[j], q_ref[j])]
    print(d, R, pl, "rows whose q differs:", bad[:16], "est mismatches:", G.n_mismatch(est.cpu().numpy(), est_ref))
    assert not bad, (d, R, pl, bad[:16])
    assert G.bits_equal(p.l1.cpu().numpy(), l1)
    assert G.bits_equal(est.cpu().numpy(), est_ref), (d, R, pl, "est")
    if pl == "q":
        return
    assert np.array_equal(p.kmax.cpu().numpy(), kmax), (d, R, pl, "kmax")
    if pl == "codes4":
        fits = kmax <= 7
        assert fits[ROW_K_LO] and not fits[ROW_K_HI]
        got = F.unpack_nibbles(p.nib.cpu().numpy())
        assert np.array_equal(got[fits], codes[fits]), (d, R, "nibbles")
        ok = kmax <= 127                                # past 7 too: the int8 code's low nibble
        assert np.array_equal(got.view(np.uint8)[ok] & 0xF, codes.view(np.uint8)[ok] & 0xF), (d, R, "low nibbles")
    else:
        fits = kmax <= 127
        assert np.array_equal(p.codes.cpu().numpy()[fits], codes[fits]), (d, R, pl, "codes")


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("nonfinite", [False, True])
def test_stream_nibbles_three_tiles(gpu_ready, R, nonfinite):
    """codes4: largest counts 7 and 8 in neighbouring clients, signed zeros, the non-finite clients."""
    from uqdme_amd.pipeline import codes4_fits
    assert codes4_fits(N, 12288, R)
    run_pipeline(12288, R, 7, nonfinite, "codes4", form="stream-nibbles")


@pytest.mark.parametrize("R,k_lo", [(1, 7), (6.5, 255)])
@pytest.mark.parametrize("nonfinite", [False, True])
@pytest.mark.parametrize("pl", ["codes", "q"])
def test_three_tiles_int8_and_q(gpu_ready, R, k_lo, nonfinite, pl):
    """The int8 and q pipelines on the same batches, and at R = 6.5 with largest counts 255 and 256."""
    run_pipeline(12288, R, k_lo, nonfinite, pl)


@pytest.mark.parametrize("R,k_lo", [(1, 7), (6.5, 255)])
@pytest.mark.parametrize("pl", ["codes", "q"])
def test_partial_last_tile(gpu_ready, R, k_lo, pl):
    run_pipeline(8192 + 20, R, k_lo, False, pl)


def planted_row(d, R, k):
    rng = np.random.default_rng(d + int(R * 2) + k)
    x = rng.standard_normal(d).astype(f32)
    X = rng.random(1).astype(f32)
    x[1], x[d - 2] = f32(-0.0), f32(-1e-45)
    return plant_count(x, O.rate_to_m(R, d), X[0], d // 2 + 1, k)[None, :], X


@pytest.mark.parametrize("d,form", [(40004, "phased"), (2048, "small"), (4097, "small")])
@pytest.mark.parametrize("R,k", [(1, 7), (1, 8), (6.5, 255), (6.5, 256)])
def test_one_client_forms(api, d, form, R, k):
    """The per-tile kernels (n = 1, d = 40004) and quantize_small_kernel (d = 2048, 4097): q, codes
    and kmax of one planted client, and the mean from its codes."""
    x, X = planted_row(d, R, k)
    ref = F.make_ref(x, X, R, 1, "computed")
    zero = np.zeros(1, f32).view(np.uint32)[0]
    assert ref.q[0, 1].view(np.uint32) == zero and ref.q[0, d - 2].view(np.uint32) == zero
    assert counts(x[0], ref.m, X[0], ref.l1[0])[0].max() == k
    xd, Xd = F.dev(x), F.dev(X)
    for kind in ("Q", "QC", "C"):
        r = F.run(api, ref, xd, Xd, kind)
        F.check_plan(r.plan, form, kind)
        F.check_outputs(api, ref, r)
