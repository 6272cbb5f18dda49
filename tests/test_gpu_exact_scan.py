"""The fp64 scan (AS:635: torch cumsum = SEQUENTIAL fp64 adds, each prefix rounded to f32)
is reproduced exactly by every K2 form.  The inputs are chosen so that a plain parallel
fp64 tree scan (round-1 K2, modelled in tests/scan_models.py) would NOT match: coordinate
mixes with many tiny fractional parts, and X placed on the first f32 prefix where the tree
scan differs, so that the difference reaches the outputs.

The small-batch forms leave the fold's exact tile starts P_t in the workspace: they are compared
bit for bit with the sequential cumsum at every tile (on these inputs the tree scan's tile
prefixes differ at nearly every tile, tests/test_scan_model.py), and the maps, records and
counters beside them tell which branch of exact_fold_kernel each tile took."""
import numpy as np
import pytest
import torch

from oracle import uq_oracle as O
from oracle import uq_oracle_c as C
from tests import golden_data as G
from tests import plan_hook as H
from tests import scan_models as S

pytestmark = pytest.mark.gpu
f32 = np.float32
D = 1 << 20
# seeds of S.tiny_mix(seed, 2^20, 0.5) on which the tree scan's f32 prefixes differ at R=1
# (tools/find_scan_cases.py)
SEEDS = (6, 8, 9, 23, 65)


@pytest.fixture(scope="module")
def uq(gpu_ready):
    import uqdme
    return uqdme


@pytest.fixture(scope="module")
def cases():
    m = O.rate_to_m(1, D)
    xs, Xs = [], []
    for s in SEEDS:
        x = S.tiny_mix(s, D)
        X, i = S.exposing_X(x, m)
        assert X is not None, f"seed {s}: the tree scan no longer differs (model changed?)"
        xs.append(x)
        Xs.append(X)
    x = np.stack(xs)
    X = np.array(Xs, f32)
    ref, _ = C.quantize_batch(x, m, X, 1)
    return x, X, m, ref


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=f32)).cuda()


def fold_checked(x, X, m, ref, form, l1=None, **want):
    """One call through the C API with its own workspace: the form, q, every exact tile start
    P_t against the sequential fp64 cumsum, and the fold branch of every tile.  Returns the
    readback and the per-client branch lists."""
    from uqdme_amd import _lib as L
    lib = L.load()
    n = x.shape[0]
    q, ws, p = H.call_q(lib, L, dev(x), dev(X), m, l1d=None if l1 is None else dev(l1))
    assert p["form"] == form and p["chunks"] == 1, p
    for k, v in want.items():
        assert p[k] == v, (k, p)
    assert G.n_mismatch(q.cpu().numpy(), ref) == 0
    rb = H.fold_readback(ws, p, n)
    for j in range(n):
        exp = H.tile_starts(x[j], m, C.l1_torch_order(x[j], 1) if l1 is None else l1[j])
        bad = np.nonzero(rb[0][j] != exp)[0]
        assert bad.size == 0, ("P_t differs from the sequential cumsum", j, bad[:8], bad.size)
    return rb, p, [H.fold_branches(*rb, p, j) for j in range(n)]


def test_stream_form_exact(uq, cases):
    """n >= 256: one workgroup per client carries the exact prefix."""
    x, X, m, ref = cases
    n = x.shape[0]
    filler = torch.randn(256 - n, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    big = torch.cat([dev(x), filler])
    Xb = np.concatenate([X, np.random.default_rng(2).random(256 - n).astype(f32)])
    got = uq.quantize_dequantize(big, m=m, X=Xb, torch_threads=1)[:n].cpu().numpy()
    assert G.n_mismatch(got, ref) == 0, [G.n_mismatch(got[j], ref[j]) for j in range(n)]


def test_segmented_form_exact(uq, cases):
    """5 clients x 256 tiles: approximate sums -> maps -> exact fold -> segmented outputs."""
    x, X, m, ref = cases
    got = uq.quantize_dequantize(dev(x), m=m, X=X, torch_threads=1).cpu().numpy()
    assert G.n_mismatch(got, ref) == 0, [G.n_mismatch(got[j], ref[j]) for j in range(x.shape[0])]
    tc, q = uq.quantize_encode(dev(x), m=m, X=X, torch_threads=1, return_q=True)
    assert G.bits_equal(q.cpu().numpy(), ref)
    assert G.bits_equal(uq.decode(tc).cpu().numpy(), ref)


def test_segmented_form_exact_tile_starts_and_fold_branches(uq, cases):
    """The same five clients: every P_t, and the fold's branches the seeds reach -- irregular
    tiles resolved from the data (tile 0: too many events for a record) and walked from their
    records in LDS, beside the regular runs."""
    x, X, m, ref = cases
    rb, p, br = fold_checked(x, X, m, ref, H.SEGMENTS, V=True, prefixed=True)
    assert p["nseg"] > 1
    for j, b in enumerate(br):
        assert b["regular"] and len(b["regular"]) + len(b["from_data"]) + len(b["rec_lds"]) + len(b["rec_copied"]) \
            - len(b["other_binade"]) == p["tiles"], (j, b)
    assert any(b["from_data"] for b in br), "no tile resolved from the data"
    assert any(b["rec_lds"] for b in br), "no record walked from LDS"
    print("fold branches per client (from_data, rec_lds, rec_copied, other_binade, budget_exhausted):",
          [(len(b["from_data"]), len(b["rec_lds"]), len(b["rec_copied"]), len(b["other_binade"]), b["budget_exhausted"])
           for b in br])


def test_per_tile_form_exact_single_client(uq, cases):
    """n = 1 (the drop-in's batch): one workgroup per tile."""
    x, X, m, ref = cases
    for j in range(x.shape[0]):
        got = uq.quantize_dequantize(dev(x[j:j + 1]), m=m, X=X[j:j + 1], torch_threads=1).cpu().numpy()[0]
        assert G.n_mismatch(got, ref[j]) == 0, j


def test_unaligned_rows_exact(uq):
    """d % 4 != 0 with several clients: per-tile kernels on scalar loads."""
    d = D + 3
    m = O.rate_to_m(1, d)
    xs, Xs = [], []
    for s in SEEDS[:3]:
        x = S.tiny_mix(s, d)
        X, _ = S.exposing_X(x, m)
        xs.append(x)
        Xs.append(X if X is not None else f32(0.5))
    x = np.stack(xs)
    X = np.array(Xs, f32)
    ref, _ = C.quantize_batch(x, m, X, 1)
    got = uq.quantize_dequantize(dev(x), m=m, X=X, torch_threads=1).cpu().numpy()
    assert G.n_mismatch(got, ref) == 0
    # phased form on scalar lanes, no prefix launch (3 clients): every exact tile start
    rb, p, br = fold_checked(x, X, m, ref, H.PHASED, V=False, prefixed=False)
    assert any(b["from_data"] for b in br) and any(b["rec_lds"] for b in br), br


def test_clients_past_the_record_clients_fold_from_the_data(uq):
    """(257, 2^17 + 1): the same vector at client 0 and client 256.  Client 0 records its
    irregular tiles; client 256 (>= kRecClients) has no records and resolves them from the data.
    Both give the exact P_t and q."""
    n, d = 257, (1 << 17) + 1
    m = O.rate_to_m(1, d)
    base = np.stack([S.tiny_mix(s, d) for s in SEEDS[:4]])
    Xb = np.array([0.0, 0.25, 0.5, 0.999], f32)
    refb, _ = C.quantize_batch(base, m, Xb, 1)
    sel = np.arange(n) % 4
    rb, p, br = fold_checked(base[sel], Xb[sel], m, refb[sel], H.PHASED, V=False, prefixed=True)
    assert p["rec_clients"] == 256 and rb[3].size == 256
    assert br[0]["rec_lds"], br[0]
    assert not br[256]["rec_lds"] and not br[256]["rec_copied"]
    assert sorted(br[256]["from_data"]) == sorted(br[0]["from_data"] + br[0]["rec_lds"] + br[0]["rec_copied"])
    assert np.array_equal(rb[0][0], rb[0][256])


def test_hover_vector_exhausts_the_records_and_the_fold_prefetch(uq):
    """scan_models.hover_vector at d = 2^22 (tools/find_fold_cases.py; fractions set exactly
    through a supplied l1 = m = 2^10): 33 irregular tiles with at most 46 events each, so the
    client's record budget (32) runs out and one tile is resolved from the data although it has
    few events, and the records' 750 events overflow the fold's LDS prefetch (256), so records are
    copied one by one.  q and every P_t stay exact."""
    d = 1 << 22
    x, l1, m = S.hover_vector(d)
    x, X, l1 = x[None], np.array([0.5], f32), np.array([l1], f32)
    ref = C.quantize_with_l1(x[0], m, X[0], l1[0])[None]
    rb, p, br = fold_checked(x, X, m, ref, H.SEGMENTS, l1=l1, V=True, prefixed=False, l1_given=True, tiles=1024)
    b = br[0]
    assert b["budget_exhausted"] and int(rb[3][0]) == 33, rb[3]
    assert len(b["from_data"]) == 1 and not b["other_binade"], b
    assert b["rec_lds"] and b["rec_copied"] and len(b["rec_lds"]) + len(b["rec_copied"]) == 32, b
    assert len(b["regular"]) == 1024 - 33


def test_tiny_mix_whose_records_overflow_the_fold_prefetch(uq):
    """tiny_mix(29, 2^22, 0.99, 1e-5) at R = 1 (found by tools/find_fold_cases.py among 4000
    vectors): 9 recorded irregular tiles with 274 events by the census model, more than the 256 the
    fold prefetches into LDS, so at least one record is copied when its tile comes up."""
    d = 1 << 22
    m = O.rate_to_m(1, d)
    x = S.tiny_mix(29, d, 0.99, 1e-5)[None]
    X = np.array([0.37], f32)
    ref, _ = C.quantize_batch(x, m, X, 1)
    rb, p, br = fold_checked(x, X, m, ref, H.SEGMENTS, V=True, prefixed=False, tiles=1024)
    b = br[0]
    print("recorded tiles and events:", int(rb[3][0]), [rb[4](0, r) for r in range(1, int(rb[3][0]) + 1)])
    assert b["rec_lds"] and b["rec_copied"] and not b["budget_exhausted"], b


@pytest.mark.parametrize("mix,scale,R", [(0.9, 1e-3, 2), (0.3, 1e-6, 4), (0.99, 1e-5, 0.5)])
def test_tiny_mixes_all_forms(uq, mix, scale, R):
    """Other mixes and rates (more ties, other binades), each client in three forms."""
    d = 1 << 18
    m = O.rate_to_m(R, d)
    x = np.stack([S.tiny_mix(100 + j, d, mix, scale) for j in range(4)])
    X = np.random.default_rng(5).random(4).astype(f32)
    ref, _ = C.quantize_batch(x, m, X, 1)
    got = uq.quantize_dequantize(dev(x), m=m, X=X, torch_threads=1).cpu().numpy()
    assert G.n_mismatch(got, ref) == 0
    one = uq.quantize_dequantize(dev(x[1:2]), m=m, X=X[1:2], torch_threads=1).cpu().numpy()[0]
    assert G.n_mismatch(one, ref[1]) == 0
    big = torch.cat([dev(x), torch.randn(252, d, device="cuda")])
    Xb = np.concatenate([X, np.full(252, 0.5, f32)])
    st = uq.quantize_dequantize(big, m=m, X=Xb, torch_threads=1)[:4].cpu().numpy()
    assert G.n_mismatch(st, ref) == 0


def test_large_d_exact(uq):
    """d = 2^22 (config C4's size): binades up to 2^21, more fine fractions per tile."""
    d = 1 << 22
    m = O.rate_to_m(1, d)
    x = np.stack([S.tiny_mix(7, d, 0.5), np.random.default_rng(8).standard_normal(d).astype(f32)])
    X = np.array([0.25, 0.75], f32)
    ref, _ = C.quantize_batch(x, m, X, 1)
    got = uq.quantize_dequantize(dev(x), m=m, X=X, torch_threads=1).cpu().numpy()
    assert G.n_mismatch(got, ref) == 0
