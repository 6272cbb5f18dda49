"""GPU: the stream kernels' tile loop (quantize_stream_kernel, one workgroup per client) at the
smallest batch that takes it, n = 256, R = 1, torch_threads = 1: q against the CPU oracle
(AS:609-641) and est against the oracle's client-ordered mean of that q (ND:137-138), bit for
bit, in every pipeline -- "q", "codes", "codes4" and "encode" agree in every bit of q and est,
with equal kmax.

Shapes by what the loop does: d = 4096 is one tile (prologue and epilogue only), 8192 one
iteration with a store phase, 12288 two, 69632 seventeen.  d = 8188 (rows 16-byte aligned, d no
multiple of 16) is the stream form with bytewise code stores and a ragged last tile; d = 8190
(rows not 16-byte aligned) leaves the stream form for the per-tile kernels, which share the
tile passes (both with pipelines "codes" and "q").  At d = 69632 the batch mixes N(0,1) clients
with tiny_mix clients, and the census (scan_models.fold_census, on the CPU) shows that it holds
every path by which a tile rejoins the common one: irregular tiles after tile 0 followed by
regular ones, regular tiles without ties, with 1..32 ties (resolved from the parity transfers)
and with more than 32 (walked by one lane)."""
import numpy as np
import pytest
import torch

from oracle import uq_oracle as O
from oracle import uq_oracle_c as C
from tests import golden_data as G
from tests import scan_models as S

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 256
D_MIX = 69632
_REF = {}


def _clients(d):
    if d != D_MIX:
        return np.random.default_rng(d).standard_normal((N, d)).astype(f32)
    rows = []
    for j in range(N):                                  # rows 0, 1, 2: seed 3 of each kind (the census below)
        seed, kind = 3 + j // 3, j % 3
        rows.append(np.random.default_rng(seed).standard_normal(d).astype(f32) if kind == 0 else
                    S.tiny_mix(seed, d) if kind == 1 else S.tiny_mix(seed, d, 0.9, 1e-3))
    return np.stack(rows)


def reference(d):
    """(x, X, m, q, est) of the batch at dimension d: computed once, shared, never written."""
    if d not in _REF:
        C.build()
        m = O.rate_to_m(1, d)
        x = _clients(d)
        X = np.random.default_rng(1000 + d).random(N).astype(f32)
        q, _ = C.quantize_batch(x, m, X, 1)
        est = C.client_mean(q, f32(N))
        for a in (x, X, q, est):
            a.setflags(write=False)
        _REF[d] = (x, X, m, q, est)
    return _REF[d]


def census(x, m):
    _, _, fr = O.fractional_parts(x, m, C.l1_torch_order(x, 1))
    return S.fold_census(fr)


def check_mix_census():
    """The d = 69632 batch reaches every rejoin of the tile loop (CPU only)."""
    x, _, m, _, _ = reference(D_MIX)
    cn, ct, cs = (census(x[j], m) for j in range(3))
    tiles = D_MIX // 4096
    irr = np.nonzero(cn["irregular"])[0]
    # the stream kernel's own test, from the exact starts: P >= 32 and the tile ends below the binade's top
    P = np.append(cn["P"], np.cumsum(O.fractional_parts(x[0], m, C.l1_torch_order(x[0], 1))[2].astype(np.float64))[-1])
    top = np.ldexp(1.0, np.frexp(np.maximum(P[:-1], 1.0))[1])
    stream_irr = np.nonzero(~((P[:-1] >= 32.0) & (P[1:] + 1.0 < top)))[0]
    for ii in (irr, stream_irr):
        late = ii[ii > 0]
        assert late.size >= 2, ii                                       # irregular tiles after tile 0 ...
        assert all(t + 1 < tiles and t + 1 not in ii for t in late[-2:]), ii     # ... followed by regular ones
    reg = ~cn["irregular"]
    assert int((reg & (cn["ties"] == 0)).sum()) >= 8                   # regular, tie-free
    few = ~cs["irregular"] & (cs["ties"] >= 1) & (cs["ties"] <= S.FAST_TIES)
    many = ~ct["irregular"] & (ct["ties"] > S.FAST_TIES)
    assert int(few.sum()) >= 4 and int(many.sum()) >= 8, (cs["ties"], ct["ties"])
    return dict(irregular=irr.tolist(), stream_irregular=stream_irr.tolist(), tie_free=int((reg & (cn["ties"] == 0)).sum()),
                few=cs["ties"][few].tolist(), many=ct["ties"][many].tolist())


def run_pipelines(d, pipelines):
    import uqdme
    x, X, m, q_ref, est_ref = reference(d)
    xd, Xd = torch.tensor(x).cuda(), torch.tensor(X).cuda()      # copies: the shared reference stays read-only
    kmax = None
    for pl in pipelines:
        p = uqdme.DMEPipeline(N, d, 1, torch_threads=1, pipeline=pl)
        assert p.m == m
        est = p.step(xd, Xd)
        torch.cuda.synchronize()
        p.check_status()
        if pl == "encode":
            q = uqdme.decode(uqdme.TypeCodes(codes=p.codes, l1=p.l1, m=p.m, overflow=p.kmax))
        else:
            q = p.q
        qn = q.cpu().numpy()
        assert G.bits_equal(qn, q_ref), (d, pl, "q", G.n_mismatch(qn, q_ref))
        assert G.bits_equal(est.cpu().numpy(), est_ref), (d, pl, "est")
        if pl != "q":                                   # "q" writes no codes, hence no kmax
            k = p.kmax.cpu().numpy()
            assert kmax is None or np.array_equal(k, kmax), (d, pl, "kmax")
            kmax = k
        del p


@pytest.mark.parametrize("d", [4096, 8192, 12288])
def test_stream_loop_few_tiles(gpu_ready, d):
    run_pipelines(d, ("q", "codes", "codes4", "encode"))


def test_stream_loop_rejoin_paths(gpu_ready):
    print("census:", check_mix_census())                # before anything runs on the GPU
    run_pipelines(D_MIX, ("q", "codes", "codes4", "encode"))


@pytest.mark.parametrize("d", [8190, 8188])
def test_stream_loop_ragged_row(gpu_ready, d):
    run_pipelines(d, ("codes", "q"))
