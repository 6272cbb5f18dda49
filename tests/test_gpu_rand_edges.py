"""GPU: the edges of Scalar_quantize (AS:755-790) and DRIVE_quantize_Hadamard (AS:707-752) that
tests/test_gpu_rand_schemes.py does not reach, bit for bit against the reference's own outputs
(tests/golden/rand_schemes_edges.*) and the NumPy restatement (tests/rand_schemes_model.py, pinned
to that fixture and to torch.rand by tests/test_rand_edges_oracle.py):

  - torch.norm's tail on DRIVE's ragged last chunks (KR4), NaN / Inf / subnormal / overflowing
    inputs, 3 to 32 bits;
  - Scalar with several min / max slices and several clients at once (KR1's block map, KR2's
    fold of the partials and of the NaN flag), up to the 64-slice cap;
  - generator start states at every edge of the walk (a 64-word group's edge, the 48-word last
    group, one word or none left in the block), for both walkers;
  - strided inputs, and calls of different shapes back to back on the shared workspace."""
import numpy as np
import pytest
import torch

from tests import golden_data as G
from tests import rand_schemes_model as M
from tests import test_gpu_rand_schemes as T
from tests.test_rand_edges_oracle import (DRIVE_SWEEP_D, PRE_SWEEP, RAGGED_D, RAGGED_STATES, SCALAR_SWEEP_D, ragged_rows,
                                          ragged_vseeds)

pytestmark = pytest.mark.gpu

MINMAX_PARTS, MINMAX_SLICE = 64, 4096                 # kMinMaxParts, kMinMaxSlice (uq_rand_kernels.h)


@pytest.fixture(scope="module")
def fx(gpu_ready):
    return M.load_fixture("rand_schemes_edges")


def test_edge_dropins_match_the_reference(fx):
    """Every case of the edge fixture through the drop-ins: the reference's output bits, its
    generator state afterwards, the input untouched."""
    meta, z = fx
    assert len(meta["cases"]) == 34
    for c in meta["cases"]:
        x = M.gen_input(c)
        T.set_global(c)
        before = T.global_sha()
        xt = torch.from_numpy(x.copy())
        out = T.dropin(c)(xt, c["bits"])
        T.check_fixture(c, z, f"out{c['idx']}", out)
        assert T.global_sha() == c["state_sha"], c
        assert G.bits_equal(xt.numpy(), x)                                  # the input is only read
        o = out.cpu().numpy()
        if c["scheme"] == "scalar" and c["d"] == 1:                         # NaN: one word taken
            assert np.isnan(o).all() and T.global_sha() != before, c
        if c["kind"] == "nan_at" and c["scheme"] == "drive":                # the NaN's chunk alone
            bad = np.isnan(o)
            assert bad[2048:4096].all() and not bad[:2048].any() and not bad[4096:].any()
            clean = z[f"out{c['clean']}"]
            assert np.array_equal(o[~bad].view(np.uint32), clean[~bad].view(np.uint32))


@pytest.mark.parametrize("d", RAGGED_D)
def test_drive_ragged_last_chunk_batched(fx, d):
    """n = 3 from three generator states at last-chunk lengths 3, 5, 6, 7, 11 and 13, alone and
    after one and two whole chunks: S per chunk, outputs and end states against the model.  Row
    0 is the fixture's input at d; every row's norm tells torch's tail order (4 by mul + add,
    then fma) from mul + add throughout (tests/test_rand_edges_oracle.py shows that on the CPU)."""
    import uqdme
    x = ragged_rows(d, ragged_vseeds(fx[0])[d])
    sts, words = T.states_of(RAGGED_STATES)
    q, new, S = uqdme.drive_quantize(torch.from_numpy(x), px_states=words, return_scale=True)
    assert S.shape == (3, (d + 2047) // 2048)
    T.check_drive_batch(x, sts, q, new, S)


def minmax_parts(d):
    return max(1, min(MINMAX_PARTS, -(-d // MINMAX_SLICE)))


@pytest.mark.parametrize("n,d", [(5, 4097), (5, 8195), (5, 65553), (3, 266241)])
def test_scalar_several_slices_and_clients(n, d):
    """2, 3, 17 and 64 min / max slices per client with several clients in one launch.  Row 0's
    minimum is its last element, row 1's maximum the first element of its last slice, row 2 is
    constant, row 3 holds one NaN as its last element (only the flag carries it across slices:
    fminf / fmaxf skip it), row 4 is plain."""
    import uqdme
    parts = minmax_parts(d)
    assert parts == {4097: 2, 8195: 3, 65553: 17, 266241: 64}[d]
    first_of_last = (parts - 1) * -(-d // parts)
    assert d - -(-d // parts) <= first_of_last < d
    x = T.scalar_rows(5, d, 600 + d % 1000)
    x[0, -1] = -50.0
    x[1, first_of_last] = 50.0
    x[2] = 0.375
    x[3, -1] = np.nan
    rows = [0, 1, 2, 3, 4] if n == 5 else [0, 1, 3]
    x = np.ascontiguousarray(x[rows])
    assert x[0].argmin() == d - 1 and x[1].argmax() == first_of_last
    sts, words = T.states_of([(41, 0), (42, 1), (43, 623), (44, 624), (45, 300)][:n])
    q, new, info = uqdme.scalar_quantize(torch.from_numpy(x), 2, px_states=words)
    T.check_scalar_batch(x, 2, sts, q, new, info)
    qn = q.cpu().numpy()
    assert list(info) == [1 if r == 2 else 0 for r in rows]
    for j, r in enumerate(rows):
        if r == 3:
            assert np.isnan(qn[j]).all()
        else:
            assert not np.isnan(qn[j]).any(), r
    assert qn[0].min() == np.float32(-50.0) == qn[0, -1]
    if n == 5:
        assert np.array_equal(new[2], words[2]) and G.bits_equal(qn[2], x[2])


def sweep_states():
    return T.states_of([(9, pre) for pre in PRE_SWEEP])


@pytest.mark.parametrize("d", SCALAR_SWEEP_D)
def test_scalar_start_state_sweep(d):
    """One launch of 17 clients that start after 0 .. 1249 draws of seed 9: every row's output and
    626 end-state words against the model.  d = 1 rows hold a NaN (any other d = 1 row is
    constant and takes no word): one word each."""
    import uqdme
    n = len(PRE_SWEEP)
    x = T.scalar_rows(n, d, 800 + d)
    if d == 1:
        x[:] = np.nan
    sts, words = sweep_states()
    q, new, info = uqdme.scalar_quantize(torch.from_numpy(x), 2, px_states=words)
    assert not info.any()                                                   # no constant row: d words each
    T.check_scalar_batch(x, 2, sts, q, new, info)
    if d == 1:
        assert np.isnan(q.cpu().numpy()).all()
        for j in range(n):
            assert np.array_equal(new[j], M.state_words(M.mt_draw(sts[j], 1)[1])), PRE_SWEEP[j]


@pytest.mark.parametrize("d", DRIVE_SWEEP_D)
def test_drive_start_state_sweep(d):
    import uqdme
    n = len(PRE_SWEEP)
    x = T.scalar_rows(n, d, 900 + d)
    sts, words = sweep_states()
    q, new, S = uqdme.drive_quantize(torch.from_numpy(x), px_states=words, return_scale=True)
    T.check_drive_batch(x, sts, q, new, S)


def test_strided_rows_give_their_contiguous_copys_bits():
    """x[:, ::2] and a column slice of a wider tensor, on the host and on the device, in both
    batch forms."""
    import uqdme
    n, d = 3, 2051
    wide = torch.from_numpy(T.scalar_rows(n, 2 * d + 9, 1200))
    _, words = T.states_of([(51, 0), (52, 623), (53, 300)])
    for make in (lambda w: w[:, ::2][:, :d], lambda w: w[:, 7:7 + d]):
        for w in (wide, wide.cuda()):
            view = make(w)
            assert not view.is_contiguous() and view.shape == (n, d)
            copy = view.contiguous()
            q0, s0, i0 = uqdme.scalar_quantize(copy, 2, px_states=words)
            q1, s1, i1 = uqdme.scalar_quantize(view, 2, px_states=words)
            assert torch.equal(q0.view(torch.int32), q1.view(torch.int32))
            assert np.array_equal(s0, s1) and np.array_equal(i0, i1)
            d0 = uqdme.drive_quantize(copy, px_states=words, return_scale=True)
            d1 = uqdme.drive_quantize(view, px_states=words, return_scale=True)
            for a, b in zip(d0, d1):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # and the bits are the model's
    x = wide[:, 7:7 + d].contiguous().numpy()
    sts, words = T.states_of([(51, 0), (52, 623), (53, 300)])
    T.check_drive_batch(x, sts, *uqdme.drive_quantize(wide.cuda()[:, 7:7 + d], px_states=words, return_scale=True))
    T.check_scalar_batch(x, 2, sts, *uqdme.scalar_quantize(wide[:, 7:7 + d], 2, px_states=words))


def test_calls_back_to_back_share_the_workspace():
    """A Scalar call, a DRIVE call and a Scalar call of another shape back to back on one stream
    (DRIVE's sign bits and the second Scalar call's partials overlap in the shared workspace, and
    DRIVE does not wait for the GPU): each gives the model's bits, and the same bits again in
    another order."""
    import uqdme
    xa = T.scalar_rows(3, 9000, 1300)
    xb = T.scalar_rows(2, 3073, 1310)
    xc = T.scalar_rows(40, 700, 1320, "lognormal")
    sa, wa = T.states_of([(61, 0), (62, 1), (63, 300)])
    sb, wb = T.states_of([(64, 623), (65, 64)])
    sc, wc = T.states_of([(100 + j, 37 * j) for j in range(40)])
    ta, tb, tc = (torch.from_numpy(v).cuda() for v in (xa, xb, xc))
    ra = uqdme.scalar_quantize(ta, 4, px_states=wa)
    rb = uqdme.drive_quantize(tb, px_states=wb, return_scale=True)
    rc = uqdme.scalar_quantize(tc, 2, px_states=wc)
    T.check_scalar_batch(xa, 4, sa, *ra)
    T.check_drive_batch(xb, sb, *rb)
    T.check_scalar_batch(xc, 2, sc, *rc)
    torch.cuda.synchronize()
    rc2 = uqdme.scalar_quantize(tc, 2, px_states=wc)
    rb2 = uqdme.drive_quantize(tb, px_states=wb, return_scale=True)
    ra2 = uqdme.scalar_quantize(ta, 4, px_states=wa)
    for one, two in ((ra, ra2), (rc, rc2)):
        assert torch.equal(one[0].view(torch.int32), two[0].view(torch.int32))
        assert np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])
    for a, b in zip(rb, rb2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
