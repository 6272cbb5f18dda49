"""CPU: the NumPy model of the mean from type codes (tests/codes_mean_model.py) against the C oracle's
client_mean on the codes and q of one real oracle batch, in both forms, from bytes and from nibbles; and the
model's own parts (packer, sign codes, the generator's promises)."""
import numpy as np
import pytest

from oracle import uq_oracle as O
from oracle import uq_oracle_c as C
from tests import biased_codes_model as B
from tests import codes_mean_model as M
from tests import golden_data as G

f32 = np.float32
N, D = 24, 3000


@pytest.fixture(scope="module")
def x():
    C.build()
    rng = np.random.default_rng(404)
    rows = [rng.standard_normal(D) if j % 3 else rng.lognormal(0, 2, D) * rng.choice([-1, 1], D) for j in range(N)]
    return np.stack(rows).astype(f32), rng.random(N).astype(f32)


def as_bytes(codes):
    return np.asarray(codes, np.int8).view(np.uint8)


def check_both_widths(codes, l1, kmax, m, form, q):
    """The model's mean from bytes and (unbiased form) from nibbles == the oracle's client mean of q, from zero
    and continuing from an est."""
    n_div = f32(N + 3)
    want = C.client_mean(q, n_div)
    got = M.mean(codes, l1, kmax, m, n_div, form, q=q)
    assert G.bits_equal(got, want), G.n_mismatch(got, want)
    h = N // 2
    first = M.mean(codes[:h], l1[:h], kmax[:h], m, n_div, form, q=q[:h])
    got = M.mean(codes[h:], l1[h:], kmax[h:], m, n_div, form, q=q[h:], est=first)
    assert G.bits_equal(got, want)
    assert G.bits_equal(got, C.client_mean_acc(q[h:], n_div, C.client_mean(q[:h], n_div)))
    if form == M.UNBIASED:
        nib = codes & np.uint8(0xF)                                  # the byte code's low nibble
        assert (kmax <= M.NIB_MAX).any() and (kmax > M.NIB_MAX).any()
        got = M.mean(nib, l1, kmax, m, n_div, form, q=q, nibbles=True)
        assert G.bits_equal(got, want), G.n_mismatch(got, want)


def test_unbiased_form_against_the_oracle(x):
    xs, X = x
    m = O.rate_to_m(2, D)
    q, l1 = C.quantize_batch(xs, m, X)
    codes = np.empty((N, D), np.uint8)
    kmax = np.empty(N, np.int32)
    for j in range(N):
        c, _, ovf = O.type_codes(xs[j], m, X[j], l1=l1[j])
        k, _ = B.counts(c)
        kmax[j] = 128 if ovf else int(k.max())
        codes[j] = as_bytes(c)
        if not ovf:
            assert G.bits_equal(B.decode(c, l1[j], m, B.UNBIASED), q[j])
    # the batch holds every kind: nibble-sized counts, counts above 63, and clients above the byte range
    assert (kmax <= 7).any() and ((kmax > 63) & (kmax <= 127)).any() and (kmax == 128).any()
    check_both_widths(codes, l1, kmax, m, M.UNBIASED, q)
    # a client above the byte range adds RN(q / n_div), whatever its codes hold
    kmax2 = kmax.copy()
    kmax2[[0, N - 1]] = 128
    codes2 = codes.copy()
    codes2[[0, N - 1]] = 0x55
    got = M.mean(codes2, l1, kmax2, m, f32(N), M.UNBIASED, q=q)
    assert G.bits_equal(got, C.client_mean(q, f32(N)))


def test_biased_form_against_the_oracle(x):
    xs, _ = x
    m = O.rate_to_m(3, D)
    q = np.empty((N, D), f32)
    l1 = np.empty(N, f32)
    codes = np.zeros((N, D), np.uint8)
    kmax = np.empty(N, np.int32)
    for j in range(N):
        q[j], l1[j], *_ = C.biased_quantize(xs[j], m, 1, 0)
        c = B.recover_codes(xs[j], q[j], l1[j], m)
        k, _ = B.counts(c)
        kmax[j] = min(int(k.max()), 128)
        if B.fits(c):
            codes[j] = as_bytes(c)
            assert G.bits_equal(B.decode(c, l1[j], m, B.BIASED), q[j])
    assert (kmax <= 127).any()
    check_both_widths(codes, l1, kmax, m, M.BIASED, q)


def test_sign_codes_negate_and_zero_keeps_its_sign():
    l1, m, nd = f32(3.7), 11, f32(5)
    t = M.table(l1, 127, m, nd, M.UNBIASED)
    assert t[0] == 0 and t[3] == f32(f32(f32(l1 * f32(3)) / f32(m)) / nd)
    tb = M.table(l1, 127, m, nd, M.BIASED)
    assert tb[3] == f32(f32(l1 * f32(f32(3) / f32(m))) / nd)
    a = M.client_adds(np.array([[3, 252, 0, 255, 127, 128]], np.uint8), [l1], [127], m, nd)[0]
    assert G.bits_equal(a, np.array([t[3], -t[3], 0.0, -0.0, t[127], -t[127]], f32))
    a = M.client_adds(np.array([[3, 12, 0, 15, 7, 8]], np.uint8), [l1], [7], m, nd, q=np.zeros((1, 6), f32), nibbles=True)[0]
    assert G.bits_equal(a, np.array([t[3], -t[3], 0.0, -0.0, t[7], -t[7]], f32))
    with pytest.raises(ValueError, match="above its kmax"):
        M.client_adds(np.array([[4]], np.uint8), [l1], [3], m, nd)
    # -0.0 survives only onto -0.0: the sum starts from +0.0
    assert G.bits_equal(M.fold(np.array([[-0.0, -0.0]], f32), est=np.array([-0.0, 0.0], f32)), np.array([-0.0, 0.0], f32))
    assert G.bits_equal(M.fold(np.array([[-0.0]], f32)), np.array([0.0], f32))


def test_packer_and_generator():
    assert M.pack_nibbles(np.array([[1, 2, 15, 0]], np.uint8)).tolist() == [[0x21, 0x0F]]
    rng = np.random.default_rng(1)
    for nib, kset in ((True, (0, 1, 7)), (False, (0, 1, 7, 63, 64, 65, 127))):
        codes, l1, kmax = M.synthetic(rng, 200, 512, kset, nibbles=nib)
        top = 15 if nib else 255
        c = codes.astype(np.int64)
        k = np.where(c > top // 2, top - c, c)
        assert np.array_equal(k.max(axis=1), kmax) and set(kmax.tolist()) == set(kset)
        assert ((codes == top).sum() > 0) and np.log2(l1.max() / l1.min()) > 8 and np.isfinite(l1).all()
        q, oc = M.overflowed(rng, 3, 512, nibbles=nib)
        assert np.isfinite(q).all() and (np.signbit(q) & (q == 0)).any() and int(oc.max()) <= top
