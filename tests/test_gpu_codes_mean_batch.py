"""GPU: the means from codes -- K3n nibbles_mean_kernel (uq_nibbles_q_mean_ld_f32) and K3c codes_mean_kernel /
codes_mean_biased_kernel (uq_codes_mean_form_f32) -- bit for bit against the NumPy model of
tests/codes_mean_model.py, on synthetic codes that no quantizer produced: client counts on either side of every
group of 32 and of K3n's chunks of 1024 clients, clients above the code's range wherever a path changes, kmax up
to 127 in the byte tables.  One finite batch per test; every call takes a prefix of it with the same n_div."""
import numpy as np
import pytest
import torch

from tests import codes_mean_model as M
from tests import golden_data as G

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT_B = 0xA5                          # pad bytes of pitched code rows
NIB_N = (1, 15, 16, 17, 31, 32, 33, 48, 1023, 1024, 1025, 1039, 1040, 1041, 1055, 1056, 1057, 2048, 2049, 2081)
NIB_TOTAL = 2081
BYTE_N = (1, 31, 32, 33, 64, 65, 1057)
BYTE_TOTAL = 1057


@pytest.fixture(scope="module")
def api(gpu_ready):
    import uqdme
    from uqdme_amd import _lib
    return uqdme.load_library(), _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def pitched(rows, ld, fill):
    """rows [n, w] on the device as the first w columns of a [n, ld] array filled with `fill`."""
    rows = np.ascontiguousarray(rows)
    out = torch.full((rows.shape[0], ld), fill, dtype=torch.from_numpy(rows[:1]).dtype, device="cuda")
    out[:, :rows.shape[1]] = torch.from_numpy(rows).cuda()
    return out


def random_est(rng, d):
    est = (rng.standard_normal(d) * np.exp2(rng.uniform(-8, 8, d))).astype(f32)
    est[::17] = f32(-0.0)              # a -0.0 stays -0.0 only under adds of -0.0
    est[5::17] = f32(0.0)
    return est


class NibBatch:
    """One batch of NIB_TOTAL clients of 4-bit codes at d with every kmax <= 7; a mixed call has the clients at OVF
    and its last client above the nibble range (kmax 8, 128, 10^6: read from q, random nibbles as their codes).
    q holds a finite row for every client that some call reads from q and NaN everywhere else, so a row read
    for a client inside the range shows."""
    OVF = {0: 8, 40: 128, 1023: 128, 1024: 10 ** 6, 1500: 8}         # (40 and 1500: inside a full group of 32)
    LAST = (8, 128, 10 ** 6)

    def __init__(self, d, ldn=None, ldq=None):
        rng = np.random.default_rng(7000 + d)
        n = NIB_TOTAL
        self.d, self.m, self.n_div = d, 3 * d + 1, f32(n)
        self.ldn, self.ldq = ldn or d // 2, ldq or d
        self.codes, self.l1, self.kmax = M.synthetic(rng, n, d, (0, 1, 2, 3, 7), nibbles=True)
        cand = sorted(set(self.OVF) | {x - 1 for x in NIB_N})
        qo, co = M.overflowed(rng, len(cand), d, nibbles=True)
        self.q = np.full((n, d), np.nan, f32)
        self.q[cand] = qo
        self.est0 = random_est(rng, d)
        self.adds_fit = M.client_adds(self.codes, self.l1, self.kmax, self.m, self.n_div, q=self.q, nibbles=True)
        adds_q = M.client_adds(co, self.l1[cand], [128] * len(cand), self.m, self.n_div, q=qo, nibbles=True)
        self.row_q = {j: adds_q[i] for i, j in enumerate(cand)}
        self.cand = {j: i for i, j in enumerate(cand)}
        # the device side: the codes, the random nibbles a client above the range has instead, q, l1 and kmax
        self.d_fit = pitched(M.pack_nibbles(self.codes), self.ldn, SENT_B)
        self.d_rand = pitched(M.pack_nibbles(co), self.ldn, SENT_B)
        self.d_q = pitched(self.q, self.ldq, float("nan"))
        self.d_l1 = dev(self.l1)
        self.d_kfit = dev(self.kmax)

    def kmax_mixed(self, n):
        """(kmax of the first n clients with OVF and client n - 1 above the range, the indices above it)."""
        k = self.kmax[:n].copy()
        over = {j: v for j, v in self.OVF.items() if j < n}
        over.setdefault(n - 1, self.LAST[n % 3])
        for j, v in over.items():
            k[j] = v
        return k, sorted(over)

    def codes_mixed(self, over):
        codes = self.d_fit.clone()
        codes[over] = self.d_rand[[self.cand[j] for j in over]]
        return codes

    def want(self, n, over=(), est=None):
        adds = self.adds_fit[:n].copy()
        for j in over:
            adds[j] = self.row_q[j]
        return M.fold(adds, est)

    def run(self, api, codes, kmax_dev, n, accumulate=0, est=None):
        lib, L = api
        out = torch.full((self.d,), float("nan"), device="cuda") if est is None else dev(est)
        L.check(lib.uq_nibbles_q_mean_ld_f32(codes.data_ptr(), self.ldn, self.d_q.data_ptr(), self.ldq, self.d_l1.data_ptr(),
                                             kmax_dev.data_ptr(), n, self.d, self.m, float(self.n_div), accumulate,
                                             out.data_ptr(), stream()), "uq_nibbles_q_mean_ld_f32")
        torch.cuda.synchronize()
        return out.cpu().numpy()


def check_nibbles(api, b, n):
    # (i) every kmax <= 7: the straight-line loop (q is all NaN for these clients and must not be read)
    got = b.run(api, b.d_fit, b.d_kfit, n)
    assert G.bits_equal(got, b.want(n)), ("fit", b.d, n, G.n_mismatch(got, b.want(n)))
    # (ii) clients above the range at 0, 1023, 1024, inside full groups and at n - 1: the mixed loop
    k, over = b.kmax_mixed(n)
    got = b.run(api, b.codes_mixed(over), dev(k), n)
    want = b.want(n, over)
    assert np.isfinite(want).all()
    assert G.bits_equal(got, want), ("mixed", b.d, n, over, G.n_mismatch(got, want))
    # (iii) continuing from a random est
    got = b.run(api, b.d_fit, b.d_kfit, n, accumulate=1, est=b.est0)
    want = b.want(n, est=b.est0)
    assert G.bits_equal(got, want), ("accumulate", b.d, n, G.n_mismatch(got, want))


@pytest.mark.parametrize("d", (4096, 8192))
def test_nibbles_mean_chunks_and_groups(api, d):
    """K3n keeps the tables of 1024 clients (one chunk) in LDS and sums full groups of 32 in two batches of 16:
      n = 1, 15, 16, 17, 31   one chunk, no full group: the client-by-client loop alone
      n = 32, 33, 48          one full group, with 0, 1 and 16 clients after it (the prefetch clamped to n - 16)
      n = 1023, 1024          the first chunk one short of full (31 groups + 31 clients) and full (32 groups)
      n = 1025 .. 1055        a second chunk of 1, 15, 16, 17, 31 clients: below one group, read at rows 1024 + jj
                              with chunk-local table rows
      n = 1056, 1057          a second chunk of exactly one group, and of one group + 1
      n = 2048, 2049, 2081    two full chunks; a third chunk of 1 client and of one group + 1
    Each n: (i) all clients inside the nibble range, (ii) clients above it (kmax 8, 128, 10^6) at 0, 1023, 1024,
    inside full groups and at n - 1, (iii) accumulate = 1 onto a random est."""
    b = NibBatch(d)
    assert G.bits_equal(M.fold(b.adds_fit), M.mean(b.codes, b.l1, b.kmax, b.m, b.n_div, q=b.q, nibbles=True))
    for n in NIB_N:
        check_nibbles(api, b, n)


def test_nibbles_mean_pitched_rows(api):
    """Rows of wider buffers (ldn = d / 2 + 4, ldq = d + 4) with sentinel pads: the same bits, three chunks."""
    d = 4096
    b = NibBatch(d, ldn=d // 2 + 4, ldq=d + 4)
    for n in (1057, NIB_TOTAL):
        check_nibbles(api, b, n)
    assert bool((b.d_fit[:, d // 2:] == SENT_B).all()) and bool(torch.isnan(b.d_q[:, d:]).all())


# ---- K3c: int8 codes ---------------------------------------------------------------------------------------------

LAYOUTS = {                            # d, ldc, ldq: which kernel instance the columns select
    "aligned": (4096, 4096, 4096),     # <VEC, ALL>: whole workgroups of 8-byte loads
    "tail": (4112, 4112 + 16, 4112),   # <VEC>: a second workgroup with 2 threads inside d
    "bytewise": (1000, 1003, 1001),    # <false>: ldc no multiple of 16
}
BYTE_OVF = (0, 31, 32, 40, 64, 700, 1056)


class ByteBatch:
    """BYTE_TOTAL clients of int8 codes with kmax from {0, 1, 7, 63, 64, 65, 127} (`fit`), and the same batch
    with the clients at BYTE_OVF at kmax 128, random bytes as their codes and finite q rows (`over`)."""

    def __init__(self, layout, form):
        self.d, self.ldc, self.ldq = LAYOUTS[layout]
        rng = np.random.default_rng(9000 + self.d + form)
        n, d = BYTE_TOTAL, self.d
        self.form, self.m, self.n_div = form, 2 * d + 3, f32(n + 2)
        self.codes, self.l1, self.kmax = M.synthetic(rng, n, d, (0, 1, 7, 63, 64, 65, 127))
        qo, co = M.overflowed(rng, len(BYTE_OVF), d)
        self.q = np.full((n, d), np.nan, f32)
        self.q[list(BYTE_OVF)] = qo
        self.codes_over = self.codes.copy()
        self.codes_over[list(BYTE_OVF)] = co
        self.kmax_over = self.kmax.copy()
        self.kmax_over[list(BYTE_OVF)] = 128
        self.est0 = random_est(rng, d)
        args = (self.m, self.n_div, form)
        self.adds = {                  # (batch, with q) -> what each client adds
            ("fit", False): M.client_adds(self.codes, self.l1, self.kmax, *args),
            ("over", False): M.client_adds(self.codes_over, self.l1, self.kmax_over, *args),       # saturated codes
            ("over", True): M.client_adds(self.codes_over, self.l1, self.kmax_over, *args, q=self.q),
        }
        self.adds[("fit", True)] = self.adds[("fit", False)]
        self.dev = {"fit": (pitched(self.codes, self.ldc, SENT_B), dev(self.kmax)),
                    "over": (pitched(self.codes_over, self.ldc, SENT_B), dev(self.kmax_over))}
        self.d_q = pitched(self.q, self.ldq, float("nan"))
        self.d_l1 = dev(self.l1)

    def run(self, api, batch, with_q, n, accumulate):
        lib, L = api
        codes, kmax = self.dev[batch]
        out = dev(self.est0) if accumulate else torch.full((self.d,), float("nan"), device="cuda")
        L.check(lib.uq_codes_mean_form_f32(codes.data_ptr(), self.ldc, self.d_q.data_ptr() if with_q else None, self.ldq,
                                           self.d_l1.data_ptr(), kmax.data_ptr(), n, self.d, self.m, self.form,
                                           float(self.n_div), accumulate, out.data_ptr(), stream()), "uq_codes_mean_form_f32")
        torch.cuda.synchronize()
        return out.cpu().numpy()


@pytest.mark.parametrize("form", (M.UNBIASED, M.BIASED))
@pytest.mark.parametrize("layout", tuple(LAYOUTS))
def test_codes_mean_tables_to_127_and_overflowed_clients(api, layout, form):
    """K3c stages the tables of 32 clients at a time, each wave filling a client's entries k = lane, lane + 64:
    kmax 63, 64, 65 and 127 sit on either side of that loop's second trip.  n = 1, 31 (no full group), 32, 33,
    64, 65 (one and two groups, with one client after them), 1057 (33 groups + 1).  Four batches per n: every
    client inside the byte range without q and with q (q all NaN: never read), and clients at kmax 128 at 0, 31,
    32, 40, 64, 700, 1056 without q (their saturated codes are added) and with q (the mixed loop reads those
    clients from q); each from zero and onto a random est."""
    b = ByteBatch(layout, form)
    assert ((b.kmax > 63) & (b.kmax <= 127)).sum() > 100
    for n in BYTE_N:
        for batch in ("fit", "over"):
            for with_q in (False, True):
                for acc in (0, 1):
                    want = M.fold(b.adds[(batch, with_q)][:n], b.est0 if acc else None)
                    assert np.isfinite(want).all()
                    got = b.run(api, batch, with_q, n, acc)
                    assert G.bits_equal(got, want), (layout, form, n, batch, with_q, acc, G.n_mismatch(got, want))
    codes, _ = b.dev["over"]
    assert bool((codes[:, b.d:] == SENT_B).all())
