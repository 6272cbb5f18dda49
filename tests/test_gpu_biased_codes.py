"""Type codes of the biased type quantizer on the GPU.

The yardsticks all exist without the codes: uq_type_biased_f32 (pinned to the reference by
tests/test_gpu_biased.py), the reference's fixtures, and the oracle's codec_encode.  Every case
runs the plain call, the out + codes call and the codes-only call with the same policy
(check_case) and asserts:
  out equal bit for bit in the first two; codes and kmax equal in the last two; decode(codes) ==
  out bit for bit for unflagged rows; the codes equal the model's recovered codes where L1 is
  finite and > 0; kmax within its bounds (>= every coded count, <= the largest + 1, 128 exactly
  for the rows that must not be decoded); and the dispatch plan of the three calls.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import uq_oracle_c as C
from oracle.uq_oracle import rate_to_m
from tests import biased_codes_model as M
from tests import biased_plan_hook as H
from tests import golden_data as G

pytestmark = pytest.mark.gpu
f32 = np.float32
TORCH, LOWEST, HOST_CHECK = H.POLICY_TORCH, H.POLICY_LOWEST, H.HOST_CHECK
FINE, FULLC, AMB, REPLAYED = 16, 32, 1, 8           # info flags


@pytest.fixture(scope="module")
def uq(gpu_ready):
    import uqdme
    C.build()
    return uqdme


def _rt():
    from uqdme_amd import _lib, _runtime
    return _lib, _runtime


def shifted(a, off):
    """a's values in a fresh device tensor whose data pointer is `off` elements past an
    allocation boundary (off 0: aligned)."""
    base = torch.empty(a.numel() + off, dtype=a.dtype, device="cuda")
    v = base[off:].view(a.shape)
    v.copy_(a)
    return v


def call(x, m, T, policy, mode, offs=(0, 0)):
    """One C-ABI call on x [n, d] (device): mode 'plain' (uq_type_biased_f32), 'both' or 'codes'
    (uq_type_biased_codes_f32, without out).  offs: element offsets of out and codes."""
    _lib, rt = _rt()
    lib = _lib.load()
    dev = rt.device()
    n, d = x.shape
    out = codes = kmax = None
    if mode != "codes":
        out = shifted(torch.empty((n, d), dtype=torch.float32, device=dev), offs[0])
    if mode != "plain":
        codes = shifted(torch.full((n, d), 99, dtype=torch.int8, device=dev), offs[1])
        kmax = torch.full((n,), -7, dtype=torch.int32, device=dev)
    l1 = torch.empty(n, dtype=torch.float32, device=dev)
    info = torch.empty((n, 2), dtype=torch.int32, device=dev)
    ws = rt.workspace_for("uq_biased_workspace_bytes" if mode == "plain" else "uq_biased_codes_workspace_bytes", dev, n, d, T)
    p, sp = rt.ptr, rt.stream_ptr(dev)
    if mode == "plain":
        rc = lib.uq_type_biased_f32(p(x), p(out), n, d, m, T, policy, p(l1), p(info), p(ws), ws.numel(), sp)
    else:
        rc = lib.uq_type_biased_codes_f32(p(x), p(out), p(codes), p(kmax), n, d, m, T, policy, p(l1), p(info), p(ws),
                                          ws.numel(), sp)
    _lib.check(rc, mode)
    plan = H.last_plan(lib)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()          # noqa: E731
    return SimpleNamespace(out=host(out), codes=host(codes), kmax=host(kmax), l1=host(l1), info=host(info), plan=plan,
                           dcodes=codes, dkmax=kmax, dl1=l1, dout=out)


def decode_biased(uq, r, m):
    tc = uq.TypeCodes(codes=r.dcodes, l1=r.dl1, m=m, overflow=r.dkmax, form="biased")
    return uq.decode(tc).cpu().numpy()


def check_case(uq, x, m, policy, T=1, x_off=0, offs=(0, 0), front=None):
    """The three calls and every common assertion (module docstring); returns (plain, both)."""
    xh = np.ascontiguousarray(x, f32)
    n, d = xh.shape
    xd = shifted(torch.as_tensor(xh), x_off)
    r0 = call(xd, m, T, policy, "plain", offs)
    r1 = call(xd, m, T, policy, "both", offs)
    r2 = call(xd, m, T, policy, "codes", offs)
    assert G.bits_equal(r0.out, r1.out), f"out differs in {G.n_mismatch(r0.out, r1.out)} places"
    for r in (r1, r2):
        assert G.bits_equal(r0.l1, r.l1) and np.array_equal(r0.info, r.info)
    assert np.array_equal(r1.codes, r2.codes), int((r1.codes != r2.codes).sum())
    assert np.array_equal(r1.kmax, r2.kmax), (r1.kmax, r2.kmax)
    # the plan: the codes calls take the plain call's path; 16-byte accesses also need the codes rows 4-byte aligned
    x_al, o_al, c_al = x_off % 4 == 0, offs[0] % 4 == 0, offs[1] % 4 == 0
    for r, v4 in ((r0, x_al and o_al), (r1, x_al and o_al and c_al), (r2, x_al and c_al)):
        assert r.plan["vec4"] == (v4 and d % 4 == 0), r.plan
        assert {k: v for k, v in r.plan.items() if k != "vec4"} == {k: v for k, v in r0.plan.items() if k != "vec4"}
    if front is not None:
        assert r0.plan["front"] == front, r0.plan
    dec = decode_biased(uq, r1, m)
    flagged = r1.kmax == 128
    for j in range(n):
        k, _ = M.counts(r1.codes[j])
        kc = int(k.max())
        l1 = r0.l1[j]
        hard = (not np.isfinite(l1)) or bool(r0.info[j, 1] & 6)
        if flagged[j]:
            assert hard or kc >= 127, (j, kc, l1, r0.info[j])      # (a provisional 128 lowered to 127 flags too)
            continue
        assert not hard, j
        assert kc <= r1.kmax[j] <= kc + 1, (j, kc, r1.kmax[j])
        assert G.bits_equal(dec[j], r0.out[j]), (j, G.n_mismatch(dec[j], r0.out[j]))
        if l1 > 0:
            rec = M.recover_codes(xh[j], r0.out[j], l1, m)
            assert np.array_equal(rec, r1.codes[j].astype(np.int64)), (j, int((rec != r1.codes[j]).sum()))
            assert int(k.sum()) <= m and (np.any(xh[j] == 0) or int(k.sum()) == m), j
    return r0, r1


# ---- 1: KB-small ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 5, 100, 1023, 4097, 32767])
def test_small_front(uq, d):
    rng = np.random.default_rng(d)
    x = rng.standard_normal((3, d)).astype(f32)
    x[1] = rng.integers(-3, 4, d)                              # ties: the index-order ranks in one workgroup
    ran = 0
    for R in ((4,) if d == 1 else (0.5, 1, 4)):
        m = rate_to_m(R, d)
        if m < 1:
            continue
        check_case(uq, x, m, LOWEST, front=H.SMALL)
        ran += 1
    assert ran >= 1
    uq.check_status()


# ---- 2, 4: the full front, fine clients, float4 path, KB6p -----------------------------------
@pytest.mark.parametrize("d", [32768, 65536])
def test_full_front_fine_clients(uq, d):
    rng = np.random.default_rng(d + 1)
    x = rng.standard_normal((2, d)).astype(f32)
    for policy in (TORCH, LOWEST):
        r0, r1 = check_case(uq, x, rate_to_m(1, d), policy, front=H.FULL)
        assert r0.plan["vec4"]
        assert np.all(r0.info[:, 1] & FINE) and np.any(r0.info[:, 0] != 0), r0.info    # KB6f + KB6p ran
        assert np.all(r1.kmax < 128)
    uq.check_status()


# ---- 3: the scalar paths ---------------------------------------------------------------------
@pytest.mark.parametrize("d,x_off,out_off,codes_off", [(32773, 0, 0, 0), (32768, 1, 0, 0), (32768, 0, 1, 0),
                                                      (32768, 0, 0, 1), (32768, 0, 0, 2)])
def test_scalar_paths(uq, d, x_off, out_off, codes_off):
    rng = np.random.default_rng(d + 7 * x_off + 11 * out_off + 13 * codes_off)
    x = rng.standard_normal((2, d)).astype(f32)
    x[1] = np.round(x[1] * 4) / 4                              # a full client beside the fine one
    for policy in (TORCH, LOWEST):
        check_case(uq, x, rate_to_m(1, d), policy, x_off=x_off, offs=(out_off, codes_off), front=H.FULL)
    uq.check_status()


# ---- 5: tie-heavy "full" clients: the index-order rank path, KB7 and KB6 part 2 ---------------
@pytest.mark.parametrize("policy", [TORCH, LOWEST])
def test_tie_heavy_full_clients(uq, policy):
    d = 32768
    x = np.random.default_rng(55).integers(-3, 4, (2, d)).astype(f32)
    r0, _ = check_case(uq, x, rate_to_m(1, d), policy, front=H.FULL)
    assert np.all(r0.info[:, 1] & FULLC) and np.all(r0.info[:, 1] & AMB), r0.info
    assert np.all((r0.info[:, 1] & REPLAYED) != 0) == (policy == TORCH)
    uq.check_status()


# ---- 6: fine clients with a replayed threshold tie (KB6t) -------------------------------------
def test_fine_clients_with_replayed_ties(uq):
    """Gaussian rows on a grid of 2^-10: every magnitude occurs a few times, so the threshold key
    is shared (ambiguous) while its fine bin stays small (a fine client)."""
    d = 65536
    x = (np.round(np.random.default_rng(66).standard_normal((3, d)) * 1024) / 1024).astype(f32)
    r0, _ = check_case(uq, x, rate_to_m(1, d), TORCH, front=H.FULL)
    want = FINE | AMB | REPLAYED
    assert np.any((r0.info[:, 1] & want) == want), r0.info
    uq.check_status()


# ---- 7: the levels replay ---------------------------------------------------------------------
def test_levels_replay(uq):
    n, d = 32, 8200
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, d)).astype(f32)
    x[::3] = rng.integers(-3, 4, (len(range(0, n, 3)), d))
    r0, _ = check_case(uq, x, rate_to_m(1, d), TORCH, front=H.FULL)
    assert (r0.plan["ties"], r0.plan["replay"]) == (H.FORK, H.LEVELS), r0.plan
    assert int((r0.info[:, 1] & REPLAYED != 0).sum()) >= n // 3
    uq.check_status()


# ---- 8: a forced replay failure ---------------------------------------------------------------
def test_forced_replay_failure(uq):
    _lib, _ = _rt()
    n, d = 3, 65536
    x = np.random.default_rng(88).integers(-3, 4, (n, d)).astype(f32)
    m = rate_to_m(1, d)
    assert _lib.load().uq_test_force_replay_failure(1) == 0
    try:
        r0, r1 = check_case(uq, x, m, TORCH, front=H.FULL)
        with pytest.raises(uq.UQError):
            uq.check_status()
    finally:
        assert _lib.load().uq_test_force_replay_failure(0) == 1
    assert not np.any(r0.info[:, 1] & REPLAYED) and np.all(r0.info[:, 1] & AMB)
    low = call(torch.as_tensor(x).cuda(), m, 1, LOWEST, "both")     # the defined fallback: the lowest-index result
    assert G.bits_equal(r1.out, low.out) and np.array_equal(r1.codes, low.codes)
    uq.check_status()


# ---- 9: the host-check variants ---------------------------------------------------------------
@pytest.mark.parametrize("n,d,ties", [(3, 4097, True), (3, 4097, False), (2, 65536, True), (32, 8200, True),
                                      (32, 8200, False)])
def test_host_check_gives_the_same_bits(uq, n, d, ties):
    rng = np.random.default_rng(n * d + ties)
    x = rng.standard_normal((n, d)).astype(f32)
    if ties:
        x[n // 2] = rng.integers(-3, 4, d)
    m = rate_to_m(1, d)
    r0, r1 = check_case(uq, x, m, TORCH | HOST_CHECK)
    if d <= 32767:
        assert r0.plan["front"] == H.SMALL_CHECKED and r0.plan["ran"] == int(ties), r0.plan
    elif n >= 32:
        assert r0.plan["ties"] == H.CHECKED and r0.plan["ran"] == int(ties), r0.plan
    ref = call(torch.as_tensor(x).cuda(), m, 1, TORCH, "both")
    assert G.bits_equal(r1.out, ref.out) and np.array_equal(r1.codes, ref.codes)
    assert np.all(np.abs(r1.kmax - ref.kmax) <= 1)
    uq.check_status()


# ---- 10: cand_multi ---------------------------------------------------------------------------
def test_cand_multi(uq):
    d = (1 << 17) + 21
    x = np.random.default_rng(10).standard_normal((2, d)).astype(f32)
    r0, _ = check_case(uq, x, rate_to_m(1, d), TORCH, front=H.FULL)
    assert r0.plan["cand_multi"], r0.plan
    uq.check_status()


# ---- 11-14: Delta = 0, all-zero rows, zeros picked by the adjustment, -0.0 ---------------------
@pytest.mark.parametrize("d", [100, 32768])
def test_special_rows(uq, d):
    rng = np.random.default_rng(d + 3)
    m = 100 if d > 100 else 21
    x = np.zeros((6, d), f32)
    x[0, d // 3] = -2.5                                        # one-hot: k' = m there, Delta = 0
    # x[1]: all zero
    x[2, 5], x[2, 9] = 3e-13, -2e-13                           # L1 ~ 1e-12: Delta ~ -m/2, zeros take the +1s
    x[3] = rng.standard_normal(d) * (rng.random(d) < 0.05)     # many exact zeros
    x[4] = rng.standard_normal(d)                              # m << d: most counts 0, half of them negative
    x[5] = -np.abs(rng.standard_normal(d))
    r0, r1 = check_case(uq, x, m, LOWEST, front=H.SMALL if d <= 32767 else H.FULL)
    assert np.all(r1.kmax < 128)
    assert r0.info[0, 0] == 0 and r1.codes[0, d // 3] == -m - 1 and r1.kmax[0] == m
    assert not r1.codes[0].astype(bool).sum() > 1
    assert r0.info[1, 0] == -m and not r1.codes[1].any() and r1.kmax[1] <= 1
    assert G.bits_equal(r0.out[1], np.zeros(d, f32))          # +0.0 everywhere
    k2, _ = M.counts(r1.codes[2])
    assert r0.info[2, 0] < -2 and int(k2.sum()) < m           # the adjustment went to zero coordinates
    zero = x[2] == 0
    assert not r1.codes[2][zero].any() and G.bits_equal(r0.out[2][zero], np.zeros(int(zero.sum()), f32))
    for j in (4, 5):                                           # -0.0 <-> code -1
        negz = (r0.out[j] == 0) & np.signbit(r0.out[j])
        assert negz.sum() > 0 and np.all(r1.codes[j][negz] == -1) and np.all(x[j][negz] < 0)
        assert np.array_equal(r1.codes[j] == -1, negz)
    uq.check_status()


# ---- 15: flagged rows -------------------------------------------------------------------------
@pytest.mark.parametrize("d,policy", [(4096, LOWEST), (32768, TORCH)])
def test_flagged_rows(uq, d, policy):
    rng = np.random.default_rng(d + 15)
    m = rate_to_m(1, d)
    assert m > 127
    x = rng.standard_normal((4, d)).astype(f32)
    x[1] = 0
    x[1, 17] = 3.0                                             # one-hot at m > 127: its count saturates
    x[3, 40] = np.inf                                          # L1 and m' not finite
    r0, r1 = check_case(uq, x, m, policy)
    assert r1.kmax.tolist()[1] == 128 and r1.kmax[3] == 128 and r1.kmax[0] < 128 and r1.kmax[2] < 128, r1.kmax
    assert r1.codes[1, 17] == 127
    tc = uq.TypeCodes(codes=r1.dcodes, l1=r1.dl1, m=m, overflow=r1.dkmax, form="biased")
    with pytest.raises(OverflowError):
        tc.check()
    # the mean with q beside the codes reads the flagged rows from q: the float mean's bits
    # (row 3 is NaN-laden in both: compared as bits)
    est = uq.codes_mean(tc, 4.0, q=r1.dout).cpu().numpy()
    ref = uq.client_mean(r1.dout, 4.0).cpu().numpy()
    assert G.bits_equal(est[np.isfinite(ref)], ref[np.isfinite(ref)]) and np.array_equal(np.isnan(est), np.isnan(ref))
    tc3 = uq.TypeCodes(codes=r1.dcodes[:3], l1=r1.dl1[:3], m=m, overflow=r1.dkmax[:3], form="biased")
    assert G.bits_equal(uq.codes_mean(tc3, 3.0, q=r1.dout[:3]).cpu().numpy(), uq.client_mean(r1.dout[:3], 3.0).cpu().numpy())
    uq.check_status()


# ---- the reference's fixtures through the GPU -------------------------------------------------
def test_reference_fixtures_decode_bit_exact(uq):
    n, bad = 0, []
    for sp, x, q, l1, m in M.qualifying_fixtures():
        tc = uq.biased_quantize_encode(torch.as_tensor(x).cuda().view(1, -1), m=m, torch_threads=sp["threads"], ties="torch")
        tc.check()
        assert tc.form == "biased" and G.bits_equal(tc.l1.cpu().numpy(), np.array([l1], f32)), sp["idx"]
        if not G.bits_equal(uq.decode(tc).cpu().numpy()[0], q):
            bad.append(sp["idx"])
        n += 1
    assert n >= 90, n
    assert not bad, f"decode(codes) differs from the reference on fixtures {bad}"
    uq.check_status()


# ---- the mean from codes ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def mean_batches(uq):
    """{d: (m, plain out [70, d], codes call)} computed once and left unchanged."""
    res = {}
    for d in (4096, 4104, 4099, 4112):
        x = torch.as_tensor(np.random.default_rng(d).standard_normal((70, d)).astype(f32)).cuda()
        m = rate_to_m(2, d)
        res[d] = (m, call(x, m, 1, LOWEST, "plain"), call(x, m, 1, LOWEST, "codes"))
    return res


def mean_form(r, m, n, d, form, n_div, acc, est, ldc=None, q=None):
    _lib, rt = _rt()
    dev = rt.device()
    codes = r.dcodes[:n]
    if ldc is not None:
        wide = torch.zeros((n, ldc), dtype=torch.int8, device=dev)
        wide[:, :d] = codes
        codes = wide
    _lib.check(_lib.load().uq_codes_mean_form_f32(rt.ptr(codes), ldc or d, rt.ptr(q), d, rt.ptr(r.dl1), rt.ptr(r.dkmax), n, d,
                                                  m, form, n_div, int(acc), rt.ptr(est), rt.stream_ptr(dev)), "mean")
    return est


@pytest.mark.parametrize("d", [4096, 4104, 4099, 4112])
def test_biased_mean_from_codes(uq, mean_batches, d):
    """uq_codes_mean_form_f32(UQ_FORM_BIASED) == uq_client_mean_f32 over the plain call's out: the
    ALL, vector, and bytewise instances (d = 4096, 4112, 4104 / 4099), table groups of 32, the
    16-client batches and the remainder loop, accumulate off and on, ldc > d once."""
    m, plain, cod = mean_batches[d]
    assert np.all(cod.kmax < 128)
    init = torch.as_tensor(np.random.default_rng(1).standard_normal(d).astype(f32)).cuda()
    for n in (1, 31, 32, 33, 70):
        for acc in (False, True):
            ref = uq.client_mean(plain.dout[:n], float(n), est=init.clone(), accumulate=acc)
            est = mean_form(cod, m, n, d, M.BIASED, float(n), acc, init.clone())
            assert torch.equal(est.view(torch.int32), ref.view(torch.int32)), (n, acc)
    ref = uq.client_mean(plain.dout[:33], 33.0)
    est = mean_form(cod, m, 33, d, M.BIASED, 33.0, False, torch.empty(d, device="cuda"), ldc=d + 16)
    assert torch.equal(est.view(torch.int32), ref.view(torch.int32))
    uq.check_status()


def test_unbiased_form_is_todays_entries(uq):
    _lib, rt = _rt()
    lib, dev = _lib.load(), rt.device()
    for n, d in ((33, 4096), (5, 4099)):
        x = torch.as_tensor(np.random.default_rng(n).standard_normal((n, d)).astype(f32)).cuda()
        tc = uq.quantize_encode(x, 2, X=np.random.default_rng(2).random(n).astype(f32), torch_threads=1)
        assert tc.form == "unbiased"
        p, sp, m = rt.ptr, rt.stream_ptr(dev), tc.m
        a, b = torch.empty((n, d), device=dev), torch.empty((n, d), device=dev)
        _lib.check(lib.uq_codes_decode_f32(p(tc.codes), p(tc.l1), n, d, m, p(a), sp), "decode")
        _lib.check(lib.uq_codes_decode_form_f32(p(tc.codes), p(tc.l1), n, d, m, M.UNBIASED, p(b), sp), "decode form")
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        ea, eb = torch.empty(d, device=dev), torch.empty(d, device=dev)
        _lib.check(lib.uq_codes_mean_f32(p(tc.codes), p(tc.l1), p(tc.overflow), n, d, m, float(n), 0, p(ea), sp), "mean")
        _lib.check(lib.uq_codes_mean_form_f32(p(tc.codes), d, None, d, p(tc.l1), p(tc.overflow), n, d, m, M.UNBIASED,
                                              float(n), 0, p(eb), sp), "mean form")
        assert torch.equal(ea.view(torch.int32), eb.view(torch.int32))
        assert torch.equal(uq.codes_mean(tc, n).view(torch.int32), ea.view(torch.int32))
        # the biased table gives other low bits for these codes: the forms are not interchangeable
        _lib.check(lib.uq_codes_decode_form_f32(p(tc.codes), p(tc.l1), n, d, m, M.BIASED, p(b), sp), "decode form")
        assert not torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.allclose(a, b, rtol=1e-6)
    uq.check_status()


# ---- messages ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1000, 65536])
def test_messages(uq, d):
    rng = np.random.default_rng(d + 9)
    x = torch.as_tensor(rng.standard_normal((3, d)).astype(f32)).cuda()
    tc, q = uq.biased_quantize_encode(x, 1, torch_threads=1, with_q=True)
    codes, l1 = tc.codes.cpu().numpy(), tc.l1.cpu().numpy()
    msgs = uq.encode_messages(tc, exact_zero_signs=True)
    assert msgs.form == "biased"
    plain = uq.encode_messages(uq.TypeCodes(codes=tc.codes, l1=tc.l1, m=tc.m, overflow=tc.overflow), exact_zero_signs=True)
    for j, (mb, mp) in enumerate(zip(msgs.messages(), plain.messages())):
        exp = C.codec_encode(codes[j], tc.m, l1[j], True)
        assert mp == exp, j                                   # the flag off: byte for byte the oracle's message
        flagged = bytearray(exp)
        flagged[6] |= 2                                       # UQ_TC_BIASED_FORM in the flags half-word
        assert mb == bytes(flagged), j
    back = uq.decode_messages(msgs)
    assert back.form == "biased" and back.m == tc.m
    assert torch.equal(back.codes, tc.codes) and torch.equal(back.l1.view(torch.int32), tc.l1.view(torch.int32))
    assert torch.equal(uq.decode(back).view(torch.int32), q.view(torch.int32))
    host = uq.TypeMessages.from_messages(msgs.messages(), d)
    assert host.form == "biased" and host.exact_zero_signs
    assert torch.equal(uq.decode(uq.decode_messages(host)).view(torch.int32), q.view(torch.int32))
    with pytest.raises(ValueError, match="form"):
        uq.TypeMessages.from_messages([msgs.message(0), plain.message(1)], d)
    print(f"UQR1 biased d={d} R=1: {msgs.bits_per_dim():.3f} bits per coordinate")
    uq.check_status()


# ---- the Python surface -----------------------------------------------------------------------
def test_python_surface(uq):
    rng = np.random.default_rng(123)
    n, d = 5, 40000
    xh = rng.standard_normal((n, d)).astype(f32)
    x = torch.as_tensor(xh).cuda()
    ref = uq.biased_quantize(x, 1, torch_threads=1)
    tc, q = uq.biased_quantize_encode(x, 1, torch_threads=1, with_q=True)
    assert torch.equal(q.view(torch.int32), ref.view(torch.int32)) and tc.form == "biased" and tc.m == rate_to_m(1, d)
    only = uq.biased_quantize_encode(x, 1, torch_threads=1)
    assert torch.equal(only.codes, tc.codes) and torch.equal(only.overflow, tc.overflow)
    assert torch.equal(uq.decode(only).view(torch.int32), ref.view(torch.int32))
    back = uq.TypeCodes.from_bytes(only.to_bytes(), device="cuda")
    assert back.form == "biased" and torch.equal(uq.decode(back).view(torch.int32), ref.view(torch.int32))
    est = uq.biased_quantize_mean(x, 1, torch_threads=1)
    assert torch.equal(est.view(torch.int32), uq.client_mean(ref, n).view(torch.int32))
    acc = uq.biased_quantize_mean(x, 1, n_div=7.0, torch_threads=1, est=est.clone(), accumulate=True)
    assert torch.equal(acc.view(torch.int32), uq.client_mean(ref, 7.0, est=est.clone(), accumulate=True).view(torch.int32))
    xh[2] = 0
    xh[2, 11] = -1.0                                           # a flagged row (its count is m > 127)
    x = torch.as_tensor(xh).cuda()
    ref = uq.biased_quantize(x, 1, torch_threads=1)
    assert int(uq.biased_quantize_encode(x, 1, torch_threads=1).overflow[2]) == 128
    est = uq.biased_quantize_mean(x, 1, torch_threads=1)
    assert torch.equal(est.view(torch.int32), uq.client_mean(ref, n).view(torch.int32))
    with pytest.raises(uq.UQError):
        uq.biased_quantize_encode(x, m=0)
    uq.check_status()
