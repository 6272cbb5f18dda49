"""GPU: the edges of the QUIC-FL receiver (AS:526-532, before its inverse RHT) through the C ABI
itself (uq_quicfl_receive_ws_f32 / uq_quicfl_receive_f32 by ctypes), every message of every case
against oracle/uq_eden.py quicfl_receive_pre bit for bit:

  * masks placed on the seams of qfl_recv_rounds and of the team / jump runs: a row with every
    coordinate exact, a row with none, and a row with the coordinates around the 624-word rounds,
    the 640-lane loads and every run start of the form under test, in the dense and the compact
    layout (distinct value per compact slot, so a wrong slot base shows);
  * mask bytes other than 0 and 1 (KQ2c counts nonzero bytes by a popcount trick, the others
    test != 0); a mask base that is not 16-byte aligned (KQ2c's bytewise path);
  * D that is no power of two (the lookup has no RHT): D % 624 == 0, a last round of one
    coordinate, team runs without rounds, the jump form;
  * prng seeds 0, 2^31 and 2^32 - 1, and the call without a workspace.

The form of every call is read back through the plan hook."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import uq_eden as E
from tests import quicfl_plan_hook as H

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from quicfl_tables import recv_table  # noqa: E402

BAD_EXACT = 32                                     # UQ_QFL_BAD_EXACT
KINDS = {0: torch.int64, 1: torch.uint8, 2: torch.int32}
TABLES = {h: recv_table(2, h) for h in (48, 64)}   # [4, 48] (h = word % 48) and [4, 64] (a mask)
DENSE, COMPACT = 0, 1
JUNK = np.float32(-3.0)                            # in exact_vals wherever no exact value belongs
GENERAL_D = [625, 4368, 4992, 4993, 5617, 8191, 32449]   # nch = 2, 7, 8, 9, 10, 14 and 53 (52 * 624 + 1)
_cache = {}


@pytest.fixture(scope="module")
def lib(gpu_ready):
    from uqdme_amd._lib import load
    return load()


def _batch(n, D, seed):
    """X in 0..3, scales and prng seeds of a batch (host), once per shape."""
    key = ("batch", n, D, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        _cache[key] = (rng.integers(0, 4, (n, D)).astype(np.int64), rng.uniform(0.3, 40.0, n).astype(np.float32),
                       [int(s) for s in rng.integers(0, 1 << 16, n)])
    return _cache[key]


def _values(mask, layout):
    """exact_vals [n, D] for a mask: the value of a row's k-th exact coordinate is k + 0.5, at its
    coordinate (dense) or in slot k (compact), JUNK everywhere else; and the rows' counts."""
    n, D = mask.shape
    vals = np.full((n, D), JUNK, np.float32)
    cnt = np.zeros(n, np.int32)
    for j in range(n):
        pos = np.flatnonzero(mask[j])
        cnt[j] = pos.size
        slot = np.arange(pos.size, dtype=np.float32) + np.float32(0.5)
        if layout == DENSE:
            vals[j, pos] = slot
        else:
            vals[j, :pos.size] = slot
    return vals, cnt


def _expect(X, h_len, seeds, scale, mask):
    key = ("exp", X.shape, h_len, tuple(seeds), mask.tobytes())
    if key not in _cache:
        rows = []
        for j in range(X.shape[0]):
            k = int(np.count_nonzero(mask[j]))
            rows.append(E.quicfl_receive_pre(X[j], TABLES[h_len], h_len, seeds[j] & 0xFFFFFFFF, mask[j],
                                             np.arange(k, dtype=np.float32) + np.float32(0.5), scale[j]))
        _cache[key] = np.stack(rows)
    return _cache[key]


def _receive(lib, X, kind, h_len, seeds, scale, mask=None, vals=None, layout=DENSE, count=None, ws=True, mask_offset=None):
    """One uq_quicfl_receive_ws_f32 call (ws=False: uq_quicfl_receive_f32) on host arrays ->
    (out [n, D], info [n], the call's plan).  mask_offset: the mask's base address is that many
    bytes past a 16-byte boundary, inside a larger allocation."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n, D = X.shape
    p = ctypes.c_void_p
    Xd = torch.from_numpy(X).to(KINDS[kind]).to(dev).contiguous()
    tab = torch.from_numpy(TABLES[h_len]).to(dev).contiguous()
    sd = torch.from_numpy(np.array([s & 0xFFFFFFFF for s in seeds], np.uint32).view(np.int32)).to(dev)
    scd = torch.from_numpy(np.asarray(scale, np.float32)).to(dev)
    md = vd = cd = None
    if mask is not None:
        off = mask_offset or 0
        buf = torch.zeros(n * D + 64, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        md = buf[off:off + n * D]
        md.copy_(torch.from_numpy(np.ascontiguousarray(mask, np.uint8).reshape(-1)))
        assert md.data_ptr() % 16 == off % 16
        vd = torch.from_numpy(vals).to(dev).contiguous()
    if count is not None:
        cd = torch.from_numpy(np.asarray(count, np.int32)).to(dev)
    out = torch.full((n, D), float("nan"), dtype=torch.float32, device=dev)
    info = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ptr = lambda t: p(0 if t is None else t.data_ptr())  # noqa: E731
    stream = p(torch.cuda.current_stream(dev).cuda_stream)
    head = (ptr(Xd), kind, n, D, ptr(tab), TABLES[h_len].shape[0], h_len, ptr(sd), ptr(md), ptr(vd), layout, ptr(cd),
            ptr(scd), ptr(out), ptr(info))
    if ws:
        wb = ctypes.c_size_t()
        assert lib.uq_quicfl_receive_workspace_bytes(n, D, ctypes.byref(wb)) == 0
        wsd = torch.empty(max(int(wb.value), 1), dtype=torch.uint8, device=dev)
        rc = lib.uq_quicfl_receive_ws_f32(*head, ptr(wsd), wb.value, stream)
    else:
        rc = lib.uq_quicfl_receive_f32(*head, stream)
    assert rc == 0, lib.uq_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy(), H.last_plan(lib, H.RECEIVER)


def _same_bits(out, exp):
    bad = np.flatnonzero(out.view(np.uint32).reshape(-1) != exp.view(np.uint32).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:8] // out.shape[1], bad[:8] % out.shape[1])


def _run_starts(plan, D):
    """The first round of every run but the first, for the plan's form."""
    nch = (D + 623) // 624
    if plan["form"] == H.JUMP:
        return [r * plan["L"] for r in range(1, plan["R"]) if r * plan["L"] < nch]
    if plan["form"] == H.TEAM:
        per = (nch + 6) // 7
        return [r * per for r in range(1, 7) if r * per < nch]
    return []


def _placed_mask(plan, D):
    """Row 0: every coordinate; row 1: the seams (rounds of 624 words, loads of 640 lanes, the
    last coordinate, and around every run start s: s * 624 - 1, s * 624, s * 624 + 623); row 2: none."""
    m = np.zeros((3, D), np.uint8)
    m[0] = 1
    pos = {0, 623, 624, 639, 640, D - 1}
    for s in _run_starts(plan, D):
        pos |= {s * 624 - 1, s * 624, s * 624 + 623}
    m[1, sorted(i for i in pos if 0 <= i < D)] = 1
    return m


def _hooked(lib, hooks):
    class Ctx:
        def __enter__(self):
            self.prev = lib.uq_test_set_quicfl_hooks(hooks)

        def __exit__(self, *a):
            lib.uq_test_set_quicfl_hooks(self.prev)
    return Ctx()


# form by (D, hooks) at n = 3 with a workspace
FORMS = {(8192, 0): H.TEAM, (8192, 4): H.TEAM, (8192, 2): H.ONE_WAVE,
         (32768, 0): H.JUMP, (32768, 4): H.TEAM, (32768, 2): H.ONE_WAVE}


@pytest.mark.parametrize("D,hooks", sorted(FORMS))
def test_placed_masks(lib, D, hooks):
    """C1.  Dense, compact with exact_count and compact without; int64, uint8 and int32 X; h_len 48
    and 64.  info is 0 everywhere, and a count off by one sets UQ_QFL_BAD_EXACT in that row only."""
    n = 3
    X, scale, seeds = _batch(n, D, 11)
    plan = H.plan(lib, H.RECEIVER, n, D, hooks)
    assert plan["form"] == FORMS[D, hooks]
    if plan["form"] == H.JUMP:
        assert plan["R"] >= 2 and plan["L"] >= 1
    mask = _placed_mask(plan, D)
    assert len(_run_starts(plan, D)) == {H.ONE_WAVE: 0, H.TEAM: 6, H.JUMP: plan["R"] - 1}[plan["form"]]
    with _hooked(lib, hooks):
        for h_len in (48, 64):
            exp = _expect(X, h_len, seeds, scale, mask)
            for layout, counted in ((DENSE, False), (COMPACT, True), (COMPACT, False)):
                vals, cnt = _values(mask, layout)
                for kind in (0, 1, 2):
                    out, info, got = _receive(lib, X, kind, h_len, seeds, scale, mask, vals, layout, cnt if counted else None)
                    assert got == plan, (got, plan)
                    assert info.tolist() == [0, 0, 0], (h_len, layout, counted, kind, info)
                    _same_bits(out, exp)
            vals, cnt = _values(mask, COMPACT)
            for d in (1, -1):
                off = cnt.copy()
                off[1] += d
                out, info, _ = _receive(lib, X, 0, h_len, seeds, scale, mask, vals, COMPACT, off)
                assert info.tolist() == [0, BAD_EXACT, 0], (d, info)


@pytest.mark.parametrize("D,hooks", sorted(FORMS))
def test_mask_bytes_other_than_0_and_1(lib, D, hooks):
    """C2.  2, 0x7F, 0x80 and 0xFF on the exact coordinates (every byte of every word in row 0):
    the oracle's mask != 0, compact layout with counts, info 0."""
    n = 3
    X, scale, seeds = _batch(n, D, 12)
    plan = H.plan(lib, H.RECEIVER, n, D, hooks)
    mask = _placed_mask(plan, D)
    pat = np.array([2, 0x7F, 0x80, 0xFF, 0xFF, 2, 0x7F, 0x80, 0x80], np.uint8)     # (period 9: every byte lane gets each)
    mask = np.where(mask != 0, pat[np.arange(D) % pat.size][None, :], 0).astype(np.uint8)
    assert set(np.unique(mask).tolist()) == {0, 2, 0x7F, 0x80, 0xFF}
    vals, cnt = _values(mask, COMPACT)
    assert cnt[0] == D and cnt[2] == 0
    with _hooked(lib, hooks):
        for h_len in (48, 64):
            out, info, got = _receive(lib, X, 1, h_len, seeds, scale, mask, vals, COMPACT, cnt)
            assert got == plan and got["form"] == FORMS[D, hooks]
            assert info.tolist() == [0, 0, 0], info
            _same_bits(out, _expect(X, h_len, seeds, scale, mask))


@pytest.mark.parametrize("offset", [1, 8])
def test_mask_base_not_16_byte_aligned(lib, offset):
    """C3.  (3, 32768), the jump form, compact layout: the mask's base 1 and 8 bytes past a 16-byte
    boundary takes KQ2c's bytewise count; the same results as the aligned call."""
    n, D = 3, 32768
    X, scale, seeds = _batch(n, D, 13)
    plan = H.plan(lib, H.RECEIVER, n, D, 0)
    assert plan["form"] == H.JUMP
    mask = _placed_mask(plan, D)
    vals, cnt = _values(mask, COMPACT)
    exp = _expect(X, 48, seeds, scale, mask)
    ref, rinfo, got = _receive(lib, X, 0, 48, seeds, scale, mask, vals, COMPACT, cnt)
    assert got == plan and rinfo.tolist() == [0, 0, 0]
    out, info, got = _receive(lib, X, 0, 48, seeds, scale, mask, vals, COMPACT, cnt, mask_offset=offset)
    assert got == plan and info.tolist() == [0, 0, 0]
    _same_bits(out, ref)
    _same_bits(out, exp)


def test_general_D_reaches_every_form(lib):
    forms = {D: H.plan(lib, H.RECEIVER, 3, D, 0)["form"] for D in GENERAL_D}
    assert set(forms.values()) == {H.ONE_WAVE, H.TEAM, H.JUMP}, forms
    assert forms[625] == H.ONE_WAVE and forms[4368] == H.TEAM and forms[32449] == H.JUMP
    assert all(D & (D - 1) for D in GENERAL_D)


@pytest.mark.parametrize("D", GENERAL_D)
def test_general_D(lib, D):
    """C4.  The header puts no power-of-two condition on the receiver's D.  4992 = 8 * 624 (no
    partial round; team runs of 2 rounds, the last three without any), 4993 and 5617 a last round
    of one coordinate (team runs 5 and 6 without rounds), 4368 the team kernel's shortest
    message, 32449 = 52 * 624 + 1 the jump form.  A random 1 % mask plus the last coordinate."""
    n = 3
    X, scale, seeds = _batch(n, D, 14)
    rng = np.random.default_rng(D)
    mask = (rng.random((n, D)) < 0.01).astype(np.uint8)
    mask[:, D - 1] = 1
    for hooks in (0, 4, 2):
        plan = H.plan(lib, H.RECEIVER, n, D, hooks)
        with _hooked(lib, hooks):
            for h_len in (48, 64):
                exp = _expect(X, h_len, seeds, scale, mask)
                for layout in (DENSE, COMPACT):
                    vals, cnt = _values(mask, layout)
                    for kind in (0, 1):
                        out, info, got = _receive(lib, X, kind, h_len, seeds, scale, mask, vals, layout,
                                                  cnt if layout == COMPACT else None)
                        assert got == plan, (got, plan)
                        assert info.tolist() == [0, 0, 0], (hooks, h_len, layout, kind, info)
                        _same_bits(out, exp)


@pytest.mark.parametrize("D", [8192, 32768])
def test_seeds_at_the_int32_boundaries(lib, D):
    """C5.  prng seeds 0, 2^31 and 2^32 - 1 as int32 bit patterns (init_genrand takes them as uint32)."""
    n = 3
    X, scale, _ = _batch(n, D, 15)
    seeds = [0, 1 << 31, (1 << 32) - 1]
    mask = (np.random.default_rng(D + 1).random((n, D)) < 0.004).astype(np.uint8)
    vals, cnt = _values(mask, COMPACT)
    exp = _expect(X, 48, seeds, scale, mask)
    for hooks in (0, 4, 2):
        with _hooked(lib, hooks):
            out, info, got = _receive(lib, X, 1, 48, seeds, scale, mask, vals, COMPACT, cnt)
        assert got == H.plan(lib, H.RECEIVER, n, D, hooks) and got["form"] == FORMS[D, hooks]
        assert info.tolist() == [0, 0, 0]
        _same_bits(out, exp)


def test_no_workspace_takes_the_team_kernel(lib):
    """C5.  uq_quicfl_receive_f32 (no workspace) at (1, 32768): the plan says team."""
    n, D = 1, 32768
    X, scale, seeds = _batch(n, D, 16)
    mask = (np.random.default_rng(5).random((n, D)) < 0.004).astype(np.uint8)
    mask[0, [0, D - 1]] = 1
    for layout in (DENSE, COMPACT):
        vals, cnt = _values(mask, layout)
        out, info, got = _receive(lib, X, 0, 64, seeds, scale, mask, vals, layout, cnt if layout == COMPACT else None,
                                  ws=False)
        assert got == H.plan(lib, H.RECEIVER, n, D, 0, has_ws=False) and got["form"] == H.TEAM
        assert H.plan(lib, H.RECEIVER, n, D, 0)["form"] == H.JUMP            # (with one it would jump)
        assert info.tolist() == [0]
        _same_bits(out, _expect(X, 64, seeds, scale, mask))
