"""The biased quantizer's dispatch table (host only: uq_test_biased_plan launches nothing).

uq_type_biased_f32 computes one plan (biased_plan, csrc/uq_biased.hip) from (n, d, tie_policy,
alignment) and launches what it names; the hook reports the same plan.  Both sides of each
threshold are pinned twice: against rows derived by hand from the rule, and against `rule`, a
restatement of it that shares nothing with the library."""
import ctypes

import pytest

import uqdme
from tests import biased_plan_hook as H

L, T, TH = H.POLICY_LOWEST, H.POLICY_TORCH, H.POLICY_TORCH | H.HOST_CHECK
SMALL_MAX, CHECK_MAX_N = 32767, 64            # KB-small: d < GRAIN; host-checked up to 64 clients
LEVEL_MIN, LEVEL_MIN_N, LEVEL_BIG_D = 8192, 32, 1 << 21       # KB7a: d > 8192 and (n >= 32 or d >= 2^21)
LEVEL_STOP, LEVEL_MARGIN, HEAVY = 16384, 3, 2


@pytest.fixture(scope="module")
def lib():
    return uqdme.load_library()


def rule(n, d, policy, x_aligned=True, out_aligned=True):
    """What a call of this shape runs, restated from the dispatch rules."""
    cap = min(max(d, 1), max(4096, d // 8))
    p = dict(front=H.NONE, ties=H.LOWEST, replay=H.NO_REPLAY, levels=0, lsplit=0, lgrid=0, S=min(n, 256), vec4=False,
             cand_multi=False, cspans=-(-(cap // 2) // 8192), cap=cap, capf=cap // 2, tiles=-(-d // 4096),
             clear_bits=False, ran=-1)
    if n == 0 or d == 0:
        return p
    torch, check = (policy & 3) == T, bool(policy & H.HOST_CHECK)
    if d <= SMALL_MAX and not torch:
        p["front"] = H.SMALL
    elif d <= SMALL_MAX and check and n <= CHECK_MAX_N:
        p["front"] = H.SMALL_CHECKED
    else:
        p["front"] = H.FULL
    p["vec4"] = x_aligned and out_aligned and d % 4 == 0
    p["cand_multi"] = n <= 16 and p["cspans"] > 1
    if not torch:
        return p
    kb7a = not (d <= LEVEL_MIN or (n < LEVEL_MIN_N and d < LEVEL_BIG_D))
    p["ties"] = H.CHECKED if check and kb7a else H.FORK
    p["replay"] = H.LEVELS if kb7a else H.ONE_KERNEL
    p["clear_bits"] = not kb7a
    if kb7a:
        levels, r = LEVEL_MARGIN, d
        while r > LEVEL_STOP:
            levels, r = levels + 1, (r + 1) // 2
        p.update(levels=levels, lsplit=min(HEAVY, levels), lgrid=min(2048, p["S"] * 256 // 4))
    return p


ONE = dict(replay=H.ONE_KERNEL, levels=0, lsplit=0, lgrid=0)
ROWS = [        # (n, d, policy, expected fields), derived by hand
    (4, 32767, L, dict(front=H.SMALL)),
    (4, 32768, L, dict(front=H.FULL, ties=H.LOWEST, replay=H.NO_REPLAY, levels=0, clear_bits=False)),
    (64, 32767, TH, dict(front=H.SMALL_CHECKED, ties=H.CHECKED, replay=H.LEVELS, levels=4, lsplit=2, S=64, lgrid=2048)),
    (8, 32767, TH, dict(front=H.SMALL_CHECKED, ties=H.FORK, clear_bits=True, **ONE)),
    (65, 32767, TH, dict(front=H.FULL, ties=H.CHECKED, replay=H.LEVELS)),
    (8, 32767, T, dict(front=H.FULL, ties=H.FORK, **ONE)),
    (1024, 8192, T, dict(front=H.FULL, ties=H.FORK, S=256, clear_bits=True, **ONE)),
    (32, 8193, T, dict(ties=H.FORK, replay=H.LEVELS, levels=3, lsplit=2, S=32, lgrid=2048, clear_bits=False)),
    (31, 8193, T, dict(ties=H.FORK, **ONE)),
    (31, 1 << 21, T, dict(ties=H.FORK, replay=H.LEVELS, levels=10, S=31, lgrid=1984)),
    (31, (1 << 21) - 1, T, dict(ties=H.FORK, **ONE)),
    (1, (1 << 21) + 3, T, dict(replay=H.LEVELS, levels=11)),
    (1, 1 << 22, T, dict(ties=H.FORK, replay=H.LEVELS, levels=11, S=1, lgrid=64)),
    (1, 1 << 22, TH, dict(front=H.FULL, ties=H.CHECKED, replay=H.LEVELS, levels=11, S=1, lgrid=64)),
    (1, 1 << 20, TH, dict(front=H.FULL, ties=H.FORK, **ONE)),
    (1024, 1 << 20, T, dict(ties=H.FORK, replay=H.LEVELS, levels=9, lsplit=2, S=256, lgrid=2048)),
] + [row for pol in (L, T, TH) for row in (
    (16, 131088, pol, dict(cand_multi=True, cspans=2, capf=8193, cap=16386)),
    (16, 131087, pol, dict(cand_multi=False, cspans=1, capf=8192, cap=16385)),
    (17, 131088, pol, dict(cand_multi=False, cspans=2)),
    (16, 1 << 20, pol, dict(cand_multi=True, cspans=8, capf=65536, tiles=256)),
)]


@pytest.mark.parametrize("n,d,policy,want", ROWS)
def test_rows(lib, n, d, policy, want):
    p = H.plan(lib, n, d, policy)
    for key, v in want.items():
        assert p[key] == v, (n, d, policy, key, p)
    assert p["ran"] == -1
    assert p == rule(n, d, policy), (n, d, policy)


def test_both_sides_of_every_threshold(lib):
    """Every (n, d) pair of the thresholds' neighbours, every policy, against the restated rule."""
    ns = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1024, 65535]
    ds = [1, 4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385, 32767, 32768, 32769, 65536, 131087, 131088, (1 << 20) - 1,
          1 << 20, (1 << 21) - 1, 1 << 21, (1 << 21) + 3, 1 << 22, (1 << 31) - 1]
    for n in ns:
        for d in ds:
            for policy in (L, T, TH, L | H.HOST_CHECK):
                assert H.plan(lib, n, d, policy) == rule(n, d, policy), (n, d, policy)


def test_vec4_needs_both_pointers_aligned_and_whole_float4s(lib):
    for d in (4096, 4097, 4098, 1 << 20, (1 << 20) + 2):
        for xa in (False, True):
            for oa in (False, True):
                for policy in (L, T, TH):
                    assert H.plan(lib, 4, d, policy, xa, oa)["vec4"] == (xa and oa and d % 4 == 0), (d, xa, oa)
                    assert H.plan(lib, 4, d, policy, xa, oa) == rule(4, d, policy, xa, oa)


def test_empty_calls_and_bad_arguments(lib):
    for n, d in ((0, 4096), (5, 0), (0, 0)):
        for policy in (L, T, TH):
            assert H.plan(lib, n, d, policy)["front"] == H.NONE
            assert H.plan(lib, n, d, policy) == rule(n, d, policy)
    buf = (ctypes.c_int64 * len(H.FIELDS))()
    k = len(H.FIELDS)
    assert lib.uq_test_biased_plan(65536, 4096, T, 1, 1, buf, k) == -1            # UQ_E_INVALID, as the entry point
    assert lib.uq_test_biased_plan(65535, 4096, T, 1, 1, buf, k) == 0
    assert lib.uq_test_biased_plan(1, 1 << 31, T, 1, 1, buf, k) == -1
    assert lib.uq_test_biased_plan(-1, 4096, T, 1, 1, buf, k) == -1
    assert lib.uq_test_biased_plan(1, -1, T, 1, 1, buf, k) == -1
    for policy in (2, 3, 6, 8, -1):
        assert lib.uq_test_biased_plan(1, 4096, policy, 1, 1, buf, k) == -1, policy
    assert lib.uq_test_biased_plan(1, 4096, T, 1, 1, None, k) == -1
    assert lib.uq_test_last_biased_plan(None, k) == -1
    assert lib.uq_type_biased_f32(None, None, 65536, 4096, 1, 1, T, None, None, None, 0, None) == -1
    assert lib.uq_type_biased_f32(None, None, 1, 1 << 31, 1, 1, T, None, None, None, 0, None) == -1
    assert lib.uq_type_biased_f32(None, None, 1, 4096, 1, 1, 2, None, None, None, 0, None) == -1
    assert lib.uq_type_biased_f32(None, None, 1, 4096, 1, 1, T, None, None, None, 0, None) == -1      # null x / out
    assert lib.uq_test_last_biased_plan(buf, k) == 0 and buf[0] == H.NONE         # a refused call launched nothing
    buf[1] = 77
    assert lib.uq_test_biased_plan(4, 32768, L, 1, 1, buf, 1) == 0 and (buf[0], buf[1]) == (H.FULL, 77)   # cap respected


# uq_biased_workspace_bytes (n, d, T) of every shape above, as the library gave them before the
# layout read its sizes from the plan
WORKSPACE = {
    (1, 1048576, 1): 17488128, (1, 1048576, 3): 17487872,
    (1, 2097155, 1): 34938880, (1, 2097155, 3): 34938880,
    (1, 4194304, 1): 69838080, (1, 4194304, 3): 69837824,
    (4, 32767, 1): 2323712, (4, 32767, 3): 2323712,
    (4, 32768, 1): 2324224, (4, 32768, 3): 2324224,
    (8, 32767, 1): 4643840, (8, 32767, 3): 4643840,
    (16, 131087, 1): 35467008, (16, 131087, 3): 35464960,
    (16, 131088, 1): 35467008, (16, 131088, 3): 35464960,
    (16, 1048576, 1): 279761920, (16, 1048576, 3): 279757824,
    (17, 131088, 1): 37683456, (17, 131088, 3): 37681408,
    (31, 8193, 1): 5694976, (31, 8193, 3): 5694976,
    (31, 2097151, 1): 1082981376, (31, 2097151, 3): 1082981376,
    (31, 2097152, 1): 1082985216, (31, 2097152, 3): 1082981376,
    (32, 8193, 1): 5878784, (32, 8193, 3): 5878784,
    (64, 32767, 1): 37131264, (64, 32767, 3): 37131264,
    (65, 32767, 1): 37712640, (65, 32767, 3): 37712640,
    (1024, 8192, 1): 85684480, (1024, 8192, 3): 85684480,
    (1024, 1048576, 1): 5018046720, (1024, 1048576, 3): 5017784576,
}


def test_workspace_sizes_unchanged(lib):
    shapes = sorted({(n, d) for n, d, _, _ in ROWS})
    assert sorted({k[:2] for k in WORKSPACE}) == shapes
    for (n, d, t), want in WORKSPACE.items():
        b = ctypes.c_size_t()
        assert lib.uq_biased_workspace_bytes(n, d, t, ctypes.byref(b)) == 0
        assert b.value == want, (n, d, t)
