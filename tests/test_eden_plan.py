"""The EDEN / RHT dispatch table (host only: uq_test_eden_plan launches nothing).

Every uq_eden_* and uq_rht_f32 call, and QUIC-FL's RHT front and inverse, computes one plan
(eden_plan, csrc/uq_eden.hip) from (op, n, dim, nbits, norm mode) and launches what it names;
the hook reports the same plan.  Both sides of each threshold are pinned twice: against rows
derived by hand from the rule, and against `rule`, a restatement of it that shares nothing
with the library."""
import ctypes

import pytest

import uqdme
from tests import eden_plan_hook as H

SEG_NORM_MAX_N, SEG_DOT_MAX_N, SEG_MIN_D, CHUNK = 256, 128, 16384, 2048
TRANSFORMS = (H.COMPRESS, H.DECOMPRESS, H.RHT_FORWARD, H.RHT_INVERSE, H.QFL_FRONT, H.QFL_INVERSE)


@pytest.fixture(scope="module")
def lib():
    return uqdme.load_library()


def rule(op, n, dim, nbits=1, mode=0):
    """What a call of this op and shape runs, restated from the dispatch rules."""
    p = 0 if dim <= 1 else (dim - 1).bit_length()
    D = dim if op == H.NORM else 1 << p
    pow2 = D >= 1 and D & (D - 1) == 0
    seg = 1 <= n <= SEG_NORM_MAX_N and pow2 and D >= SEG_MIN_D
    out = dict(D=D, p=p, norm=H.NO_NORM, dot=H.NO_DOT, first_bits=0, passes=[], unused=[0] * 16, copy_back=False,
               seg_tab_cap=min(256, max(32, D // 512)) if seg else 0)
    if n == 0 or dim == 0:
        return out
    chains = H.CHAINS_WHOLE if D % CHUNK == 0 else H.CHAINS_GENERIC
    if op == H.COMPRESS:
        if not seg and nbits == 1 and D % CHUNK == 0:
            out.update(norm=H.FUSED_NORM, dot=H.FUSED_REDO)
        else:
            out.update(norm=H.SEG_NORM if seg else chains, dot=H.SEG_DOT if seg and n <= SEG_DOT_MAX_N else H.ONE_WAVE)
    elif op == H.QFL_FRONT:
        out["norm"] = H.SEG_NORM if seg else chains
    elif op == H.NORM:
        out["norm"] = {0: H.SEG_NORM if seg else chains, 1: chains, 2: H.SEG_NORM if seg else H.NO_NORM}[mode]
        return out
    first = 14 if p == 22 and op != H.RHT_INVERSE else 12
    lo = 0
    while True:
        k = min(p - lo, 8 if lo else first)
        last, cols = lo + k >= p, D >> k
        if lo == 0 and k == 14 and not last:
            s = (H.LOW16K, D >> 14)
        elif lo == 0 and k == 12:                          # (the receiver's D % 16 == 0 always holds at D >= 4096)
            s = (H.LOW4096, D >> 12)
        elif lo > 0 and k == 8 and (1 << lo) % 64 == 0:    # (passes after the first are plain)
            s = (H.HIGH256, cols // 64)
        elif lo > 0 and k <= 6 and n * (cols // 256) >= 1024:
            s = (H.SMALL, -(-cols // 256))
        else:
            s = (H.GENERIC, cols if lo == 0 else cols // 32)
        out["passes"].append((lo, k, *s))
        lo += k
        if lo >= p:
            break
    out["first_bits"] = first
    out["unused"] = [0] * (16 - 4 * len(out["passes"]))
    out["copy_back"] = op == H.RHT_FORWARD and len(out["passes"]) % 2 == 1
    return out


C, DE, F, I, N, QF, QI = H.COMPRESS, H.DECOMPRESS, H.RHT_FORWARD, H.RHT_INVERSE, H.NORM, H.QFL_FRONT, H.QFL_INVERSE
LOW, HIGH = H.LOW4096, H.HIGH256
ROWS = [        # (op, n, dim, nbits, mode, expected fields), derived by hand
    # the segmented norm: 1 <= n <= 256, D a power of two >= 2^14; its dot up to 128 clients
    (C, 256, 1 << 14, 1, 0, dict(norm=H.SEG_NORM, dot=H.ONE_WAVE, seg_tab_cap=32)),
    (C, 257, 1 << 14, 1, 0, dict(norm=H.FUSED_NORM, dot=H.FUSED_REDO, seg_tab_cap=0)),
    (C, 128, 1 << 14, 1, 0, dict(norm=H.SEG_NORM, dot=H.SEG_DOT)),
    (C, 129, 1 << 14, 1, 0, dict(norm=H.SEG_NORM, dot=H.ONE_WAVE)),
    (C, 129, 1 << 14, 2, 0, dict(norm=H.SEG_NORM, dot=H.ONE_WAVE)),
    (C, 1, 1 << 13, 1, 0, dict(norm=H.FUSED_NORM, dot=H.FUSED_REDO)),
    (C, 1, 1 << 13, 2, 0, dict(norm=H.CHAINS_WHOLE, dot=H.ONE_WAVE)),
    (C, 1, 1 << 14, 1, 0, dict(norm=H.SEG_NORM, dot=H.SEG_DOT)),
    (C, 1, (1 << 13) + 1, 1, 0, dict(D=1 << 14, norm=H.SEG_NORM, dot=H.SEG_DOT)),          # the padded D decides
    # fused KE2+4: not segmented, 1 bit, D a multiple of 2048
    (C, 257, 1 << 14, 2, 0, dict(norm=H.CHAINS_WHOLE, dot=H.ONE_WAVE)),
    (C, 257, 1024, 1, 0, dict(norm=H.CHAINS_GENERIC, dot=H.ONE_WAVE)),
    (C, 257, 2048, 1, 0, dict(norm=H.FUSED_NORM, dot=H.FUSED_REDO)),
    (C, 1024, 1 << 20, 1, 0, dict(norm=H.FUSED_NORM, dot=H.FUSED_REDO, passes=[(0, 12, LOW, 256), (12, 8, HIGH, 64)])),
    (C, 101, 1 << 22, 1, 0, dict(norm=H.SEG_NORM, dot=H.SEG_DOT, seg_tab_cap=256, first_bits=14)),
    (QF, 4, 1 << 20, 0, 0, dict(norm=H.SEG_NORM, dot=H.NO_DOT, passes=[(0, 12, LOW, 256), (12, 8, HIGH, 64)])),
    (QF, 300, 1 << 14, 0, 0, dict(norm=H.CHAINS_WHOLE, dot=H.NO_DOT)),                     # (never fused: no bins)
    (QF, 300, 1000, 0, 0, dict(norm=H.CHAINS_GENERIC, D=1024)),
    (DE, 4, 1 << 20, 1, 0, dict(norm=H.NO_NORM, dot=H.NO_DOT, passes=[(0, 12, LOW, 256), (12, 8, HIGH, 64)])),
    # pass lists: 12 bits first (14 at p = 22), then 8 at most each
    (F, 1, 1 << 11, 0, 0, dict(passes=[(0, 11, H.GENERIC, 1)], copy_back=True)),
    (F, 1, 1 << 12, 0, 0, dict(passes=[(0, 12, LOW, 1)], copy_back=True)),
    (F, 1, 1 << 13, 0, 0, dict(passes=[(0, 12, LOW, 2), (12, 1, H.GENERIC, 128)], copy_back=False)),
    (F, 1, 1 << 19, 0, 0, dict(passes=[(0, 12, LOW, 128), (12, 7, H.GENERIC, 128)], copy_back=False)),
    (F, 1, 1 << 20, 0, 0, dict(passes=[(0, 12, LOW, 256), (12, 8, HIGH, 64)], copy_back=False)),
    (F, 1, (1 << 21) - 5, 0, 0, dict(D=1 << 21, copy_back=True,
                                     passes=[(0, 12, LOW, 512), (12, 8, HIGH, 128), (20, 1, H.SMALL, 4096)])),
    (F, 1, (1 << 22) - 5, 0, 0, dict(first_bits=14, passes=[(0, 14, H.LOW16K, 256), (14, 8, HIGH, 256)], copy_back=False)),
    (F, 1, 1 << 23, 0, 0, dict(passes=[(0, 12, LOW, 2048), (12, 8, HIGH, 512), (20, 3, H.SMALL, 4096)], copy_back=True)),
    (F, 1, 1 << 28, 0, 0, dict(passes=[(0, 12, LOW, 1 << 16), (12, 8, HIGH, 1 << 14), (20, 8, HIGH, 1 << 14)],
                               copy_back=True)),
    (DE, 3, 1 << 22, 2, 0, dict(first_bits=14, passes=[(0, 14, H.LOW16K, 256), (14, 8, HIGH, 256)])),
    (QI, 4, 1 << 22, 0, 0, dict(first_bits=14, passes=[(0, 14, H.LOW16K, 256), (14, 8, HIGH, 256)])),
    # uq_rht_f32's inverse keeps 12 bits at p = 22
    (I, 2, 1 << 22, 0, 0, dict(first_bits=12, copy_back=False,
                               passes=[(0, 12, LOW, 1024), (12, 8, HIGH, 256), (20, 2, H.SMALL, 4096)])),
    (I, 2, 1 << 21, 0, 0, dict(passes=[(0, 12, LOW, 512), (12, 8, HIGH, 128), (20, 1, H.SMALL, 4096)])),
    (I, 2, 1 << 12, 0, 0, dict(passes=[(0, 12, LOW, 1)], copy_back=False)),
    # a short pass: a thread per column from 1024 workgroups on (p = 13: k = 1, 16 per client)
    (C, 63, 1 << 13, 2, 0, dict(passes=[(0, 12, LOW, 2), (12, 1, H.GENERIC, 128)])),
    (C, 64, 1 << 13, 2, 0, dict(passes=[(0, 12, LOW, 2), (12, 1, H.SMALL, 16)])),
    # the norm entry's modes (D as given, not padded)
    (N, 4, 1 << 14, 0, 0, dict(norm=H.SEG_NORM, passes=[], seg_tab_cap=32)),
    (N, 4, 1 << 14, 0, 1, dict(norm=H.CHAINS_WHOLE, seg_tab_cap=32)),
    (N, 4, 1 << 14, 0, 2, dict(norm=H.SEG_NORM)),
    (N, 257, 1 << 14, 0, 0, dict(norm=H.CHAINS_WHOLE, seg_tab_cap=0)),
    (N, 257, 1 << 14, 0, 2, dict(norm=H.NO_NORM)),                                          # refused by the entry
    (N, 4, 20000, 0, 0, dict(D=20000, norm=H.CHAINS_GENERIC)),
    (N, 4, 20480, 0, 0, dict(D=20480, norm=H.CHAINS_WHOLE)),
    (N, 4, 20480, 0, 2, dict(norm=H.NO_NORM)),
]


@pytest.mark.parametrize("op,n,dim,nbits,mode,want", ROWS)
def test_rows(lib, op, n, dim, nbits, mode, want):
    p = H.plan(lib, op, n, dim, nbits, mode)
    for key, v in want.items():
        assert p[key] == v, (op, n, dim, nbits, mode, key, p)
    assert p == rule(op, n, dim, nbits, mode), (op, n, dim, nbits, mode)


def test_both_sides_of_every_threshold(lib):
    """Every (n, dim) pair of the thresholds' neighbours, every op, against the restated rule."""
    ns = [1, 2, 63, 64, 127, 128, 129, 255, 256, 257, 1023, 1024, 65535]
    dims = [1, 2, 3, 1000, 1024, 2047, 2048, 2049, 4095, 4096, 4097, 1 << 13, (1 << 13) + 1, 1 << 14, (1 << 14) + 1,
            1 << 17, 1 << 18, 1 << 19, 1 << 20, (1 << 21) - 5, 1 << 21, (1 << 22) - 3, 1 << 22, (1 << 22) + 1, 1 << 23,
            1 << 27, 1 << 28]
    for n in ns:
        for dim in dims:
            for op in TRANSFORMS:
                for nbits in (1, 2) if op == H.COMPRESS else (1,):
                    assert H.plan(lib, op, n, dim, nbits) == rule(op, n, dim, nbits), (op, n, dim, nbits)
            for mode in (0, 1, 2):
                assert H.plan(lib, N, n, dim, 0, mode) == rule(N, n, dim, 0, mode), (n, dim, mode)


def test_pass_lists_cover_every_bit_once(lib):
    for p in range(0, 29):
        for op in TRANSFORMS:
            for n in (1, 70, 2000):
                pl = H.plan(lib, op, n, 1 << p)
                assert (pl["D"], pl["p"]) == (1 << p, p) and 1 <= len(pl["passes"]) <= 3
                lo = 0
                for s_lo, k, kern, gx in pl["passes"]:
                    assert s_lo == lo and gx >= 1 and kern in range(1, 6)
                    lo += k
                assert lo == p, (op, n, p, pl)
                assert pl["first_bits"] == (14 if p == 22 and op != I else 12)
                assert pl["copy_back"] == (op == F and len(pl["passes"]) % 2 == 1)


def test_empty_calls_and_bad_arguments(lib):
    for n, dim in ((0, 4096), (5, 0), (0, 0)):
        for op in range(7):
            p = H.plan(lib, op, n, dim)
            assert (p["norm"], p["dot"], p["passes"]) == (H.NO_NORM, H.NO_DOT, [])
            assert p == rule(op, n, dim)
    k = H.NFIELDS
    buf = (ctypes.c_int64 * k)()
    assert lib.uq_test_eden_plan(7, 1, 4096, 1, 0, buf, k) == -1                  # UQ_E_INVALID
    assert lib.uq_test_eden_plan(-1, 1, 4096, 1, 0, buf, k) == -1
    assert lib.uq_test_eden_plan(C, -1, 4096, 1, 0, buf, k) == -1
    assert lib.uq_test_eden_plan(C, 1, -1, 1, 0, buf, k) == -1
    assert lib.uq_test_eden_plan(N, 1, 4096, 1, 3, buf, k) == -1
    assert lib.uq_test_eden_plan(C, 1, 4096, 1, 0, None, k) == -1
    assert lib.uq_test_last_eden_plan(C, None, k) == -1
    assert lib.uq_test_last_eden_plan(7, buf, k) == -1
    # refused calls launched nothing: no passes, no forms
    assert lib.uq_eden_compress_f32(None, 1, 16, 3, None, None, None, None, None, 0, None) == -1
    assert lib.uq_eden_f32(None, None, 4, 4096, 1, None, None, None, None, 0, None) == -1           # null signs
    assert lib.uq_rht_f32(None, None, 1, 16, 0, None, None, None, 0, None) == -1
    assert lib.uq_eden_norm_f32(None, 1, 4096, 0, None, None, 0, None) == -1
    for op in (C, DE, F, N):
        p = H.last_plan(lib, op)
        assert (p["norm"], p["dot"], p["passes"]) == (H.NO_NORM, H.NO_DOT, []), op
    buf[1] = 77
    assert lib.uq_test_eden_plan(C, 4, 1 << 20, 1, 0, buf, 1) == 0 and (buf[0], buf[1]) == (1 << 20, 77)   # cap respected


# uq_eden_workspace_bytes, uq_eden_norm_workspace_bytes, uq_quicfl_workspace_bytes and
# uq_quicfl_receive_workspace_bytes at NS x DS (n-major), as the library gave them before the
# layouts read the plan
NS = (1, 128, 129, 256, 257, 1024)
DS = (1000, 1 << 13, 1 << 14, 1 << 20, (1 << 22) - 3, 1 << 22)
WORKSPACE = {
    "uq_eden_workspace_bytes": [
        6144, 41984, 220160, 6621952, 23333632, 23333632,
        657152, 5244672, 27971840, 847417600, 2986512640, 2986512640,
        663040, 5286400, 28191744, 854039296, 3009846016, 3009846016,
        1314048, 10489088, 55943424, 1694834944, 5973025024, 5973025024,
        1319936, 10530816, 21057536, 1347424256, 5389684736, 5389684736,
        5255424, 41955584, 83898624, 5368721664, 21474849024, 21474849024,
    ],
    "uq_eden_norm_workspace_bytes": [
        0, 0, 137216, 1378048, 0, 2361088,
        0, 0, 17484288, 176327168, 0, 302156288,
        0, 0, 17621504, 177705216, 0, 304517376,
        0, 0, 34968576, 352654336, 0, 604312576,
        0, 0, 0, 0, 0, 0,
        0, 0, 0, 0, 0, 0,
    ],
    "uq_quicfl_workspace_bytes": [
        9664, 634352, 1210200, 13437784, 38897712, 38897712,
        1107712, 6612736, 30388480, 1064079616, 3605827840, 3605827840,
        1117120, 6665152, 30627264, 1068529144, 3630134776, 3630134776,
        2215168, 13225216, 60776704, 2066800896, 7150297344, 7150297344,
        2224576, 13277632, 25909696, 1713143480, 6563856056, 6563856056,
        8859904, 52900096, 103231744, 6672511232, 25999864064, 25999864064,
    ],
    "uq_quicfl_receive_workspace_bytes": [
        0, 0, 0, 2190680, 4039200, 4039200,
        0, 0, 0, 31006720, 31006720, 31006720,
        0, 0, 0, 29959992, 29959992, 29959992,
        0, 0, 0, 41549824, 41549824, 41549824,
        0, 0, 0, 39144184, 39144184, 39144184,
        0, 0, 0, 104808448, 104808448, 104808448,
    ],
}


def test_workspace_sizes_unchanged(lib):
    for fn, want in WORKSPACE.items():
        got = []
        for n in NS:
            for d in DS:
                b = ctypes.c_size_t()
                assert getattr(lib, fn)(n, d, ctypes.byref(b)) == 0
                got.append(b.value)
        assert got == want, fn
