"""Test infrastructure: the EDEN / RHT dispatch plan (uq_test_eden_plan, uq_test_last_eden_plan
in include/uq_dme.h) as a dict."""
import ctypes

MAX_PASSES = 4
NFIELDS = 24
COMPRESS, DECOMPRESS, RHT_FORWARD, RHT_INVERSE, NORM, QFL_FRONT, QFL_INVERSE = range(7)
NO_NORM, CHAINS_WHOLE, CHAINS_GENERIC, SEG_NORM, FUSED_NORM = range(5)
NO_DOT, ONE_WAVE, SEG_DOT, FUSED_REDO = range(4)
LOW16K, LOW4096, HIGH256, SMALL, GENERIC = range(1, 6)


def _as_dict(buf):
    v = [int(t) for t in buf]
    return dict(D=v[0], p=v[1], norm=v[2], dot=v[3], first_bits=v[4],
                passes=[tuple(v[6 + 4 * i:10 + 4 * i]) for i in range(v[5])],       # (lo, k, kernel, grid x)
                unused=v[6 + 4 * v[5]:22], copy_back=bool(v[22]), seg_tab_cap=v[23])


def plan(lib, op, n, dim, nbits=1, mode=0):
    """The plan of a call of this op and shape, host only."""
    buf = (ctypes.c_int64 * NFIELDS)()
    assert lib.uq_test_eden_plan(op, n, dim, nbits, mode, buf, NFIELDS) == 0
    return _as_dict(buf)


def last_plan(lib, op):
    """The plan of this thread's last call of that op."""
    buf = (ctypes.c_int64 * NFIELDS)()
    assert lib.uq_test_last_eden_plan(op, buf, NFIELDS) == 0
    return _as_dict(buf)


def kernels(p):
    return [s[2] for s in p["passes"]]


def bits(p):
    return [s[1] for s in p["passes"]]
