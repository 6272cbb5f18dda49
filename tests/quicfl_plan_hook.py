"""Test infrastructure: the QUIC-FL dispatch plan (uq_test_quicfl_plan, uq_test_last_quicfl_plan
in include/uq_dme.h) as a dict."""
import ctypes

FIELDS = ("form", "R", "L", "two_wave", "force_timeout", "side")
SENDER, RECEIVER = 0, 1
NONE, ONE_WAVE, TEAM, JUMP = range(4)
SIDE_NONE, SIDE_PASS_A, SIDE_JUMP = range(3)          # nothing, KQ1a, KQ0s + KQ0j + KQ1ar


def _as_dict(buf):
    p = dict(zip(FIELDS, (int(v) for v in buf)))
    p["two_wave"], p["force_timeout"] = bool(p["two_wave"]), bool(p["force_timeout"])
    return p


def plan(lib, side, n, D, hooks=0, has_ws=True):
    """The plan of a call of this side and shape (D: the padded dimension), host only."""
    buf = (ctypes.c_int64 * len(FIELDS))()
    assert lib.uq_test_quicfl_plan(side, n, D, hooks, int(has_ws), buf, len(FIELDS)) == 0
    return _as_dict(buf)


def last_plan(lib, side):
    """The plan of this thread's last call of that side."""
    buf = (ctypes.c_int64 * len(FIELDS))()
    assert lib.uq_test_last_quicfl_plan(side, buf, len(FIELDS)) == 0
    return _as_dict(buf)
