"""Test infrastructure: the biased quantizer's dispatch plan (uq_test_biased_plan,
uq_test_last_biased_plan in include/uq_dme.h) as a dict."""
import ctypes

FIELDS = ("front", "ties", "replay", "levels", "lsplit", "lgrid", "S", "vec4", "cand_multi", "cspans", "cap", "capf",
          "tiles", "clear_bits", "ran")
BOOLS = ("vec4", "cand_multi", "clear_bits")
NONE, SMALL, SMALL_CHECKED, FULL = range(4)           # front
LOWEST, FORK, CHECKED = range(3)                      # ties: the tail after the selection
NO_REPLAY, ONE_KERNEL, LEVELS = range(3)              # replay
POLICY_TORCH, POLICY_LOWEST, HOST_CHECK = 0, 1, 4     # UQ_TIES_*


def _as_dict(buf):
    p = dict(zip(FIELDS, (int(v) for v in buf)))
    for k in BOOLS:
        p[k] = bool(p[k])
    return p


def plan(lib, n, d, policy, x_aligned=True, out_aligned=True):
    """The plan of a call of this shape and tie policy, host only."""
    buf = (ctypes.c_int64 * len(FIELDS))()
    assert lib.uq_test_biased_plan(n, d, policy, int(x_aligned), int(out_aligned), buf, len(FIELDS)) == 0
    return _as_dict(buf)


def last_plan(lib):
    """The plan of this thread's last uq_type_biased_f32 call; "ran": the host check's outcome."""
    buf = (ctypes.c_int64 * len(FIELDS))()
    assert lib.uq_test_last_biased_plan(buf, len(FIELDS)) == 0
    return _as_dict(buf)
