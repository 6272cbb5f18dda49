"""QUIC-FL's dispatch table (host only: uq_test_quicfl_plan launches nothing).

Each sender and receiver call computes one plan (qfl_plan, csrc/uq_quicfl.hip) from (side, n, D,
hooks, workspace) and launches what it names; the hook reports the same plan.  Both sides of each
threshold are pinned: the one-wave / team / jump split, the jump form's R and L, the two-wave
runs, and what the sender sends to the side stream.  D is the padded dimension."""
import ctypes

import pytest

import uqdme
from tests import quicfl_plan_hook as H

ONE_WAVE, TEAM, JUMP = H.ONE_WAVE, H.TEAM, H.JUMP
SIDE_OF = {ONE_WAVE: H.SIDE_PASS_A, TEAM: H.SIDE_NONE, JUMP: H.SIDE_JUMP}


@pytest.fixture(scope="module")
def lib():
    return uqdme.load_library()


def check(lib, side, n, D, form, R=None, L=None, two_wave=None, hooks=0, has_ws=True):
    p = H.plan(lib, side, n, D, hooks, has_ws)
    assert p["form"] == form, (side, n, D, hooks, p)
    assert p["force_timeout"] == bool(hooks & 1), p
    assert p["side"] == (SIDE_OF[form] if side == H.SENDER else H.SIDE_NONE), p
    if form != JUMP:
        assert (p["R"], p["L"], p["two_wave"]) == (0, 0, False), p
    else:
        assert p["R"] >= 1 and p["R"] * p["L"] >= -(-D // 624) > (p["R"] - 1) * p["L"], p     # the runs cover the rounds
        assert p["two_wave"] == (n * p["R"] > 1024) and n * p["R"] <= 2048, p
    for key, v in (("R", R), ("L", L), ("two_wave", two_wave)):
        assert v is None or p[key] == v, (side, n, D, key, p)
    return p


SENDER = [
    (1, 2048, ONE_WAVE, {}), (1, 4096, TEAM, {}), (256, 4096, TEAM, {}), (257, 4096, ONE_WAVE, {}),
    (1, 8192, JUMP, dict(R=14, L=1)), (4, 8192, JUMP, dict(R=7, L=2)), (128, 32768, JUMP, dict(R=3, L=18)),
    (129, 32768, TEAM, {}), (257, 32768, ONE_WAVE, {}), (257, 65536, JUMP, dict(R=3, L=36, two_wave=False)),
    (342, 131072, JUMP, dict(R=4, L=53, two_wave=True)), (150, 1 << 18, JUMP, {}), (151, 1 << 18, TEAM, {}),
    (256, 1 << 18, TEAM, {}), (257, 1 << 18, JUMP, dict(R=7, L=61, two_wave=True)), (934, 1 << 18, JUMP, {}),
    (935, 1 << 18, ONE_WAVE, {}), (1024, 1 << 20, JUMP, dict(R=2, L=841, two_wave=True)), (1025, 1 << 20, ONE_WAVE, {}),
]
RECEIVER = [
    (1, 4096, ONE_WAVE, {}), (1, 8192, TEAM, {}), (1, 32768, JUMP, dict(R=27, L=2)), (8, 32768, TEAM, {}),
    (128, 65536, TEAM, {}), (257, 32768, ONE_WAVE, {}), (257, 65536, JUMP, dict(R=3, L=36)),
    (342, 131072, JUMP, dict(R=4, L=53, two_wave=True)), (170, 1 << 18, JUMP, {}), (171, 1 << 18, TEAM, {}),
    (257, 1 << 18, JUMP, {}), (1024, 1 << 18, JUMP, dict(R=2, L=211)), (1025, 1 << 18, ONE_WAVE, {}),
]


@pytest.mark.parametrize("n,D,form,kw", SENDER)
def test_sender_forms(lib, n, D, form, kw):
    check(lib, H.SENDER, n, D, form, **kw)


@pytest.mark.parametrize("n,D,form,kw", RECEIVER)
def test_receiver_forms_with_a_workspace(lib, n, D, form, kw):
    check(lib, H.RECEIVER, n, D, form, **kw)


def test_sender_under_the_hooks(lib):
    """Hook 2: the one-wave form for every shape.  Hook 4: the team kernel wherever it can run
    (n <= 256, 6 * 624 <= D <= 2^23), else the one-wave form, never the jump form.  Hook 1: as 4,
    with force_timeout."""
    shapes = [(n, D) for n, D, _, _ in SENDER] + [(300, 65536), (1, 1 << 24), (1, 1 << 23), (256, 3744), (1, 3743)]
    for n, D in shapes:
        check(lib, H.SENDER, n, D, ONE_WAVE, hooks=2)
        team = n <= 256 and 3744 <= D <= 1 << 23
        for hooks in (4, 1, 5):
            p = check(lib, H.SENDER, n, D, TEAM if team else ONE_WAVE, hooks=hooks)
            assert p["force_timeout"] == bool(hooks & 1)
        check(lib, H.SENDER, n, D, ONE_WAVE, hooks=3)                 # bit 1 wins over the others
    check(lib, H.SENDER, 300, 65536, ONE_WAVE, hooks=4)
    check(lib, H.SENDER, 1, 1 << 24, ONE_WAVE, hooks=4)


def test_receiver_without_a_workspace_and_under_the_hooks(lib):
    check(lib, H.RECEIVER, 1, 32768, TEAM, has_ws=False)
    check(lib, H.RECEIVER, 257, 65536, ONE_WAVE, has_ws=False)
    for n, D, _, _ in RECEIVER:
        team = n <= 256 and 7 * 624 <= D <= 1 << 23
        for hooks in (1, 4, 5):                                       # any hook: no jump form
            check(lib, H.RECEIVER, n, D, TEAM if team else ONE_WAVE, hooks=hooks)
        for hooks in (2, 3, 6, 7):
            check(lib, H.RECEIVER, n, D, ONE_WAVE, hooks=hooks)
    check(lib, H.RECEIVER, 1, 4367, ONE_WAVE, hooks=4)                # the team kernel's 7 runs of one round
    check(lib, H.RECEIVER, 1, 4368, TEAM, hooks=4)


def test_workspace_sizes_follow_the_plan(lib):
    """The receiver's workspace is the jump form's region (streams, R blocks and run records per
    message), 0 without it, whatever the hooks say."""
    for n, D, form, _ in RECEIVER:
        b = ctypes.c_size_t()
        assert lib.uq_quicfl_receive_workspace_bytes(n, D, ctypes.byref(b)) == 0
        p = H.plan(lib, H.RECEIVER, n, D, hooks=0)
        want = 4 * (n * 33 * 624 + n * p["R"] * (4 * 624 + 2)) if form == JUMP else 0
        assert b.value == want, (n, D)


def test_empty_calls_and_bad_arguments(lib):
    assert H.plan(lib, H.SENDER, 0, 4096)["form"] == H.NONE and H.plan(lib, H.RECEIVER, 5, 0)["form"] == H.NONE
    buf = (ctypes.c_int64 * 6)()
    assert lib.uq_test_quicfl_plan(2, 1, 4096, 0, 1, buf, 6) == -1                # UQ_E_INVALID
    assert lib.uq_test_quicfl_plan(0, -1, 4096, 0, 1, buf, 6) == -1
    assert lib.uq_test_quicfl_plan(0, 1, 4096, 0, 1, None, 6) == -1
    assert lib.uq_test_last_quicfl_plan(3, buf, 6) == -1
    buf[1] = 77
    assert lib.uq_test_quicfl_plan(0, 1, 8192, 0, 1, buf, 1) == 0 and (buf[0], buf[1]) == (JUMP, 77)   # cap respected
