"""GPU: uq_randperm_prefix at batch scale -- the branches of its plan that only a large n B reaches (B the MT19937
blocks a client's stream may touch): a run length set by the batch with a short last run, L = B (one run, no
jump taken), the 1024-run limit, a jump-form batch processed in client groups that reuse the workspace, and the
1 GiB cap of the default workspace.  Every case asserts the plan it was written for against the NumPy port
(tests/randperm_model.py: plan, group) and compares every row bit for bit with torch.randperm on the CPU.
The client states tile 4 generator states, so the reference is 4 CPU permutations and no host jump is paid."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import randperm_model as M

pytestmark = pytest.mark.gpu

# (seed, pre-draws): freshly seeded (left = 1), mid-block, at next = 623 (one word left), in the second block
STARTS = ((101, 0), (202, 300), (303, 623), (404, 1000))


def generator(seed, pre):
    g = torch.Generator()
    g.manual_seed(seed)
    for _ in range(pre):
        torch.randint(0, 100, (1,), generator=g)
    return g


@pytest.fixture(scope="module")
def rp(gpu_ready):
    import uqdme  # noqa: F401
    from uqdme_amd import randperm
    return randperm


@pytest.fixture(scope="module")
def states(rp):
    from uqdme_amd import _mtstate
    s = np.stack([_mtstate.generator_words(generator(*a))[1] for a in STARTS])
    for r in s:
        _mtstate.check_state(r)
    assert [(int(r[0]), int(r[1])) for r in s] == [(1, 0), (325, 300), (2, 623), (249, 376)]     # (left, next)
    return s


_refs = {}


def references(D, k):
    """torch.randperm(D)[:k] from each of the 4 states, on the CPU (computed once per shape, never changed)."""
    if (D, k) not in _refs:
        _refs[(D, k)] = torch.stack([torch.randperm(D, generator=generator(*a))[:k] for a in STARTS])
    return _refs[(D, k)]


def one_client_bytes(D, k):
    import uqdme
    one = ctypes.c_size_t(0)
    assert uqdme.load_library().uq_randperm_prefix_workspace_bytes(1, D, k, ctypes.byref(one)) == 0
    return one.value


def run(rp, states, n, D, k, *, workspace_bytes, group, groups, index=True, bits=True, shift=0):
    """One call on the tiled states; asserts the plan and every row; -> seconds of the call."""
    from uqdme_amd import _runtime
    dev = _runtime.device()
    sel = (np.arange(n) + shift) % 4
    sd = torch.from_numpy(np.ascontiguousarray(states[sel]).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx, bt = rp.prefix_from_states(sd, n, D, k, dev, index=index, bits=bits, workspace_bytes=workspace_bytes)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    plan = rp.last_plan()
    form, R, L, K = M.plan(n, D, k)
    assert (plan["form"], plan["runs"], plan["run_blocks"], plan["K"]) == (form, R, L, K), plan
    assert (plan["group"], plan["groups"]) == (group, groups), plan
    ref = references(D, k)
    for s in range(4):
        rows = slice((s - shift) % 4, n, 4)                   # the clients that start from state s
        if index:
            got = idx[rows]
            assert got.shape[0] == len(range(n)[rows])
            bad = (got != ref[s].to(dev)).any(dim=1)
            assert not bool(bad.any()), (n, D, k, "index rows of state", s, torch.nonzero(bad).flatten()[:8].tolist())
        if bits:
            want = torch.from_numpy(M.drop_bits(ref[s].numpy(), D).view(np.int32)).to(dev)
            bad = (bt[rows] != want).any(dim=1)
            assert not bool(bad.any()), (n, D, k, "drop bits of state", s, torch.nonzero(bad).flatten()[:8].tolist())
    return dt


# n, D, k -> the plan's (R, L) and the (group, groups) of a workspace of 64 single clients' worth
GROUPED = (
    ((2500, 20000, 20000), (2, 21), (65, 39)),        # L set by the batch: runs of 21 and 13 blocks; last group of 30
    ((4096, 20000, 20000), (1, 34), (67, 62)),        # L = B: no jump taken; last group of 9
    ((5000, 20000, 10000), (1, 18), (66, 76)),        # L = B at k < D; last group of 50
    ((1300, 65536, 32768), (3, 18), (64, 21)),        # three runs of 18 blocks; last group of 20
)


@pytest.mark.parametrize("shape,runs,grouping", GROUPED)
def test_jump_form_in_client_groups(rp, states, shape, runs, grouping):
    """A private workspace of 64 single clients' worth: L follows the whole n, while xs / parts are reused group
    after group and the last group is short.  Index rows and drop bits of every client."""
    n, D, k = shape
    assert M.plan(n, D, k)[:3] == (M.JUMP, *runs)
    ws = 64 * one_client_bytes(D, k)
    group = M.group(n, D, k, ws)
    assert (group, -(-n // group)) == grouping and n % group != 0
    run(rp, states, n, D, k, workspace_bytes=ws, group=group, groups=grouping[1])


def test_one_run_whole_batch_in_one_group(rp, states):
    """L = B = 34 with every client in one launch: R = 1, all jump polynomials zero."""
    n, D, k = 4096, 20000, 20000
    assert M.plan(n, D, k)[:3] == (M.JUMP, 1, 34)
    run(rp, states, n, D, k, workspace_bytes=M.workspace_bytes(n, D, k, n), group=n, groups=1, shift=1)


def test_default_workspace_hits_its_cap(rp, states):
    """128 x 2^20, k = 2^19 on a stream's default workspace: uq_randperm_prefix_workspace_bytes stops at 1 GiB,
    which holds 98 clients, so the call runs groups of 98 and 30.  L = 27, 32 runs.  Drop bits only.
    The default workspace belongs to the (device, stream) and only grows, so on a stream that an earlier test
    left a larger one on the call would take one group: the call runs on a stream of its own, whose workspace
    is the one this call asks for, and that workspace is released afterwards."""
    import uqdme
    from uqdme_amd import _runtime
    n, D, k = 128, 1 << 20, 1 << 19
    assert M.plan(n, D, k)[:3] == (M.JUMP, 32, 27)
    b = ctypes.c_size_t(0)
    assert uqdme.load_library().uq_randperm_prefix_workspace_bytes(n, D, k, ctypes.byref(b)) == 0
    group = M.group(n, D, k, b.value)
    assert b.value <= M.WORKSPACE_CAP < M.workspace_bytes(n, D, k, group + 1) and b.value == M.workspace_bytes(n, D, k, group)
    assert group == 98
    dev = _runtime.device()
    side = torch.cuda.Stream(dev)
    key = (dev.index, side.cuda_stream)
    assert key not in _runtime._ws_cache
    try:
        with torch.cuda.stream(side):
            run(rp, states, n, D, k, workspace_bytes=None, group=group, groups=2, index=False)
            assert _runtime._ws_cache[key].numel() == b.value
    finally:
        torch.cuda.synchronize()
        _runtime._ws_cache.pop(key, None)


@pytest.mark.parametrize("D,runs,shift", ((10_223_000, (964, 17), 2), (10_222_000, (1024, 16), 0)))
def test_run_limit_boundary(rp, states, D, runs, shift):
    """n = 1, k = D on either side of the 1024 runs a client may have: B = 16385 blocks take 964 runs of 17, B = 16383
    take 1024 runs of 16.  The first call of a process also pays the host's progression of about 1000 jump
    polynomials; the call's time is printed (measured: see the commit message)."""
    assert M.plan(1, D, D)[:3] == (M.JUMP, *runs)
    dt = run(rp, states, 1, D, D, workspace_bytes=None, group=1, groups=1, bits=False, shift=shift)
    print(f"randperm_prefix(D = k = {D}, n = 1): R = {runs[0]}, L = {runs[1]}: {dt:.3f} s (first call of this plan)")


def test_consecutive_streams_at_n_40(rp):
    """n = 40 clients from a generator= (one host jump each): 40 successive torch.randperm calls, the generator
    left where they leave it; in groups of 7 clients."""
    n, D, k = 40, 20000, 20000
    g, t = generator(5, 17), generator(5, 17)
    refs = torch.stack([torch.randperm(D, generator=t)[:k] for _ in range(n)])
    ws = 7 * one_client_bytes(D, k)
    group = M.group(n, D, k, ws)
    got, bits = rp.randperm_prefix(D, k, n, generator=g, return_bits=True, workspace_bytes=ws)
    plan = rp.last_plan()
    assert (plan["form"], plan["runs"], plan["run_blocks"], plan["K"]) == M.plan(n, D, k) == (M.JUMP, 3, 16, D - 1), plan
    assert (plan["group"], plan["groups"]) == (group, -(-n // group)) and plan["groups"] > 1, plan
    assert torch.equal(got.cpu(), refs)
    assert torch.equal(g.get_state(), t.get_state())
    bits = bits.cpu().numpy().view(np.uint32)
    for j in (0, group - 1, group, n - 1):
        assert np.array_equal(bits[j], M.drop_bits(refs[j].numpy(), D)), j
