"""CPU: `bench.py --gpus N` starting its own N ranks (spawn_ranks) and the launcher check
(world_from_env), with a stub worker in place of the GPU bench: the ranks get the
torch.distributed.run environment (a real gloo all_reduce over it), rank 0's JSON line is
forwarded, and a failing rank makes the launch fail without leaving its peers behind."""
import io
import json
import os
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = r'''
import json, os, sys, time
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
mode = sys.argv[1]
if mode == "fail" and rank == 1:
    sys.exit(3)
if mode == "fail":
    time.sleep(600)                  # a peer blocked forever (e.g. in a collective)
import torch, torch.distributed as dist
sys.path.insert(0, sys.argv[2])
import bench
dist.init_process_group("gloo")
t = torch.tensor([float(rank + 1)])
dist.all_reduce(t)
print(f"rank {rank} says hello")     # non-zero ranks: must not reach the forwarded stdout
probe = {"k2_ms": [1.7 + rank, 1.9 + rank], "k2_ms_chosen": 1.7 + rank, "k2_ms_median_unprobed": 1.8 + rank}
per_rank = bench.gather_per_rank(dist, rank, bench.rank_record(rank, int(os.environ["LOCAL_RANK"]),
                                                                [0.5, 1.7 + rank, 0.3, 0.01], probe, 0.05 * (rank + 1)))
if rank == 0:
    print(json.dumps({"n_gpus": world, "sum": t.item(), "local": int(os.environ["LOCAL_RANK"]),
                      "addr": os.environ["MASTER_ADDR"], "per_rank": per_rank}))
else:
    assert per_rank is None
dist.destroy_process_group()
'''


@pytest.fixture()
def stub(tmp_path):
    p = tmp_path / "stub.py"
    p.write_text(STUB)
    return str(p)


def test_spawn_ranks_forwards_rank0_json(stub):
    out = io.StringIO()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    rc = bench.spawn_ranks(3, [sys.executable, stub, "ok", ROOT], env=env, out=out)
    assert rc == 0
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    per_rank = j.pop("per_rank")
    assert j == {"n_gpus": 3, "sum": 6.0, "local": 0, "addr": "127.0.0.1"}
    # every rank's own K2 time, probe and spread on rank 0's line, in rank order
    assert [r["rank"] for r in per_rank] == [0, 1, 2] and [r["local_rank"] for r in per_rank] == [0, 1, 2]
    assert [r["quantize_ms"] for r in per_rank] == [1.7, 2.7, 3.7]
    assert [r["quantize_ms_median_unprobed"] for r in per_rank] == [1.8, 2.8, 3.8]
    assert all(r["probe_spread_ms"] == 0.2 for r in per_rank)
    assert [r["elapsed_s"] for r in per_rank] == [0.05, 0.1, 0.15]
    assert "rank 1 says hello" not in out.getvalue() and "rank 2 says hello" not in out.getvalue()


def test_spawn_ranks_fails_when_a_rank_fails(stub):
    out = io.StringIO()
    rc = bench.spawn_ranks(3, [sys.executable, stub, "fail", ROOT], out=out, grace_s=1.0)
    assert rc == 1


def test_plain_run_is_the_default():
    args = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert args.full is False and args.dump_outputs is None and args.steps == 3 and args.warmup == 1
    args = bench.parse(["--full", "--dump-outputs", "out"])
    assert args.full is True and args.dump_outputs == "out"


def test_dump_outputs_files(tmp_path, monkeypatch):
    """--dump-outputs on a stand-in pipeline with host tensors: float32 files, small outputs
    whole, large ones as the same seeded sample in every run."""
    import types

    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    n, d = 8, 4096
    g = torch.Generator().manual_seed(3)
    q = torch.randn(n, d, generator=g)
    pipe = types.SimpleNamespace(
        q=q, l1=q.abs().sum(1), kmax=torch.arange(n, dtype=torch.int32), codes=None,
        nib=torch.randint(0, 256, (n, d // 2), generator=g, dtype=torch.uint8))
    est = q.mean(0)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), pipe, est, "codes4", 1234)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["codes_sample.npy", "est.npy", "kmax.npy", "l1.npy", "q_first.npy", "q_sample.npy"]
    for nm in names:
        a, b = np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)
        assert a.dtype == np.float32 and np.array_equal(a, b), nm
    assert np.array_equal(np.load(tmp_path / "a" / "est.npy"), est.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "q_first.npy"), q[0].numpy())
    idx = np.sort(np.random.default_rng(1234).integers(0, n * d, size=1000, dtype=np.int64))
    assert np.array_equal(np.load(tmp_path / "a" / "q_sample.npy"), q.numpy().reshape(-1)[idx])
    cs = np.load(tmp_path / "a" / "codes_sample.npy")
    assert cs.shape == (1000,) and cs.min() >= 0 and cs.max() <= 255
    # an encode-only step has no q; a q-only step no codes; ranks of a larger world name their files
    bench.dump_outputs(str(tmp_path / "c"), pipe, None, "q", 1234, rank=1, world=2)
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == ["l1_rank1.npy", "q_first_rank1.npy",
                                                                 "q_sample_rank1.npy"]


def test_world_must_match_gpus(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    args = bench.parse(["--gpus", "8"])
    with pytest.raises(SystemExit):
        bench.world_from_env(args)
    args = bench.parse([])
    assert bench.world_from_env(args) == 2 and args.gpus == 2
    monkeypatch.delenv("WORLD_SIZE")
    args = bench.parse([])
    assert bench.world_from_env(args) == 1 and args.gpus == 1
