"""GPU: bench.py as a command at a small shape (256 clients x d = 2^15, the codes4 pipeline): a
plain run and a --full run print one result line each and dump the same outputs, and the dumped
arrays are what the library's one-shot API computes from the same seeded inputs, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, SEED = 256, 1 << 15, 4321


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--clients", str(N), "--dim", str(D), "--seed", str(SEED), "--probe-candidates", "2", "--probe-min", "2",
           *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(gpu_ready, tmp_path):
    import uqdme
    plain = run_bench("--dump-outputs", str(tmp_path / "plain"))
    full = run_bench("--full", "--dump-outputs", str(tmp_path / "full"))
    for j in (plain, full):
        assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["dtype"] == "f32"
        assert j["unit"] == "M-vectors/s" and j["higher_is_better"] is True
        # value and ms_per_step say the same thing (ms_per_step is printed to 1e-4 ms: <= 1 % here)
        assert j["value"] == pytest.approx(N / j["ms_per_step"] / 1e3, rel=1e-2)
        assert j["config"]["pipeline"] == "codes4"
    # the plain run measures nothing beside its headline; --full keeps every other leg
    assert plain["full"] is False and plain["pipelines"] == {}
    assert "cpu_baseline" not in plain and "parity_sample" not in plain
    assert full["full"] is True and full["parity_sample"]["bit_mismatches"] == 0
    assert full["parity_sample"]["clients_checked"] == N and full["cpu_baseline"]["value"] > 0
    assert {"q", "codes", "encode", "biased", "eden", "codec", "quicfl"} <= set(full["pipelines"])
    assert full["pipelines"]["codec"]["roundtrip_ok"] is True

    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == ["codes_sample.npy", "est.npy", "kmax.npy", "l1.npy", "q_first.npy", "q_sample.npy"]
    got = {}
    for nm in names:
        a, b = np.load(tmp_path / "plain" / nm), np.load(tmp_path / "full" / nm)
        assert a.dtype == np.float32 and a.shape == b.shape, nm
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), nm
        got[nm[:-4]] = a
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the same inputs as bench.py draws them, through the one-shot API
    g = torch.Generator(device="cuda").manual_seed(SEED)
    x = torch.randn(N, D, generator=g, device="cuda", dtype=torch.float32)
    X = torch.rand(N, generator=torch.Generator().manual_seed(SEED))
    q = uqdme.quantize_dequantize(x, 1, X=X, torch_threads=1)
    est = uqdme.client_mean(q, N).cpu().numpy()
    q = q.cpu().numpy()
    assert np.array_equal(got["est"].view(np.uint32), est.view(np.uint32))
    assert np.array_equal(got["q_first"].view(np.uint32), q[0].view(np.uint32))
    idx = np.sort(np.random.default_rng(SEED).integers(0, N * D, size=bench.DUMP_SAMPLE, dtype=np.int64))
    assert got["q_sample"].shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(got["q_sample"].view(np.uint32), q.reshape(-1)[idx].view(np.uint32))
    l1 = x.abs().sum(1, dtype=torch.float64).cpu().numpy()
    # an f32 sum of D terms in any order is within D * 2^-24 (relative) of the exact sum of |x|
    assert np.allclose(got["l1"], l1, rtol=D * 2.0 ** -24, atol=0)
    assert got["kmax"].min() >= 1 and got["kmax"].max() <= 127
    assert got["codes_sample"].min() >= 0 and got["codes_sample"].max() <= 255
