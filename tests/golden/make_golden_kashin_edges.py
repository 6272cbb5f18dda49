"""Golden vectors for the corners of Kashin_quantize that kashin_vectors.* leaves out: rates 3, 5,
6, 7 and 8, the 8-bit input whose top coordinate the reference puts in bin 256, the lengths at
which torch.norm's chunks and tails change, the loop's parameters (niters, err, eta, delta) and
d = 2^21.  Produced like make_golden_kashin.py, by the reference's own
KashinStochasticQuantizationSender(...).compress(data) and its receiver on torch CPU with one
thread (build container only: the reference is not on the GPU machine).

Each case has an explicit quantizer seed (no draw of the global generator: those are pinned by
kashin_vectors.*).  Stored: the input's spec "x" (tests/kashin_model.gen_input), bits, seed, niters,
err, eta, delta, the number of forward transforms the reference ran (counted by wrapping
HadamardSender.randomized_hadamard_transform), min and step, the bins as u16 (8 bits reach 256)
and the output.  Outputs of fewer than 8192 coordinates and their bins are stored in full,
longer ones as a sha256 each and the output at 4096 sampled positions
(tests/kashin_model.sample_positions).  A case whose min, step, bins and output are all the bits
of an earlier case's (a client that left the loop before the larger niters mattered) stores
`same_as`, that case's index, in place of the arrays.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kashin_edges.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.kashin_model import gen_input, sample_positions  # noqa: E402

REF = "/root/reference/NMSE_Results/Codes"
RATES = (3, 5, 6, 7, 8)
RATE_DIMS = (13, 1741, 5000)
SMALL_NORM_DIMS = (4, 6, 8, 12, 15, 16)
CHUNK_NORM_DIMS = (2047, 2055, 2056, 4100, 4103, 6147, 6150)
TOP_BIN = {"dist": "normal_f32", "d": 2048, "seed": 5238}        # 8 bits, quantizer seed 37: bin 256 at 1399
ERR_BATCH = {"dist": "normal_row", "n": 24, "d": 5000, "seed": 11}


def main():
    sys.path.insert(0, REF)
    import All_Schemes as AS  # noqa: E402  (the reference)
    torch.set_num_threads(1)
    arrays, cases = {}, []
    count = [0]
    orig = AS.HadamardSender.randomized_hadamard_transform

    def counted(self, vec, seed):
        count[0] += 1
        return orig(self, vec, seed)

    AS.HadamardSender.randomized_hadamard_transform = counted

    def run(group, x, bits, seed, niters=3, err=1e-6, eta=0.9, delta=1.0):
        k = len(cases)
        c = {"idx": k, "group": group, "x": x, "bits": bits, "seed": seed, "niters": niters, "err": err, "eta": eta,
             "delta": delta}
        v = gen_input(x)
        data = {"vec": torch.tensor(v.copy(), dtype=torch.float32), "seed": seed, "nbits": bits, "rotation_seed": 123,
                "nlevels": 2 ** bits, "niters": niters, "err": err}
        count[0] = 0
        msg = AS.KashinStochasticQuantizationSender(device="cpu", eta=eta, delta=delta).compress(data)
        c["iters"] = count[0]
        out = AS.KashinStochasticQuantizationReceiver(device="cpu").decompress(msg).numpy()
        assert out.dtype == np.float32 and out.shape == (x["d"],)
        assert np.array_equal(data["vec"].numpy().view(np.uint32), v.view(np.uint32))      # the input is only read
        bins = msg["data"]["bins"].numpy()
        assert bins.dtype == np.float32 and np.array_equal(bins, np.floor(bins)) and bins.min() >= 0
        assert bins.max() <= 2 ** bits
        c["D"], c["bins_max"] = int(bins.size), int(bins.max())
        bins = bins.astype(np.uint16)
        ms = np.array([msg["data"]["min"].item(), msg["data"]["step"].item()], np.float32)
        if out.size < 8192:
            mine = (ms.tobytes(), out.tobytes(), bins.tobytes())
            for e in (e["idx"] for e in cases if f"out{e['idx']}" in arrays):
                if mine == tuple(arrays[f"{a}{e}"].tobytes() for a in ("ms", "out", "bins")):
                    c["same_as"] = e
                    break
            else:
                arrays[f"ms{k}"], arrays[f"out{k}"], arrays[f"bins{k}"] = ms, out, bins
        else:
            c["sha"] = hashlib.sha256(out.tobytes()).hexdigest()
            c["bins_sha"] = hashlib.sha256(bins.tobytes()).hexdigest()
            arrays[f"ms{k}"], arrays[f"out{k}_s"] = ms, out[sample_positions(k, out.size)]
        cases.append(c)
        return c, bins

    def normal(d, seed):
        return {"dist": "normal", "d": d, "seed": seed}

    k = 0
    for bits in RATES:
        for d in RATE_DIMS:
            run("rates", normal(d, 8000 + 13 * k), bits, (17 * k + 3) % 100)
            k += 1
        run("rates", {"dist": "lognormal", "d": 100, "seed": 8100 + bits}, bits, 40 + bits)

    c, bins = run("top_bin", TOP_BIN, 8, 37)
    assert int((bins == 256).sum()) == 1 and int(bins[1399]) == 256 and bins.max() == 256, np.flatnonzero(bins > 255)

    for d in SMALL_NORM_DIMS + CHUNK_NORM_DIMS:
        run("norm_edges", normal(d, 8200 + d), 1, d % 100)

    for d in (100, 5000):
        for niters in (1, 2, 4, 5):
            c, _ = run("niters", normal(d, 8300 + niters), 1, 20 + niters, niters=niters)
            assert c["iters"] == niters if niters <= 2 else 2 <= c["iters"] <= niters, c    # (no exit at i = 0)
        run("eta", normal(d, 8310), 1, 31, eta=0.75)
        for delta in (0.5, 2.0):
            run("delta", normal(d, 8320), 1, 32, delta=delta)
    for niters in (4, 5):
        its = [run("err1", dict(ERR_BATCH, row=j), 1, j, niters=niters, err=1.0)[0]["iters"] for j in range(8)]
        assert niters != 4 or its == [2, 4, 3, 4, 2, 4, 2, 3], its
        assert len(set(its)) >= 2, its
        for j in range(4):
            run("err1", {"dist": "normal_row", "n": 24, "d": 100, "seed": 11, "row": j}, 1, j, niters=niters, err=1.0)

    run("large", normal(1 << 21, 8400), 1, 41)

    np.savez_compressed(os.path.join(HERE, "kashin_edges.npz"), **arrays)
    json.dump({"cases": cases}, open(os.path.join(HERE, "kashin_edges.json"), "w"), indent=1)
    size, old = (os.path.getsize(os.path.join(HERE, f)) for f in ("kashin_edges.npz", "kashin_vectors.npz"))
    print(len(cases), "cases;", size, "bytes (kashin_vectors.npz:", old, ");",
          {g: sorted({c["iters"] for c in cases if c["group"] == g}) for g in sorted({c["group"] for c in cases})})
    assert size <= old


if __name__ == "__main__":
    main()
