"""Known NMSE answers for the DME loop with EDEN at a fractional rate, made by running the
REFERENCE's own functions in the driver's call order (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nmse_eden_frac.py

As make_golden_nmse_schemes.py (ND = NMSE_Results/Codes/Normal_dist.py), with the rate 1.5: per
client EDEN_quantize_Hadamard(v, 1.5) then Type_unbiased_quantize(v, 1.5) (ND:135-138's order), all
drawing from the global torch RNG seeded 42, vectors from np.random seeded 42, NMSE as ND:151-157,
d = 2048, n in {1, 6}, two instances each.  Every EDEN call's rotation seed, scale bits and message
nbits are recorded, so the scale and the rest can be checked apart.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/NMSE_Results/Codes")
import All_Schemes as AS  # noqa: E402  (the reference module)

DIM, RATE = 2048, 1.5
SCHEMES = [("eden", RATE), ("unbiased", RATE)]


def main():
    torch.set_num_threads(1)
    fns = {"eden": AS.EDEN_quantize_Hadamard, "unbiased": AS.Type_unbiased_quantize}
    gens = {"normal": lambda: np.random.normal(0, 1, DIM),
            "lognormal": lambda: np.random.lognormal(mean=1, sigma=2, size=DIM)}
    seen = []
    orig = AS.EdenSender.compress

    def recording_compress(self, data):
        out = orig(self, data)
        assert isinstance(out["nbits"], tuple) and out["nbits"][:2] == (1, 2) and out["nbits"][2] == RATE - 1
        seen.append((int(out["seed"]), int(np.float32(out["scale"].item()).view(np.uint32))))
        return out
    AS.EdenSender.compress = recording_compress
    res, scales = {}, {}
    for dist in gens:
        np.random.seed(42)
        torch.manual_seed(42)
        rows = []
        for n in (1, 6):
            for inst in range(2):
                vecs, norms = [], []
                for _ in range(n):
                    v = np.asarray(gens[dist](), dtype=np.float64)
                    norms.append(np.linalg.norm(v) ** 2)
                    vecs.append(torch.as_tensor(v, dtype=torch.float32))
                vns = sum(norms)
                emp = torch.stack(vecs).sum(dim=0) / n
                est = {k: torch.zeros(DIM) for k in SCHEMES}
                for j, v in enumerate(vecs):
                    for k in SCHEMES:
                        del seen[:]
                        est[k] += torch.as_tensor(fns[k[0]](v, k[1])) / n
                        if k[0] == "eden":
                            assert len(seen) == 1
                            scales.setdefault(dist, []).append([n, inst, j, k[1], seen[0][0], seen[0][1]])
                row = {"n": n, "inst": inst}
                for k in SCHEMES:
                    row[k[0]] = float(torch.norm(est[k] - emp).pow(2) / (50 * vns * n))
                rows.append(row)
                print(dist, row, flush=True)
        res[dist] = rows
    with open(os.path.join(HERE, "nd_nmse_eden_frac.json"), "w") as f:
        json.dump({"dim": DIM, "rate": RATE, "rows": res,
                   "eden_scales_fields": ["n", "inst", "client", "bits", "seed", "scale_bits"], "eden_scales": scales}, f, indent=1)


if __name__ == "__main__":
    main()
