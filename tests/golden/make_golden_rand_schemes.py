"""Golden vectors for Scalar_quantize (AS:755-790) and DRIVE_quantize_Hadamard (AS:707-752),
produced by running the reference's own functions on torch CPU (build container only: the
reference is not on the GPU machine).

Each case: torch.manual_seed(gseed), `pre` torch.randint(0, 100, (1,)) draws (one generator
word each, so the stream starts at left = 1, 623 or mid-block), the call, and the sha256 of
torch.default_generator.get_state() after it.  Inputs are regenerated from their spec
(tests/rand_schemes_model.gen_input); outputs below 65536 coordinates are stored in full, longer
ones as a sha256 and 4096 samples.  `pairs` are two calls back to back.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rand_schemes.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.rand_schemes_model import gen_input  # noqa: E402

REF = "/root/reference/NMSE_Results/Codes"
SCALAR_D = (1, 2, 5, 623, 624, 625, 1251, 2048, 5000, 65553)
DRIVE_D = (1, 2, 3, 5, 1000, 2048, 2049, 3073, 4096, 5000, 6768)


def state_sha():
    return hashlib.sha256(torch.default_generator.get_state().numpy().tobytes()).hexdigest()


def main():
    sys.path.insert(0, REF)
    import All_Schemes as AS  # noqa: E402  (the reference)
    torch.set_num_threads(1)
    arrays, cases, pairs = {}, [], []

    def call(c, x):
        if c["scheme"] == "scalar":
            return AS.Scalar_quantize(x.copy(), c["bits"])
        return AS.DRIVE_quantize_Hadamard(x.copy(), 1)

    def start(c):
        torch.manual_seed(c["gseed"])
        for _ in range(c["pre"]):
            torch.randint(0, 100, (1,))

    def store(key, c, out):
        out = out.numpy().astype(np.float32)
        assert out.shape == (c["d"],)
        if out.size < 65536:
            arrays[key] = out
        else:
            pos = np.random.default_rng(len(cases)).choice(out.size, 4096, replace=False).astype(np.int64)
            c["sha"] = hashlib.sha256(out.tobytes()).hexdigest()
            arrays[key + "_pos"] = pos
            arrays[key + "_s"] = out[pos]

    def run(scheme, kind, d, bits=1, pre=0):
        k = len(cases)
        c = {"idx": k, "scheme": scheme, "kind": kind, "d": d, "bits": bits, "vseed": 3000 + 7 * k, "gseed": 100 + k,
             "pre": pre}
        x = gen_input(c)
        start(c)
        store(f"out{k}", c, call(c, x))
        c["state_sha"] = state_sha()
        cases.append(c)

    k = 0
    for d in SCALAR_D:
        for bits in (1, 2, 4):
            run("scalar", "normal", d, bits, pre=k % 2)
            k += 1
    for d in (5, 1251, 5000, 65553):
        for bits in (1, 2, 4):
            run("scalar", "lognormal", d, bits, pre=k % 2)
            k += 1
    for d in (1, 5, 2048):
        run("scalar", "constant", d, 2, pre=d % 2)
    run("scalar", "nan", 1251, 2, pre=1)
    run("scalar", "inf", 625, 1, pre=0)
    run("scalar", "normal", 5000, 2, pre=300)
    run("scalar", "normal", 5, 0, pre=1)                    # 2**0 - 1 < 1: no draw (AS:772)
    for d in DRIVE_D:
        run("drive", "normal", d, pre=k % 2)
        k += 1
    run("drive", "lognormal", 5000, pre=1)
    run("drive", "lognormal", 6768, pre=0)
    run("drive", "zeros", 3073, pre=1)
    run("drive", "zero_pairs", 5000, pre=0)
    run("drive", "normal", 4096, pre=300)
    run("drive", "normal", 70001, pre=1)

    for scheme, d, bits in (("scalar", 1251, 2), ("drive", 3073, 1)):
        j = len(pairs)
        c = {"idx": j, "scheme": scheme, "kind": "normal", "d": d, "bits": bits, "vseed": 9000 + j, "gseed": 77 + j,
             "pre": 1}
        x = gen_input(c)
        start(c)
        for t in range(2):
            arrays[f"pair{j}_{t}"] = call(c, x).numpy().astype(np.float32)
        c["state_sha"] = state_sha()
        pairs.append(c)

    np.savez_compressed(os.path.join(HERE, "rand_schemes_vectors.npz"), **arrays)
    json.dump({"cases": cases, "pairs": pairs}, open(os.path.join(HERE, "rand_schemes_vectors.json"), "w"), indent=1)
    print(len(cases), "cases,", len(pairs), "pairs;", os.path.getsize(os.path.join(HERE, "rand_schemes_vectors.npz")),
          "bytes")


if __name__ == "__main__":
    main()
