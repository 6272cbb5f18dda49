"""Edge-case golden vectors for Scalar_quantize (AS:755-790) and DRIVE_quantize_Hadamard
(AS:707-752), produced by running the reference's own functions on torch CPU (build container
only: the reference is not on the GPU machine).  A second fixture beside rand_schemes_vectors.*
(make_golden_rand_schemes.py), which stays as it is.

DRIVE: last chunks of every length L % 8 (torch.norm's tail after the 8-wide vectors, at input
seeds where the tail's 4 + fma order and a plain mul + add tail give different outputs), a NaN in
one chunk of three, -inf, subnormal and overflowing inputs, signed zeros.  Scalar: a NaN at d = 1,
-inf, both infinities, an overflowing span, subnormals, a span of a few ulps, 3 to 32 bits, a
NaN in the last of three min / max slices, and d = 266241 (the 64-slice cap).  The generator
starts after 0, 1, 63, 575, 577, 623 or 624 one-word draws.

Each case as in make_golden_rand_schemes.py: torch.manual_seed(gseed), `pre` draws, the call, the
sha256 of torch.default_generator.get_state() after it; inputs from their spec
(tests/rand_schemes_model.gen_input); outputs below 65536 coordinates in full, longer ones as a
sha256 and 4096 samples.  Rerunning reproduces both files byte for byte.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rand_edges.py
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
DRIVE_PRE = (0, 1, 63, 575, 577, 623, 624)
SCALAR_PRE = (0, 623, 624)
# (d, vseed): "normal" inputs whose last chunk's norm, and with it the output, depends on the
# order of the tail after the 8-wide vectors (tests/test_rand_edges_oracle.py checks that it does)
DRIVE_RAGGED = ((3, 23), (5, 13), (6, 8), (7, 19), (9, 13), (11, 122), (13, 60), (15, 20), (2051, 6), (2053, 77),
                (2055, 34), (4099, 37), (6147, 9))


def state_sha():
    return hashlib.sha256(torch.default_generator.get_state().numpy().tobytes()).hexdigest()


def main():
    sys.path.insert(0, REF)
    import All_Schemes as AS  # noqa: E402  (the reference)
    torch.set_num_threads(1)
    arrays, cases = {}, []

    def call(c, x):
        if c["scheme"] == "scalar":
            return AS.Scalar_quantize(x.copy(), c["bits"])
        return AS.DRIVE_quantize_Hadamard(x.copy(), 1)

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

    def run(scheme, kind, d, bits=1, pre=0, vseed=None, gseed=None, **extra):
        k = len(cases)
        c = {"idx": k, "scheme": scheme, "kind": kind, "d": d, "bits": bits,
             "vseed": 4000 + 7 * k if vseed is None else vseed, "gseed": 500 + k if gseed is None else gseed,
             "pre": pre, **extra}
        x = gen_input(c)
        torch.manual_seed(c["gseed"])
        for _ in range(pre):
            torch.randint(0, 100, (1,))
        store(f"out{k}", c, call(c, x))
        c["state_sha"] = state_sha()
        cases.append(c)
        return c

    for k, (d, vseed) in enumerate(DRIVE_RAGGED):
        clean = run("drive", "normal", d, pre=DRIVE_PRE[k % 7], vseed=vseed)
    # a NaN in the middle chunk only of the d = 6147 case above (same input, same words): the
    # other two chunks are the clean case's
    assert clean["d"] == 6147
    run("drive", "nan_at", 6147, pre=clean["pre"], vseed=clean["vseed"], gseed=clean["gseed"], at=3000,
        clean=clean["idx"])
    run("drive", "ninf_at", 4099, pre=1, at=4097)
    run("drive", "subnormal", 700, pre=63)
    run("drive", "subnormal", 2051, pre=575)
    run("drive", "normal_1e19", 700, pre=577)
    run("drive", "neg_zero_third", 1001, pre=623)

    run("scalar", "nan", 1, 2, pre=624)                      # den is NaN, not 0: one word is taken
    run("scalar", "nan", 1, 2, pre=0)
    run("scalar", "ninf_at", 625, 2, pre=623, at=208)
    run("scalar", "pm_inf", 700, 2, pre=624)
    run("scalar", "huge_span", 700, 2, pre=0)
    run("scalar", "subnormal", 700, 2, pre=623)
    run("scalar", "few_ulps", 700, 2, pre=624)
    for k, bits in enumerate((3, 8, 16, 24, 25, 32)):
        run("scalar", "lognormal", 700, bits, pre=SCALAR_PRE[k % 3])
    run("scalar", "nan_at", 9000, 2, pre=623, at=8999)       # 3 slices, the NaN in the last
    run("scalar", "normal", 266241, 2, pre=624)              # 64 slices (the cap)

    np.savez_compressed(os.path.join(HERE, "rand_schemes_edges.npz"), **arrays)
    json.dump({"cases": cases}, open(os.path.join(HERE, "rand_schemes_edges.json"), "w"), indent=1)
    print(len(cases), "cases;", os.path.getsize(os.path.join(HERE, "rand_schemes_edges.npz")), "bytes")


if __name__ == "__main__":
    main()
