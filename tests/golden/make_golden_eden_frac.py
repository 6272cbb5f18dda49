"""Golden fixtures for EDEN at fractional rates 1 < nbits < 2, made by running the REFERENCE itself
(build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eden_frac.py

Calls EdenSender.compress / EdenReceiver.decompress (NMSE_Results/Codes/All_Schemes.py:352-425) on
torch CPU with one thread and chosen rotation seeds, and EDEN_quantize_Hadamard (AS:792-811) after
torch.manual_seed for the drop-in.  Inputs are generator specs (tests/golden_data.spec_gen).  Every
case stores the sha256 of its bins and of its output, the scale's bits and the message's nbits
tuple.  Cases up to d = 1024 store their bins and outputs in full (eden_frac_vectors.npz); longer
ones 4096 sampled outputs at positions default_rng(idx).choice(d, 4096), one file per length
(eden_frac_outs_d<d>.npz: each stays below the size limit of a committed file).
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
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, "/root/reference/NMSE_Results/Codes")
import All_Schemes as AS  # noqa: E402  (the reference module)
from golden_data import sha, spec_gen  # noqa: E402

f32 = np.float32
DIMS = (1, 3, 5, 31, 33, 333, 623, 625, 1000, 1024, 4096, 5000, 8192, 16384, 65536, 172554, 1 << 20)
NBITS = (1.5, 1.25, 1.3, 1.999, 1.0000001)
SEEDS = (0, 42, 99, 123456789)          # (the last: outside the drop-in's 0..99, a row of its own)
FULL = 1024                             # bins and outputs in full up to this length
NSAMPLE = 4096                          # sampled outputs of a longer case


def sample_pos(idx, dim):
    return np.random.default_rng(idx).choice(dim, NSAMPLE, replace=False).astype(np.int64)


def run(S, R, x, nbits, seed):
    data = S.compress({"vec": torch.from_numpy(x.copy()), "seed": seed, "nbits": nbits})
    out = R.decompress(data).numpy().astype(f32)
    return data, data["bins"].numpy().astype(np.uint8), out


def main():
    torch.set_num_threads(1)
    S = AS.EdenSender(device="cpu")
    R = AS.EdenReceiver(device="cpu")
    arrs, meta, outs = {}, {"cases": [], "edges": [], "dropin": []}, {}
    idx = 0
    for dim in DIMS:
        for ni, nbits in enumerate(NBITS):
            for seed in SEEDS:
                sp = {"dist": "lognormal" if (ni + dim) % 2 else "normal", "d": dim, "seed": 1500 + dim % 1000 + seed % 1000}
                x = spec_gen(sp)
                data, bins, out = run(S, R, x, nbits, seed)
                t = data["nbits"]
                case = dict(sp, idx=idx, nbits=nbits, rseed=seed, D=int(bins.shape[0]),
                            scale_bits=int(f32(data["scale"].item()).view(np.uint32)), bins_sha=sha(bins), out_sha=sha(out),
                            msg_nbits=[int(t[0]), int(t[1]), float(t[2])], pdrop=float(data["pdrop"]))
                if dim <= FULL:
                    arrs[f"bins{idx}"] = bins
                    arrs[f"out{idx}"] = out
                else:
                    outs.setdefault(dim, {})[f"outs{idx}"] = out[sample_pos(idx, dim)]
                meta["cases"].append(case)
                print(idx, dim, nbits, seed, case["scale_bits"], flush=True)
                idx += 1
    # edge rows: all zeros, one NaN, one-hot (inputs by rule, outputs in full)
    for name, dim in (("zeros", 1000), ("nan", 1000), ("onehot", 1000), ("zeros", 64), ("nan", 4096)):
        x = np.zeros(dim, f32) if name != "nan" else spec_gen({"dist": "normal", "d": dim, "seed": 77})
        if name == "nan":
            x[dim // 3] = np.nan
        if name == "onehot":
            x[dim // 2] = 3.5
        for nbits, seed in ((1.5, 7), (1.3, 42)):
            data, bins, out = run(S, R, x, nbits, seed)
            k = len(meta["edges"])
            arrs[f"ebins{k}"] = bins
            arrs[f"eout{k}"] = out
            meta["edges"].append({"k": k, "name": name, "d": dim, "nbits": nbits, "rseed": seed,
                                  "scale_bits": int(f32(data["scale"].item()).view(np.uint32))})
    # the drop-in: the rotation seed drawn from the global generator, one word per call
    for tseed, nbits in ((0, 1.5), (1, 1.25), (2, 1.999)):
        x = spec_gen({"dist": "normal", "d": 2000, "seed": 1900 + tseed})
        torch.manual_seed(tseed)
        drawn = int(torch.randint(0, 100, (1,)).item())
        after = int(torch.randint(0, 1 << 30, (1,)).item())       # the word after the call's one draw
        torch.manual_seed(tseed)
        out = AS.EDEN_quantize_Hadamard(torch.from_numpy(x.copy()), nbits)
        assert int(torch.randint(0, 1 << 30, (1,)).item()) == after
        arrs[f"dout{tseed}"] = np.asarray(out, f32)
        meta["dropin"].append({"tseed": tseed, "nbits": nbits, "drawn_seed": drawn, "next_word": after, "d": 2000,
                               "spec_seed": 1900 + tseed})
    np.savez_compressed(os.path.join(HERE, "eden_frac_vectors.npz"), **arrs)
    for dim, a in outs.items():
        np.savez_compressed(os.path.join(HERE, f"eden_frac_outs_d{dim}.npz"), **a)
    with open(os.path.join(HERE, "eden_frac_vectors.json"), "w") as f:
        json.dump(meta, f, indent=0)


if __name__ == "__main__":
    main()
