"""Golden fixtures for EDEN's receiver-side coordinate drop, made by running the REFERENCE itself
(build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eden_drop.py

Every case is one reference wrapper call spelled out on torch CPU with one thread (AS = NMSE_Results/Codes/
All_Schemes.py:792-811): torch.manual_seed(gseed), `pre` one-word draws, the rotation seed from the global
generator (AS:800), EdenSender.compress with the message field pdrop (AS:384), EdenReceiver.decompress
(AS:398-426: round(D * p) coordinates of the rotated vector zeroed by torch.randperm(D) on the global
generator, the rest divided by 1 - p).  The rates below 1 bit (nbits < 1, AS:414-415) run alone through
EDEN_quantize_Hadamard itself and, combined with pdrop = 0.5, through the same spelled-out call.

Stored per case: the drawn seed, the scale's bits, the sha256 of the bins, the total drop share p as the
reference computes it (AS:413-417) and k = round(D * p), the count of exact zeros of the output, the sha256 of
the output and of the global generator's state afterwards; the output in full up to d = 65536 (eden_drop.npz;
the 65536 ones in eden_drop_outs_d65536.npz), above that 4096 sampled entries at
default_rng(idx).choice(d, 4096) (eden_drop_outs_d<d>.npz).  Inputs are generator specs
(tests/golden_data.spec_gen).
"""
from __future__ import annotations

import hashlib
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
SMALL = (1, 2, 5, 64, 1000, 2048, 4099)
BITS = (1, 2, 1.5, 1.3)
PDROP = (0.5, 1 - 0.3, 0.25, 0.999, 1e-7)          # (the last: k = 0, the division alone)
SUB1 = (0.5, 0.3, 0.75)                             # the reference's own spellings below 1 bit
PRE = (0, 1, 3, 700)
FULL = 65536
NSAMPLE = 4096


def sample_pos(idx, dim):
    return np.random.default_rng(idx).choice(dim, NSAMPLE, replace=False).astype(np.int64)


def state_sha():
    return hashlib.sha256(torch.default_generator.get_state().numpy().tobytes()).hexdigest()


def total_p(nbits, pdrop):
    """AS:413-417"""
    p = 0
    if not isinstance(nbits, tuple) and nbits < 1:
        p = 1 - nbits
    if pdrop > 0:
        p += (1 - p) * pdrop
    return p


def run(S, R, x, nbits, pdrop, gseed, pre):
    torch.manual_seed(gseed)
    for _ in range(pre):
        torch.randint(0, 100, (1,))
    seed = int(torch.randint(0, 100, (1,)).item())                                # AS:800
    data = S.compress({"vec": torch.from_numpy(x.copy()), "seed": seed, "nbits": nbits, "pdrop": pdrop})
    out = R.decompress(data).numpy().astype(f32)
    return seed, data, out, state_sha()


def main():
    torch.set_num_threads(1)
    S = AS.EdenSender(device="cpu")
    R = AS.EdenReceiver(device="cpu")
    arrs, meta, outs = {}, {"cases": []}, {}

    def add(dim, nbits, pdrop, wrapper=False):
        idx = len(meta["cases"])
        gseed, pre = 4000 + idx, PRE[idx % len(PRE)]
        sp = {"dist": "lognormal" if idx % 3 == 0 else "normal", "d": dim, "seed": 2600 + idx}
        x = spec_gen(sp)
        seed, data, out, st = run(S, R, x, nbits, pdrop, gseed, pre)
        if wrapper:                                   # the reference's own wrapper: the same call
            torch.manual_seed(gseed)
            for _ in range(pre):
                torch.randint(0, 100, (1,))
            w = np.asarray(AS.EDEN_quantize_Hadamard(torch.from_numpy(x.copy()), nbits), f32)
            assert sha(w) == sha(out) and state_sha() == st
        bins = data["bins"].numpy().astype(np.uint8)
        D = int(bins.shape[0])
        p = total_p(data["nbits"], data["pdrop"])
        t = data["nbits"]
        case = dict(sp, idx=idx, nbits=nbits, pdrop=pdrop, gseed=gseed, pre=pre, rseed=seed, D=D, p=float(p),
                    k=int(round(D * p)), scale_bits=int(f32(data["scale"].item()).view(np.uint32)), bins_sha=sha(bins),
                    out_sha=sha(out), nzero=int((out == 0).sum()), state_sha=st, wrapper=bool(wrapper),
                    msg_nbits=[int(t[0]), int(t[1]), float(t[2])] if isinstance(t, tuple) else float(t))
        if dim < FULL:
            arrs[f"out{idx}"] = out
        elif dim == FULL:
            outs.setdefault(dim, {})[f"out{idx}"] = out
        else:
            outs.setdefault(dim, {})[f"outs{idx}"] = out[sample_pos(idx, dim)]
        meta["cases"].append(case)
        print(idx, dim, nbits, pdrop, seed, case["k"], case["nzero"], flush=True)

    # every rate with every pdrop, two pdrops per (length, rate), rotating
    t = 0
    for dim in SMALL:
        for nbits in BITS:
            for _ in range(2):
                add(dim, nbits, PDROP[t % len(PDROP)])
                t += 1
    # the rates below 1 bit: alone (through the wrapper too) and combined with pdrop = 0.5
    for dim in (5, 1000, 2048):
        for r in SUB1:
            add(dim, r, 0, wrapper=True)
            add(dim, r, 0.5)
    add(65536, 2, 0.5)
    add(65536, 0.5, 0, wrapper=True)
    add(172554, 1, 1 - 0.3)
    add(172554, 1.5, 0.5)
    add(1 << 20, 1, 0.5)
    add(1 << 20, 2, 0.25)
    add(1 << 20, 0.5, 0, wrapper=True)
    np.savez_compressed(os.path.join(HERE, "eden_drop.npz"), **arrs)
    for dim, a in outs.items():
        np.savez_compressed(os.path.join(HERE, f"eden_drop_outs_d{dim}.npz"), **a)
    with open(os.path.join(HERE, "eden_drop.json"), "w") as f:
        json.dump(meta, f, indent=0)


if __name__ == "__main__":
    main()
