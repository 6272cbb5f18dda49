"""Golden vectors for Kashin_quantize (AS:834-854), produced by running the reference's own
functions on torch CPU with one thread (build container only: the reference is not on the GPU
machine).

Each case: torch.manual_seed(gseed), `pre` torch.randint(0, 100, (1,)) draws, the call, and the
sha256 of torch.default_generator.get_state() after it.  Stored: the output, the sender's message
(bins as u8, min, step), the number of forward transforms the reference ran (counted by wrapping
HadamardSender.randomized_hadamard_transform) and, for inputs torch.bernoulli refuses,
`raises: true` with the state sha.  Inputs are regenerated from their spec
(tests/kashin_model.gen_input); outputs below 65536 coordinates are stored in full, longer ones
(and their bins) as a sha256 and 4096 samples.

The early-exit cases (two forward transforms, AS:236 at i = 1) are searched among small seeds.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kashin.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.kashin_model import gen_input  # noqa: E402

REF = "/root/reference/NMSE_Results/Codes"
DIMS = (2, 3, 5, 7, 13, 14, 27, 28, 1000, 1740, 1741, 2048, 2049, 3481, 3482, 5000)


def state_sha():
    return hashlib.sha256(torch.default_generator.get_state().numpy().tobytes()).hexdigest()


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

    def start(c):
        torch.manual_seed(c["gseed"])
        for _ in range(c["pre"]):
            torch.randint(0, 100, (1,))

    def reference(c, x):
        """(out or None when the call raises, transforms, state sha, message or None)."""
        start(c)
        count[0] = 0
        try:
            out = np.asarray(AS.Kashin_quantize(x.copy(), c["bits"]), np.float32)
        except RuntimeError:
            return None, count[0], state_sha(), None
        n, sha = count[0], state_sha()
        # the same call in its parts, for the sender's message (AS:839-852)
        start(c)
        v = torch.tensor(x.copy(), dtype=torch.float32)
        data = {"vec": v.clone(), "seed": int(torch.randint(0, 100, (1,)).item()), "nbits": c["bits"],
                "rotation_seed": 123, "nlevels": 2 ** c["bits"], "niters": 3}
        msg = AS.KashinStochasticQuantizationSender(device="cpu").compress(data)
        again = AS.KashinStochasticQuantizationReceiver(device="cpu").decompress(msg).numpy()
        assert np.array_equal(again.view(np.uint32), out.view(np.uint32))
        c["seed_drawn"] = data["seed"]
        return out, n, sha, msg["data"]

    def run(dist, d, bits, seed, pre=0, want_iters=None):
        k = len(cases)
        c = {"idx": k, "dist": dist, "d": d, "bits": bits, "seed": seed, "gseed": 500 + k, "pre": pre}
        x = gen_input(c)
        out, n, sha, msg = reference(c, x)
        c["state_sha"], c["iters"], c["raises"] = sha, n, out is None
        if want_iters is not None:
            assert n == want_iters, (c, n)
        if out is not None:
            assert out.shape == (d,)
            bins = msg["bins"].numpy()
            assert bins.min() >= 0 and bins.max() <= 255 and np.array_equal(bins, np.floor(bins))
            bins = bins.astype(np.uint8)
            arrays[f"ms{k}"] = np.array([msg["min"].item(), msg["step"].item()], np.float32)
            if out.size < 65536:
                arrays[f"out{k}"] = out
                arrays[f"bins{k}"] = bins
            else:
                pos = np.random.default_rng(k).choice(out.size, 4096, replace=False).astype(np.int64)
                c["sha"] = hashlib.sha256(out.tobytes()).hexdigest()
                c["bins_sha"] = hashlib.sha256(bins.tobytes()).hexdigest()
                arrays[f"out{k}_pos"] = pos
                arrays[f"out{k}_s"] = out[pos]
        cases.append(c)
        return c

    k = 0
    for dist in ("normal", "lognormal"):
        for d in DIMS:
            for bits in (1, 2, 4):
                run(dist, d, bits, 4000 + 11 * k, pre=(0, 1, 0, 1, 300)[k % 5])
                k += 1
    run("normal", 70001, 1, 7001, pre=1)               # D = 131072: two FWHT passes
    run("normal", 1 << 20, 1, 7002, pre=0)             # D = 2^21: three
    for d in (5, 2048, 3000):
        run("onehot", d, 1, 7 + d, pre=d % 2, want_iters=3)
        run("constant", d, 2, 0, pre=1, want_iters=3)
    raising = [run("normal", 1, 1, 7100, pre=0), run("normal", 1, 2, 7101, pre=1), run("zeros", 8, 1, 0, pre=1),
               run("nan", 100, 2, 7102, pre=0), run("inf", 100, 1, 7103, pre=300)]
    assert all(c["raises"] for c in raising)

    # early exits: inputs whose loop breaks at i = 1
    def search(dist, d, bits, seeds, keep):
        found = 0
        for s in seeds:
            c = {"dist": dist, "d": d, "bits": bits, "seed": s, "gseed": 0, "pre": 0}
            _, n, _, _ = reference(c, gen_input(c))
            if n == 2:
                run(dist, d, bits, s, pre=found % 2, want_iters=2)
                found += 1
                if found == keep:
                    break
        return found

    normal = search("normal", 3, 1, range(300), 2) + search("normal", 4, 2, range(300), 1)
    ints = sum(search("smallint", d, 1 + d % 2, range(150), 1) for d in (5, 6, 7, 8, 12))
    assert normal >= 1 and ints >= 3 and normal + ints >= 4, (normal, ints)

    # d = 0: recorded, not asserted (what the reference does with an empty vector)
    c = {"idx": len(cases), "dist": "zeros", "d": 0, "bits": 1, "seed": 0, "gseed": 999, "pre": 0}
    out, n, sha, _ = reference(c, np.zeros(0, np.float32))
    start(c)
    torch.randint(0, 100, (1,))
    c.update(state_sha=sha, iters=n, raises=out is None, draws_one_word=sha == state_sha())
    cases.append(c)

    np.savez_compressed(os.path.join(HERE, "kashin_vectors.npz"), **arrays)
    json.dump({"cases": cases}, open(os.path.join(HERE, "kashin_vectors.json"), "w"), indent=1)
    print(len(cases), "cases;", os.path.getsize(os.path.join(HERE, "kashin_vectors.npz")), "bytes;",
          sum(c["iters"] == 2 for c in cases), "early exits; d = 0:", cases[-1])


if __name__ == "__main__":
    main()
