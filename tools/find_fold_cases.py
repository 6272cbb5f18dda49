"""Search inputs that drive exact_fold_kernel's rare branches (run offline; what it finds goes
into tests/test_gpu_exact_scan.py, what it does not into DESIGN.md section 2).

    python tools/find_fold_cases.py [log2 d = 22] [seeds = 200] [processes = 8]

Per vector the census of tests.scan_models.fold_census: irregular tiles, recorded ones (events <=
kRecEvents), the recorded tiles' events summed (> kFoldEvents: a record is copied, not walked from
LDS), recorded tiles > kRecPerClient (budget exhausted), regular maps of another binade than the
exact start.  Space: tiny_mix over seeds x mix in {0.3, 0.5, 0.9, 0.95, 0.99} x scale in {1e-3 ..
1e-6} at R = 1, and the constructed hover vector (scan_models.hover_vector)."""
import os
import sys
from multiprocessing import Pool

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from oracle import uq_oracle as O, uq_oracle_c as C
from tests import scan_models as S

MIXES = (0.3, 0.5, 0.9, 0.95, 0.99)
SCALES = (1e-3, 1e-4, 1e-5, 1e-6)


def summary(c):
    irr = c["irregular"]
    return dict(irregular=int(irr.sum()), recorded=c["n_recorded"], rec_events=c["rec_events"],
                max_events_recorded=int(c["events"][c["recorded"]].max(initial=0)),
                unrecorded=int((irr & ~c["recorded"]).sum()), other_binade=int(c["other_binade"].sum()),
                ties_max=int(c["ties"].max()), ties_0=int((~irr & (c["ties"] == 0)).sum()),
                ties_fast=int((~irr & (c["ties"] > 0) & (c["ties"] <= S.FAST_TIES)).sum()),
                ties_slow=int((c["ties"] > S.FAST_TIES).sum()))


def one(args):
    seed, d, mix, scale = args
    x = S.tiny_mix(seed, d, mix, scale)
    _, _, fr = O.fractional_parts(x, O.rate_to_m(1, d), C.l1_torch_order(x, 1))
    return args, summary(S.fold_census(fr))


if __name__ == "__main__":
    ld = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    procs = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    d = 1 << ld
    x, l1, m = S.hover_vector(d)
    _, _, fr = O.fractional_parts(x, m, l1)
    print("hover", d, summary(S.fold_census(fr)), flush=True)
    C.lib()
    work = [(s, d, mix, sc) for mix in MIXES for sc in SCALES for s in range(seeds)]
    top = dict(recorded=(0, None), rec_events=(0, None), other_binade=(0, None), irregular=(0, None))
    with Pool(procs) as pool:
        for i, (args, sm) in enumerate(pool.imap_unordered(one, work, chunksize=4)):
            for k in top:
                if sm[k] > top[k][0]:
                    top[k] = (sm[k], args)
            if sm["recorded"] > S.REC_PER_CLIENT or sm["rec_events"] > S.FOLD_EVENTS or sm["other_binade"]:
                print("FOUND", args, sm, flush=True)
            if (i + 1) % 200 == 0:
                print(i + 1, "of", len(work), top, flush=True)
    print("maxima over", len(work), "vectors:", top)
