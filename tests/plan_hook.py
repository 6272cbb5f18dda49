"""Test infrastructure: the unbiased dispatcher's plan (uq_test_unbiased_plan,
uq_test_last_unbiased_plan in include/uq_dme.h) as a dict, and the fold's workspace arrays
read back through the offsets the plan gives."""
import ctypes

import numpy as np

FIELDS = ("form", "V", "Q", "C", "CV", "l1_given", "chunks", "nj", "prefixed", "R", "nseg", "tiles", "p_off",
          "map0_off", "map1_off", "rec_off", "cnt_off", "rec_bytes", "rec_per_client", "rec_clients", "rec_events",
          "fold_events")
NONE, SMALL, STREAM, NIBBLES, SEGMENTS, PHASED = range(6)
FORM_NAMES = ("none", "small", "stream", "stream-nibbles", "segments", "phased")
IRR_MAP = (1 << 64) - 1


def _as_dict(buf):
    p = dict(zip(FIELDS, (int(v) for v in buf)))
    for k in ("V", "Q", "C", "CV", "l1_given", "prefixed"):
        p[k] = bool(p[k])
    return p


def plan(lib, n, d, ldq=None, ldc=None, x16=True, out16=True, codes16=True, out=True, codes=False, nib=False,
         l1=False, slots=1024):
    """(rc, plan) of a call of this shape, host only."""
    buf = (ctypes.c_int64 * len(FIELDS))()
    rc = lib.uq_test_unbiased_plan(n, d, d if ldq is None else ldq, d if ldc is None else ldc, int(x16), int(out16),
                                   int(codes16), int(out), int(codes), int(nib), int(l1), slots, buf, len(FIELDS))
    return rc, (_as_dict(buf) if rc == 0 else None)


def last_plan(lib):
    """The plan of this thread's last unbiased call."""
    buf = (ctypes.c_int64 * len(FIELDS))()
    assert lib.uq_test_last_unbiased_plan(buf, len(FIELDS)) == 0
    return _as_dict(buf)


def fold_readback(ws, p, n):
    """From a workspace (torch uint8 tensor) after a segments / phased call of one chunk with plan
    p: (P [n, tiles] u64 bits of the exact tile starts, map0, map1, counters [min(n, rec_clients)],
    count(client, record number) -> that record's event count)."""
    raw = ws.cpu().numpy()
    t = p["tiles"]

    def arr(off):
        return raw[off:off + n * t * 8].view(np.uint64).reshape(n, t).copy()

    nc = min(n, p["rec_clients"])
    cnt = raw[p["cnt_off"]:p["cnt_off"] + 4 * nc].view(np.uint32).copy()

    def count(client, rno):
        o = p["rec_off"] + (client * p["rec_per_client"] + (rno - 1)) * p["rec_bytes"]
        return int(raw[o:o + 4].view(np.uint32)[0])

    return arr(p["p_off"]), arr(p["map0_off"]), arr(p["map1_off"]), cnt, count


def fold_branches(P, m0, m1, cnt, count, p, client):
    """Which branch of exact_fold_kernel each tile of one client took, from the readback:
    a dict branch -> list of tiles.  Regular maps whose binade is P_t's are walked in the run
    ('regular'); 'other_binade' maps and unrecorded irregular tiles are resolved 'from_data'
    (listed under both); recorded ones are walked from LDS while the running sum of the client's
    record counts fits fold_events ('rec_lds'), else copied ('rec_copied')."""
    out = {k: [] for k in ("regular", "from_data", "rec_lds", "rec_copied", "other_binade")}
    nrec = min(int(cnt[client]), p["rec_per_client"]) if client < p["rec_clients"] else 0
    fits, off = {}, 0
    for r in range(1, nrec + 1):            # the fold's prefetch: records in number order while they fit
        c = count(client, r)
        fits[r] = off + c <= p["fold_events"]
        if fits[r]:
            off += c
    for t in range(P.shape[1]):
        a, b = int(m0[client, t]), int(m1[client, t])
        if a == IRR_MAP:
            if b == 0:
                out["from_data"].append(t)
            else:
                out["rec_lds" if fits[b] else "rec_copied"].append(t)
        elif (a >> 53) != (int(P[client, t]) >> 52):
            out["other_binade"].append(t)
            out["from_data"].append(t)
        else:
            out["regular"].append(t)
    out["budget_exhausted"] = client < p["rec_clients"] and int(cnt[client]) > p["rec_per_client"]
    return out


def tile_starts(x, m, l1):
    """The oracle's exact tile starts of one vector: the sequential fp64 cumsum (AS:635) of its
    fractional parts before each 4096-element tile, as u64 bits (P_0 = 0)."""
    from oracle import uq_oracle as O
    _, _, fr = O.fractional_parts(x, m, l1)
    c = np.cumsum(fr.astype(np.float64))
    tiles = -(-x.shape[0] // 4096)
    P = np.zeros(tiles, np.float64)
    P[1:] = c[np.arange(1, tiles) * 4096 - 1]
    return P.view(np.uint64)


def call_q(lib, L, xd, Xd, m, T=1, l1d=None):
    """uq_type_unbiased_f32 on device tensors (l1d: supplied norms) with a workspace of its own:
    (q, workspace, plan)."""
    import torch
    n, d = xd.shape
    b = ctypes.c_size_t()
    L.check(lib.uq_workspace_bytes(n, d, T, ctypes.byref(b)), "ws")
    ws = torch.zeros(max(b.value, 1 << 16), dtype=torch.uint8, device="cuda")
    q = torch.empty_like(xd)
    L.check(lib.uq_type_unbiased_f32(xd.data_ptr(), q.data_ptr(), n, d, m, Xd.data_ptr(), None if l1d is None else l1d.data_ptr(), None, T,
                                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "uq_type_unbiased_f32")
    torch.cuda.synchronize()
    return q, ws, last_plan(lib)
