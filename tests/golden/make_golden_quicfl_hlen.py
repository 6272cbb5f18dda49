"""Golden vectors for QUIC-FL with an h_len that is not a power of two (h = word % h_len takes the
division, not the mask), produced by running the reference's own QuicFLSender.compress (AS:455-503)
and QuicFLReceiver.decompress (AS:526-535) here.

Both constructors take a `prefix` (AS:431, AS:509) and h_len travels in data.txt and in the message
(AS:502, AS:528).  Per case this script writes a temporary prefix with synthetic tables of that h_len
for the four bit widths the constructors load (tests/golden/quicfl_tables.py: sender_tables,
data_txt and recv_table [2^b, h_len]), runs the reference on it and commits inputs and outputs.  The
data.txt files are literals built here, so the reference's `eval` (AS:450) only reads text from
this script.  Separate from the other generators: no existing fixture is rewritten.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_quicfl_hlen.py
"""
import io
import json
import os
import shutil
import struct
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from quicfl_tables import SR_BITS, data_txt, recv_table, sender_tables  # noqa: E402

REF = "/root/reference/NMSE_Results/Codes"
# (nbits, h_len, dim, input seed, message seed, rotation seed, global seed, draws before the call)
CASES = [(1, 48, 1000, 11, 17, 123, 301, 0), (1, 48, 5000, 12, 99, 7, 302, 623),
         (3, 5, 1000, 13, 3, 41, 303, 1), (3, 5, 5000, 14, 64, 123, 304, 700),
         (2, 255, 1000, 15, 8, 9, 305, 624), (2, 255, 5000, 16, 55, 77, 306, 5)]


def write_prefix(root, h_len):
    os.makedirs(root, exist_ok=True)
    for b in (1, 2, 3, 4):
        fn = os.path.join(root, f"{b}_X_{SR_BITS[b]}_h_256_q_")
        X, p = sender_tables(b, h_len=h_len)
        torch.save(torch.from_numpy(X), fn + "sender_table_X.pt")
        torch.save(torch.from_numpy(p), fn + "sender_table_p.pt")
        torch.save(torch.from_numpy(recv_table(b, h_len)), fn + "recv_table.pt")
        with open(fn + "data.txt", "w") as f:
            f.write(data_txt(b, h_len=h_len))
    return root + "/"


def gen_state():
    st = torch.default_generator.get_state().numpy()
    _, left, _, nxt = struct.unpack_from("<QiiQ", st, 0)
    words = np.frombuffer(st[24:24 + 624 * 8].tobytes(), dtype=np.uint64).astype(np.uint32)
    return int(left), int(nxt), words


def save_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp per member, so a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def main():
    sys.path.insert(0, REF)
    import All_Schemes as AS  # noqa: E402  (the reference)
    torch.set_num_threads(1)
    tmp = tempfile.mkdtemp(prefix="qfl_hlen_")
    pairs, arrays, cases = {}, {}, []
    try:
        for k, (nbits, h_len, dim, vseed, seed, rot, gseed, pre) in enumerate(CASES):
            if h_len not in pairs:
                prefix = write_prefix(os.path.join(tmp, str(h_len)), h_len)
                pairs[h_len] = (AS.QuicFLSender(device="cpu", prefix=prefix), AS.QuicFLReceiver(device="cpu", prefix=prefix))
            tx, rx = pairs[h_len]
            x = np.random.RandomState(vseed).normal(0, 1.5, dim).astype(np.float32)
            torch.manual_seed(gseed)
            if pre:
                torch.rand(pre)                      # move the global generator off its seeded state
            left0, next0, words0 = gen_state()
            msg = tx.compress({"vec": torch.from_numpy(x.copy()), "seed": seed, "nbits": nbits, "rotation_seed": rot})
            left1, next1, words1 = gen_state()
            X = msg["X"].numpy()
            assert X.dtype == np.int64 and X.min() >= 0 and X.max() < (1 << nbits) and msg["h_len"] == h_len
            ei = np.flatnonzero(msg["exact_indeces"].numpy()).astype(np.int32)
            assert ei.size >= 2, (k, ei.size)        # exact coordinates in every case
            out = rx.decompress(msg).numpy().astype(np.float32)
            assert out.shape == (dim,)
            arrays[f"x{k}"] = x
            arrays[f"X{k}"] = X.astype(np.uint8)
            arrays[f"ei{k}"] = ei
            arrays[f"ev{k}"] = msg["exact_values"].numpy().astype(np.float32)
            arrays[f"st0_{k}"] = words0
            arrays[f"st1_{k}"] = words1
            arrays[f"rx{k}"] = out
            cases.append({"idx": k, "nbits": nbits, "h_len": h_len, "dim": dim, "D": int(X.size), "vseed": vseed,
                          "seed": seed, "rotation_seed": rot, "gseed": gseed, "pre": pre, "prng_seed": int(msg["prng_seed"]),
                          "scale_bits": int(np.float32(msg["scale"].item()).view(np.uint32)), "n_exact": int(ei.size),
                          "left0": left0, "next0": next0, "left1": left1, "next1": next1})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    save_npz(os.path.join(HERE, "quicfl_hlen_vectors.npz"), arrays)
    json.dump({"cases": cases}, open(os.path.join(HERE, "quicfl_hlen_vectors.json"), "w"), indent=1)
    print(len(cases), "cases; exact coordinates:", [c["n_exact"] for c in cases])


if __name__ == "__main__":
    main()
