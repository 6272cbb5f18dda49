"""CPU: the QUIC-FL sender and receiver restatements (oracle/uq_quicfl.py compress, oracle/uq_eden.py
quicfl_decompress) against the reference's own QuicFLSender.compress and QuicFLReceiver.decompress
outputs for h_len values that are not powers of two -- 48, 5 and 255, where h = word % h_len is a
division (tests/golden/make_golden_quicfl_hlen.py) -- bit for bit; and word % h_len against
torch.randint itself, the boundary values 1 and 256 included."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import uq_eden as E
from oracle import uq_quicfl as Q

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, HERE)
from quicfl_tables import DATA, recv_table, sender_tables  # noqa: E402


def load():
    meta = json.load(open(os.path.join(HERE, "quicfl_hlen_vectors.json")))
    z = np.load(os.path.join(HERE, "quicfl_hlen_vectors.npz"))
    return meta, z


@pytest.mark.parametrize("h", [1, 3, 5, 33, 48, 100, 255, 256])
def test_randint_is_word_mod_h_len(h):
    g = torch.Generator().manual_seed(77 + h)
    got = torch.randint(0, h, (2000,), generator=g).numpy()
    assert np.array_equal(got, (E.mt19937(77 + h, 2000) % np.uint32(h)).astype(np.int64))


def test_fixture_covers_the_cases():
    meta, z = load()
    assert sorted({(c["nbits"], c["h_len"], c["dim"]) for c in meta["cases"]}) == [
        (1, 48, 1000), (1, 48, 5000), (2, 255, 1000), (2, 255, 5000), (3, 5, 1000), (3, 5, 5000)]
    assert all(c["n_exact"] >= 2 and c["n_exact"] == z[f"ei{c['idx']}"].size for c in meta["cases"])
    assert all(c["h_len"] & (c["h_len"] - 1) for c in meta["cases"])


def test_oracles_match_reference_at_odd_h_len():
    meta, z = load()
    for c in meta["cases"]:
        k, b, h = c["idx"], c["nbits"], c["h_len"]
        tX, tp = sender_tables(b, h_len=h)
        msg, gst = Q.compress(z[f"x{k}"], b, c["seed"], c["rotation_seed"], tX, tp, DATA[b]["delta"], h,
                              (c["left0"], c["next0"], z[f"st0_{k}"]))
        assert msg["prng_seed"] == c["prng_seed"] and msg["h_len"] == h and msg["X"].size == c["D"]
        assert int(np.float32(msg["scale"]).view(np.uint32)) == c["scale_bits"], k
        assert np.array_equal(msg["X"], z[f"X{k}"].astype(np.int64)), k
        assert np.array_equal(np.flatnonzero(msg["exact_indeces"]), z[f"ei{k}"]), k
        assert msg["exact_values"].view(np.uint32).tolist() == z[f"ev{k}"].view(np.uint32).tolist(), k
        assert (gst[0], gst[1]) == (c["left1"], c["next1"]) and np.array_equal(gst[2], z[f"st1_{k}"]), k
        # the receiver oracle on the reference's message (not on the sender oracle's)
        mask = np.zeros(c["D"], bool)
        mask[z[f"ei{k}"]] = True
        out = E.quicfl_decompress(z[f"X{k}"], recv_table(b, h), h, c["prng_seed"], mask, z[f"ev{k}"],
                                  np.uint32(c["scale_bits"]).view(np.float32), c["rotation_seed"], c["dim"])
        assert out.view(np.uint32).tolist() == z[f"rx{k}"].view(np.uint32).tolist(), k


def test_receive_pre_is_decompress_before_the_inverse_rht():
    meta, z = load()
    c = meta["cases"][0]
    k, b, h = c["idx"], c["nbits"], c["h_len"]
    mask = np.zeros(c["D"], np.uint8)
    mask[z[f"ei{k}"]] = 0x80                                      # any nonzero byte marks a coordinate
    sc = np.uint32(c["scale_bits"]).view(np.float32)
    pre = E.quicfl_receive_pre(z[f"X{k}"], recv_table(b, h), h, c["prng_seed"], mask, z[f"ev{k}"], sc)
    assert pre.dtype == np.float32 and pre.shape == (c["D"],)
    assert np.array_equal(pre[z[f"ei{k}"]].view(np.uint32), (z[f"ev{k}"] / sc).astype(np.float32).view(np.uint32))
    out = E.inverse_rht(pre, c["rotation_seed"])[:c["dim"]]
    assert out.view(np.uint32).tolist() == z[f"rx{k}"].view(np.uint32).tolist()
    # a length that is no power of two (the lookup has no RHT): the first coordinates of the same stream
    short = E.quicfl_receive_pre(z[f"X{k}"][:625], recv_table(b, h), h, c["prng_seed"], mask[:625],
                                 z[f"ev{k}"][:int(np.count_nonzero(mask[:625]))], sc)
    assert np.array_equal(short.view(np.uint32), pre[:625].view(np.uint32))
