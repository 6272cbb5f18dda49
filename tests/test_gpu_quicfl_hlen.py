"""GPU: QUIC-FL with an h_len that is not a power of two, and with the C ABI's boundary values 1 and
256.  h = word % h_len (AS:465/469, AS:528) is a mask for a power of two and a division otherwise,
at five sites of csrc/uq_quicfl_kernels.h (pass A in qfl_pass_a for KQ1 / KQ1a / KQ1ar / the team
and run kernels, the fused receiver, qfl_recv_rounds); the published tables use 64, 32 and 16, so
only these cases run the division.  Every form of sender, receiver and fused quantize (hooks 0, 4
and 2, the form read back through the plan hook), uint8 and int64 X, every row against the oracle
(oracle/uq_quicfl.py, oracle/uq_eden.py) bit for bit; and the reference's own outputs at h_len 48, 5
and 255 (tests/golden/make_golden_quicfl_hlen.py) through QuicFLSender / QuicFLReceiver."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import uq_eden as E
from oracle import uq_quicfl as Q
from tests import quicfl_plan_hook as H

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, HERE)
from quicfl_tables import DATA, recv_table, sender_tables  # noqa: E402

# (nbits, h_len, dim, input seed): D = 1024 the one-wave kernels, 8192 the sender's jump form with
# the receiver's team kernel, 32768 both jump forms.  The seeds were chosen on the CPU so that the
# oracle finds at least 2 exact coordinates in every row (asserted in _case).
CASES = [(1, 48, 700, 3), (1, 48, 5000, 1), (1, 48, 20000, 1), (3, 5, 5000, 2), (2, 255, 20000, 2), (4, 33, 700, 1),
         (2, 256, 5000, 3), (1, 1, 5000, 4)]
# forms (sender, receiver) without hooks by padded dim; hook 4 gives the team kernels from D = 8192
# here (1024 is below their shortest message), hook 2 the one-wave kernels
FORMS0 = {1024: (H.ONE_WAVE, H.ONE_WAVE), 8192: (H.JUMP, H.TEAM), 32768: (H.JUMP, H.JUMP)}
_cache = {}


def _tables(nbits, h_len):
    key = ("tab", nbits, h_len)
    if key not in _cache:
        tX, tp = sender_tables(nbits, h_len=h_len)
        _cache[key] = (tX, tp, dict(DATA[nbits], h_len=h_len), recv_table(nbits, h_len))
    return _cache[key]


def _sender(nbits, h_len):
    key = ("snd", nbits, h_len)
    if key not in _cache:
        import uqdme
        tX, tp, dd, _ = _tables(nbits, h_len)
        _cache[key] = uqdme.QuicFLSender(tables={nbits: (tX, tp, dd)})
    return _cache[key]


def _case(nbits, h_len, dim, vseed):
    """Three rows (n = 1 takes the first) with the oracle's message, end state and decompressed
    row of each, computed once per case."""
    import uqdme_amd.quicfl as q
    key = (nbits, h_len, dim)
    if key in _cache:
        return _cache[key]
    tX, tp, dd, rt = _tables(nbits, h_len)
    rng = np.random.default_rng(vseed * 1000 + h_len)
    x = (rng.standard_normal((3, dim)) * rng.uniform(0.5, 3, (3, 1))).astype(np.float32)
    seeds = [int(s) for s in rng.integers(0, 100, 3)]
    rots = [int(s) for s in rng.integers(0, 200, 3)]
    g = torch.Generator()
    states = np.empty((3, 626), np.uint32)
    oracle = []
    for j in range(3):
        g.manual_seed(int(j * 7919 + dim + h_len))
        torch.rand(1 + int(rng.integers(0, 1300)), generator=g)              # off the block edge
        states[j] = q.generator_words(g)[1]
        exp, gst = Q.compress(x[j], nbits, seeds[j], rots[j], tX, tp, dd["delta"], h_len,
                              (int(states[j, 0]), int(states[j, 1]), states[j, 2:]))
        assert int(exp["exact_indeces"].sum()) >= 2, (key, j)                # the oracle alone
        rec = E.quicfl_decompress(exp["X"], rt, h_len, exp["prng_seed"], exp["exact_indeces"], exp["exact_values"],
                                  exp["scale"], rots[j], dim)
        oracle.append((exp, gst, rec))
    _cache[key] = (torch.from_numpy(x), seeds, rots, states, oracle)
    return _cache[key]


def _form(lib, side, n, D, hooks):
    """The form of this thread's last call of that side, which is what the host plans for the shape."""
    p = H.last_plan(lib, side)
    assert p == H.plan(lib, side, n, D, hooks), (p, side, n, D, hooks)
    return p["form"]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("nbits,h_len,dim,vseed", CASES)
def test_every_form_matches_oracle_at_h_len(gpu_ready, nbits, h_len, dim, vseed, n):
    import uqdme_amd.quicfl as q
    from uqdme_amd._lib import load
    lib = load()
    rt, snd = _tables(nbits, h_len)[3], _sender(nbits, h_len)
    x, seeds, rots, states, oracle = _case(nbits, h_len, dim, vseed)
    x, seeds, rots, states = x[:n], seeds[:n], rots[:n], states[:n]
    D = 1 << (dim - 1).bit_length()
    seen = set()
    for hooks in (0, 4, 2):
        want = FORMS0[D] if hooks == 0 else ((H.ONE_WAVE,) * 2 if hooks == 2 or D == 1024 else (H.TEAM,) * 2)
        prev = lib.uq_test_set_quicfl_hooks(hooks)
        try:
            for dt in (torch.uint8, torch.int64):
                m, st = q.quicfl_compress(x, nbits, seeds, rots, sender=snd, px_states=states, x_dtype=dt, _state_out=True)
                assert _form(lib, H.SENDER, n, D, hooks) == want[0], (hooks, dt)
                out = q.quicfl_decompress_messages(m, rt).cpu().numpy()
                assert _form(lib, H.RECEIVER, n, D, hooks) == want[1], (hooks, dt)
                assert m.X.dtype == dt and m.h_len == h_len
                for j in range(n):
                    exp, gst, rec = oracle[j]
                    tag = (hooks, dt, j)
                    assert np.array_equal(m.X[j].cpu().numpy().astype(np.int64), exp["X"]), tag
                    assert np.array_equal(m.exact_mask[j].cpu().numpy(), exp["exact_indeces"]), tag
                    cnt = int(m.exact_count[j])
                    assert cnt == int(exp["exact_indeces"].sum()) and cnt >= 2, tag
                    assert (m.exact_vals[j, :cnt].cpu().numpy().view(np.uint32).tolist()
                            == exp["exact_values"].view(np.uint32).tolist()), tag
                    assert np.float32(m.scale[j].item()).view(np.uint32) == np.float32(exp["scale"]).view(np.uint32), tag
                    assert (st[j, 0], st[j, 1]) == (gst[0], gst[1]) and np.array_equal(st[j, 2:], gst[2]), tag
                    assert out[j].view(np.uint32).tolist() == rec.view(np.uint32).tolist(), tag
            fo, fst, fsc = q.quicfl_quantize(x, nbits, seeds, rots, sender=snd, recv_table=rt, px_states=states)
            assert _form(lib, H.SENDER, n, D, hooks) == want[0], hooks
            fo = fo.cpu().numpy()
            for j in range(n):
                exp, gst, rec = oracle[j]
                assert fo[j].view(np.uint32).tolist() == rec.view(np.uint32).tolist(), (hooks, j)
                assert np.float32(fsc[j].item()).view(np.uint32) == np.float32(exp["scale"]).view(np.uint32), (hooks, j)
                assert (fst[j, 0], fst[j, 1]) == (gst[0], gst[1]) and np.array_equal(fst[j, 2:], gst[2]), (hooks, j)
            seen.add(want)
        finally:
            lib.uq_test_set_quicfl_hooks(prev)
    assert len(seen) == (1 if D == 1024 else 3)


@pytest.mark.parametrize("hooks", [0, 4, 2])
def test_reference_fixtures_at_odd_h_len(gpu_ready, hooks):
    """The reference's own compress and decompress outputs at h_len 48, 5 and 255 (dims 1000 and
    5000) through QuicFLSender.compress and QuicFLReceiver.decompress on the same synthetic
    tables: message, scale, the global generator's end state and the decompressed vector."""
    import uqdme
    import uqdme_amd.quicfl as q
    from uqdme_amd._lib import load
    lib = load()
    meta = json.load(open(os.path.join(HERE, "quicfl_hlen_vectors.json")))
    z = np.load(os.path.join(HERE, "quicfl_hlen_vectors.npz"))
    assert len(meta["cases"]) == 6
    prev = lib.uq_test_set_quicfl_hooks(hooks)
    try:
        for c in meta["cases"]:
            k, b, h = c["idx"], c["nbits"], c["h_len"]
            rt, snd = _tables(b, h)[3], _sender(b, h)
            rx = uqdme.QuicFLReceiver(tables={b: rt})
            torch.manual_seed(c["gseed"])
            if c["pre"]:
                torch.rand(c["pre"])
            w0 = q.generator_words(torch.default_generator)[1]
            assert (w0[0], w0[1]) == (c["left0"], c["next0"]) and np.array_equal(w0[2:], z[f"st0_{k}"])
            msg = snd.compress({"vec": torch.from_numpy(z[f"x{k}"]), "seed": c["seed"], "nbits": b,
                                "rotation_seed": c["rotation_seed"]})
            D = c["D"]
            sform = _form(lib, H.SENDER, 1, D, hooks)
            assert sform == (H.ONE_WAVE if hooks == 2 or D == 1024 else H.TEAM if hooks == 4 else H.JUMP)
            assert msg["prng_seed"] == c["prng_seed"] and msg["dim"] == c["dim"] and msg["h_len"] == h
            assert np.array_equal(msg["X"].cpu().numpy(), z[f"X{k}"].astype(np.int64)), k
            assert np.array_equal(np.flatnonzero(msg["exact_indeces"].cpu().numpy()), z[f"ei{k}"]), k
            assert msg["exact_values"].cpu().numpy().view(np.uint32).tolist() == z[f"ev{k}"].view(np.uint32).tolist(), k
            assert int(msg["scale"].cpu().numpy().view(np.uint32)) == c["scale_bits"], k
            w1 = q.generator_words(torch.default_generator)[1]
            assert (w1[0], w1[1]) == (c["left1"], c["next1"]) and np.array_equal(w1[2:], z[f"st1_{k}"]), k
            out = rx.decompress(msg).cpu().numpy()
            rform = _form(lib, H.RECEIVER, 1, D, hooks)
            assert rform == (H.ONE_WAVE if hooks == 2 or D == 1024 else H.TEAM)
            assert out.view(np.uint32).tolist() == z[f"rx{k}"].view(np.uint32).tolist(), k
    finally:
        lib.uq_test_set_quicfl_hooks(prev)
