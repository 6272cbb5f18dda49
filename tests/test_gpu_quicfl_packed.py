"""QUIC-FL messages at their rate on the GPU: the converters against the NumPy model of the layout
(tests/quicfl_packed_model.py), the packed sender and receiver against the u8 entry points at the smallest shapes
that reach each dispatch form (one-wave, team, jump and its two-wave instance), fused against the converter path
through the test hook, the reference's own fixtures, malformed index lists, and payload_bits / nbytes."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import quicfl_packed_model as PM
from tests import quicfl_plan_hook as H

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, HERE)
from quicfl_tables import DATA, sender_tables  # noqa: E402

FUSED, CONVERTER = 1, 2
X_RANGE, BAD_EXACT = 8, 32


@pytest.fixture(scope="module")
def uq(gpu_ready):
    import uqdme
    return uqdme


@pytest.fixture(scope="module")
def lib(uq):
    return uq.load_library()


@pytest.fixture(scope="module")
def sender(uq):
    return uq.QuicFLSender(tables={b: (*sender_tables(b), DATA[b]) for b in (1, 2, 3, 4)})


@pytest.fixture(scope="module")
def recv():
    return (json.load(open(os.path.join(HERE, "quicfl_recv_vectors.json"))), np.load(os.path.join(HERE, "quicfl_recv_vectors.npz")))


def packed_form(lib, side):
    buf = (ctypes.c_int64 * 4)()
    assert lib.uq_test_last_quicfl_packed_plan(side, buf, 4) == 0
    return int(buf[1])


def words(t):
    return t.cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class hooks:
    """uq_test_set_quicfl_hooks / uq_test_set_quicfl_packed_hooks for a block"""

    def __init__(self, lib, qfl=0, packed=0):
        self.lib, self.new = lib, (qfl, packed)

    def __enter__(self):
        self.old = (self.lib.uq_test_set_quicfl_hooks(self.new[0]), self.lib.uq_test_set_quicfl_packed_hooks(self.new[1]))

    def __exit__(self, *a):
        self.lib.uq_test_set_quicfl_hooks(self.old[0])
        self.lib.uq_test_set_quicfl_packed_hooks(self.old[1])


# ---- converters ---------------------------------------------------------------------------
def pack_raw(lib, X, nbits, mask):
    from uqdme_amd._runtime import ptr, stream_ptr
    from uqdme_amd.quicfl import _X_KIND
    n, D = X.shape
    pay = torch.full((n, PM.pitch(D, nbits)), -1, dtype=torch.int32, device="cuda")            # prefilled with 0xFF
    eidx = torch.full((n, D), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    pbits = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    info = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = lib.uq_quicfl_pack_x(ptr(X), _X_KIND[X.dtype], n, D, nbits, ptr(mask), ptr(pay), ptr(eidx), ptr(cnt), ptr(pbits), ptr(info),
                              stream_ptr(X.device))
    assert rc == 0, lib.uq_last_error()
    return pay, eidx, cnt, pbits, info


def unpack_raw(lib, pay, D, nbits, eidx, cnt):
    from uqdme_amd._runtime import ptr, stream_ptr
    n = pay.shape[0]
    X = torch.full((n, D), 255, dtype=torch.uint8, device="cuda")
    mask = torch.full((n, D), 255, dtype=torch.uint8, device="cuda")
    info = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = lib.uq_quicfl_unpack_x(ptr(pay), n, D, nbits, ptr(eidx), ptr(cnt), ptr(X), ptr(mask), ptr(info), stream_ptr(pay.device))
    assert rc == 0, lib.uq_last_error()
    return X, mask, info


def edge_masks(D):
    """none set, all set, and single bits at the edges of halfwords, rounds (624) and the row, wherever < D"""
    out = [np.zeros(D, bool), np.ones(D, bool)]
    for i in sorted({0, 15, 16, 623, 624, 1247, 1248, D - 1}):
        if i < D:
            m = np.zeros(D, bool)
            m[i] = True
            out.append(m)
    return out


@pytest.mark.parametrize("D", [1, 16, 32, 64, 1024, 2048, 8192])
@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
def test_converters_against_the_model(lib, D, nbits):
    n = 3
    rng = np.random.default_rng(1000 * nbits + D)
    masks = edge_masks(D)
    masks += [rng.random(D) < 0.02] * (-len(masks) % n)
    for g in range(0, len(masks), n):
        mk = np.stack(masks[g:g + n])
        X = rng.integers(0, 1 << nbits, (n, D)).astype(np.uint8)
        model = [PM.pack(X[j], nbits, mk[j]) for j in range(n)]
        Xd = torch.from_numpy(X).cuda()
        if g == 0:                                           # the other X kinds once per shape
            Xd = Xd.to(torch.int64)
        elif g == n:
            Xd = Xd.to(torch.int32)
        md = torch.from_numpy(mk.astype(np.uint8)).cuda()
        pay, eidx, cnt, pbits, info = pack_raw(lib, Xd, nbits, md)
        assert np.array_equal(words(pay), np.stack([m[0] for m in model]))                     # every word of the pitch
        assert cnt.tolist() == [m[1].size for m in model] and info.tolist() == [0] * n
        assert pbits.tolist() == [m[2] for m in model] == [nbits * D + 64 * c for c in cnt.tolist()]
        for j in range(n):
            assert np.array_equal(eidx[j, :model[j][1].size].cpu().numpy(), model[j][1])
            assert (eidx[j, model[j][1].size:] == -1).all()                                    # nothing behind the list
        X2, m2, info2 = unpack_raw(lib, pay, D, nbits, eidx, cnt)
        assert torch.equal(X2, torch.from_numpy(X).cuda()) and torch.equal(m2, md) and info2.tolist() == [0] * n
    # X = 2^nbits in one row: flagged there, stored as 0; the other rows as they were
    X = rng.integers(0, 1 << nbits, (n, D)).astype(np.uint8)
    X[1, D // 2] = 1 << nbits
    pay, eidx, cnt, pbits, info = pack_raw(lib, torch.from_numpy(X).cuda(), nbits, torch.zeros((n, D), dtype=torch.uint8, device="cuda"))
    assert info.tolist() == [0, X_RANGE, 0] and cnt.tolist() == [0, 0, 0]
    X[1, D // 2] = 0
    assert np.array_equal(words(pay), np.stack([PM.pack(X[j], nbits)[0] for j in range(n)]))


# ---- sender, receiver, fused == converter ------------------------------------------------------
def gen_rows(n, dim, seed, flat_row=None):
    """Gaussian rows of differing scales on the device; flat_row: a one-hot row, whose rotation has every
    coordinate at +-1 / sqrt(D) of the norm, so no coordinate is exact"""
    dev = "cuda" if n * dim > (1 << 16) else "cpu"          # (small shapes from the CPU generator: the same rows anywhere)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = (torch.randn((n, dim), generator=g, device=dev) * (1.0 + (torch.arange(n, device=dev) % 3)[:, None])).cuda()
    if flat_row is not None:
        x[flat_row] = 0
        x[flat_row, dim // 3] = 2.5
    return x


def states(n, seed):
    """n torch CPU generators at different positions of their streams, as px_states rows"""
    from uqdme_amd.quicfl import generator_words
    rows = []
    for j in range(n):
        g = torch.Generator()
        g.manual_seed(seed + j)
        torch.rand(1 + 97 * j, generator=g)
        rows.append(generator_words(g)[1])
    return np.stack(rows)


# name -> (n, dim, QUIC-FL hooks, sender's form, two-wave, row without exact coordinates, all of nbits 1..4)
SEND = {
    "one-wave 700": (1, 700, 0, H.ONE_WAVE, False, None, False),
    "one-wave 2048": (1, 2048, 0, H.ONE_WAVE, False, None, True),
    "one-wave 3 x 4096": (3, 4096, 2, H.ONE_WAVE, False, 1, False),
    "team 4096": (1, 4096, 0, H.TEAM, False, None, True),
    "team 3 x 5000": (3, 5000, 4, H.TEAM, False, None, False),
    "jump 8192": (1, 8192, 0, H.JUMP, False, None, True),
    "jump 2^15": (1, 1 << 15, 0, H.JUMP, False, None, False),
    "jump 17 x 2^15": (17, 1 << 15, 0, H.JUMP, False, 5, False),
    "jump two-wave 257 x 2^18": (257, 1 << 18, 0, H.JUMP, True, None, False),
}
SEND_CASES = [(k, b) for k, v in SEND.items() for b in ((1, 2, 3, 4) if v[6] else (1, 4))]


def send_pair(uq, lib, sender, name, nbits, packed_hook=0):
    """the u8 and the packed message of a SEND shape from the same inputs, seeds and generators, with end states"""
    n, dim, qh, form, w2, flat, _ = SEND[name]
    x = gen_rows(n, dim, 7 + n, flat)
    seeds, rots = list(range(3, 3 + n)), list(range(50, 50 + n))
    gens = dict(px_states=states(n, 11)) if n <= 32 else dict(px_seeds=list(range(1000, 1000 + n)))
    with hooks(lib, qh, packed_hook):
        u8, st_u = uq.quicfl_compress(x, nbits, seeds, rots, sender=sender, _state_out=True, **gens)
        plan_u = H.last_plan(lib, H.SENDER)
        pk, st_p = uq.quicfl_compress(x, nbits, seeds, rots, sender=sender, packed=True, _state_out=True, **gens)
        plan_p = H.last_plan(lib, H.SENDER)
        pform = packed_form(lib, H.SENDER)
    assert plan_u == plan_p and plan_p["form"] == form and plan_p["two_wave"] == w2, (plan_u, plan_p)
    assert pform == (CONVERTER if packed_hook else FUSED)
    return u8, st_u, pk, st_p


def assert_same_message(uq, u8, st_u, pk, st_p, flat):
    n, D = u8.X.shape
    nbits = u8.nbits
    assert pk.packed and pk.X is None and pk.exact_mask is None and not u8.packed
    assert pk.payload.shape == (n, PM.pitch(D, nbits)) and pk.exact_index.shape == (n, D)
    un = uq.quicfl_unpack(pk)
    assert torch.equal(un.X, u8.X) and torch.equal(un.exact_mask, u8.exact_mask)
    cnt = u8.exact_count
    assert torch.equal(pk.exact_count, cnt) and same_bits(pk.scale, u8.scale)
    assert int(cnt.max()) > 0 and (flat is None or int(cnt[flat]) == 0)                        # checked, not assumed
    keep = torch.arange(D, device="cuda")[None, :] < cnt.cuda()[:, None]
    assert same_bits(pk.exact_vals[keep], u8.exact_vals[keep])
    assert torch.equal(pk.exact_index[keep].long(), torch.nonzero(u8.exact_mask)[:, 1])        # ascending, row by row
    assert (st_u is None and st_p is None) or np.array_equal(st_u, st_p)
    # the message's size, and the converter on the u8 message gives the packed sender's rows
    bits = nbits * D + 64 * cnt.to(torch.int64)
    assert torch.equal(pk.payload_bits.cpu(), bits)
    assert pk.nbytes == int(((bits + 7) // 8).sum()) == int(bits.sum()) // 8
    again = uq.quicfl_pack(u8)
    assert torch.equal(again.payload, pk.payload) and torch.equal(again.payload_bits, pk.payload_bits)
    assert torch.equal(again.exact_index[keep], pk.exact_index[keep]) and torch.equal(again.exact_count, cnt)
    # every bit of the pitch that names no coordinate is 0 (the planes hold X and nothing else)
    if D % 32:
        assert all(PM.unused_bits_zero(words(pk.payload)[j], D, nbits) for j in range(n))


@pytest.mark.parametrize("name,nbits", SEND_CASES)
def test_sender_packed_is_the_u8_message(uq, lib, sender, name, nbits):
    u8, st_u, pk, st_p = send_pair(uq, lib, sender, name, nbits)
    assert_same_message(uq, u8, st_u, pk, st_p, SEND[name][5])


# name of the SEND shape whose messages the receiver takes -> the receiver's form (1 x 4096, 1 x 8192, 1 x 2^15)
RECV = {"team 4096": H.ONE_WAVE, "jump 8192": H.TEAM, "jump 2^15": H.JUMP}


def receive_both(uq, lib, u8, pk, tab, form, packed_hook=0):
    with hooks(lib, 0, packed_hook):
        a = uq.quicfl_decompress_messages(u8, tab)
        plan_u = H.last_plan(lib, H.RECEIVER)
        b = uq.quicfl_decompress_messages(pk, tab)
        plan_p = H.last_plan(lib, H.RECEIVER)
        assert packed_form(lib, H.RECEIVER) == (CONVERTER if packed_hook else FUSED)
    assert plan_u == plan_p and plan_p["form"] == form, (plan_u, plan_p)
    return a, b


@pytest.mark.parametrize("name", list(RECV))
@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
def test_receiver_packed_is_the_u8_receiver(uq, lib, sender, recv, name, nbits):
    u8, st_u, pk, st_p = send_pair(uq, lib, sender, name, nbits)
    a, b = receive_both(uq, lib, u8, pk, recv[1][f"recv{nbits}"], RECV[name])
    assert same_bits(a, b)


# SEND shape (one per form of the sender) -> the form the receiver takes on its messages (one per form too)
BOTH = {"one-wave 3 x 4096": H.ONE_WAVE, "team 3 x 5000": H.TEAM, "jump 17 x 2^15": H.TEAM, "jump 2^15": H.JUMP}


@pytest.mark.parametrize("name", list(BOTH))
def test_fused_is_the_converter_path(uq, lib, sender, recv, name):
    nbits = 2
    u8, st_u, pk, st_p = send_pair(uq, lib, sender, name, nbits)
    u8c, st_uc, pkc, st_pc = send_pair(uq, lib, sender, name, nbits, packed_hook=1)
    assert torch.equal(pk.payload, pkc.payload) and torch.equal(pk.payload_bits, pkc.payload_bits)
    assert torch.equal(pk.exact_count, pkc.exact_count) and same_bits(pk.scale, pkc.scale)
    keep = torch.arange(pk.exact_index.shape[1], device="cuda")[None, :] < pk.exact_count.cuda()[:, None]
    assert torch.equal(pk.exact_index[keep], pkc.exact_index[keep]) and same_bits(pk.exact_vals[keep], pkc.exact_vals[keep])
    assert np.array_equal(st_p, st_pc)
    tab = recv[1][f"recv{nbits}"]
    form = BOTH[name]
    a, b = receive_both(uq, lib, u8, pk, tab, form)
    ac, bc = receive_both(uq, lib, u8, pk, tab, form, packed_hook=1)
    assert same_bits(a, b) and same_bits(b, bc) and same_bits(a, ac)


# ---- the reference's fixtures ----------------------------------------------------------------
def test_reference_sender_fixtures_through_the_packed_sender(uq, sender):
    from uqdme_amd.quicfl import generator_words
    from tests.test_gpu_quicfl_sender import gen, set_global
    meta = json.load(open(os.path.join(HERE, "quicfl_sender_vectors.json")))
    z = np.load(os.path.join(HERE, "quicfl_sender_vectors.npz"))
    checked = 0
    for c in meta["cases"]:
        k = c["idx"]
        if c["tables"] != "pub" or "error" in c or c["D"] > (1 << 17):
            continue
        x = z[f"x{k}"] if c.get("x_stored") else gen(c["kind"], c["vseed"], c["dim"])
        set_global(c["gseed"], c["pre"])
        _, w = generator_words(torch.default_generator)
        pk, new = uq.quicfl_compress(torch.from_numpy(x).view(1, -1), c["nbits"], [c["seed"]], [c["rotation_seed"]], sender=sender,
                                     px_states=w[None, :], packed=True, _state_out=True)
        un = uq.quicfl_unpack(pk)
        cnt = int(pk.exact_count[0])
        assert np.array_equal(un.X[0].cpu().numpy().astype(np.int64), z[f"X{k}"].astype(np.int64)), k
        assert np.array_equal(np.flatnonzero(un.exact_mask[0].cpu().numpy()), z[f"ei{k}"]), k
        assert np.array_equal(pk.exact_index[0, :cnt].cpu().numpy(), z[f"ei{k}"]), k
        assert pk.exact_vals[0, :cnt].cpu().numpy().view(np.uint32).tolist() == z[f"ev{k}"].view(np.uint32).tolist(), k
        assert int(pk.scale[0].cpu().numpy().view(np.uint32)) == c["scale_bits"], k
        assert (new[0][0], new[0][1]) == (c["left1"], c["next1"]) and np.array_equal(new[0][2:], z[f"st1_{k}"]), k
        checked += 1
    assert checked >= 8


def test_reference_receiver_fixtures_through_the_packed_receiver(uq, recv):
    rmeta, rz = recv
    checked = 0
    for c in rmeta["cases"]:
        i = c["idx"]
        X = rz[f"X{i}"].astype(np.int64)
        if "error" in c or f"out{i}" not in rz.files or X.min() < 0 or X.max() >= (1 << c["nbits"]):
            continue
        D = X.shape[0]
        mask = rz[f"mask{i}"].astype(bool) if f"mask{i}" in rz.files else np.zeros(D, bool)
        vals = np.zeros(D, np.float32)
        v = rz[f"vals{i}"] if f"vals{i}" in rz.files else np.zeros(0, np.float32)
        if v.size != int(mask.sum()):
            continue                                         # (a broadcast value: the drop-in's affair)
        vals[:v.size] = v
        msg = uq.QuicFLMessages(torch.from_numpy(X)[None], torch.from_numpy(mask)[None], torch.from_numpy(vals)[None].cuda(),
                                torch.tensor([v.size], dtype=torch.int32), torch.tensor([c["scale"]], dtype=torch.float32),
                                torch.tensor([c["prng_seed"]]), torch.tensor([c["rotation_seed"]]), c["dim"], c["nbits"], c["h_len"])
        pk = uq.quicfl_pack(msg)
        assert pk.packed and int(pk.payload_bits[0]) == c["nbits"] * D + 64 * v.size
        out = uq.quicfl_decompress_messages(pk, rz[f"recv{c['nbits']}"])[0].cpu().numpy()
        assert out.view(np.uint32).tolist() == rz[f"out{i}"].view(np.uint32).tolist(), i
        checked += 1
    assert checked >= 8


# ---- malformed lists ---------------------------------------------------------------------------
@pytest.mark.parametrize("packed_hook", [0, 1])
def test_bad_lists_flag_their_row_only(uq, lib, sender, recv, packed_hook):
    from uqdme_amd._runtime import ptr, stream_ptr
    nbits, n, D = 2, 5, 4096
    x = gen_rows(n, D, 99)
    pk = uq.quicfl_compress(x, nbits, list(range(n)), list(range(n)), sender=sender, px_seeds=list(range(n)), packed=True)
    cnt = pk.exact_count.clone()
    assert int(cnt.min()) >= 3
    good = uq.quicfl_decompress_messages(uq.quicfl_unpack(pk), recv[1][f"recv{nbits}"])
    eidx = pk.exact_index.clone()
    cnt[0] = D + 1                                           # a count above D
    eidx[1, 1] = D                                           # an index >= D
    eidx[2, 0], eidx[2, 1] = pk.exact_index[2, 1], pk.exact_index[2, 0]        # a descending pair
    eidx[3, 2] = eidx[3, 1]                                  # a duplicate
    tab = torch.as_tensor(recv[1][f"recv{nbits}"], dtype=torch.float32).cuda().contiguous()
    G = 4096                                                 # guard floats on either side of pre
    buf = torch.full((G + n * D + G,), float("nan"), dtype=torch.float32, device="cuda")
    pre = buf[G:G + n * D]
    info = torch.zeros(n, dtype=torch.int32, device="cuda")
    seeds32 = pk.prng_seeds.to(torch.int32).cuda()
    cd = cnt.to(torch.int32).cuda()
    wb = ctypes.c_size_t()
    assert lib.uq_quicfl_receive_packed_workspace_bytes(n, D, ctypes.byref(wb)) == 0
    ws = torch.empty(wb.value, dtype=torch.uint8, device="cuda")
    with hooks(lib, 0, packed_hook):
        rc = lib.uq_quicfl_receive_packed_f32(ptr(pk.payload), nbits, n, D, ptr(tab), tab.shape[0], tab.shape[1], ptr(seeds32),
                                              ptr(eidx), ptr(pk.exact_vals), ptr(cd), ptr(pk.scale), ptr(pre), ptr(info), ptr(ws),
                                              wb.value, stream_ptr(pre.device))
    assert rc == 0, lib.uq_last_error()
    assert packed_form(lib, H.RECEIVER) == (CONVERTER if packed_hook else FUSED)
    assert [f & BAD_EXACT for f in info.tolist()] == [BAD_EXACT] * 4 + [0] and [f & ~BAD_EXACT for f in info.tolist()] == [0] * n
    from uqdme_amd.eden import randomized_inverse_hadamard_transform
    out4 = randomized_inverse_hadamard_transform(pre.view(n, D)[4:5].clone(), pk.rotation_seeds[4:5])
    assert same_bits(out4, good[4:5])                        # the well-formed row is right
    assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n * D:]).all()                   # nothing outside pre
    assert not torch.isnan(pre).any()                        # and every coordinate of every row was written
