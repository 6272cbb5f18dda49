"""The unbiased dispatcher's decision table (host only: uq_test_unbiased_plan launches nothing).

unbiased_codes_impl picks one of five K2 forms and a template instance of it from the call's
shape; it launches what plan_unbiased / chunk_plan (csrc/uq_unbiased.hip) return, and the hook
reports the same plan.  Each threshold is pinned on both sides, with 1024 resident stream
workgroups (slots) so that the segment split does not depend on a device."""
import ctypes

import pytest

import uqdme
from tests import plan_hook as H


@pytest.fixture(scope="module")
def lib():
    return uqdme.load_library()


def expect(lib, want, *a, **k):
    rc, p = H.plan(lib, *a, **k)
    assert rc == 0, (a, k, lib.uq_last_error())
    form = want.pop("form")
    assert H.FORM_NAMES[p["form"]] == form, (a, k, p)
    for key, v in want.items():
        assert p[key] == v, (a, k, key, p)
    return p


def test_small_until_grain_then_phased(lib):
    expect(lib, dict(form="small", V=True, tiles=8, chunks=1), 1, 32767)
    expect(lib, dict(form="phased", V=True, prefixed=False, tiles=8, chunks=1, nj=1), 1, 32768)
    expect(lib, dict(form="small", V=True), 1, 4099)               # n = 1 is V for any d
    expect(lib, dict(form="phased", V=False), 1, 32768, x16=False)  # ... with an aligned x
    expect(lib, dict(form="phased", V=False), 1, 4099, out16=False)
    expect(lib, dict(form="small", V=True), 1, 4099, out=False, out16=False, codes=True)
    expect(lib, dict(form="phased", V=False), 2, 4099)             # unaligned rows never take the small kernel


def test_prefix_launch_from_four_clients(lib):
    expect(lib, dict(form="phased", V=True, prefixed=True, nj=4), 4, 32768)
    expect(lib, dict(form="phased", V=True, prefixed=False, nj=3), 3, 32768)


def test_segments_from_1024_tiles(lib):
    expect(lib, dict(form="phased", V=True, tiles=8, prefixed=True), 127, 32768)       # 1016 tiles
    expect(lib, dict(form="segments", V=True, tiles=8, R=1, nseg=8), 128, 32768)       # 1024 tiles
    expect(lib, dict(form="segments", R=2, nseg=5, tiles=9), 128, 36864)
    expect(lib, dict(form="segments", R=2, nseg=128, tiles=256, prefixed=True), 6, 1 << 20)
    expect(lib, dict(form="segments", R=2, nseg=256, tiles=512, prefixed=False), 3, 1 << 21)
    # the split follows the resident workgroups: fewer slots, longer segments
    expect(lib, dict(form="segments", R=7, nseg=37), 6, 1 << 20, slots=256)
    # unaligned rows cannot stream
    expect(lib, dict(form="phased", V=False), 6, (1 << 20) + 3)


def test_stream_from_256_clients(lib):
    expect(lib, dict(form="stream", V=True, chunks=1), 256, 32768)
    expect(lib, dict(form="small", V=True), 256, 32764)
    expect(lib, dict(form="phased", V=False, prefixed=True), 256, 32769)
    expect(lib, dict(form="segments", V=True), 255, 32768)
    for kind in (dict(out=True, codes=False), dict(out=True, codes=True), dict(out=False, codes=True)):
        p = expect(lib, dict(form="stream"), 256, 32768, **kind)
        assert (p["Q"], p["C"]) == (kind["out"], kind["codes"])


def test_pitches_and_alignment(lib):
    d = 8192
    expect(lib, dict(form="phased", V=False), 300, d, ldq=d + 3)
    expect(lib, dict(form="small", V=True, C=True, CV=True), 300, d, ldq=d + 64, ldc=d + 256, codes=True)
    expect(lib, dict(form="small", V=True, CV=False), 300, d, ldq=d + 64, ldc=d + 5, codes=True)
    expect(lib, dict(form="small", CV=False), 300, 4100, codes=True)                   # d % 16 != 0
    expect(lib, dict(form="stream", CV=False), 256, 32772, codes=True)
    expect(lib, dict(form="stream", CV=True), 256, 32768, codes=True)
    expect(lib, dict(form="stream", CV=False), 256, 32768, codes=True, codes16=False)  # base off by 1
    expect(lib, dict(form="stream", CV=False), 256, 32768, codes=True, ldc=32768 + 7)
    expect(lib, dict(form="small", CV=True), 1, 4096, codes=True, ldc=4099)            # one row: any pitch
    expect(lib, dict(form="small", CV=True), 300, d)                                   # without codes CV is set
    # pitches below d are refused as the calls refuse them
    assert H.plan(lib, 300, d, ldq=d - 1)[0] == -1
    assert H.plan(lib, 300, d, ldc=d - 1, codes=True)[0] == -1
    assert H.plan(lib, 300, d, ldc=d - 1, codes=False)[0] == 0


def test_chunks_of_65535_clients(lib):
    expect(lib, dict(form="phased", V=False, chunks=1, nj=65535, tiles=1), 65535, 5)
    expect(lib, dict(form="phased", V=False, chunks=2, nj=1, prefixed=False), 65536, 5)
    expect(lib, dict(form="phased", V=False, chunks=2, nj=2), 65537, 5)
    expect(lib, dict(form="small", chunks=1), 65536, 8)


def test_l1_given_is_recorded(lib):
    for n, d in ((300, 4096), (256, 32768), (3, 32768)):
        assert expect(lib, dict(form=H.FORM_NAMES[H.plan(lib, n, d)[1]["form"]]), n, d, l1=True)["l1_given"]
        assert not H.plan(lib, n, d)[1]["l1_given"]


def test_nibbles_only_in_the_stream_form(lib):
    p = expect(lib, dict(form="stream-nibbles", V=True, Q=True, C=True, CV=True), 256, 4096, ldc=2048, codes=True,
               nib=True)
    assert p["tiles"] == 1
    expect(lib, dict(form="stream-nibbles"), 256, 36864, ldc=36864 // 2 + 16, codes=True, nib=True)
    # the entry point refuses what is not the stream form before anything is planned or launched
    a = ctypes.c_void_p(256)
    for n, d in ((255, 4096), (256, 4100)):
        rc = lib.uq_type_unbiased_nibbles_ld_f32(a, a, d, a, d // 2 + (-(d // 2)) % 16, a, n, d, 100, a, None, None, 1,
                                                 a, 1 << 40, None)
        assert rc == -1, (n, d)
        assert b"4-bit codes need n >= 256" in lib.uq_last_error()
        assert H.plan(lib, n, d, ldc=d // 2, codes=True, nib=True)[0] == -1


def test_nothing_to_write_and_empty_batches(lib):
    assert H.plan(lib, 4, 100, out=False, codes=False)[0] == -1
    assert b"nothing to write" in lib.uq_last_error()
    a = ctypes.c_void_p(256)
    rc = lib.uq_type_unbiased_codes_ld_f32(a, None, 100, None, 100, None, 4, 100, 10, a, None, None, 1, a, 1 << 40, None)
    assert rc == -1 and b"nothing to write" in lib.uq_last_error()
    for n, d in ((0, 100), (4, 0)):
        rc, p = H.plan(lib, n, d)
        assert rc == 0 and p["form"] == H.NONE
    assert H.plan(lib, -1, 100)[0] == -1


def test_constants_and_offsets(lib):
    """The record geometry the GPU tests read back with, and the workspace offsets: three u64
    [n][tiles] arrays, the records, their counters, all inside uq_workspace_bytes."""
    n, d = 6, 1 << 20
    p = H.plan(lib, n, d)[1]
    assert (p["rec_per_client"], p["rec_clients"], p["rec_events"], p["fold_events"]) == (32, 256, 48, 256)
    assert p["rec_bytes"] == 16 + 48 * (8 * 3 + 8 + 16 * 4)
    sz = n * p["tiles"] * 8
    assert p["p_off"] == 256 and p["map0_off"] >= p["p_off"] + sz and p["map1_off"] >= p["map0_off"] + sz
    assert p["rec_off"] >= p["map1_off"] + sz
    assert p["cnt_off"] >= p["rec_off"] + n * 32 * p["rec_bytes"]
    b = ctypes.c_size_t()
    assert lib.uq_workspace_bytes(n, d, 1, ctypes.byref(b)) == 0 and b.value >= p["cnt_off"] + 4 * n
    # a short buffer gets the fields that fit
    buf = (ctypes.c_int64 * 3)(-7, -7, -7)
    assert lib.uq_test_unbiased_plan(n, d, d, d, 1, 1, 1, 1, 0, 0, 0, 1024, buf, 2) == 0
    assert list(buf) == [H.SEGMENTS, 1, -7]
