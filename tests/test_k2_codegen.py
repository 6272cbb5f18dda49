"""CPU: what the stream kernels compile to for gfx950 (tools/k2_codegen.py).  The tile loop keeps
no scratch: a spilled loop invariant comes back through a scratch load once per tile, scratch
loads share vmcnt with the tile's buffer stores and loads and retire in issue order, so a wait
for one is a wait for an HBM round trip in the middle of a tile.  The only vector-memory waits
inside the loop are to be the four before the staging writes of the prefetched tile, and with
the loads issued after the stores they count 3, 2, 1, 0.

Where this stands: every stream and small instantiation has 0 spilled VGPRs and 0 B of scratch
(was 15 / 64 B in <1,1,1,1>, 8 / 36 B in <1,1,1,0> and <1,0,1,0>) and exactly the four staging
waits.  In <1,1,1,1> (the bench step) the last of them also waits for the codes store of the
tile before, issued right after pass 2: with no store acknowledged before the q stores and the
loads go out its K2 takes 1.67-1.71 ms on MI355X against 1.63-1.65 ms for the parent commit,
which waited for its first store by accident, and 1.62-1.63 ms this way."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("k2_codegen", os.path.join(ROOT, "tools", "k2_codegen.py"))
K = importlib.util.module_from_spec(spec)
spec.loader.exec_module(K)

pytestmark = pytest.mark.skipif(not K.have_hipcc(), reason="hipcc is absent")


@pytest.fixture(scope="module")
def rep():
    return K.report()


@pytest.mark.parametrize("inst", ["1,1,1,1", "1,1,1,0", "1,0,1,0"])
def test_stream_loop_has_no_scratch_and_only_the_staging_waits(rep, inst):
    r = rep[f"quantize_stream_kernel<{inst}>"]
    md = r["meta"]
    print(inst, md, r["waits"])
    assert md[".vgpr_count"] <= 128                    # __launch_bounds__(256, 4): four workgroups per CU
    assert md[".group_segment_fixed_size"] <= 40960    # ... and their LDS
    assert md[".private_segment_fixed_size"] == 0
    assert r["loop"] is not None
    assert [v for _, v, _ in r["waits"]] == [3, 2, 1, 0], r["waits"]
    assert all(nxt.startswith("ds_write_b128") for _, _, nxt in r["waits"]), r["waits"]


def test_every_k2_instantiation_is_reported(rep):
    names = sorted(rep)
    assert sum(n.startswith("quantize_stream_kernel<") for n in names) == 6, names
    assert sum(n.startswith("quantize_small_kernel<") for n in names) == 5, names
    for n in names:
        assert set(rep[n]["meta"]) == set(K.KEYS), n
