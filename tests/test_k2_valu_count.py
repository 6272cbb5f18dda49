"""CPU: the vector-ALU instructions the stream kernels' tile loop issues (tools/k2_codegen.py,
tile_loop_valu), against the counts of commit 6a72f20 ("K2 stream loop: no scratch, only the four
staging waits"), taken with `python tools/k2_codegen.py --git 6a72f20` (profiles/k2_valu_parent.txt).

Two static counts per instantiation: every v_* instruction inside the tile loop (rare paths
included: the loop's code size), and those of the hot blocks that each thread runs once per full
regular tile of 16 elements (div4, pass 1 with its scan, pass 2).  Neither may grow, and the hot
count of <1,1,1,1>, the bench step's instantiation, stays strictly below the parent's 546 (34.1
per element; 474, 29.6 per element, when this test was written)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("k2_codegen", os.path.join(ROOT, "tools", "k2_codegen.py"))
K = importlib.util.module_from_spec(spec)
spec.loader.exec_module(K)

pytestmark = pytest.mark.skipif(not K.have_hipcc(), reason="hipcc is absent")

# commit 6a72f20: (v_* in the tile loop, v_* in the hot blocks)
PARENT = {"1,1,1,1": (2383, 546), "1,1,1,0": (2364, 530), "1,0,1,0": (2312, 481)}


@pytest.fixture(scope="module")
def rep():
    return K.report()


@pytest.mark.parametrize("inst", sorted(PARENT))
def test_valu_counts_do_not_exceed_the_parents(rep, inst):
    r = rep[f"quantize_stream_kernel<{inst}>"]
    in_loop, hot = PARENT[inst]
    print(inst, "in loop", r["valu_loop"], "of", in_loop, "hot", r["valu_hot"], "of", hot, r["hot_path"])
    parts = [part for _, part, _ in r["hot_path"]]
    assert parts.count("div4") == 4 and "pass 1" in parts and "pass 2" in parts, r["hot_path"]   # the blocks were found
    assert 0 < r["valu_loop"] <= in_loop
    assert 0 < r["valu_hot"] <= hot


def test_bench_instantiation_hot_path_is_below_the_parents(rep):
    r = rep["quantize_stream_kernel<1,1,1,1>"]
    print("hot", r["valu_hot"], r["valu_hot"] / 16, r["hot_path"])
    assert r["valu_hot"] < PARENT["1,1,1,1"][1]
