"""Resource usage of the Soft-NMS kernel (csrc/softnms.hip), read from the code objects inside libmmtpsm.so like
tests/test_mask_nms_resources.py does for the mask NMS (no GPU): both instances are in the table, neither spills a register or
uses scratch memory, and the LDS is what the design needs and nothing else."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd", "tools"))

KERNEL = "soft_nms_kernel"
MAX_N, THREADS = 2048, 512


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    import codeobj
    if not os.path.exists(codeobj.LIB) or not os.path.exists(os.path.join(codeobj.LLVM, "clang-offload-bundler")):
        pytest.skip("library or LLVM tools not present")
    t = codeobj.kernel_table(workdir=str(tmp_path_factory.mktemp("co")))
    d = codeobj.demangle(sorted(t))
    return {d[n]: t[n] for n in t if KERNEL in d[n]}


def test_both_methods_are_shipped(table):
    names = sorted(n.split("(anonymous namespace)::")[-1].split("(")[0] for n in table)
    assert names == [KERNEL + "<0>", KERNEL + "<1>"], sorted(table)


def test_no_spills_no_scratch_and_the_lds_of_the_design(table):
    assert table
    for n, r in table.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        # one block of 512 threads = two waves per SIMD: nowhere near a register limit with four candidates per thread
        assert r["vgpr"] + r["agpr"] <= 128, (n, r)
        # the boxes of a segment (16 B each) for the broadcast of the picked one, and two sets of one 8-byte slot per wave
        assert r["lds"] == MAX_N * 16 + 2 * (THREADS // 64) * 8, (n, r)
