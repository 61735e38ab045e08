"""Resource usage of the mask NMS kernels (csrc/masknms.hip), read from the code objects inside libmmtpsm.so like
tests/test_bitmask_resources.py does for the mask-word geometry (no GPU): both kernels are in the table, and neither spills a
vector register or uses scratch memory."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd", "tools"))

KERNELS = ("mask_nms_pair_kernel", "mask_nms_sweep_kernel")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    import codeobj
    if not os.path.exists(codeobj.LIB) or not os.path.exists(os.path.join(codeobj.LLVM, "clang-offload-bundler")):
        pytest.skip("library or LLVM tools not present")
    t = codeobj.kernel_table(workdir=str(tmp_path_factory.mktemp("co")))
    d = codeobj.demangle(sorted(t))
    return {d[n]: t[n] for n in t if d[n].split("(")[0] in KERNELS}


def test_both_kernels_are_shipped(table):
    assert sorted(n.split("(")[0] for n in table) == sorted(KERNELS), sorted(table)


def test_no_spills_no_scratch(table):
    assert table
    for n, r in table.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["vgpr"] <= 128, (n, r)    # the sweep is one block of up to 1024 threads: 4 waves per SIMD
        assert r["lds"] <= 16 * 8, (n, r)  # the sweep's kept set, one bit per position
