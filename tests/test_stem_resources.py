"""Resource usage of the stem's backward kernels (csrc/stem_bwd.hip), read from the code objects inside libmmtpsm.so like
tests/test_gconv_resources.py does for the grouped kernels (no GPU): both kernels of the file are shipped, and neither spills a
vector register or uses scratch memory."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd", "tools"))

KERNELS = ("maxpool_bwd_kernel", "stem_wgrad_kernel")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    import codeobj
    if not os.path.exists(codeobj.LIB) or not os.path.exists(os.path.join(codeobj.LLVM, "clang-offload-bundler")):
        pytest.skip("library or LLVM tools not present")
    t = codeobj.kernel_table(workdir=str(tmp_path_factory.mktemp("co")))
    d = codeobj.demangle(sorted(t))
    return {d[n]: t[n] for n in t if any(k in d[n] for k in KERNELS)}


def test_both_kernels_are_shipped(table):
    for k in KERNELS:
        assert sum(k in n for n in table) == 1, (k, sorted(table))
    assert len(table) == 2, sorted(table)


def test_no_spills_no_scratch(table):
    assert table
    for n, r in table.items():
        print(n, r)
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["vgpr"] <= 512, (n, r)
    wg = next(r for n, r in table.items() if "stem_wgrad_kernel" in n)
    assert wg["vgpr"] <= 256, wg   # the launch puts two blocks of four waves on a CU: two waves per SIMD share its 512 registers
