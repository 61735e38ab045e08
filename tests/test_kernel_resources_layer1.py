"""Resource usage of layer1's fused conv2 + conv3 kernel, read from the code object inside libmmtpsm.so (no GPU; modelled on
tests/test_kernel_resources.py): conv3x3_c64_kernel<1> / <2> hold conv3's A fragments, a panel's accumulators and two panels' residual
values in registers at two blocks per CU -- nothing of it may live in scratch memory, and the un-fused form keeps its budget."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd", "tools"))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    import codeobj
    if not os.path.exists(codeobj.LIB) or not os.path.exists(os.path.join(codeobj.LLVM, "clang-offload-bundler")):
        pytest.skip("library or LLVM tools not present")
    t = codeobj.kernel_table(workdir=str(tmp_path_factory.mktemp("co")))
    return t, codeobj.demangle(sorted(t))


def test_fused_layer1_kernel_has_no_scratch_and_no_spilled_vgprs(table):
    t, d = table
    forms = {d[n]: t[n] for n in t if "conv3x3_c64_kernel<" in d[n]}
    assert sorted(n[n.index("<"):n.index(">") + 1] for n in forms) == ["<0>", "<1>", "<2>"], sorted(forms)
    for n, r in forms.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        # two blocks of four waves per CU (80 KB of LDS each): 256 registers per lane; the un-fused form stays far below
        assert r["vgpr"] <= (128 if "<0>" in n else 256), (n, r)
