"""Resource usage of the grouped 3x3 convolution kernels (csrc/conv_group.hip), read from the code objects inside libmmtpsm.so like
tests/test_kernel_resources.py does for the dense kernels (no GPU): every kernel of the file is in the table -- gconv_fwd_kernel (forward, and the stride-1 data gradient on transformed weights) in six forms,
three slab widths x two strides; gconv_wgrad_kernel likewise; gconv_dgrad_s2_kernel, the stride-2 data gradient, per slab width; the
weight transform of the data gradient -- and none of them spills a vector register or uses scratch memory."""
import os
import re
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
    d = codeobj.demangle(sorted(t))
    return {d[n]: t[n] for n in t if "gconv_" in d[n]}


def _forms(table, kernel):
    return sorted(re.search(kernel + r"<([^>]*)>", n).group(1).replace(" ", "") for n in table if kernel + "<" in n)


def test_every_kernel_of_the_file_is_shipped(table):
    assert any("gconv_flip_kernel" in n for n in table), sorted(table)
    # <channels of the slab, input channels per 16-channel output slice, stride, output rows per tile>
    assert _forms(table, "gconv_fwd_kernel") == ["32,16,1,8", "32,16,2,4", "32,32,1,8", "32,32,2,4", "64,64,1,8", "64,64,2,2"]
    assert _forms(table, "gconv_wgrad_kernel") == ["32,16,1,8", "32,16,2,4", "32,32,1,8", "32,32,2,4", "64,64,1,4", "64,64,2,2"]
    assert _forms(table, "gconv_dgrad_s2_kernel") == ["32,16", "32,32", "64,64"]
    assert len(table) == 16, sorted(table)


def test_no_spills_no_scratch(table):
    assert table
    for n, r in table.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["vgpr"] <= 512, (n, r)   # (unified register file: 256-thread blocks may take all of it)
