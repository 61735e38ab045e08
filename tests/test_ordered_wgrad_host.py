"""The ordered stem weight-gradient entry points, host side (no GPU): declared in include/mmtpsm.h, bound by _hip.py with matching
argument counts, exported by the built library, and the finish kernel they add in the code-object table without spills or scratch."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mmt-psm_amd")
for p in (ROOT, PKG, os.path.join(PKG, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

ENTRY_POINTS = {   # name -> (return type, argument count)
    "mmt_stem_wgrad_ordered": ("int", 10),
    "mmt_stem_wgrad_ws_floats": ("long", 3),
}
LIB = os.path.join(PKG, "libmmtpsm.so")


def _declarations():
    text = open(os.path.join(ROOT, "include", "mmtpsm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|long)\s+(mmt_\w+)\s*\(([^)]*)\)\s*;", text):
        args = m.group(3).strip()
        out[m.group(2)] = (m.group(1), 0 if args in ("", "void") else len(args.split(",")))
    return out


def test_header_declares_the_entry_points():
    decl = _declarations()
    for name, want in ENTRY_POINTS.items():
        assert decl.get(name) == want, (name, decl.get(name))
    # the unordered entry points keep their signatures
    assert decl["mmt_gconv3x3_wgrad"] == ("int", 11) and decl["mmt_stem_wgrad"] == ("int", 8)


def test_binding_binds_them_with_matching_argument_counts():
    from maskrcnn_benchmark import _hip as H
    for name, (ret, n) in ENTRY_POINTS.items():
        table = H._SIGS_LONG if ret == "long" else H._SIGS   # (bound with the result type the header declares)
        assert name in table and len(table[name]) == n, name
    # the workspace size travels as a long, and the queries are not recorded into launch plans
    assert H._SIGS["mmt_stem_wgrad_ordered"][8] is ctypes.c_long
    assert "mmt_stem_wgrad_ws_floats" in H._NO_RECORD


def test_library_exports_them():
    if not os.path.exists(LIB):
        pytest.skip("libmmtpsm.so is not built")
    try:
        L = ctypes.CDLL(LIB)
    except OSError as e:
        pytest.skip("libmmtpsm.so does not load here: %s" % e)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name   # (a symbol lookup: no call)


def test_finish_kernel_uses_no_spills_and_no_scratch(tmp_path):
    import codeobj
    if not os.path.exists(codeobj.LIB) or not os.path.exists(os.path.join(codeobj.LLVM, "clang-offload-bundler")):
        pytest.skip("library or LLVM tools not present")
    table = codeobj.kernel_table(workdir=str(tmp_path))
    names = codeobj.demangle(sorted(table))
    wide = {names[n]: r for n, r in table.items() if "ordered_finish_wide_kernel" in names[n]}
    # one per stage-one layout: the stem's
    assert len(wide) == 1 and "SwFinishMap" in next(iter(wide)), sorted(wide)
    for n, r in wide.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert "gconv_" not in n and "stem_wgrad_kernel" not in n   # (the names tests/test_gconv_resources.py / test_stem_resources.py collect)
