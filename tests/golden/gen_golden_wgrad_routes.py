"""Records tests/golden/wgrad_routes.npz: what the weight gradient's shape queries answered before its routing had one owner --
mmt_conv_wgrad_<q>(a) for q in QUERIES over the grid of tests/wgrad_route_cases.py, and the floats of mmt_conv_wgrad_group_workspace
over its batches.  Needs a build that still exports the two queries: commit 1ee94b0 ("Pin the operand-prep kernels bit for bit; NaN
and inf survive a conv"), the parent of the change that replaced them with mmt_conv_wgrad_route.  No device is needed.

    (check out 1ee94b0 next to this file and tests/wgrad_route_cases.py, build the library)  python tests/golden/gen_golden_wgrad_routes.py

answers: one row per grid point, two int32 columns (a query that returns an error code leaves the code in its column); group_ws:
one int64 per point of the batch grid (-1: the query refused the batch)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wgrad_route_cases as C  # noqa: E402

QUERIES = ("splits", "planes_splits")   # int mmt_conv_wgrad_<q>(const mmt_conv_args*)


def set_leg(L, mode, leg):
    assert L.mmt_set_conv_precision(mode) == 0
    for k in C.SWITCHES:
        os.environ.pop(k, None)
    if C.SWITCH_LEGS[leg] is not None:
        os.environ[C.SWITCH_LEGS[leg]] = "0"


def main():
    from maskrcnn_benchmark import _hip
    L = ctypes.CDLL(_hip.LIB_PATH)
    ask = [getattr(L, "mmt_conv_wgrad_" + q) for q in QUERIES]
    rows, last = [], None
    for mode, io, leg, case in C.grid():
        if (mode, leg) != last:
            set_leg(L, mode, leg)
            last = (mode, leg)
        a = ctypes.byref(C.fill(_hip.ConvArgs(), case, io))
        rows.append(tuple(f(a) for f in ask))
    ws = []
    specs = C.batches()
    need = ctypes.c_long(0)
    for mode, leg, name in C.batch_grid():
        set_leg(L, mode, leg)
        arr = C.fill_jobs(_hip.WgradJob, specs[name])
        rc = L.mmt_conv_wgrad_group_workspace(arr, len(specs[name]), ctypes.byref(need))
        ws.append(-1 if rc else need.value)
    for k in C.SWITCHES:
        os.environ.pop(k, None)
    path = os.path.join(HERE, "wgrad_routes.npz")
    np.savez_compressed(path, answers=np.asarray(rows, dtype=np.int32), cases=np.asarray(C.cases(), dtype=np.int32),
                        group_ws=np.asarray(ws, dtype=np.int64))
    print("wrote", path, len(rows), "rows,", len(ws), "batch rows,", os.path.getsize(path), "bytes;", len(C.cases()), "cases")


if __name__ == "__main__":
    main()
