"""Records tests/golden/conv_routes.npz: what the six shape queries of the convolution library answered before the routing had one
owner -- mmt_conv_<q> for q in QUERIES, and mmt_conv_<PLAN>(a, &tile_rows, &ksplit) -- over the grid of tests/conv_route_cases.py.
Needs a build that still exports the six: commit 4143384 ("Pin the selection and NMS kernels at
their limits, ties and chains"), the parent of the change that replaced them with mmt_conv_route.  No device is needed.

    (check out 4143384 next to this file and tests/conv_route_cases.py, build the library)  python tests/golden/gen_golden_conv_routes.py

One row per grid point, seven int16 columns: variant, ksplit, wants_planes, writes_rb, pg_wanted, pg_plan's tile rows and K ranges (a
query that returns an error code leaves the code in its columns)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_route_cases as C  # noqa: E402


QUERIES = ("variant", "ksplit", "wants_planes", "writes_rb", "pg_wanted")   # int mmt_conv_<q>(const mmt_conv_args*)
PLAN = "pg_plan"


def main():
    from maskrcnn_benchmark import _hip
    L = ctypes.CDLL(_hip.LIB_PATH)
    ask = [getattr(L, "mmt_conv_" + q) for q in QUERIES]
    plan = getattr(L, "mmt_conv_" + PLAN)
    for k in C.SWITCHES:
        os.environ.pop(k, None)
    rows = []
    last = (None, None)
    r_, k_ = ctypes.c_int(0), ctypes.c_int(0)
    for mode, io_x, leg, case, filling in C.grid():
        if (mode, leg) != last:
            assert L.mmt_set_conv_precision(mode) == 0
            for k in C.SWITCHES:
                os.environ.pop(k, None)
            if C.SWITCH_LEGS[leg] is not None:
                os.environ[C.SWITCH_LEGS[leg]] = "0"
            last = (mode, leg)
        a = ctypes.byref(C.fill(_hip.ConvArgs, case, io_x, filling, True))
        r_.value = k_.value = 0
        rc = plan(a, ctypes.byref(r_), ctypes.byref(k_))
        rows.append(tuple(f(a) for f in ask) + (rc if rc else r_.value, rc if rc else k_.value))
    for k in C.SWITCHES:
        os.environ.pop(k, None)
    t = np.asarray(rows, dtype=np.int16)
    assert (t == np.asarray(rows)).all()
    path = os.path.join(HERE, "conv_routes.npz")
    np.savez_compressed(path, answers=t, cases=np.asarray(C.cases(), dtype=np.int32))
    print("wrote", path, t.shape, os.path.getsize(path), "bytes;", len(C.cases()), "cases")


if __name__ == "__main__":
    main()
