"""mmt_conv_route (csrc/conv_route.hip) decides what the six shape queries it replaced decided: tests/golden/conv_routes.npz holds
the answers of those six (tile variant, K ranges, "wants planes", "writes y_rb", "plane-fed wanted", the plane-fed plan)
at the last commit that had them (tests/golden/gen_golden_conv_routes.py), over the grid of tests/conv_route_cases.py; here the same
seven numbers are derived from the route, case by case.  No device is needed: the route is host code.

How a legacy answer reads off the route (`A`: what the filling promises -- the shape filling carried placeholder pointers for x and
the weight planes, now MMT_ASSUME_X | MMT_ASSUME_W_PLANES; the other two fillings hold the pointers):
  variant       tag of route(LIB, A)
  ksplit        ksplit of route(LIB, A); 1 on the tap-strip kernel (the query counted the tiled kernels' ranges)
  wants_planes  mode 3 and family == STRIP of route(LIB, A | X_PLANES): the query did not ask for the planes to exist
  writes_rb     writes_rb of route(F16, A | X_PLANES | F16_SCALARS) (the query planted the scalars)
  pg_wanted     bit PG of `wanted` there (the query planted the planes of x)
  pg_plan       (pg_rows, pg_ksplit) there

The legacy answers contradicted each other for the SHAPE filling, and the table pins them as they were: (2, 256, 128, 128) -> 256, 3x3
wants planes, yet its variant is 1, not 4 (nobody promised the planes to that query); layer1's (2, 64, 200, 304) -> 64, 3x3 "writes
y_rb" although the patch kernel it runs on cannot (the shape filling has no fp32 weight, without which it is not that kernel's call).
Production never relied on either: _hip.planes_wanted_3x3 and conv_pg_plan ask with the shape filling and the promises spelled out,
_hip._conv_kind with the `kind` filling plus promised planes and scalars, the profiling brackets and _rb_produce with the launch's."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_route_cases as C  # noqa: E402

WGRAD_SWITCHES = ("MMT_WGRAD_PLANES", "MMT_WGRAD_GROUP")   # bits 6, 7 of mmt_conv_switches(): tests/test_wgrad_route.py


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    L = ctypes.CDLL(H.LIB_PATH)   # (the bare library: no device, no launch)
    L.mmt_conv_route.argtypes = [ctypes.POINTER(H.ConvArgs), ctypes.c_int, ctypes.c_int, ctypes.POINTER(H.ConvRoute)]
    prev = L.mmt_get_conv_precision()
    old = {k: os.environ.pop(k, None) for k in C.SWITCHES + WGRAD_SWITCHES}
    yield H, L
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    L.mmt_set_conv_precision(prev)


def test_routes_answer_what_the_six_queries_answered(hip):
    H, L = hip
    table = np.load(os.path.join(ROOT, "tests", "golden", "conv_routes.npz"))
    assert (table["cases"] == np.asarray(C.cases(), dtype=np.int32)).all(), "the grid moved: the table no longer lines up"
    want = table["answers"]
    STRIP, PG = H.ROUTE_STRIP, H.ROUTE_PG
    rL, rP, rF = H.ConvRoute(), H.ConvRoute(), H.ConvRoute()
    got = np.zeros_like(want)
    last, n = (None, None), 0
    for mode, io_x, leg, case, filling in C.grid():
        if (mode, leg) != last:
            assert L.mmt_set_conv_precision(mode) == 0
            for k in C.SWITCHES:
                os.environ.pop(k, None)
            if C.SWITCH_LEGS[leg] is not None:
                os.environ[C.SWITCH_LEGS[leg]] = "0"
            mask = (63 if leg == 0 else 63 & ~(1 << (leg - 1))) | 192   # (bits 6, 7: the weight gradient's two, left on here)
            assert L.mmt_conv_switches() == mask
            last = (mode, leg)
        a = ctypes.byref(C.fill(H.ConvArgs, case, io_x, filling, False))
        A = (H.ASSUME_X | H.ASSUME_W_PLANES) if filling == "shape" else 0
        rc = (L.mmt_conv_route(a, H.ENTRY_LIB, A, ctypes.byref(rL)),
              L.mmt_conv_route(a, H.ENTRY_LIB, A | H.ASSUME_X_PLANES, ctypes.byref(rP)),
              L.mmt_conv_route(a, H.ENTRY_F16, A | H.ASSUME_X_PLANES | H.ASSUME_F16_SCALARS, ctypes.byref(rF)))
        if any(rc):
            assert rc[0] == rc[1] == rc[2]
            got[n] = (rc[0], rc[0], 0, 0, 0, rc[0], rc[0])
        else:
            assert rL.switches == mask
            got[n] = (rL.tag, 1 if rL.family == STRIP else rL.ksplit, int(mode == 3 and rP.family == STRIP), rF.writes_rb,
                      rF.wanted >> PG & 1, rF.pg_rows, rF.pg_ksplit)
        n += 1
    assert n == len(want)
    bad = np.nonzero((got != want).any(axis=1))[0]
    rows = list(C.grid())
    assert len(bad) == 0, "%d of %d rows differ; first: %r legacy %r route %r" % (
        len(bad), n, rows[bad[0]], want[bad[0]].tolist(), got[bad[0]].tolist())


def test_route_names_the_launch_it_describes(hip):
    """the fields a launcher switches on, on the shapes the GPU tests launch: family, tile, K ranges, the form of x"""
    H, L = hip
    L.mmt_set_conv_precision(3)
    r = H.ConvRoute()

    def route(case, entry, assume, filling="kind"):
        assert L.mmt_conv_route(ctypes.byref(C.fill(H.ConvArgs, case, 0, filling, False)), entry, assume, ctypes.byref(r)) == 0
        return r
    planes = H.ASSUME_X_PLANES | H.ASSUME_F16_SCALARS
    r = route((2, 256, 128, 128, 256, 3, 1, 1, 1, 0, 0), H.ENTRY_F16, planes)
    assert (r.family, r.tag, r.bm, r.bn, r.strip_tw, r.ksplit, r.x_form) == (H.ROUTE_STRIP, 4, 256, 128, 128, 1, 2)
    r = route((2, 512, 32, 32, 512, 3, 1, 1, 1, 0, 0), H.ENTRY_F16, planes)
    assert (r.family, r.tag, r.bm, r.bn, r.kgroups, r.ksplit, r.x_form) == (H.ROUTE_PG, 5, 64, 128, 4, 2, 2)
    r = route((2, 64, 32, 32, 64, 1, 1, 0, 1, 0, 0), H.ENTRY_F16, planes)          # M = 128 * 16: the row-resident kernel's smallest
    assert (r.family, r.tag, r.bm, r.bn, r.ksplit, r.x_form, r.writes_rb) == (5, 2, 128, 32, 1, 0, 1) and r.panels >= 1
    r = route((2, 64, 32, 31, 64, 1, 1, 0, 1, 0, 0), H.ENTRY_F16, planes)
    assert (r.family, r.tag, r.bm, r.bn) == (3, 2, 64, 64)
    r = route((2, 64, 200, 304, 64, 3, 1, 1, 1, 0, 0), H.ENTRY_F16, planes)        # layer1's patch kernel: no plane store
    assert (r.family, r.writes_rb) == (8, 0)
    r = route((2, 256, 128, 128, 256, 3, 1, 1, 1, 0, 0), H.ENTRY_LIB, 0, "launch")  # 3-term bf16 split, planes of x in the block
    assert (r.family, r.tag, r.x_form) == (H.ROUTE_STRIP, 4, 1)
    L.mmt_set_conv_precision(0)
    r = route((2, 256, 128, 128, 3, 1, 1, 0, 1, 0, 0), H.ENTRY_LIB, 0)
    assert (r.family, r.tag, r.bm, r.bn) == (1, 0, 128, 32)
    r = route((2, 256, 128, 128, 256, 3, 1, 1, 1, 0, 0), H.ENTRY_F16, planes)
    assert r.family == H.ROUTE_NONE and r.writes_rb == 0
