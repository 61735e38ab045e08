"""mmt_conv_wgrad_route (csrc/conv_route.hip: wgrad_route) decides what the weight gradient's two shape queries and the plan of its
grouped launches decided: tests/golden/wgrad_routes.npz holds the answers of the two queries mmt_conv_wgrad_<q>, q = splits and
planes_splits, and of mmt_conv_wgrad_group_workspace at the last commit that had the two (tests/golden/gen_golden_wgrad_routes.py), over the grid and
the batches of tests/wgrad_route_cases.py; here the same numbers are derived from the route, row by row.  No device is needed.

How a legacy answer reads off the route:
  splits         `splits` of route(have = 0) -- the query knew nothing of maxima or planes, and the ranges do not depend on them
  planes_splits  `splits` of route(have = MMT_WG_HAVE_PLANES) when its family is plane-fed, else 0 (also for a block the library
                 refuses: the legacy query looked at no pointer, and every such block of the grid is past its 2^29-element limit)
  group floats   mmt_conv_wgrad_group_workspace, which now plans from the jobs' routes"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wgrad_route_cases as C  # noqa: E402


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    L = ctypes.CDLL(H.LIB_PATH)   # (the bare library: no device, no launch)
    L.mmt_conv_wgrad_route.argtypes = [ctypes.POINTER(H.ConvArgs), ctypes.c_int, ctypes.POINTER(H.WgradRoute)]
    L.mmt_conv_wgrad_group_workspace.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_long)]
    prev = L.mmt_get_conv_precision()
    old = {k: os.environ.pop(k, None) for k in C.SWITCHES}
    yield H, L
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    L.mmt_set_conv_precision(prev)


def _set_leg(L, mode, leg):
    assert L.mmt_set_conv_precision(mode) == 0
    for k in C.SWITCHES:
        os.environ.pop(k, None)
    if C.SWITCH_LEGS[leg] is not None:
        os.environ[C.SWITCH_LEGS[leg]] = "0"
    mask = 192 if leg == 0 else 192 & ~(64 << (leg - 1))
    assert L.mmt_conv_switches() & 192 == mask
    return mask


def test_routes_answer_what_the_queries_answered(hip):
    H, L = hip
    table = np.load(os.path.join(ROOT, "tests", "golden", "wgrad_routes.npz"))
    assert (table["cases"] == np.asarray(C.cases(), dtype=np.int32)).all(), "the grid moved: the table no longer lines up"
    want = table["answers"]
    r0, rP, rM = H.WgradRoute(), H.WgradRoute(), H.WgradRoute()
    F16, NONE = 5, H.WGRAD_NONE
    got = np.zeros_like(want)
    last, n = None, 0
    for mode, io, leg, case in C.grid():
        if (mode, leg) != last:
            mask = _set_leg(L, mode, leg)
            last = (mode, leg)
        a = C.fill(H.ConvArgs(), case, io)
        rc = (L.mmt_conv_wgrad_route(ctypes.byref(a), 0, ctypes.byref(r0)),
              L.mmt_conv_wgrad_route(ctypes.byref(a), H.WG_HAVE_PLANES, ctypes.byref(rP)))
        if any(rc):
            assert rc[0] == rc[1]
            got[n] = (rc[0], 0)
        else:
            planes = rP.family in (H.WGRAD_PLANES_1, H.WGRAD_PLANES_3)
            got[n] = (r0.splits, rP.splits if planes else 0)
            K = case[5] * case[5] * case[1]
            for r in (r0, rP):
                assert r.switches & 192 == mask
                assert r.ws_floats == (r.splits * case[4] * K if r.splits > 1 else 0), (mode, io, leg, case)
                assert r.family not in (H.WGRAD_PLANES_1, H.WGRAD_PLANES_3) or (r is rP and mode == 3 and leg != 1)
            # with both maxima: the fp16 split where mode 3, fp32 storage, Cin % 4 == 0, Cout % 4 == 0 and both operands below 2^31
            # bytes meet (the conditions of the launch at the commit before the route), else no kernel (MMT_EINVAL); the same ranges
            N, Cin, Hh, W, Cout = case[:5]
            takes = (mode == 3 and io == 0 and Cin % 4 == 0 and Cout % 4 == 0 and N * Hh * W * Cin * 4 < 2 ** 31
                     and N * a.Ho * a.Wo * Cout * 4 < 2 ** 31)
            assert L.mmt_conv_wgrad_route(ctypes.byref(a), H.WG_HAVE_MAXIMA, ctypes.byref(rM)) == 0
            assert rM.family == (F16 if takes else NONE), (mode, io, leg, case)
            assert (rM.splits, rM.mps, rM.ws_floats) == (r0.splits, r0.mps, r0.ws_floats)
            if not planes:   # planes nobody takes change nothing
                assert all(getattr(r0, f) == getattr(rP, f) for f, _ in H.WgradRoute._fields_), (mode, io, leg, case)
        n += 1
    assert n == len(want)
    bad = np.nonzero((got != want).any(axis=1))[0]
    rows = list(C.grid())
    assert len(bad) == 0, "%d of %d rows differ; first: %r legacy %r route %r" % (
        len(bad), n, rows[bad[0]], want[bad[0]].tolist(), got[bad[0]].tolist())


def test_group_workspace_is_what_it_was(hip):
    H, L = hip
    want = np.load(os.path.join(ROOT, "tests", "golden", "wgrad_routes.npz"))["group_ws"]
    specs = C.batches()
    need, r = ctypes.c_long(0), H.WgradRoute()
    got = []
    for mode, leg, name in C.batch_grid():
        _set_leg(L, mode, leg)
        arr = C.fill_jobs(H.WgradJob, specs[name])
        rc = L.mmt_conv_wgrad_group_workspace(ctypes.addressof(arr), len(specs[name]), ctypes.byref(need))
        got.append(-1 if rc else need.value)
        if mode == 3 and leg == 0 and name in ("planes_13", "pipe_7"):   # every job rides in a group: the in-group ranges of its route
            total = 0
            for j, (case, planes, maxima, _, _) in zip(arr, specs[name]):
                have = (H.WG_HAVE_PLANES if planes else 0) | (H.WG_HAVE_MAXIMA if maxima else 0)
                assert L.mmt_conv_wgrad_route(ctypes.byref(j.a), have, ctypes.byref(r)) == 0
                assert r.group_kind == (1 if planes else 2 + r.decode) and r.group_splits <= max(1, (r.splits + 3) // 4)
                if r.group_splits > 1:
                    total += r.group_splits * case[4] * case[5] * case[5] * case[1]
            assert total == need.value, name
    assert got == want.tolist()
    assert L.mmt_conv_wgrad_group_workspace(ctypes.addressof(C.fill_jobs(H.WgradJob, specs["one"])), 97, ctypes.byref(need)) != 0   # n <= 96


# (mode, have, io_bf16, (N, Cin, H, W, Cout), k) -> (family, terms, decode, vec4, bf, splits, mps, LDS bytes, dbias summed in the kernel):
# the launch mmt_conv_wgrad / mmt_conv_wgrad_planes issued for the shape at the commit before the route, read off their code -- on the
# shapes tests/test_wgrad_bits_gpu.py launches, then the two families only operands past 2^31 bytes reach, then a refused call
M, P = 1, 2
LAUNCHES = {
    "planes_three_tap": (M | P, (7, 2, 0, 0, 0, 2, 0, 147456, 1)),
    "planes_one_tap": (M | P, (6, 2, 0, 0, 0, 2, 0, 147456, 1)),
    "f16_decode2": (M, (5, 2, 2, 1, 0, 2, 512, 65536, 1)),
    "f16_decode1": (M, (5, 2, 1, 1, 0, 3, 352, 65536, 1)),
    "f16_decode0": (M, (5, 2, 0, 1, 0, 2, 512, 65536, 1)),
    "bf16x3": (0, (4, 3, 2, 1, 0, 2, 512, 73728, 1)),
    "cout6": (0, (4, 3, 2, 0, 0, 2, 512, 73728, 1)),
    "bf16_x": (0, (4, 1, 2, 1, 1, 2, 512, 65536, 1)),
    "bf16_dy": (0, (4, 1, 2, 1, 2, 2, 512, 65536, 1)),
    "bf16_x_dy": (0, (4, 1, 2, 1, 3, 2, 512, 65536, 1)),
    "fp32_fast": (0, (1, 0, 2, 1, 0, 2, 512, 65536, 0)),
    "fp32_slow": (0, (2, 0, 0, 1, 0, 2, 512, 65536, 0)),
}
BEYOND = [
    (2, 0, 0, (1, 128, 2048, 2048, 128), 1, (3, 2, 2, 1, 0, 512, 8192, 65536, 1)),    # x = 2^31 bytes: the register-splitting kernel
    (2, 0, 0, (1, 128, 2048, 2048, 6), 1, (2, 0, 2, 0, 0, 512, 8192, 65536, 0)),      # ... and Cout % 4 != 0: fp32
    (3, M, 0, (1, 64, 32, 32, 6), 1, (0, 0, 2, 0, 0, 2, 512, 65536, 1)),              # maxima, Cout % 4 != 0: MMT_EINVAL at the launch
    (3, 0, 1, (1, 64, 32, 32, 64), 1, (0, 0, 2, 1, 1, 2, 512, 65536, 1)),             # bf16 storage outside mode 1: the same
]


def test_route_names_the_launch_it_describes(hip):
    H, L = hip
    import test_wgrad_bits_gpu as B
    r = H.WgradRoute()
    rows = [(B.CASES[n][0], have, (C.IO_X if B.CASES[n][4] else 0) | (C.IO_DY if B.CASES[n][5] else 0), B.CASES[n][2], B.CASES[n][3], lit)
            for n, (have, lit) in sorted(LAUNCHES.items())]
    assert len(rows) == len(B.CASES)
    for mode, have, io, (N, Cin, Hh, W, Cout), k, lit in rows + BEYOND:
        assert L.mmt_set_conv_precision(mode) == 0
        a = C.fill(H.ConvArgs(), (N, Cin, Hh, W, Cout, k, 1, k // 2), io)
        assert L.mmt_conv_wgrad_route(ctypes.byref(a), have, ctypes.byref(r)) == 0
        got = (r.family, r.terms, r.decode, r.vec4, r.bf, r.splits, r.mps, r.lds_bytes, r.dbias_in_kernel)
        assert got == lit, (mode, have, io, (N, Cin, Hh, W, Cout), k, got)
    # the group of two of the GPU test: both plane-fed jobs keep one range inside the group
    L.mmt_set_conv_precision(3)
    for k in (3, 1):
        a = C.fill(H.ConvArgs(), B.PL[:4] + (B.PL[4], k, 1, k // 2))
        assert L.mmt_conv_wgrad_route(ctypes.byref(a), M | P, ctypes.byref(r)) == 0
        assert (r.group_kind, r.group_splits, r.group_mps) == (1, 1, 0)
