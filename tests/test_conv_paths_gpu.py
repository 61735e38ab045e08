"""The Python side of the convolution family (maskrcnn_benchmark/_hip.py: conv_forward, its launch plans, conv_forward's data-gradient
form through layers.fused._dgrad, conv_wgrad, conv_wgrad_group): WHICH path a call takes, how many library calls it costs, and that the
general path and the plan path give the same bits.  Nothing here checks arithmetic against a reference (tests/test_f16x2_gpu.py,
test_pgemm_gpu.py, test_wgrad_group_gpu.py do); it pins the host-side behaviour a restructuring of the binding must not move.

The expected counts (EXPECT, WGRAD_EXPECT) are literals recorded from a run of this file against the binding as it stood BEFORE the
launch paths were merged into one (the commit that added the ResNeXt backbones); the file passes there unedited.  The shapes are the
smallest the library's own shape queries accept for each kind (the strip kernel declines fp32 tensors below 256 tiles).

Per forward case, three calls with the same weight object and a fresh input tensor holding the same values:
  * call 1 leaves exactly one launch plan whose template holds no pointer; calls 2 and 3 (the plan path) leave none; the bf16x3 cases none
    at all;
  * the F16_STATS delta names the kind (`tiled` / `conv` = tap-strip / `pg` = plane-fed) and the passes that go with it, the C_CALLS
    delta is the recorded one, both identical for calls 2 and 3;
  * y of calls 1, 2, 3 and of a fourth call with FAST_PLANS off are bitwise equal (shapes whose launch is not split over K);
  * with PROFILE (and PROFILE_ALL) the recorded number of 7-entry records with the recorded key tag, y bitwise equal again;
  * the statistics slot of y is current and holds max |y|."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, ROOT)


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    prev = H.get_conv_precision()
    H.set_conv_precision(3)
    H.set_f16x2(True)
    yield H
    H.PROFILE, H.PROFILE_ALL, H.FAST_PLANS, H.WGRAD_GROUP = None, False, True, True
    H.set_f16x2(None)
    H.set_conv_precision(prev)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _shape_args(H, N, Cin, Hh, W, Cout, k, pad):
    """the bare shape; what the caller promises to supply goes into the route question (_route)"""
    a = H.ConvArgs()
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW = N, Hh, W, Cin, Cout, k, k
    a.stride, a.pad, a.Ho, a.Wo, a.out_stride = 1, pad, Hh + 2 * pad - k + 1, W + 2 * pad - k + 1, 1
    return a


def _route(H, entry, a, planes=False):
    """the library's route for a shape-only block: x and the weight planes promised, planes of x and the fp16 scalars on request"""
    return H.conv_route(a, entry, H.ASSUME_X | H.ASSUME_W_PLANES | ((H.ASSUME_X_PLANES | H.ASSUME_F16_SCALARS) if planes else 0))


def _wants_planes(H, a):
    return H.get_conv_precision() == 3 and _route(H, H.ENTRY_LIB, a, True).family == H.ROUTE_STRIP


def _strip_shape(H):
    """the smallest 3x3 shape the tap-strip kernel takes (the library's own answer: for fp32 tensors it wants 256 tiles of 256 pixels x
    128 channels before it gives up the tiled kernel's in-register split, so the first two candidates are declined today)"""
    for s in ((1, 128, 4, 64, 64), (1, 128, 8, 128, 64), (2, 128, 64, 128, 512), (2, 128, 128, 128, 256)):
        if _wants_planes(H, _shape_args(H, s[0], s[1], s[2], s[3], s[4], 3, 1)):
            return s
    raise AssertionError("no strip-shaped candidate")


def _pg_shape(H):
    """the smallest 3x3 shape that runs plane-fed in ONE K range and that the strip kernel does not take"""
    for s in ((2, 128, 16, 16, 128), (2, 128, 32, 32, 128), (2, 128, 64, 64, 128), (4, 128, 64, 64, 128)):
        rows, ks = H.conv_pg_plan(s[0], s[1], s[2], s[3], s[4], 3, 3, 1, 1)
        a = _shape_args(H, s[0], s[1], s[2], s[3], s[4], 3, 1)
        if rows != 0 and ks == 1 and not _wants_planes(H, a) and _route(H, H.ENTRY_F16, a, True).wanted >> H.ROUTE_PG & 1 == 1:
            return s
    raise AssertionError("no plane-fed candidate with one K range")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return _cl((torch.randn(*shape, generator=g) * scale).cuda())


def _case(H, name):
    """-> (x0, call): call(x) runs the case on the input x (a fresh tensor per call) with one weight object"""
    from maskrcnn_benchmark.layers import fused
    if name in ("tiled_1x1", "bf16x3_1x1"):
        x0, w = _rand((2, 64, 16, 16), 1).relu(), _rand((64, 64, 1, 1), 2, 0.1)
        s, b = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda") * 0.1
        return x0, lambda x: H.conv_forward(x, w, s, b, 1, 0, relu=True)
    if name == "rows_1x1":   # M = 2048 = 128 * 16: the smallest shape that reaches the row-resident kernel on the fp16 split
        x0, w = _rand((2, 64, 32, 32), 1).relu(), _rand((64, 64, 1, 1), 2, 0.1)
        s, b = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda") * 0.1
        return x0, lambda x: H.conv_forward(x, w, s, b, 1, 0, relu=True)
    if name == "tiled_3x3_res":
        x0, w = _rand((2, 64, 16, 16), 3).relu(), _rand((64, 64, 3, 3), 4, 0.05)
        s, b = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda") * 0.1
        return x0, lambda x: H.conv_forward(x, w, s, b, 1, 1, relu=True, res=x, res_mode=1)
    if name == "tiled_3x3_rb":   # layer1's 3x3 as a producing site: the patch kernel it runs on has no plane store
        x0, w = _rand((2, 64, 16, 16), 3).relu(), _rand((64, 64, 3, 3), 4, 0.05)
        s, b = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda") * 0.1
        return x0, lambda x: H.conv_forward(x, w, s, b, 1, 1, relu=True, rb_site=("y", w.data_ptr()))
    if name == "pg_rb":
        N, Cin, Hh, W, Cout = _pg_shape(H)
        x0, w = _rand((N, Cin, Hh, W), 7).relu(), _rand((Cout, Cin, 3, 3), 8, 0.03)
        return x0, lambda x: H.conv_forward(x, w, None, None, 1, 1, relu=True, rb_site=("y", w.data_ptr()))
    if name in ("strip", "bf16x3_strip"):
        N, Cin, Hh, W, Cout = _strip_shape(H)
        x0, w = _rand((N, Cin, Hh, W), 5).relu(), _rand((Cout, Cin, 3, 3), 6, 0.03)
        if name == "strip":
            return x0, lambda x: H.conv_forward(x, w, None, None, 1, 1, relu=True)
        return x0, lambda x: H.conv_forward(x, w, None, None, 1, 1, relu=True, want_planes=True)
    if name == "pg":
        N, Cin, Hh, W, Cout = _pg_shape(H)
        x0, w = _rand((N, Cin, Hh, W), 7).relu(), _rand((Cout, Cin, 3, 3), 8, 0.03)
        b = torch.randn(Cout, device="cuda") * 0.1
        return x0, lambda x: H.conv_forward(x, w, None, b, 1, 1, relu=True)
    if name.startswith("dgrad_"):
        _, kind, epi = name.split("_")
        if kind == "tiled":
            N, C, Hh, W, k = 2, 64, 16, 16, 1
        else:
            N, C, Hh, W, _ = _pg_shape(H)
            k = 3
        g0, w = _rand((N, C, Hh, W), 9, 1e-2), _rand((C, C, k, k), 10, 0.05)
        other = _rand((N, C, Hh, W), 11)
        if epi == "mask":
            return g0, lambda g: fused._dgrad(g, w, (N, C, Hh, W), 1, k // 2, None, mask=other)
        return g0, lambda g: fused._dgrad(g, w, (N, C, Hh, W), 1, k // 2, None, res=other, res_mode=1)
    raise KeyError(name)


STAT_KEYS = ("tiled", "conv", "pg", "rb_split", "rb_epi", "amax_pass", "weight_pack", "fallback", "wgrad", "wgrad_pl", "wgrad_grouped")


def _counted(H, fn):
    """fn() -> (result, {F16_STATS key: delta, non-zero ones}, C_CALLS delta, launch plans added)"""
    s0, c0, p0 = dict(H.F16_STATS), H.C_CALLS[0], set(H._PLAN)
    y = fn()
    torch.cuda.synchronize()
    d = {k: H.F16_STATS.get(k, 0) - s0.get(k, 0) for k in STAT_KEYS}
    return y, {k: v for k, v in d.items() if v}, H.C_CALLS[0] - c0, [k for k in H._PLAN if k not in p0]


def measure(H, name):
    """everything the assertions below look at, for one forward case"""
    if name.startswith("bf16x3"):
        H.set_f16x2(False)
    x0, call = _case(H, name)
    torch.cuda.synchronize()
    out = {"stats": [], "calls": [], "plans": [], "equal": [], "null_template": None}
    ys = []
    for i in range(4):
        H.FAST_PLANS = i < 3
        y, st, nc, added = _counted(H, lambda: call(x0.clone()))
        H.FAST_PLANS = True
        if i == 0 and name.endswith("_rb"):
            H.rb_scales_update()   # (the end of a step: the site has a scale from now on, the launches below may write y's planes)
        ys.append(y)
        out["stats"].append(st)
        out["calls"].append(nc)
        out["plans"].append(len(added))
        if i == 0 and added:
            t = H.ConvArgs.from_buffer_copy(H._PLAN[added[0]][0])
            out["null_template"] = all(getattr(t, f) is None for f, typ in H.ConvArgs._fields_ if typ is ctypes.c_void_p)
    out["equal"] = [bool(torch.equal(ys[0], y)) for y in ys[1:]]
    prof = []
    for every in (False, True):
        H.PROFILE, H.PROFILE_ALL = [], every
        try:
            y = call(x0.clone())
            torch.cuda.synchronize()
            rec = H.PROFILE
        finally:
            H.PROFILE, H.PROFILE_ALL = None, False
        prof.append([len(rec), sorted(set(r[3][0] for r in rec)), sorted(set(len(r) for r in rec)), bool(torch.equal(ys[0], y))])
    out["profile"] = prof
    y = ys[2]
    am = getattr(y, "_mmt_amax", None)
    out["amax"] = None if am is None else [am[1] == y._version, am[0].pool.dev[am[0].idx][0].item() == y.abs().max().item()]
    out["planes"] = H.planes_of(y) is not None
    rb = getattr(y, "_mmt_rb", None)
    out["rb"] = None if rb is None else [len(rb), rb[2] == y._version, rb[3], rb[4], rb[0].shape[1] == y.numel()]
    return out


# recorded on the parent commit (see the module docstring).  stats / calls: F16_STATS and C_CALLS deltas of call 1, of calls 2 and 3 (the
# plan path) and of the call with FAST_PLANS off; profile: (records, key tag) under PROFILE and under PROFILE with PROFILE_ALL;
# planes: bf16 planes on y; rb: y's row-blocked planes record as [entries, current, kind, images, whole tensor] or None
def _f16(kind, c1, c2, c4, profile, passes=("amax_pass",), rb=None):
    plan = dict({kind: 1}, **{k: 1 for k in passes})
    return {"kind": kind, "stats_first": dict(plan, weight_pack=1), "stats_plan": plan, "stats_general": plan, "calls": [c1, c2, c2, c4],
            "profile": profile, "planes": False, "rb": rb}


_SPLIT = ("amax_pass", "rb_split")
EXPECT = {
    # first call: bf16 weight pack + reduction pass over the fresh x + fp16 weight pack (2) + launch; plan path: pass + launch
    "tiled_1x1": _f16("tiled", 5, 2, 3, [(0, None), (1, "fwd2")]),
    "rows_1x1": _f16("tiled", 5, 2, 3, [(0, None), (1, "fwd2")]),   # (the row-resident kernel; recorded on the parent of the commit that added the case)
    "tiled_3x3_res": _f16("tiled", 5, 2, 3, [(0, None), (1, "fwd2")]),
    "tiled_3x3_rb": _f16("tiled", 5, 2, 3, [(0, None), (1, "fwd2")]),
    # the plane-fed kinds add the row-blocked split pass of x
    "pg_rb": _f16("pg", 6, 3, 4, [(1, "fwd5"), (1, "fwd5")], _SPLIT, rb=[5, True, "epi", None, True]),
    "strip": _f16("conv", 6, 3, 4, [(1, "fwd4"), (1, "fwd4")], _SPLIT),
    "pg": _f16("pg", 6, 3, 4, [(1, "fwd5"), (1, "fwd5")], _SPLIT),
    # the data-gradient form packs the flipped bf16 planes in every call (a weight outside a flat model) and no forward planes
    "dgrad_tiled_mask": _f16("tiled", 5, 3, 3, [(0, None), (1, "fwd2")]),
    "dgrad_tiled_res": _f16("tiled", 5, 3, 3, [(0, None), (1, "fwd2")]),
    "dgrad_pg_mask": _f16("pg", 6, 4, 4, [(1, "fwd5"), (1, "fwd5")], _SPLIT),
    "dgrad_pg_res": _f16("pg", 6, 4, 4, [(1, "fwd5"), (1, "fwd5")], _SPLIT),
    # 3-term bf16 split: weight pack + split pass of x + launch / weight pack + launch, nothing counted in F16_STATS
    "bf16x3_strip": {"kind": None, "stats_first": {}, "stats_plan": {}, "stats_general": {}, "calls": [3, 3, 3, 3],
                     "profile": [(1, "fwd4"), (1, "fwd4")], "planes": True, "rb": None},
    "bf16x3_1x1": {"kind": None, "stats_first": {}, "stats_plan": {}, "stats_general": {}, "calls": [2, 2, 2, 2],
                   "profile": [(0, None), (1, "fwd2")], "planes": False, "rb": None},
}

FORWARD_CASES = ("tiled_1x1", "rows_1x1", "tiled_3x3_res", "tiled_3x3_rb", "pg_rb", "strip", "pg", "dgrad_tiled_mask", "dgrad_tiled_res", "dgrad_pg_mask", "dgrad_pg_res",
                 "bf16x3_strip", "bf16x3_1x1")


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_forward_paths(hip, name):
    H = hip
    got = measure(H, name)
    print(name, got)
    exp = EXPECT[name]
    f16 = not name.startswith("bf16x3")
    # launch plans: one from the first call, its template free of pointers; none from the plan path or on the bf16x3 split
    assert got["plans"] == ([1, 0, 0, 0] if f16 else [0, 0, 0, 0])
    assert got["null_template"] is (True if f16 else None)
    # the path taken and what it cost
    assert got["stats"][0] == exp["stats_first"]
    assert got["stats"][1] == got["stats"][2] == exp["stats_plan"]
    assert got["stats"][3] == exp["stats_general"]
    if f16:
        assert got["stats"][1].get(exp["kind"]) == 1 and got["stats"][3].get(exp["kind"]) == 1
        assert not any(k in got["stats"][1] for k in ("tiled", "conv", "pg") if k != exp["kind"])
    assert got["calls"] == exp["calls"]
    assert got["calls"][1] == got["calls"][2]
    # same bits whichever path issued the launch
    assert got["equal"] == [True, True, True]
    # profiling brackets
    for p, (n, tag) in zip(got["profile"], exp["profile"]):
        assert p[0] == n and p[3] is True
        if n:
            assert p[1] == [tag] and p[2] == [7]
    # the output's statistics
    if f16:
        assert got["amax"] == [True, True]
    else:
        assert got["amax"] is None
    assert got["planes"] is exp["planes"]
    assert got["rb"] == exp["rb"]


def test_shapes_are_not_split_over_k(hip):
    """bitwise comparison above is meaningful only for launches that are not split over K with atomics"""
    H = hip
    for s, k, pad in (((2, 64, 16, 16, 64), 1, 0), ((2, 64, 16, 16, 64), 3, 1), (_strip_shape(H), 3, 1)):
        r = _route(H, H.ENTRY_LIB, _shape_args(H, s[0], s[1], s[2], s[3], s[4], k, pad))
        assert (1 if r.family == H.ROUTE_STRIP else r.ksplit) == 1, (s, k)
    s = _pg_shape(H)
    assert H.conv_pg_plan(s[0], s[1], s[2], s[3], s[4], 3, 3, 1, 1)[1] == 1


# the two layers the restructuring was specified with, and one wide enough for the plane-fed weight-gradient kernel (W % 32 == 0)
WGRAD_LAYERS = {"1x1": (2, 64, 16, 16, 64, 1, False), "3x3_planes": (2, 128, 16, 16, 128, 3, True),
                "3x3_planes_w32": (2, 128, 32, 32, 128, 3, True)}
# recorded on the parent commit: [F16_STATS deltas, C_CALLS delta] of the layer through conv_wgrad / through conv_wgrad_group
WGRAD_EXPECT = {"1x1": {"single": [{"wgrad": 1}, 1], "group": [{"wgrad_grouped": 1}, 1]},
                "3x3_planes": {"single": [{"wgrad": 1}, 1], "group": [{"wgrad_grouped": 1}, 1]},
                "3x3_planes_w32": {"single": [{"wgrad_pl": 1}, 1], "group": [{"wgrad_grouped": 1}, 1]}}


def measure_wgrad(H, name):
    N, Cin, Hh, W, Cout, k, planes = WGRAD_LAYERS[name]
    out = {}
    dws = []
    for route in ("single", "group"):
        x, dy = _rand((N, Cin, Hh, W), 21).relu(), _rand((N, Cout, Hh, W), 22, 1e-3)
        for t in (x, dy):
            t._mmt_amax = H._amax_of(t)
            if planes:
                H.f16_split_pg(t)
        dw = _cl(torch.zeros(Cout, Cin, k, k, device="cuda"))
        if route == "single":
            _, st, nc, _ = _counted(H, lambda: H.conv_wgrad(x, dy, (Cout, Cin, k, k), 1, k // 2, dw))
        else:
            _, st, nc, _ = _counted(H, lambda: H.conv_wgrad_group([(x, dy, (Cout, Cin, k, k), 1, k // 2, dw, None, None)]))
        out[route] = [st, nc]
        dws.append(dw)
    bound = torch.nn.grad.conv2d_weight(x.double().cpu().abs(), (Cout, Cin, k, k), dy.double().cpu().abs(), stride=1, padding=k // 2)
    out["err"] = ((dws[0].double().cpu() - dws[1].double().cpu()).abs() / bound.clamp_min(1e-300)).max().item()
    out["nonzero"] = bool(dws[0].abs().max().item() > 0)
    return out


@pytest.mark.parametrize("name", sorted(WGRAD_LAYERS))
def test_wgrad_paths(hip, name):
    H = hip
    got = measure_wgrad(H, name)
    print(name, got)
    exp = WGRAD_EXPECT[name]
    assert got["single"] == exp["single"]
    assert got["group"] == exp["group"]
    assert got["nonzero"]
    assert got["err"] <= 3e-6   # the bound tests/test_wgrad_group_gpu.py holds the grouped route to against the single launches
