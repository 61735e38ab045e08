"""One NaN, +inf or -inf in an operand of a convolution must reach every output that depends on it, on every route and in both
arithmetics of mode 3 (the two-term fp16 split and the 3-term bf16 split), through the launch-plan path and the general path -- and
everything else must stay right.  A NaN that a clamp, an fmaxf or a range guard turns into a finite number leaves the losses finite and
the optimiser's non-finite guard blind.

The reference is the same operation in fp64 (im2col + matrix product) WITH the bad value in place: an output is `affected` where the
reference is not finite.  Affected outputs must be non-finite (which non-finite value is not asked); all others must lie within the
convolution family's bound, 1e-5 max |ref| (tests/test_f16x2_gpu.py), of the reference.

Shapes: the smallest ones tests/test_conv_paths_gpu.py derives for each route."""
import pytest
import torch
import torch.nn.functional as F

from test_conv_paths_gpu import WGRAD_LAYERS, _cl, _pg_shape, _rand, _shape_args, _strip_shape

pytestmark = pytest.mark.gpu

BAD = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}
ARITH = ("f16x2", "bf16x3")
ROUTE_DMA, ROUTE_ROWS, ROUTE_STRIP, ROUTE_PG, ROUTE_C64 = 3, 5, 6, 7, 8      # include/mmtpsm.h: MMT_ROUTE_*


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    prev = H.get_conv_precision()
    H.set_conv_precision(3)
    H.rb_reset()
    yield H
    H.FAST_PLANS = True
    H.set_f16x2(None)
    H.set_conv_precision(prev)
    H.rb_reset()


def conv_ref(x, w, pad, scale=None, shift=None, res=None, relu=False):
    """fp64 convolution (stride 1) by im2col on the device: x (N, Cin, H, W), w (Cout, Cin, k, k)"""
    N, _, Hh, W = x.shape
    k = w.shape[2]
    cols = F.unfold(x.double(), k, padding=pad)                             # (N, Cin k k, L)
    y = (w.double().reshape(w.shape[0], -1) @ cols).reshape(N, w.shape[0], Hh + 2 * pad - k + 1, W + 2 * pad - k + 1)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


def dgrad_ref(g, w, pad):
    """fp64 data gradient of a stride-1 convolution: the convolution of g with the flipped, transposed weight"""
    k = w.shape[2]
    return conv_ref(g, w.flip(2, 3).transpose(0, 1), k - 1 - pad)


def wgrad_ref(x, dy, k, pad):
    cols = F.unfold(x.double(), k, padding=pad)                             # (N, Cin k k, L)
    dw = torch.einsum("nol,nkl->ok", dy.double().reshape(dy.shape[0], dy.shape[1], -1), cols)
    return dw.reshape(dy.shape[1], x.shape[1], k, k)


def check(y, ref, what):
    """affected = the reference is not finite there: y must not be finite either; everywhere else |y - ref| <= 1e-5 max |ref|"""
    y, ref = y.double(), ref.to(y.device)
    affected = ~torch.isfinite(ref)
    assert affected.any() and not affected.all(), what
    lost = affected & torch.isfinite(y)
    assert not lost.any(), "%s: %d of %d affected outputs are finite, e.g. %r" % (what, int(lost.sum()), int(affected.sum()),
                                                                                 y[lost][:4].tolist())
    bound = 1e-5 * float(ref[~affected].abs().max())
    err = (y - ref)[~affected].abs()
    assert bool((err <= bound).all()), "%s: unaffected outputs off by %.3g (bound %.3g)" % (what, float(err[err == err].max()) if (err == err).any() else float("nan"), bound)


def set_arith(H, arith):
    H.set_f16x2(arith == "f16x2")


def poison(t, idx, bad):
    """a fresh dense tensor with the values of t and `bad` at idx (an (n, c, h, w) index)"""
    t = t.clone()
    t[idx] = bad
    return t


# ------------------------------------------------------------------------------------------ forward routes
def fwd_case(H, name):
    """-> (x, w, kwargs of conv_forward, pad, reference kwargs, route family, F16_STATS kind)"""
    if name in ("tiled_1x1", "rows_1x1"):
        hw = 16 if name == "tiled_1x1" else 32      # M = 2048: the smallest shape that reaches the row-resident kernel
        x, w = _rand((2, 64, hw, hw), 1), _rand((64, 64, 1, 1), 2, 0.1)
        s, b = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda") * 0.1
        return x, w, dict(scale=s, shift=b), 0, dict(scale=s, shift=b), ROUTE_DMA if hw == 16 else ROUTE_ROWS, "tiled"
    if name == "tiled_3x3":     # (a residual keeps the shape off layer1's patch kernel)
        x, w, r = _rand((2, 64, 16, 16), 3), _rand((64, 64, 3, 3), 4, 0.05), _rand((2, 64, 16, 16), 5)
        return x, w, dict(res=r, res_mode=1), 1, dict(res=r), ROUTE_DMA, "tiled"
    if name == "c64_3x3":
        x, w = _rand((2, 64, 16, 16), 3), _rand((64, 64, 3, 3), 4, 0.05)
        s, b = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda") * 0.1
        return x, w, dict(scale=s, shift=b), 1, dict(scale=s, shift=b), ROUTE_C64, "tiled"
    if name == "pg":
        N, Cin, Hh, W, Cout = _pg_shape(H)
        x, w = _rand((N, Cin, Hh, W), 7), _rand((Cout, Cin, 3, 3), 8, 0.03)
        b = torch.randn(Cout, device="cuda") * 0.1
        return x, w, dict(shift=b), 1, dict(shift=b), ROUTE_PG, "pg"
    if name == "strip":
        N, Cin, Hh, W, Cout = _strip_shape(H)
        x, w = _rand((N, Cin, Hh, W), 5), _rand((Cout, Cin, 3, 3), 6, 0.03)
        return x, w, {}, 1, {}, ROUTE_STRIP, "conv"
    raise KeyError(name)


def family(H, x, w, pad, res_mode=0):
    a = _shape_args(H, x.shape[0], x.shape[1], x.shape[2], x.shape[3], w.shape[0], w.shape[2], pad)
    a.res_mode = res_mode
    return H.conv_route(a, H.ENTRY_F16, H.ASSUME_X | H.ASSUME_W | H.ASSUME_W_PLANES | H.ASSUME_X_PLANES | H.ASSUME_F16_SCALARS).family


def run_paths(H, call, kind, f16):
    """three calls through the launch-plan path (the second and third replay the plan) and one with FAST_PLANS off -> outputs 2, 3, 4"""
    outs = []
    for i in range(4):
        H.FAST_PLANS = i < 3
        s0 = dict(H.F16_STATS)
        y = call()
        torch.cuda.synchronize()
        if f16 and kind is not None:
            assert H.F16_STATS.get(kind, 0) - s0.get(kind, 0) == 1, (kind, i)
        if i:
            outs.append(y)
    H.FAST_PLANS = True
    return outs


FWD = ("tiled_1x1", "tiled_3x3", "rows_1x1", "c64_3x3", "pg", "strip")


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("name", FWD)
def test_forward_bad_value_in_x(hip, name, arith, bad):
    H = hip
    set_arith(H, arith)
    x, w, kw, pad, rkw, fam, kind = fwd_case(H, name)
    if arith == "f16x2":
        assert family(H, x, w, pad, kw.get("res_mode", 0)) == fam
    xb = poison(x, (1, 5, 7, 9), BAD[bad])
    ref = conv_ref(xb, w, pad, **rkw)
    for i, y in enumerate(run_paths(H, lambda: H.conv_forward(_cl(xb.clone()), w, stride=1, pad=pad, **kw), kind, arith == "f16x2")):
        check(y, ref, "%s %s %s call %d" % (name, arith, bad, i + 2))


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("name", FWD)
def test_forward_bad_value_in_w(hip, name, arith, bad):
    """a loose weight (packed per call): its output channel is non-finite everywhere"""
    H = hip
    set_arith(H, arith)
    x, w, kw, pad, rkw, fam, kind = fwd_case(H, name)
    k = w.shape[2]
    wb = _cl(poison(w, (3, 5, k // 2, k // 2), BAD[bad]))
    ref = conv_ref(x, wb, pad, **rkw)
    assert not torch.isfinite(ref[:, 3]).any() and torch.isfinite(ref[:, :3]).all() and torch.isfinite(ref[:, 4:]).all()
    for i, y in enumerate(run_paths(H, lambda: H.conv_forward(_cl(x.clone()), wb, stride=1, pad=pad, **kw), kind, arith == "f16x2")):
        check(y, ref, "%s %s %s call %d" % (name, arith, bad, i + 2))


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("arith", ARITH)
def test_bad_value_in_a_flat_models_weight(hip, arith, bad):
    """the weight planes of a flattened model, re-packed in bulk by refresh_planes() after the parameter buffer was rewritten through
    raw pointers (what SGD and the EMA do): forward and data-gradient forms"""
    from torch import nn
    from maskrcnn_benchmark.layers import Conv2d
    from maskrcnn_benchmark.engine.flat import flatten_model
    H = hip
    set_arith(H, arith)
    torch.manual_seed(3)
    m = nn.Sequential(Conv2d(64, 128, 3, 1, 1), Conv2d(128, 64, 1, 1, 0)).cuda()
    flat = flatten_model(m)
    x = _rand((2, 64, 16, 16), 31)
    xg = x.clone().requires_grad_(True)
    m[1](m[0](xg)).sum().backward()       # registers the data-gradient forms
    flat.refresh_planes()
    m[1].weight.data[3, 5, 0, 0] = BAD[bad]           # (through .data: the version counter does not move, the planes are trusted)
    flat.refresh_planes()
    with torch.no_grad():
        h = m[0](x)
        y = m[1](h)
    ref = conv_ref(conv_ref(x, m[0].weight, 1, shift=m[0].bias), m[1].weight, 0, shift=m[1].bias)
    check(y, ref, "flat forward %s %s" % (arith, bad))
    # the data gradient through the poisoned layer: input channel 5 of layer 1 receives g[:, 3] * bad
    hg = h.detach().clone().requires_grad_(True)
    g = _rand((2, 64, 16, 16), 32, 1e-2)
    m[1](hg).backward(g)
    check(hg.grad, dgrad_ref(g, m[1].weight.detach(), 0), "flat data gradient %s %s" % (arith, bad))


# ------------------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("kind", ["tiled", "pg"])
def test_data_gradient_bad_value_in_g(hip, kind, arith, bad):
    from maskrcnn_benchmark.layers import fused
    H = hip
    set_arith(H, arith)
    if kind == "tiled":
        N, C, Hh, W, k = 2, 64, 16, 16, 1
    else:
        N, C, Hh, W, _ = _pg_shape(H)
        k = 3
    g, w = _rand((N, C, Hh, W), 9, 1e-2), _rand((C, C, k, k), 10, 0.05)
    gb = poison(g, (1, 5, 7, 9), BAD[bad])
    ref = dgrad_ref(gb, w, k // 2)
    for i, y in enumerate(run_paths(H, lambda: fused._dgrad(_cl(gb.clone()), w, (N, C, Hh, W), 1, k // 2, None), kind, arith == "f16x2")):
        check(y, ref, "dgrad %s %s %s call %d" % (kind, arith, bad, i + 2))


# ------------------------------------------------------------------------------------------ a chain of launches
@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("arith", ARITH)
def test_chain_of_convolutions(hip, arith, bad):
    """3x3 -> ReLU'd 3x3 -> 1x1, the bad value in the first input: the second and third launches consume tensors whose statistics their
    producers recorded and (fp16 split, plane-fed shapes, from the second step on) whose row-blocked planes the producer's epilogue wrote
    with the site's scale of the step before.  ReLU keeps NaN (max(NaN, 0) is NaN in the reference)."""
    H = hip
    set_arith(H, arith)
    N, C, Hh, W, Cout = _pg_shape(H)
    x = _rand((N, C, Hh, W), 41)
    w1, w2, w3 = _rand((Cout, C, 3, 3), 42, 0.03), _rand((Cout, Cout, 3, 3), 43, 0.03), _rand((64, Cout, 1, 1), 44, 0.1)

    def chain(xin):
        y1 = H.conv_forward(xin, w1, stride=1, pad=1, rb_site=("y", w1.data_ptr()))
        y2 = H.conv_forward(y1, w2, stride=1, pad=1, relu=True, rb_site=("y", w2.data_ptr()))
        return y1, y2, H.conv_forward(y2, w3, stride=1, pad=0)

    chain(_cl(x.clone()))          # a first step: the producing sites record their maxima
    H.rb_scales_update()
    xb = poison(x, (1, 5, 7, 9), BAD[bad])
    ref = conv_ref(conv_ref(conv_ref(xb, w1, 1), w2, 1, relu=True), w3, 0)
    for step in range(2):
        y1, y2, y3 = chain(_cl(xb.clone()))
        torch.cuda.synchronize()
        if arith == "f16x2":
            assert H._rb_of(y1) is not None and H._rb_of(y1)[3] == "epi"     # the second launch was fed the producer's planes
        check(y3, ref, "chain %s %s step %d" % (arith, bad, step))
        H.rb_scales_update()


# ------------------------------------------------------------------------------------------ weight gradient
def _wgrad(H, name, route, x, dy):
    N, Cin, Hh, W, Cout, k, planes = WGRAD_LAYERS[name]
    x, dy = _cl(x.clone()), _cl(dy.clone())
    for t in (x, dy):
        t._mmt_amax = H._amax_of(t)
        if planes and H.F16X2:
            H.f16_split_pg(t)
    dw = _cl(torch.zeros(Cout, Cin, k, k, device="cuda"))
    s0 = dict(H.F16_STATS)
    if route == "single":
        H.conv_wgrad(x, dy, (Cout, Cin, k, k), 1, k // 2, dw)
    else:
        H.conv_wgrad_group([(x, dy, (Cout, Cin, k, k), 1, k // 2, dw, None, None)])
    torch.cuda.synchronize()
    return dw, {k_: H.F16_STATS.get(k_, 0) - s0.get(k_, 0) for k_ in ("wgrad", "wgrad_pl", "wgrad_grouped")}


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("where", ["x", "dy"])
@pytest.mark.parametrize("name,route", [("1x1", "single"), ("3x3_planes_w32", "single"), ("3x3_planes", "group")])
def test_weight_gradient_bad_value(hip, name, route, where, arith, bad):
    H = hip
    set_arith(H, arith)
    N, Cin, Hh, W, Cout, k, planes = WGRAD_LAYERS[name]
    x, dy = _rand((N, Cin, Hh, W), 21), _rand((N, Cout, Hh, W), 22, 1e-3)
    if where == "x":
        x = poison(x, (1, 5, 7, 9), BAD[bad])
    else:
        dy = poison(dy, (1, 3, 7, 9), BAD[bad])
    dw, st = _wgrad(H, name, route, x, dy)
    if arith == "f16x2":
        want = {"wgrad": 0, "wgrad_pl": 0, "wgrad_grouped": 0}
        want["wgrad_grouped" if route == "group" else ("wgrad_pl" if name == "3x3_planes_w32" else "wgrad")] = 1
        assert st == want
    check(dw, wgrad_ref(x, dy, k, k // 2), "wgrad %s %s %s %s %s" % (name, route, where, arith, bad))
