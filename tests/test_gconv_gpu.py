"""The grouped 3x3 convolution kernels (include/mmtpsm.h: mmt_gconv3x3_forward / _dgrad / _wgrad; csrc/conv_group.hip) against the
fp64 tensor formulation on the CPU (tests/grouped_formulations.py): the four ResNeXt 32x8d stage widths at stride 1 and 2, odd
maps, a many-tile map and the teacher's batch.

Bar: every tensor within 1e-5 * max |reference| -- the project's fp32-grade bar for convolutions (tests/test_f16x2_gpu.py,
tests/test_legacy_boundary_gpu.py).  torch's own fp32 grouped convolution sits at 1.8e-7 .. 3.2e-7 of max |y| on these inputs, bf16
products at 2.4e-3 .. 3.1e-3: exact fp32 products with fp32 accumulation have ~30x of room, a wrong arithmetic cannot pass.  The
measured worst deviation of every case is printed."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

BAR = 1e-5

CASES = [(2, 256, 8, 40, 40, 1), (2, 512, 16, 40, 40, 2), (2, 512, 16, 20, 20, 1), (2, 1024, 32, 20, 20, 2), (2, 1024, 32, 10, 10, 1),
         (2, 2048, 64, 10, 10, 2), (2, 2048, 64, 5, 5, 1),
         (1, 256, 8, 37, 53, 1), (1, 512, 16, 37, 53, 2),
         (1, 256, 8, 136, 200, 1),
         (8, 256, 8, 24, 24, 1)]


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    return H


def _inputs(case):
    N, C, Cg, Hh, Ww, stride = case
    g = torch.Generator().manual_seed(1000 + C + 7 * Cg + 13 * Hh + stride)
    x = torch.relu(torch.randn((N, C, Hh, Ww), generator=g))
    w = torch.randn((C, Cg, 3, 3), generator=g) * (2.0 / (9 * Cg)) ** 0.5
    Ho, Wo = (Hh - 1) // stride + 1, (Ww - 1) // stride + 1
    dy = torch.randn((N, C, Ho, Wo), generator=g)
    scale = 0.5 + torch.rand((C,), generator=g)
    shift = torch.randn((C,), generator=g) * 0.1
    return x, w, dy, scale, shift


def _dev(t):
    return t.cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.cuda()


def _rel(got, ref):
    return ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _report(case, what, dev):
    print("gconv %-22s %-28s worst |got - fp64| / max |fp64| = %.3e" % (case, what, dev))
    assert dev <= BAR, (case, what, dev)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward(hip, case):
    import grouped_formulations as gf
    stride = case[5]
    x, w, dy, scale, shift = _inputs(case)
    xd, wd = _dev(x), _dev(w)
    y = hip.gconv3x3_forward(xd, wd, None, None, stride, relu=False)
    ref = gf.gconv_forward(x, w, None, None, stride, False)
    assert tuple(y.shape) == tuple(ref.shape)
    _report(case, "forward plain", _rel(y, ref))
    y = hip.gconv3x3_forward(xd, wd, scale.cuda(), shift.cuda(), stride, relu=True)
    _report(case, "forward scale/shift/relu", _rel(y, gf.gconv_forward(x, w, scale, shift, stride, True)))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_data_gradient(hip, case):
    import grouped_formulations as gf
    N, C, Cg, Hh, Ww, stride = case
    x, w, dy, scale, shift = _inputs(case)
    wd, dyd = _dev(w), _dev(dy)
    ref, _ = gf.gconv_grads(x, w, dy, stride)
    # every element has one owner and is written, zeros included (stride 2: rows / columns no tap reaches): a NaN-filled destination
    out = _dev(torch.full((N, C, Hh, Ww), float("nan")))
    dx = hip.gconv3x3_dgrad(dyd, wd, (Hh, Ww), stride, out=out)
    assert dx.data_ptr() == out.data_ptr()
    assert not torch.isnan(dx).any().item(), "an element of dx was not written"
    _report(case, "dgrad plain", _rel(dx, ref))
    ref, _ = gf.gconv_grads(x, w, dy, stride, scale=scale, mask=x)
    out = _dev(torch.full((N, C, Hh, Ww), float("nan")))
    dx = hip.gconv3x3_dgrad(dyd, wd, (Hh, Ww), stride, scale=scale.cuda(), mask=_dev(x), out=out)
    assert not torch.isnan(dx).any().item(), "an element of dx was not written"
    _report(case, "dgrad scale + mask", _rel(dx, ref))
    assert (dx.cpu()[x <= 0] == 0).all().item()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_weight_gradient(hip, case):
    import grouped_formulations as gf
    N, C, Cg, Hh, Ww, stride = case
    x, w, dy, scale, shift = _inputs(case)
    xd, dyd = _dev(x), _dev(dy)
    _, ref = gf.gconv_grads(x, w, dy, stride, rowscale=scale)
    dw = _dev(torch.zeros((C, Cg, 3, 3)))
    hip.gconv3x3_wgrad(xd, dyd, (C, Cg, 3, 3), stride, dw, scale.cuda())
    _report(case, "wgrad into zeros", _rel(dw, ref))
    g = torch.Generator().manual_seed(5)
    base = torch.randn((C, Cg, 3, 3), generator=g) * ref.abs().max().float()
    dw = _dev(base.clone())
    hip.gconv3x3_wgrad(xd, dyd, (C, Cg, 3, 3), stride, dw, scale.cuda())
    _report(case, "wgrad += (non-zero dst)", _rel(dw, ref + base.double()))
    _, ref = gf.gconv_grads(x, w, dy, stride)
    dw = _dev(torch.zeros((C, Cg, 3, 3)))
    hip.gconv3x3_wgrad(xd, dyd, (C, Cg, 3, 3), stride, dw)
    _report(case, "wgrad without rowscale", _rel(dw, ref))


def test_unsupported_widths_are_refused(hip):
    """32x4d's Cg = 4 (and anything else outside 8 / 16 / 32 / 64) is refused, by the binding and by the library"""
    x = _dev(torch.zeros((1, 128, 8, 8)))
    w = _dev(torch.zeros((128, 4, 3, 3)))
    with pytest.raises(RuntimeError):
        hip.gconv3x3_forward(x, w)
    y = torch.empty_like(x)
    assert hip.lib().mmt_gconv3x3_forward(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 1, 8, 8, 128, 4, 1, 0, hip._stream()) == -22
    assert hip.lib().mmt_gconv3x3_forward(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 1, 8, 8, 128, 8, 3, 0, hip._stream()) == -22
    assert hip.lib().mmt_gconv3x3_wgrad(x.data_ptr(), y.data_ptr(), None, w.data_ptr(), 1, 8, 8, 128, 4, 1, hip._stream()) == -22
    assert hip.lib().mmt_gconv3x3_dgrad(y.data_ptr(), w.data_ptr(), None, None, w.data_ptr(), x.data_ptr(), 1, 8, 8, 128, 4, 1,
                                        hip._stream()) == -22


def test_not_offered_with_bf16_storage(hip):
    x = _dev(torch.zeros((1, 256, 8, 8)))
    w = _dev(torch.zeros((256, 8, 3, 3)))
    prev = hip.get_conv_precision()
    hip.set_conv_precision(1)
    hip.set_bf16_storage(True)
    try:
        with pytest.raises(NotImplementedError):
            hip.gconv3x3_forward(x, w)
    finally:
        hip.set_bf16_storage(False)
        hip.set_conv_precision(prev)
