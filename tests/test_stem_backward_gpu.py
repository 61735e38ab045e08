"""The stem's backward kernels (include/mmtpsm.h: mmt_maxpool3x3s2_backward, mmt_stem_wgrad; csrc/stem_bwd.hip) and the autograd
node built on them (layers/fused.py::StemFn) against the fp64 formulations of tests/stem_formulations.py.

Max-pool backward: tie-rich quantised inputs and integer gradients, so the result is EXACT (torch.equal) -- the first-maximum rule,
the (y > 0) mask and "every element is written" (a NaN-filled destination) are all visible; then real gradients within
1e-6 * max |g| (an element has at most 4 addends: 3 roundings of at most 4 max |g|, below 7.2e-7 max |g|).
Weight gradient and the whole stem: 1e-5 * max |reference|, the project's fp32-grade convolution bar (tests/test_gconv_gpu.py);
the measured worst deviations are printed."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import stem_formulations as sf  # noqa: E402

BAR = 1e-5
WGRAD_CASES = [(2, 32, 32), (2, 38, 50), (1, 37, 53), (1, 8, 8), (4, 160, 160)]   # (N, H, W)


@pytest.fixture()
def hip():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    return H


def _dev(t):
    return t.cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.cuda()


@pytest.mark.parametrize("shape", sf.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_backward(hip, shape):
    y, g = sf.pool_inputs(shape)
    ref = sf.maxpool_backward_reference(y, g)
    out = _dev(torch.full(shape, float("nan")))
    dy = hip.maxpool3x3s2_backward(_dev(y), _dev(g), out=out)
    assert dy.data_ptr() == out.data_ptr()
    assert not torch.isnan(dy).any().item(), "an element of dy was not written"
    assert torch.equal(dy.cpu().double(), ref), (dy.cpu().double() - ref).abs().max().item()
    assert (dy.cpu()[y <= 0] == 0).all().item()
    # the pool this is the gradient of: the library's own forward picks the same maxima
    assert torch.equal(hip.maxpool3x3s2(_dev(y)).cpu(), torch.nn.functional.max_pool2d(y, 3, 2, 1))
    y, g = sf.pool_inputs(shape, real_g=True)
    ref = sf.maxpool_backward_reference(y, g)
    dy = hip.maxpool3x3s2_backward(_dev(y), _dev(g))
    dev = (dy.cpu().double() - ref).abs().max().item() / g.abs().max().item()
    print("maxpool backward %-16s real g: worst |got - fp64| / max |g| = %.3e" % (shape, dev))
    assert dev <= 1e-6, (shape, dev)


def test_maxpool_backward_refusals(hip):
    y = _dev(torch.zeros((1, 6, 8, 8)))
    g = _dev(torch.zeros((1, 6, 4, 4)))
    with pytest.raises(RuntimeError):
        hip.maxpool3x3s2_backward(y, g)
    assert hip.lib().mmt_maxpool3x3s2_backward(y.data_ptr(), g.data_ptr(), y.data_ptr(), 1, 8, 8, 6, hip._stream()) == -22
    assert hip.lib().mmt_maxpool3x3s2_backward(y.data_ptr(), g.data_ptr(), y.data_ptr(), 1, 0, 8, 8, hip._stream()) == -22
    with pytest.raises(RuntimeError):
        hip.maxpool3x3s2_backward(torch.zeros((1, 8, 8, 8)), torch.zeros((1, 8, 4, 4)))
    with pytest.raises(RuntimeError):   # g is not the pooled shape
        hip.maxpool3x3s2_backward(_dev(torch.zeros((1, 8, 8, 8))), _dev(torch.zeros((1, 8, 5, 4))))


def _wgrad_inputs(case):
    N, Hh, Ww = case
    gen = torch.Generator().manual_seed(100 + N + 7 * Hh + 13 * Ww)
    x = torch.randn((N, 3, Hh, Ww), generator=gen)
    dy = torch.randn((N, 64, (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1), generator=gen)
    scale = 0.5 + torch.rand((64,), generator=gen)
    return x, dy, scale


def _report(case, what, got, ref):
    dev = ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
    print("stem wgrad %-16s %-26s worst |got - fp64| / max |fp64| = %.3e" % (case, what, dev))
    assert dev <= BAR, (case, what, dev)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_weight_gradient(hip, case):
    x, dy, scale = _wgrad_inputs(case)
    xd, dyd = x.cuda(), _dev(dy)
    ref = sf.stem_wgrad_reference(x, dy, scale)
    dw = _dev(torch.zeros((64, 3, 7, 7)))
    assert hip.stem_wgrad(xd, dyd, dw, scale.cuda()) is dw
    _report(case, "into zeros", dw, ref)
    gen = torch.Generator().manual_seed(5)
    base = torch.randn((64, 3, 7, 7), generator=gen) * ref.abs().max().float()
    dw = _dev(base.clone())
    hip.stem_wgrad(xd, dyd, dw, scale.cuda())
    _report(case, "+= (non-zero dst)", dw, ref + base.double())
    dw = _dev(torch.zeros((64, 3, 7, 7)))
    hip.stem_wgrad(xd, dyd, dw)
    _report(case, "without rowscale", dw, sf.stem_wgrad_reference(x, dy))


def test_stem_weight_gradient_refusals(hip):
    x, dy, _ = _wgrad_inputs((1, 8, 8))
    dw = _dev(torch.zeros((64, 3, 7, 7)))
    with pytest.raises(RuntimeError):
        hip.stem_wgrad(x, _dev(dy), dw)                                   # a CPU image
    with pytest.raises(RuntimeError):
        hip.stem_wgrad(x.cuda(), _dev(dy[:, :, :3]), dw)                  # dy is not the convolution's output shape
    with pytest.raises(RuntimeError):
        hip.stem_wgrad(x.cuda(), _dev(dy), torch.zeros((64, 3, 7, 7)).cuda())   # dw not in the parameter's channels-last layout
    assert hip.lib().mmt_stem_wgrad(x.cuda().data_ptr(), None, None, dw.data_ptr(), 1, 8, 8, hip._stream()) == -22


def _stem(trainable):
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.backbone import backbone as B
    gen = torch.Generator().manual_seed(3)
    m = B.StemWithFixedBatchNorm(make_default_cfg())
    with torch.no_grad():
        m.conv1.weight.copy_(torch.randn(m.conv1.weight.shape, generator=gen) * 0.05)
        m.bn1.weight.copy_(torch.rand(64, generator=gen) + 0.5)
        m.bn1.bias.copy_(torch.randn(64, generator=gen) * 0.2)
        m.bn1.running_mean.copy_(torch.randn(64, generator=gen) * 0.1)
        m.bn1.running_var.copy_(torch.rand(64, generator=gen) + 0.5)
    m.cuda()
    m.conv1.weight.requires_grad_(trainable)
    return m


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 37, 53)], ids=["fused-size", "odd-size"])
def test_one_stem_forward_and_backward(hip, shape):
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=gen) * 60.0        # mean-subtracted BGR-255 pixels
    frozen, train = _stem(False), _stem(True)
    out_f = frozen(x.cuda())
    assert not out_f.requires_grad
    n0 = hip.C_CALLS[0]
    out = train(x.cuda())
    assert out.requires_grad and torch.equal(out.detach(), out_f), (out.detach() - out_f).abs().max().item()
    with torch.no_grad():   # a no-grad pass of a trainable stem is the frozen stem's pass
        assert torch.equal(train(x.cuda()), out_f)
    r = torch.randn(out.shape, generator=gen)
    s, b = frozen.bn1.folded()
    ref_out, ref_dw = sf.stem_with_grad(x, frozen.conv1.weight.detach().cpu(), s.cpu(), b.cpu(), r)
    dev = (out.detach().cpu().double() - ref_out).abs().max().item() / ref_out.abs().max().item()
    print("stem %-16s out: worst |got - fp64| / max |fp64| = %.3e" % (shape, dev))
    assert dev <= BAR
    (out * _dev(r)).sum().backward()
    assert frozen.conv1.weight.grad is None
    g = train.conv1.weight.grad
    assert g is not None and g.shape == ref_dw.shape
    dev = (g.cpu().double() - ref_dw).abs().max().item() / ref_dw.abs().max().item()
    print("stem %-16s d conv1.weight: worst |got - fp64| / max |fp64| = %.3e" % (shape, dev))
    assert dev <= BAR, dev
    assert hip.C_CALLS[0] > n0


def test_trainable_stem_not_offered_with_bf16_storage(hip):
    m = _stem(True)
    prev = hip.get_conv_precision()
    hip.set_conv_precision(1)
    hip.set_bf16_storage(True)
    try:
        with pytest.raises(NotImplementedError, match="FREEZE_CONV_BODY_AT"):
            m(torch.zeros((1, 3, 32, 32)).cuda())
    finally:
        hip.set_bf16_storage(False)
        hip.set_conv_precision(prev)
