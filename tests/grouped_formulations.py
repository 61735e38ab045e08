"""fp64 tensor formulations of the grouped 3x3 convolution (include/mmtpsm.h: mmt_gconv3x3_*) and of the reference's ResNeXt
bottleneck (reference modeling/backbone/resnet.py:206-274 with FrozenBatchNorm2d folded into a scale and a shift per channel,
layers/batch_norm.py:19-24), on the CPU: what tests/test_gconv_gpu.py and tests/test_resnext_model_gpu.py compare against."""
import torch
import torch.nn.functional as F


def gconv_forward(x, w, scale=None, shift=None, stride=1, relu=False):
    """y = relu?(conv2d(x, w, pad 1, stride, groups = C / Cg) * scale[co] + shift[co]) in double"""
    C, Cg = w.shape[0], w.shape[1]
    y = F.conv2d(x.double(), w.double(), None, stride, 1, 1, C // Cg)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def gconv_grads(x, w, dy, stride=1, scale=None, mask=None, rowscale=None):
    """(dx, dw) of the kernels' conventions through autograd in double: dx = (mask > 0) * d/dx <dy * scale, conv(x, w)>,
    dw = rowscale[co] * d/dw <dy, conv(x, w)>"""
    C, Cg = w.shape[0], w.shape[1]
    xd = x.double().clone().requires_grad_(True)
    wd = w.double().clone().requires_grad_(True)
    y = F.conv2d(xd, wd, None, stride, 1, 1, C // Cg)
    g = dy.double()
    dx, = torch.autograd.grad(y, xd, g * scale.double().view(1, -1, 1, 1) if scale is not None else g, retain_graph=True)
    dw, = torch.autograd.grad(y, wd, g)
    if mask is not None:
        dx = dx * (mask > 0).double()
    if rowscale is not None:
        dw = dw * rowscale.double().view(-1, 1, 1, 1)
    return dx, dw


def bottleneck(x, w1, w2, w3, wd, bn, stride, num_groups, stride_in_1x1):
    """the reference's Bottleneck.forward with folded FrozenBN, in double; bn = (s1, b1, s2, b2, s3, b3, sd, bd)"""
    s1, b1, s2, b2, s3, b3, sd, bd = [None if t is None else t.double().view(1, -1, 1, 1) for t in bn]
    stride_1x1, stride_3x3 = (stride, 1) if stride_in_1x1 else (1, stride)
    o = torch.relu(F.conv2d(x, w1, None, stride_1x1) * s1 + b1)
    o = torch.relu(F.conv2d(o, w2, None, stride_3x3, 1, 1, num_groups) * s2 + b2)
    o = F.conv2d(o, w3) * s3 + b3
    idt = x if wd is None else F.conv2d(x, wd, None, stride) * sd + bd
    return torch.relu(o + idt)


def bottleneck_with_grads(x, w1, w2, w3, wd, bn, stride, num_groups, stride_in_1x1, g):
    """(out, dx, dw1, dw2, dw3, dwd) for the loss <g, out>, all in double"""
    leaves = [t.double().clone().requires_grad_(True) for t in (x, w1, w2, w3, wd)]
    out = bottleneck(*leaves, bn, stride, num_groups, stride_in_1x1)
    grads = torch.autograd.grad(out, leaves, g.double())
    return (out.detach(),) + tuple(grads)


def level_weights(level, shape):
    """R_l of the backbone-gradient loss sum_l <P_l, R_l> (tests/golden/gen_golden_resnext.py and tests/test_resnext_model_gpu.py
    draw the same tensors from here)"""
    g = torch.Generator().manual_seed(7700 + level)
    return torch.randn(tuple(shape), generator=g)
