"""fp64 tensor formulations of the stem's backward on the CPU (plain torch), the references of tests/test_stem_backward_gpu.py:

  * the gradient of the 3x3 / stride 2 / pad 1 max pool with the (y > 0) mask of its input's ReLU, once through F.max_pool2d's
    autograd and once restated explicitly (the window's FIRST maximum in (kh, kw) scan order receives the window's gradient; taps
    outside the image never win) -- the two are asserted equal on the tie-rich inputs of the tests, once;
  * the weight gradient of the 7x7 / stride 2 / pad 3 convolution (torch.nn.grad.conv2d_weight);
  * the whole stem (conv -> affine -> ReLU -> max pool) under autograd."""
import torch
import torch.nn.functional as F

POOL_SHAPES = [(1, 4, 1, 1), (1, 4, 2, 2), (1, 8, 5, 7), (2, 64, 37, 53), (2, 64, 40, 40), (1, 64, 136, 200)]   # (N, C, H, W)


def pool_inputs(shape, real_g=False):
    """y: multiples of 0.25 in [-1, 2] (tied windows are frequent, many values are <= 0); g: integers with |g| <= 8 (every sum of at
    most four of them is exact in fp32), or N(0, 1)"""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(17 + C + 3 * H + 5 * W + int(real_g))
    y = torch.randint(-4, 9, shape, generator=gen).float() * 0.25
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if real_g:
        g = torch.randn((N, C, Ho, Wo), generator=gen)
    else:
        g = torch.randint(-8, 9, (N, C, Ho, Wo), generator=gen).float()
    return y, g


def maxpool_backward_autograd(y, g):
    yd = y.double().clone().requires_grad_(True)
    F.max_pool2d(yd, 3, 2, 1).backward(g.double())
    return yd.grad * (y > 0)


def maxpool_backward_first_maximum(y, g):
    N, C, H, W = y.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    yp = F.pad(y.double(), (1, 1, 1, 1), value=float("-inf"))
    win = F.unfold(yp, 3, stride=2).view(N, C, 9, -1)                      # taps in (kh, kw) scan order
    L = win.shape[-1]
    assert L >= Ho * Wo
    is_max = win == win.max(dim=2, keepdim=True).values
    rank = torch.arange(9, 0, -1).view(1, 1, 9, 1)                          # the earliest tap carries the largest rank
    first = (is_max * rank).argmax(dim=2, keepdim=True)                     # (distinct ranks: no tie left)
    onehot = torch.zeros_like(win).scatter_(2, first, 1.0)
    # unfold over the padded map may cover one window more per axis than the pool has (even H / W): those get no gradient
    Hu, Wu = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    assert (Hu, Wu) == (Ho, Wo)
    contrib = onehot * g.double().reshape(N, C, 1, Ho * Wo)
    dyp = F.fold(contrib.view(N, C * 9, L), (H + 2, W + 2), 3, stride=2)
    return dyp[:, :, 1:H + 1, 1:W + 1] * (y > 0)


_AGREED = []


def maxpool_backward_reference(y, g):
    """the explicit restatement; the first call checks, for every tie-rich input of the tests, that it IS ATen's rule"""
    if not _AGREED:
        for shape in POOL_SHAPES:
            yy, gg = pool_inputs(shape)
            a, b = maxpool_backward_autograd(yy, gg), maxpool_backward_first_maximum(yy, gg)
            assert torch.equal(a, b), (shape, (a - b).abs().max().item())
        _AGREED.append(True)
    return maxpool_backward_first_maximum(y, g)


def stem_wgrad_reference(x, dy, rowscale=None):
    """dw (64, 3, 7, 7) fp64 of conv2d(x, w, stride 2, pad 3) for the output gradient dy, rows times rowscale"""
    dw = torch.nn.grad.conv2d_weight(x.double(), (dy.shape[1], x.shape[1], 7, 7), dy.double(), stride=2, padding=3)
    if rowscale is not None:
        dw = dw * rowscale.double().view(-1, 1, 1, 1)
    return dw


def stem_with_grad(x, w, scale, shift, r):
    """(out, d <r, out> / d w) of max_pool(relu(conv(x, w, stride 2, pad 3) * scale + shift), 3, 2, 1) in fp64"""
    wd = w.double().clone().requires_grad_(True)
    y = F.conv2d(x.double(), wd, None, 2, 3) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    out = F.max_pool2d(F.relu(y), 3, 2, 1)
    (out * r.double()).sum().backward()
    return out.detach(), wd.grad
