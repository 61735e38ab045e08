"""The three-tap form of the plane-fed weight gradient (csrc/conv_wgpl.hip: wgrad_pl_body<3>): one block computes the kw taps 0, 1, 2
of its (co tile, kh, ci block) from ONE copy of the operands per 32-pixel super-step -- the x block in LDS holds the 34 pixels
w0 - 1 ... w0 + 32 of the row h + kh - pad, and the three taps' fragments are reads of that block 32 bytes apart.

What can go wrong there, and what pins it:
  * swapped taps, a halo column that is not zero, a row shift that leaks: a single 1 in x at the corners of every row, small-integer
    dy -- every dW[:, :, kh, kw] equals the fp64 reference EXACTLY (small integers are exact in fp16, their sums in fp32);
  * columns 31 / 32 take their halo from the neighbouring 32-pixel segment; the last row of an image and the first row of the next
    are neighbours in the row index of the planes and must not see each other: small integers everywhere, exact;
  * several tiles, one and several pixel ranges across blocks, accumulation into a non-zero dw, row scale, bias gradient: the
    default arithmetic's bound (3e-6 of every output's own sum |a||b|, against fp64); a second call repeats the first bit for bit;
  * the grouped launch: three jobs of different shapes, a block count that is no multiple of 8, a job with several ranges;
  * the range guard's exact path covers the block's three taps.
The one-tap form (k = 5, k = 1) is pinned by tests/test_f16x2_gpu.py::test_wgrad_from_row_blocked_planes."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

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
    H.WGRAD_GROUP = True
    H.set_f16x2(None)
    H.set_conv_precision(prev)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _planes(H, *tensors):
    """what the forward / data-gradient launch of the layer leaves behind: the recorded maximum and the row-blocked planes"""
    for t in tensors:
        t._mmt_amax = H._amax_of(t)
        H.f16_split_pg(t)


def _ints(shape, lo, hi, g):
    return _cl(torch.randint(lo, hi + 1, shape, generator=g).float().cuda())


def _ref(x, dy, k, rs=None):
    """fp64 weight gradient and every output's own sum |a||b|"""
    Cout, Cin = dy.shape[1], x.shape[1]
    xu = F.unfold(x.double(), k, padding=k // 2)
    ref = torch.einsum("nco,nko->ck", dy.double().flatten(2), xu).view(Cout, Cin, k, k)
    den = torch.einsum("nco,nko->ck", dy.double().abs().flatten(2), xu.abs()).view(Cout, Cin, k, k)
    if rs is not None:
        ref, den = ref * rs.double().view(-1, 1, 1, 1), den * rs.double().view(-1, 1, 1, 1)
    return ref, den


def _wgrad(H, x, dy, k, dw0=None, rs=None, bias=False):
    Cout, Cin = dy.shape[1], x.shape[1]
    dw = _cl(torch.zeros((Cout, Cin, k, k), device="cuda")) if dw0 is None else dw0.clone(memory_format=torch.preserve_format)
    db = torch.zeros((Cout,), device="cuda") if bias else None
    n0 = H.F16_STATS.get("wgrad_pl", 0)
    H.conv_wgrad(x, dy, (Cout, Cin, k, k), 1, k // 2, dw, rs, db)
    torch.cuda.synchronize()
    assert H.F16_STATS.get("wgrad_pl", 0) == n0 + 1   # the plane-fed kernel ran, nothing else
    return dw, db


def _splits(H, x, dy, k):
    a = H._conv_shape(H.ConvArgs(), x.shape[0], x.shape[2], x.shape[3], x.shape[1], dy.shape[1], k, k, 1, k // 2, dy.shape[2], dy.shape[3])
    r = H.WgradRoute()
    assert H.lib().mmt_conv_wgrad_route(ctypes.byref(a), H.WG_HAVE_PLANES, ctypes.byref(r)) == 0
    return r.splits if r.family in (H.WGRAD_PLANES_1, H.WGRAD_PLANES_3) else 0


@pytest.mark.parametrize("row", [0, 1, 2])
@pytest.mark.parametrize("col", [0, 31])
def test_tap_identity_exact(hip, row, col):
    H = hip
    N, Cin, Hh, W, Cout, k = 1, 128, 3, 32, 128, 3
    g = torch.Generator().manual_seed(10 * row + col)
    x = torch.zeros((N, Cin, Hh, W))
    x[0, 37, row, col] = 1.0
    x = _cl(x.cuda())
    dy = _ints((N, Cout, Hh, W), -4, 4, g)
    _planes(H, x, dy)
    dw, _ = _wgrad(H, x, dy, k)
    ref, _ = _ref(x, dy, k)
    assert ref.abs().sum().item() > 0
    for kh in range(k):
        for kw in range(k):
            assert torch.equal(dw[:, :, kh, kw].double(), ref[:, :, kh, kw]), (kh, kw)


def test_segment_and_image_boundaries_exact(hip):
    H = hip
    N, Cin, Hh, W, Cout, k = 2, 128, 2, 64, 128, 3
    g = torch.Generator().manual_seed(5)
    x = _ints((N, Cin, Hh, W), -2, 2, g)
    dy = _ints((N, Cout, Hh, W), -2, 2, g)
    _planes(H, x, dy)
    dw, db = _wgrad(H, x, dy, k, bias=True)
    ref, _ = _ref(x, dy, k)
    for kh in range(k):
        for kw in range(k):
            assert torch.equal(dw[:, :, kh, kw].double(), ref[:, :, kh, kw]), (kh, kw)
    assert torch.equal(db.double(), dy.double().sum((0, 2, 3)))


@pytest.mark.parametrize("shape,several", [((1, 256, 5, 96, 256), False), ((2, 128, 16, 32, 128), True)])
def test_tiles_and_ranges_within_the_bound(hip, shape, several):
    H = hip
    N, Cin, Hh, W, Cout = shape
    k = 3
    g = torch.Generator().manual_seed(sum(shape))
    x = _cl(torch.randn((N, Cin, Hh, W), generator=g).relu().cuda())
    dy = _cl((torch.randn((N, Cout, Hh, W), generator=g) * 1e-3).cuda())
    rs = (torch.rand(Cout, generator=g) + 0.5).cuda()
    dw0 = _cl((torch.randn((Cout, Cin, k, k), generator=g) * 1e-5).cuda())
    _planes(H, x, dy)
    sp = _splits(H, x, dy, k)
    assert sp > 1 if several else sp >= 1, sp
    dw, db = _wgrad(H, x, dy, k, dw0, rs, bias=True)
    ref, den = _ref(x, dy, k, rs)
    err = ((dw.double() - dw0.double() - ref).abs() / den.clamp_min(1e-300)).max().item()
    print("shape", shape, "ranges", sp, "err / sum|a||b|", err)
    assert err <= 3e-6, err
    rb = dy.double().sum((0, 2, 3))
    eb = (db.double() - rb).abs().max().item() / dy.double().abs().sum((0, 2, 3)).max().item()
    assert eb <= 3e-6, eb
    dw2, _ = _wgrad(H, x, dy, k, dw0, rs, bias=True)
    assert torch.equal(dw, dw2)


# (N, Cin, H, W, Cout): 3 tiles in 1 range = 3 blocks; 3 tiles in several ranges; 12 tiles in 1 range = 12 blocks
GROUP = [(2, 128, 16, 32, 128), (2, 128, 64, 64, 128), (1, 256, 8, 32, 256)]


def _group_run(H, group):
    H.WGRAD_GROUP = group
    jobs, keep = [], []
    for i, (N, Cin, Hh, W, Cout) in enumerate(GROUP):
        g = torch.Generator().manual_seed(40 + i)
        x = _cl(torch.randn((N, Cin, Hh, W), generator=g).relu().cuda())
        dy = _cl((torch.randn((N, Cout, Hh, W), generator=g) * 1e-3).cuda())
        _planes(H, x, dy)
        rs = (torch.rand(Cout, generator=g) + 0.5).cuda()
        dw0 = _cl((torch.randn((Cout, Cin, 3, 3), generator=g) * 1e-5).cuda())
        dw = dw0.clone(memory_format=torch.preserve_format)
        db = torch.zeros((Cout,), device="cuda") if i == 1 else None
        jobs.append((x, dy, (Cout, Cin, 3, 3), 1, 1, dw, rs, db))
        keep.append((x, dy, rs, dw0, dw, db))
    n0 = H.F16_STATS.get("wgrad_grouped", 0)
    H.conv_wgrad_group(jobs)
    torch.cuda.synchronize()
    return keep, H.F16_STATS.get("wgrad_grouped", 0) - n0


def test_grouped_launch(hip):
    H = hip
    outs, n = _group_run(H, True)
    assert n == len(GROUP)
    # a job keeps a quarter of its own ranges inside a group (csrc/conv_wgrad.hip: wg_plan): the second keeps several
    assert _splits(H, outs[1][0], outs[1][1], 3) > 4 and _splits(H, outs[0][0], outs[0][1], 3) <= 4
    singles, n1 = _group_run(H, False)
    assert n1 == 0
    again, _ = _group_run(H, True)
    for sp, (x, dy, rs, dw0, dw, db), s1, a1 in zip(GROUP, outs, singles, again):
        ref, den = _ref(x, dy, 3, rs)
        got = dw.double() - dw0.double()
        assert ((got - ref).abs() / den.clamp_min(1e-300)).max().item() <= 3e-6, sp
        one = s1[4].double() - dw0.double()
        assert ((got - one).abs() / den.clamp_min(1e-300)).max().item() <= 3e-6, sp
        assert torch.equal(dw, a1[4]), sp
        if db is not None:
            rb = dy.double().sum((0, 2, 3))
            assert (db.double() - rb).abs().max().item() <= 3e-6 * dy.double().abs().sum((0, 2, 3)).max().item(), sp


@pytest.mark.parametrize("bad", ["x", "dy"])
def test_range_guard_covers_the_three_taps(hip, bad):
    H = hip
    N, C, S, Co, k = 2, 128, 32, 256, 3
    g = torch.Generator().manual_seed(23 + len(bad))
    x = torch.randn((N, C, S, S), generator=g).relu()
    dy = torch.randn((N, Co, S, S), generator=g) * 50.0
    (x if bad == "x" else dy)[N // 2, 17, S // 2 - 2, S // 2 - 1] = 1.0e8   # ONE element 10^8 x the rest: the planes are useless
    x, dy = _cl(x.cuda()), _cl(dy.cuda())
    rs = (torch.rand(Co, generator=g) + 0.5).cuda()
    _planes(H, x, dy)
    f0 = H.F16_STATS["fallback"]
    dw, db = _wgrad(H, x, dy, k, None, rs, bias=True)
    assert H.F16_STATS["fallback"] == f0
    ref, den = _ref(x, dy, k, rs)
    for kh in range(k):
        for kw in range(k):
            e = ((dw[:, :, kh, kw].double() - ref[:, :, kh, kw]).abs() / (den[:, :, kh, kw] + 1e-30)).max().item()
            assert e <= 3e-6, (kh, kw, e)
    rb = dy.double().sum((0, 2, 3))
    assert (db.double() - rb).abs().max().item() <= 3e-6 * dy.double().abs().sum((0, 2, 3)).max().item()
