"""Deterministic mode, kernel by kernel (`_hip.set_deterministic`; include/mmtpsm.h: mmt_set_deterministic): every fixed-order form that
stands in for a sum of float atomics.  Each case runs its call three times and requires bit-equal results AND closeness to an
independent reference:
  * the ordered ROIAlign backward (tile gather, per-level accumulate flag) against the opt-in dense form and the oracle;
  * bias gradients through conv_wgrad / conv_wgrad_group / fused._wgrad / LinearFn / DeconvFn against fp64, in modes 3 and 0, with
    the weight gradients of the same calls bit-identical to the default mode's;
  * the loss entry points: values against fp64 torch, gradients bit-identical to the default mode's;
  * the refusals (grouped / stem weight gradient, bf16 storage), and that a step with the mode off issues the launches it did before."""
import collections
import contextlib
import ctypes
import os
import sys

import numpy as np
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
    yield H
    H.set_deterministic(False)
    H.set_f16x2(None)
    if H.get_conv_precision() != prev:
        H.set_conv_precision(prev)


@contextlib.contextmanager
def det(H, on=True):
    H.set_deterministic(on)
    try:
        yield
    finally:
        H.set_deterministic(False)


def cl(x):  # NCHW tensor -> NHWC-dense cuda tensor
    return x.cuda().contiguous(memory_format=torch.channels_last)


def thrice(fn):
    """fn() three times -> the first result, after checking the other two are bit-equal to it"""
    outs = [fn() for _ in range(3)]
    torch.cuda.synchronize()
    flat = [o if isinstance(o, (list, tuple)) else [o] for o in outs]
    for other in flat[1:]:
        for a, b in zip(flat[0], other):
            assert torch.equal(a, b)
    return outs[0]


# ------------------------------------------------------------------------------------------ default untouched (first: before any switch here)
def test_mode_off_issues_the_launches_it_did_before(hip):
    """the C-ABI call histogram (tools/call_hist.py's counter) of one 160 x 160 step with the mode off, recorded before this test
    switches the mode on, equals the histogram of the same step after the mode has been on and off again"""
    H = hip
    import bench
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, crop=160, n_inst=4, base_lr=0.0)   # (learning rate 0: every step is the same step)
    it = cfg.MT.START_MT + 400

    def step(count):
        hist = collections.Counter()
        orig = H._check

        def counting(code, what):
            hist[what] += 1
            return orig(code, what)
        trainer.seed_rng(5)
        il, tg, ul = batch()
        if count:
            H._check = counting
        try:
            c0 = H.C_CALLS[0]
            trainer.train_step(it, il, tg, ul)
            torch.cuda.synchronize()
        finally:
            H._check = orig
        return hist, H.C_CALLS[0] - c0

    for _ in range(3):      # plain, recorded, replayed: the launch plans are warm
        step(False)
    before = step(True)
    with det(H):
        on = step(True)
    after = step(True)
    assert before == after, (before, after)
    assert any(k.endswith("_ordered") for k in on[0]) and not any(k.endswith("_ordered") for k in before[0])


# ------------------------------------------------------------------------------------------ ROIAlign backward
def _roi_case(C, sizes, clustered):
    g = torch.Generator().manual_seed(C + len(sizes))
    L, N, K = len(sizes), 2, 260
    scales = [0.25 / (1 << l) for l in range(L)]
    W0, H0 = sizes[0][1] * 4, sizes[0][0] * 4
    xy = torch.rand(K, 2, generator=g) * torch.tensor([W0 + 40., H0 + 40.]) - 30
    wh = torch.rand(K, 2, generator=g) * 150 + 1
    wh[::7] = torch.rand(wh[::7].shape, generator=g) * 3      # sub-pixel at every level
    wh[3::11] = 400.                                          # larger than the map
    lv = (torch.rand(K, generator=g) * L).long().clamp(max=L - 1)
    img = (torch.arange(K) % N).float()
    if clustered:
        # 200 ROIs of image 0 inside one 20 x 20-pixel window of P2 (80 x 80 image pixels): one texel receives hundreds of terms
        xy[:200] = 48. + torch.rand(200, 2, generator=g) * 50
        wh[:200] = 4. + torch.rand(200, 2, generator=g) * 26
        lv[:200] = 0
        img[:200] = 0.
    rois = torch.cat([img[:, None], xy, xy + wh], 1)
    return L, N, K, scales, rois, lv, [(N, C, h, w) for h, w in sizes], g


@pytest.mark.parametrize("C,sizes,clustered", [(64, [(50, 67), (25, 34), (13, 17), (7, 9)], False),
                                               (64, [(50, 67), (25, 34), (13, 17), (7, 9)], True),
                                               (256, [(64, 80), (32, 40), (16, 20), (8, 10)], False), (128, [(40, 40)], False)],
                         ids=["c64", "c64-clustered", "c256", "c128-one-level"])
def test_roi_align_backward_ordered(hip, C, sizes, clustered, monkeypatch):
    from oracle import native
    H = hip
    L, N, K, scales, rois, lv, shapes, g = _roi_case(C, sizes, clustered)
    r_d, l_d = rois.cuda(), lv.cuda().int()
    stream = torch.cuda.current_stream().cuda_stream
    for res in (7, 14):
        go = torch.randn(K, C, res, res, generator=g)
        g_d = cl(go)
        with det(H):
            plain = thrice(lambda: H.roi_align_backward(g_d, shapes, scales, r_d, l_d, res, res, 2))
        monkeypatch.setenv("MMT_ROI_BWD_DENSE", "1")
        dense = H.roi_align_backward(g_d, shapes, scales, r_d, l_d, res, res, 2)
        monkeypatch.delenv("MMT_ROI_BWD_DENSE")
        for l in range(L):
            assert torch.equal(plain[l], dense[l])              # mmt_roi_align_backward_dense, bit for bit
            idx = (lv == l).nonzero().squeeze(1)
            gr = native.roi_align_backward(go[idx], rois[idx], scales[l], res, res, *shapes[l], 2)
            np.testing.assert_allclose(plain[l].cpu().numpy(), gr.numpy(), rtol=1e-4, atol=5e-6 * max(1.0, float(gr.abs().max())))
        # `into` on levels 0 and 2: those accumulate, the others are written over NaN (straight through the C ABI)
        acc_levels = [l for l in (0, 2) if l < L]
        before = {l: torch.randn(N, sizes[l][0], sizes[l][1], C, generator=g).cuda() for l in acc_levels}

        def with_into():
            bufs = [before[l].clone() if l in before else torch.full((N, h, w, C), float("nan"), device="cuda")
                    for l, (h, w) in enumerate(sizes)]
            into = [bufs[l].permute(0, 3, 1, 2) if l in before else None for l in range(L)]
            with det(H):
                out = H.roi_align_backward(g_d, shapes, scales, r_d, l_d, res, res, 2, into=into)
            for l in acc_levels:
                assert out[l].data_ptr() == bufs[l].data_ptr()
                assert torch.equal(out[l], before[l].permute(0, 3, 1, 2) + plain[l])
            for l in range(L):
                if l not in before:
                    assert torch.equal(out[l], plain[l])
            # the other levels: really over NaN-filled memory
            p = H._pyramid([b.permute(0, 3, 1, 2) for b in bufs], scales, bufs)
            for l in acc_levels:
                bufs[l].copy_(before[l])
            mask = sum(1 << l for l in acc_levels)
            rc = H.lib().mmt_roi_align_backward_ordered(ctypes.byref(p), r_d.data_ptr(), l_d.data_ptr(), K, res, res, 2, g_d.data_ptr(),
                                                        mask, stream)
            assert rc == 0
            return [b.permute(0, 3, 1, 2) for b in bufs]
        acc = thrice(with_into)
        for l in range(L):
            if l in before:
                assert torch.equal(acc[l], before[l].permute(0, 3, 1, 2) + plain[l])
            else:
                assert not torch.isnan(acc[l]).any().item() and torch.equal(acc[l], plain[l])
    # no ROI at all: zeros where written, untouched where accumulated
    with det(H):
        z = H.roi_align_backward(cl(torch.zeros(0, C, 7, 7)), shapes, scales, torch.zeros(0, 5).cuda(), torch.zeros(0).int().cuda(), 7, 7, 2)
        assert all(float(t.abs().max()) == 0.0 for t in z)
        keep = torch.randn(shapes[0]).cuda().contiguous(memory_format=torch.channels_last)
        k0 = keep.clone()
        z = H.roi_align_backward(cl(torch.zeros(0, C, 7, 7)), shapes, scales, torch.zeros(0, 5).cuda(), torch.zeros(0).int().cuda(), 7, 7, 2,
                                 into=[keep] + [None] * (L - 1))
        assert torch.equal(z[0], k0)
        # a call the kernel does not take raises instead of falling back to the atomics
        with pytest.raises(NotImplementedError):
            H.roi_align_backward(g_d, shapes, scales, r_d, l_d, 14, 14, 0)


# ------------------------------------------------------------------------------------------ bias gradients
def _attach(H, t, planes):
    t._mmt_amax = H._amax_of(t)
    if planes:
        H.f16_split_pg(t)
    return t


def _bias_cases(H, mode):
    """-> [(name, run)]; run() -> (dw, db, dy as [M, C] fp64 cpu, what db held before)"""
    from maskrcnn_benchmark.layers import fused
    g = torch.Generator().manual_seed(11)

    def direct(N, Cin, Hh, W, Cout, k, planes, group, nonzero, via_fused=False):
        x = cl(torch.randn(N, Cin, Hh, W, generator=g).relu())
        dy = cl(torch.randn(N, Cout, Hh, W, generator=g) * 0.1 + 0.02)
        dw0 = cl(torch.randn(Cout, Cin, k, k, generator=g) * 1e-3)
        db0 = (torch.randn(Cout, generator=g) if nonzero else torch.zeros(Cout)).cuda()
        dy2 = dy.permute(0, 2, 3, 1).reshape(-1, Cout).double().cpu()

        def run():
            dw, db = dw0.clone(memory_format=torch.preserve_format), db0.clone()
            if mode == 3:
                for t in (x, dy):
                    _attach(H, t, planes)
            if via_fused:
                w = torch.empty(Cout, Cin, k, k, device="cuda").contiguous(memory_format=torch.channels_last)
                dw, db = fused._wgrad(x, dy, w, 1, k // 2, None, True)
                return dw, db, dy2, torch.zeros(Cout, dtype=torch.float64)
            if group:
                H.conv_wgrad_group([(x, dy, (Cout, Cin, k, k), 1, k // 2, dw, None, db)])
            else:
                H.conv_wgrad(x, dy, (Cout, Cin, k, k), 1, k // 2, dw, None, db)
            return dw, db, dy2, db0.double().cpu()
        return run

    def linear(R):
        x = torch.randn(R, 1024, generator=g).cuda()
        w = (torch.randn(1024, 1024, generator=g) * 0.03).cuda().requires_grad_(True)
        b = torch.zeros(1024).cuda().requires_grad_(True)
        gy = (torch.randn(R, 1024, generator=g) * 0.1 + 0.02).cuda()

        def run():
            w.grad = b.grad = None
            fused.linear(x, w, b).backward(gy)
            return w.grad, b.grad, gy.double().cpu(), torch.zeros(1024, dtype=torch.float64)
        return run

    def deconv():
        x = cl(torch.randn(5, 256, 14, 14, generator=g).relu())
        w = cl(torch.randn(256, 256, 2, 2, generator=g) * 0.05).requires_grad_(True)
        b = torch.zeros(256).cuda().requires_grad_(True)
        gy = cl(torch.randn(5, 256, 28, 28, generator=g) * 0.1 + 0.02)

        def run():
            w.grad = b.grad = None
            fused.DeconvFn.apply(x, w, b, False, False).backward(gy)
            return w.grad, b.grad, gy.permute(0, 2, 3, 1).reshape(-1, 256).double().cpu(), torch.zeros(256, dtype=torch.float64)
        return run

    return [("3x3 256->256 2x40x40, planes, one launch", direct(2, 256, 40, 40, 256, 3, True, False, True)),
            ("3x3 256->256 2x40x40, grouped", direct(2, 256, 40, 40, 256, 3, False, True, True)),
            ("1x1 256->15 2x40x36, fused._wgrad", direct(2, 256, 40, 36, 15, 1, False, False, False, via_fused=True)),
            ("1x1 256->15 2x40x36, grouped call", direct(2, 256, 40, 36, 15, 1, False, True, True)),
            ("linear R=1", linear(1)), ("linear R=1030", linear(1030)), ("deconv 256->256 5x14x14", deconv()),
            ("1x1 256->3 5x28x28", direct(5, 256, 28, 28, 3, 1, False, False, True)),
            ("1x1 16->256, M = 2 x 256 x 256", direct(2, 16, 256, 256, 256, 1, False, False, True))]


@pytest.mark.parametrize("mode", [3, 0], ids=["default-f16x2-split", "fp32-mfma"])
def test_bias_gradients_in_a_fixed_order(hip, mode):
    """fp64 column sum within 1e-6 * sum_m |dy[m, c]| per column (the issue's bound: an fp32 sum of <= 2^17 terms in a two-level
    order).  The destination is non-zero where the call takes one (the bound then also has to cover the rounding of the one final
    addition, 2^-24 |result|: those cases have M >= 1440 rows of |dy| ~ 0.08, i.e. a bound of >= 1e-4 against 6e-8 |result|);
    the autograd paths hand back a fresh tensor"""
    H = hip
    H.set_conv_precision(mode)
    H.set_f16x2(True)
    for name, run in _bias_cases(H, mode):
        dw_off, _db_off, dy2, base = run()
        with det(H):
            dw, db, _, _ = thrice(lambda: run()[:2] + (torch.zeros(1), torch.zeros(1)))
        ref = dy2.sum(0)
        bound = 1e-6 * dy2.abs().sum(0)
        err = (db.double().cpu() - base - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("bias gradient, mode %d, %s: error / bound %.3f" % (mode, name, worst))
        assert (err <= bound).all(), (name, worst)
        assert torch.equal(dw, dw_off), name                      # the weight gradient: the default mode's, bit for bit


# ------------------------------------------------------------------------------------------ losses
def _both(H, fn):
    """fn() with the mode off, then three times with it on -> (default result, ordered result)"""
    off = fn()
    with det(H):
        on = thrice(fn)
    return off, on


@pytest.mark.parametrize("P,M,NC", [(3, 7, 5), (700, 28, 3)])
def test_mask_bce_ordered(hip, P, M, NC):
    H = hip
    g = torch.Generator().manual_seed(P + NC)
    logits = torch.randn(P, NC, M, M, generator=g) * 30
    labels = (torch.rand(P, generator=g) * (NC - 1)).long() + 1
    tgt = (torch.rand(P, M, M, generator=g) > 0.5).float()
    ref = F.binary_cross_entropy_with_logits(logits.double()[torch.arange(P), labels], tgt.double())
    a, b, c = cl(logits), labels.cuda(), tgt.cuda()
    (l0, g0), (l1, g1) = _both(H, lambda: H.mask_bce(a, b, c, 0.25))
    assert l1.item() == pytest.approx(ref.item(), rel=1e-5)
    assert torch.equal(g0, g1)


@pytest.mark.parametrize("shape,nt", [((1, 4, 1, 1), 1), ((2, 64, 9, 8), 3), ((2, 64, 9, 8), 8), ((2, 512, 64, 65), 1)])
def test_mgd_level_forward_ordered(hip, shape, nt):
    H = hip
    g = torch.Generator().manual_seed(sum(shape) + nt)
    N, C, Hh, W = shape
    s = torch.randn(shape, generator=g)
    ts = [torch.randn(shape, generator=g) for _ in range(nt)]
    flips = [bool(k % 2) for k in range(nt)]
    m = (torch.rand(N, Hh, W, generator=g) > 0.4).float()
    d = [s.double() - (t.double().flip(3) if f else t.double()) for t, f in zip(ts, flips)]
    num = torch.stack([(m.double()[:, None] * x * x).sum() for x in d])
    sd, td, md = cl(s), [cl(t) for t in ts], m.cuda()
    first = torch.full((nt + 1,), 0.5).cuda()     # (an accumulator that already holds another level's sums)
    off, on = _both(H, lambda: H.mgd_level_forward(sd, td, flips, md, acc=first.clone()))
    on = on.double().cpu() - 0.5
    assert on[nt].item() == m.sum().item()
    np.testing.assert_allclose(on[:nt].numpy(), num.numpy(), rtol=2e-5, atol=1e-6)
    coef = (torch.rand(nt, generator=g) + 0.1).cuda()
    g0, g1 = _both(H, lambda: H.mgd_level_backward(sd, td, flips, md, coef))
    assert torch.equal(g0, g1)


@pytest.mark.parametrize("shape,ns,nt", [((1, 4, 1, 1), 1, 1), ((2, 64, 9, 7), 4, 4), ((2, 512, 128, 65), 2, 2)])
def test_mgd_views_forward_ordered(hip, shape, ns, nt):
    """((2, 512, 128, 65): 1 081 344 threads' worth of column pairs, above the 4096 x 256 grid)"""
    H = hip
    g = torch.Generator().manual_seed(sum(shape) + 7 * ns + nt)
    N, C, Hh, W = shape
    ss = [torch.randn(shape, generator=g) for _ in range(ns)]
    ts = [torch.randn(shape, generator=g) for _ in range(nt)]
    mirrors, flips = [bool(j % 2) for j in range(ns)], [bool((k // 2) % 2) for k in range(nt)]
    m = (torch.rand(N, Hh, W, generator=g) > 0.4).float()
    md = m.double()[:, None]
    num = torch.stack([(md * ((s.double().flip(3) if mj else s.double()) - (t.double().flip(3) if fk else t.double())) ** 2).sum()
                       for s, mj in zip(ss, mirrors) for t, fk in zip(ts, flips)])
    sd, td, mm = [cl(s) for s in ss], [cl(t) for t in ts], m.cuda()
    off, on = _both(H, lambda: H.mgd_views_forward(sd, mirrors, td, flips, mm))
    on = on.double().cpu()
    assert on[ns * nt].item() == m.sum().item()
    np.testing.assert_allclose(on[:ns * nt].numpy(), num.numpy(), rtol=2e-5)
    coef = (torch.rand(ns * nt, generator=g) + 0.1).cuda()
    g0, g1 = _both(H, lambda: H.mgd_views_backward(sd, mirrors, td, flips, mm, coef))
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("R", [1, 257, 1000])
def test_psm_rows_has_no_sum_to_order(hip, R):
    """mmt_psm_rows writes one loss per row and the host sums them with torch: the mode changes nothing, bit for bit"""
    H = hip
    g = torch.Generator().manual_seed(R)
    t, s, w = (torch.randn(2, R, 3, generator=g) * 3).cuda(), (torch.randn(R, 3, generator=g) * 3).cuda(), torch.rand(R, generator=g).cuda()
    for kind in (0, 1, 2):
        (l0, g0), (l1, g1) = _both(H, lambda: H.psm_rows(t, s, w, 0.5, 1, kind))
        assert torch.equal(l0, l1) and torch.equal(g0, g1)


@pytest.mark.parametrize("R,frac", [(1, 1.0), (1000, 0.1), (300000, 0.002), (600000, 0.3)])
def test_rpn_loss_ordered(hip, R, frac):
    """(600 000 anchors: above the 1024 x 256 grid)"""
    H = hip
    g = torch.Generator().manual_seed(R)
    obj, reg, regt = torch.randn(R, generator=g) * 3, torch.randn(R, 4, generator=g) * 0.3, torch.randn(R, 4, generator=g) * 0.3
    u = torch.rand(R, generator=g)
    pos, neg = u < frac, (u >= frac) & (u < 3 * frac)
    labels = torch.where(pos, torch.ones_like(u), torch.where(neg, torch.zeros_like(u), -torch.ones_like(u)))
    beta = 1.0 / 9
    samp = pos | neg
    n = samp.sum().clamp(min=1).double()
    d = (reg.double() - regt.double()).abs()
    wb = (torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta) * pos.double()[:, None]).sum() / n
    wo = (F.binary_cross_entropy_with_logits(obj.double(), labels.clamp(min=0).double(), reduction="none") * samp.double()).sum() / n
    args = [t.cuda() for t in (obj, reg, labels, regt, pos, neg)]
    (o0, a0, b0), (o1, a1, b1) = _both(H, lambda: tuple(t.clone() for t in H.rpn_loss(*args, beta)))
    assert o1[0].item() == pytest.approx(wo.item(), rel=1e-5, abs=1e-9)
    assert o1[1].item() == pytest.approx(wb.item(), rel=1e-5, abs=1e-9)
    assert torch.equal(a0, a1) and torch.equal(b0, b1)


@pytest.mark.parametrize("R,NC,rows", [(7, 3, False), (2000, 81, False), (70000, 3, False), (1024, 3, True)])
def test_box_loss_ordered(hip, R, NC, rows):
    """(70 000 rows: above the 256 x 256 grid; rows: the fixed-capacity form with padding rows)"""
    H = hip
    g = torch.Generator().manual_seed(R + NC)
    logits, breg = torch.randn(R, NC, generator=g) * 2, torch.randn(R, 4 * NC, generator=g) * 0.8
    labels = torch.randint(0, NC, (R,), generator=g) * (torch.rand(R, generator=g) < 0.4)
    regt = torch.randn(R, 4, generator=g) * 0.8
    if rows:
        labels[torch.randperm(R, generator=g)[:137]] = -1
    live = labels >= 0
    cnt = int(live.sum()) if rows else R
    wc = F.cross_entropy(logits.double()[live], labels[live], reduction="sum") / cnt
    idx = (4 * labels.clamp(min=0))[:, None] + torch.arange(4)[None, :]
    d = (torch.gather(breg.double(), 1, idx) - regt.double()).abs()
    wb = (torch.where(d < 1.0, 0.5 * d * d, d - 0.5) * (labels > 0).double()[:, None]).sum() / cnt
    a, b, c, e = logits.cuda(), breg.cuda(), labels.cuda(), regt.cuda()
    n_rows = live.sum().cuda() if rows else None
    (o0, d0, r0), (o1, d1, r1) = _both(H, lambda: H.box_loss(a, b, c, e, n_rows))
    assert o1[0].item() == pytest.approx(wc.item(), rel=1e-5)
    assert o1[1].item() == pytest.approx(wb.item(), rel=1e-5, abs=1e-9)
    assert torch.equal(d0, d1) and torch.equal(r0, r1)


@pytest.mark.parametrize("sizes", [[1], [5, 1, 9, 30]])
def test_ciam_dgamma_ordered(hip, sizes):
    """CIAM's gamma gradient: <dOut, A x> summed over the instances in row order (fp64 tensor formulation, the project's 2e-4)"""
    H = hip
    torch.manual_seed(sum(sizes))
    n, C = sum(sizes), 16
    x = torch.relu(torch.randn(n, C, 14, 14, device="cuda") * 0.3 + 0.1)
    group = torch.cat([torch.full((s,), 3 * i + 1, dtype=torch.int64) for i, s in enumerate(sizes)]).cuda()
    gamma = torch.full((1,), 0.7, device="cuda")
    gout = torch.randn(n, C, 14, 14, device="cuda")
    out, A, J = H.ciam_fwd(x, group, gamma)
    (dx0, dg0), (dx1, dg1) = _both(H, lambda: H.ciam_bwd(x, group, gamma, A, J, gout))
    mix = torch.matmul(A.double(), x.double().view(n, -1))                    # O = A X
    ref = (gout.double().view(n, -1) * mix).sum().item()
    mag = (gout.double().view(n, -1) * mix).abs().sum().item()
    assert abs(dg1.item() - ref) <= 2e-4 * abs(ref) + 1e-5 * mag
    assert torch.equal(dx0, dx1)


# ------------------------------------------------------------------------------------------ refusals
def test_unordered_configurations_refuse(hip):
    H = hip
    x = cl(torch.randn(2, 64, 12, 12))
    dy = cl(torch.randn(2, 64, 12, 12))
    dwg = cl(torch.zeros(64, 8, 3, 3))
    img = torch.randn(2, 3, 32, 32).cuda()
    dys = cl(torch.randn(2, 64, 16, 16))
    dws = cl(torch.zeros(64, 3, 7, 7))
    with det(H):
        with pytest.raises(NotImplementedError, match="gconv_wgrad_kernel"):
            H.gconv3x3_wgrad(x, dy, (64, 8, 3, 3), 1, dwg)
        with pytest.raises(NotImplementedError, match="stem_wgrad_kernel"):
            H.stem_wgrad(img, dys, dws)
        with pytest.raises(NotImplementedError, match="bf16"):
            H.set_bf16_storage(True)
        assert not H._BF16_STORAGE and float(dwg.abs().max()) == 0.0 and float(dws.abs().max()) == 0.0
    H.gconv3x3_wgrad(x, dy, (64, 8, 3, 3), 1, dwg)
    H.stem_wgrad(img, dys, dws)
    H.set_bf16_storage(True)
    try:
        with pytest.raises(NotImplementedError, match="bf16"):
            H.set_deterministic(True)
        assert not H.get_deterministic()
    finally:
        H.set_bf16_storage(False)
    torch.cuda.synchronize()
    assert float(dwg.abs().max()) > 0.0 and float(dws.abs().max()) > 0.0
