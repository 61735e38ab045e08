"""The loss, pooling and optimiser kernels (csrc/losses.hip, csrc/optim.hip, maxpool3x3s2) at their edges: sizes at which the
grid-stride loops loop, the smallest sizes, the widest argument values the entry points take, extreme logits, refused arguments.
Every reference is the same operation in plain torch fp64 on the CPU.

Tolerances are the ones tests/test_hip_kernels.py uses for the same kernel.  Where an extreme input needs more, the extra is an
absolute term worked out from the fp32 rounding of that operation -- U = 2^-24 (unit roundoff) times the sum of the magnitudes
that are rounded -- and the comment beside the assertion gives that bound and the largest error measured against fp64."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126     # smallest normal fp32: what lies below is lost, an absolute error of at most this much per value


@pytest.fixture(scope="module")
def hip():
    from maskrcnn_benchmark import _hip
    _hip.lib()
    assert torch.cuda.is_available()
    return _hip


def cl(x):  # NCHW cpu tensor -> NHWC-dense cuda tensor
    return x.cuda().contiguous(memory_format=torch.channels_last)


def worst(got, want, bound):
    """largest |got - want| / bound over the elements (bound > 0 elementwise)"""
    got, want, bound = (torch.as_tensor(a).double().cpu() for a in (got, want, bound))
    if got.numel() == 0:
        return 0.0
    return float(((got - want).abs() / bound).max())


# ------------------------------------------------------------------------------------------ mask BCE
@pytest.mark.parametrize("P,M,NC", [(5, 14, 2), (37, 28, 3), (3, 7, 5), (700, 28, 3)])
def test_mask_bce_extreme_logits_and_the_stride_loop(hip, P, M, NC):
    """(700, 28): 548 800 elements, above the 2048 x 256 grid"""
    g = torch.Generator().manual_seed(P + NC)
    logits = torch.randn(P, NC, M, M, generator=g) * 30
    labels = (torch.rand(P, generator=g) * (NC - 1)).long() + 1
    idx = torch.randperm(P * M * M, generator=g)[:16]                 # +-1e4 in the label's channel, where it is read
    pp, yy, xx = idx // (M * M), (idx // M) % M, idx % M
    logits[pp[:8], labels[pp[:8]], yy[:8], xx[:8]] = 1e4
    logits[pp[8:], labels[pp[8:]], yy[8:], xx[8:]] = -1e4
    tgt = (torch.rand(P, M, M, generator=g) > 0.5).float()
    gs = 0.25
    x = logits.double()[torch.arange(P), labels].requires_grad_()
    ref = F.binary_cross_entropy_with_logits(x, tgt.double())
    (ref * gs).backward()
    loss, grad = hip.mask_bce(cl(logits), labels.cuda(), tgt.cuda(), gs)
    assert torch.isfinite(loss).item() and torch.isfinite(grad).all().item()
    # every term max(x, 0) - x t + log1p(exp(-|x|)) is >= 0: a sum without cancellation, the project's 1e-5 holds at any scale
    assert loss.item() == pytest.approx(ref.item(), rel=1e-5)
    grad = grad.cpu()
    sel = torch.zeros(P, NC, dtype=torch.bool)
    sel[torch.arange(P), labels] = True
    assert (grad[~sel] == 0).all()                        # every non-label channel: exactly 0
    # grad = (sigmoid(x) - t) gs / n.  sigmoid(x) -> 1 cancels against t = 1, so beside rtol 1e-4 the absolute term is the rounding
    # of the two operands: 3 U sigmoid (expf, add, divide) + U |difference|  <=  4 U (sigmoid + t) gs / n; a sigmoid under TINY is lost.
    # Measured on the MI355X: the loss within 1.1e-7 relative; the largest gradient error 0.18 of rtol |ref| + that bound, at (700, 28, 3).
    n = P * M * M
    bound = 1e-4 * x.grad.abs() + (4 * U * (torch.sigmoid(x.detach()) + tgt.double()) + 2 * TINY) * gs / n
    w = worst(grad[sel].view(P, M, M), x.grad, bound)
    print("mask_bce P=%d M=%d NC=%d: loss rel %.2e, grad error / bound %.3f" % (P, M, NC, abs(loss.item() / ref.item() - 1), w))
    assert w <= 1.0


def test_mask_bce_of_no_positive_is_zero(hip):
    loss, grad = hip.mask_bce(torch.zeros(0, 3, 28, 28).cuda(), torch.zeros(0).long().cuda(), torch.zeros(0, 28, 28).cuda(), 0.25)
    assert loss.item() == 0.0 and grad.shape == (0, 3, 28, 28)


# ------------------------------------------------------------------------------------------ MGD
def mgd_reference(s, ts, flips, m, coef):
    """num_k = sum m (s - flip_k(t_k))^2, msum = sum m, grad = 2 m sum_k coef_k (s - flip_k(t_k)), and the magnitudes summed in
    grad (for the rounding bound); fp64, NCHW"""
    s, m = s.double(), m.double()[:, None]
    d = [s - (t.double().flip(3) if f else t.double()) for t, f in zip(ts, flips)]
    num = torch.stack([(m * x * x).sum() for x in d])
    grad = 2 * m * sum(c * x for c, x in zip(coef.double(), d))
    mag = 2 * m * sum(c.abs() * x.abs() for c, x in zip(coef.double(), d))
    return num, m.sum(), grad, mag


def mgd_check(hip, N, C, H, W, nt, mask, seed=0):
    g = torch.Generator().manual_seed(1000 * C + 10 * W + nt + seed)
    s = torch.randn(N, C, H, W, generator=g)
    ts = [torch.randn(N, C, H, W, generator=g) for _ in range(nt)]
    flips = [bool((k + seed) % 2) for k in range(nt)]
    if nt >= 3:
        flips[2] = flips[1]                       # mixed, not merely alternating
    m = {"random": (torch.rand(N, H, W, generator=g) > 0.4).float(), "zeros": torch.zeros(N, H, W), "ones": torch.ones(N, H, W)}[mask]
    coef = torch.rand(nt, generator=g) + 0.1
    num, msum, grad, mag = mgd_reference(s, ts, flips, m, coef)
    sd, td, md = cl(s), [cl(t) for t in ts], m.cuda()
    acc = hip.mgd_level_forward(sd, td, flips, md).cpu().double()
    gs = hip.mgd_level_backward(sd, td, flips, md, coef.cuda()).cpu()
    assert acc.shape == (nt + 1,)
    if mask == "zeros":
        assert (acc == 0).all() and (gs == 0).all()         # exactly
        return
    assert acc[nt].item() == msum.item()                    # a sum of 0 / 1 below 2^24: exact
    # sums of non-negative terms: the project's 2e-5 on the loss holds for each num_k
    np.testing.assert_allclose(acc[:nt].numpy(), num.numpy(), rtol=2e-5)
    if mask == "random":
        assert (gs[(m == 0)[:, None].expand_as(gs)] == 0).all()
    # grad: nt differences (U each), nt products (U each), nt - 1 additions of partial sums: at most (nt + 1) U sum_k |2 m coef_k d_k|
    # beside the project's rtol 1e-4.  Measured on the MI355X: the largest error 0.094 of rtol |ref| + bound, at (2, 64, 9, 8) with nt = 3.
    w = worst(gs, grad, 1e-4 * grad.abs() + (nt + 1) * U * mag + 1e-300)
    print("mgd (%d, %d, %d, %d) nt=%d %s: grad error / bound %.3f" % (N, C, H, W, nt, mask, w))
    assert w <= 1.0


@pytest.mark.parametrize("shape", [(1, 4, 1, 1), (2, 4, 3, 5), (1, 12, 7, 1), (2, 64, 9, 8)])
@pytest.mark.parametrize("nt", [1, 3, 8])
def test_mgd_level_small_shapes_and_teacher_counts(hip, shape, nt):
    """C4 == 1, odd W, W == 1 (the flip is the identity), nt == 8 (every teacher slot)"""
    for mask in ("random", "zeros", "ones"):
        mgd_check(hip, *shape, nt, mask)
    mgd_check(hip, *shape, nt, "random", seed=1)    # the other flips


def test_mgd_level_beyond_the_grid(hip):
    """(2, 512, 64, 65): 1 064 960 float4s, above the 4096 x 256 grid -- the stride loop runs, on an odd W"""
    mgd_check(hip, 2, 512, 64, 65, 1, "random", seed=1)


def test_mgd_level_refuses_what_it_cannot_take(hip):
    s6, m = cl(torch.randn(1, 6, 4, 4)), torch.ones(1, 4, 4).cuda()
    with pytest.raises(RuntimeError):
        hip.mgd_level_forward(s6, [s6], [False], m)
    with pytest.raises(RuntimeError):
        hip.mgd_level_backward(s6, [s6], [False], m, torch.ones(1).cuda())
    s = cl(torch.randn(1, 8, 4, 4))
    with pytest.raises(RuntimeError):
        hip.mgd_level_forward(s, [s] * 9, [False] * 9, m)
    with pytest.raises(RuntimeError):
        hip.mgd_level_backward(s, [s] * 9, [False] * 9, m, torch.ones(9).cuda())
    # the library itself, behind the binding's own check: nt = 9 and nt = 0 in the structure
    acc = torch.zeros(10).cuda()
    for nt in (9, 0):
        T = hip.MgdTeachers()
        for i in range(8):
            T.t[i] = s.data_ptr()
        T.nt = nt
        st = torch.cuda.current_stream().cuda_stream
        assert hip.lib().mmt_mgd_level_forward(s.data_ptr(), ctypes.byref(T), m.data_ptr(), 1, 4, 4, 8, acc.data_ptr(), st) != 0
        assert hip.lib().mmt_mgd_level_backward(s.data_ptr(), ctypes.byref(T), m.data_ptr(), 1, 4, 4, 8, acc.data_ptr(),
                                                torch.empty_like(s).data_ptr(), st) != 0
    torch.cuda.synchronize()
    assert (acc == 0).all()


# ------------------------------------------------------------------------------------------ mask pool
@pytest.mark.parametrize("src,dst", [((50, 70), (7, 9)), ((33, 33), (33, 33)), ((10, 10), (16, 16)), ((100, 100), (5, 5)),
                                     ((101, 67), (13, 10))])
def test_mask_pool_is_the_adaptive_average_binarised(hip, src, dst):
    """(100, 100) -> (5, 5): 400-element windows, more than one wave; (10, 10) -> (16, 16): windows of one and two pixels"""
    g = torch.Generator().manual_seed(src[0] + dst[1])
    N = 2
    # values 0..3 with window means around 0.5; and a checkerboard (every window of even area exactly 0.5) with a few cells raised
    rnd = torch.multinomial(torch.tensor([0.68, 0.22, 0.05, 0.05]), N * src[0] * src[1], True, generator=g).view(N, *src)
    yy, xx = torch.meshgrid(torch.arange(src[0]), torch.arange(src[1]), indexing="ij")
    chk = ((yy + xx) % 2).expand(N, -1, -1).clone()
    chk[torch.rand(chk.shape, generator=g) < 0.002] = 3
    for seg in (rnd, chk):
        ref = F.adaptive_avg_pool2d(seg.double()[:, None], dst)[:, 0]
        if seg is chk and src != dst:
            assert (ref == 0.5).sum() >= 4                  # windows whose mean is exactly 0.5 (one-pixel windows have none)
        want = (ref > 0.5).float()
        assert 0 < want.mean() < 1
        got = hip.mask_pool(seg.int().cuda(), *dst)
        np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())


# ------------------------------------------------------------------------------------------ PSM
def psm_inputs(NC, K, R, scale, seed):
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(K, R, NC, generator=g) * scale).clamp(-80, 80)
    s = (torch.randn(R, NC, generator=g) * scale).clamp(-80, 80)
    if scale > 1 and R > 2:
        t[:, 0, 0], t[:, 0, 1:] = 80, -80        # the widest row: every view, both signs
        s[0, 0], s[0, 1:] = -80, 80
    roww = torch.tensor([0.0, 1.0, 1.5])[torch.randint(0, 3, (R,), generator=g)]
    return t, s, roww


def psm_rows_reference(t, s, roww, temp, sharpen, kind):
    """fp64: (row loss, row gradient, bound of the fp32 rounding error of each)"""
    K, R, NC = t.shape
    t, roww = t.double(), roww.double()
    s = s.double().requires_grad_()
    tm = t.mean(0)
    A_t, A_s = t.abs().amax((0, 2)), s.detach().abs().amax(1)          # per row
    e_tm = (K + 1) * U * A_t                                           # K - 1 additions of logits up to A_t, one division
    if kind == 2:
        d = s - tm
        loss = roww * (d * d).sum(1)
        loss.sum().backward()
        e_d = e_tm[:, None] + U * d.detach().abs()
        e_loss = roww * ((2 * d.detach().abs() * e_d).sum(1) + (NC + 2) * U * (d * d).detach().sum(1))
        return loss.detach(), s.grad, e_loss, roww[:, None] * 2 * e_d
    p = F.softmax(tm, 1)
    inv = 1.0 / temp if (kind == 0 and sharpen) else 1.0
    if inv != 1.0:
        p = p ** inv
        p = p / p.sum(1, keepdim=True)
    logp = F.log_softmax(s, 1)
    if kind == 0:
        terms = -p * logp
    else:
        terms = torch.where(p > 0, p * (torch.log(p.clamp(min=1e-300)) - logp), torch.zeros_like(p))
    loss = roww * terms.sum(1)
    loss.sum().backward()
    # relative error of a probability: its exponent's argument is rounded (teacher: e_tm and the subtraction of the maximum, up to
    # 2 A_t U; student: 2 A_s U), numerator and normaliser both, times 1 / temp where the power is taken; 8 U for expf, the
    # sum, the division and powf themselves
    rel_t = ((2 * (e_tm + 2 * U * A_t)) * inv + 8 * U)[:, None]
    rel_p = (2 * (2 * U * A_s) + 8 * U)[:, None]
    lse = torch.logsumexp(s.detach(), 1, keepdim=True)
    e_logp = U * (s.detach().abs() + 3 * lse.abs() + 1)              # logp = s - (smax + logf(sum))
    pd, lp = p.detach(), logp.detach()
    if kind == 0:
        e_loss = (pd * e_logp + rel_t * pd * lp.abs()).sum(1) + (NC + 1) * U * terms.detach().abs().sum(1)
    else:
        logt = torch.log(pd.clamp(min=1e-300))
        e_loss = (pd * (e_logp + rel_t + U * logt.abs()) + rel_t * pd * (logt - lp).abs()).sum(1) \
            + (NC + 1) * U * (pd * (logt.abs() + lp.abs())).sum(1)
    e_grad = roww[:, None] * (rel_p * F.softmax(s.detach(), 1) + rel_t * pd + 2 * TINY)
    # (a probability under TINY is lost; it multiplies a logarithm that stays below 1e3 for anything fp64 holds)
    return loss.detach(), s.grad, roww * (e_loss + NC * TINY * 1e3), e_grad


@pytest.mark.parametrize("R", [1, 255, 256, 257, 1000])
def test_psm_rows_every_kind_width_and_row_count(hip, R):
    """NC up to the 16 the kernel's registers hold, K = 1, R around the block of 256; logits up to +-80.
    Beside the project's rtol 1e-4 the bound of psm_rows_reference; its widest term (K 8, +-80, temp 0.25) is 7048 U = 4.2e-4
    relative to a teacher probability.  Measured on the MI355X over all cases: the largest error is 0.50 of rtol |ref| + bound for
    the losses (R = 256) and 0.16 for the gradients."""
    worst_l = worst_g = 0.0
    for i, (NC, K) in enumerate((nc, k) for nc in (2, 3, 7, 16) for k in (1, 2, 3, 8)):
        scale = (1.0, 25.0)[(i + R) % 2]
        t, s, roww = psm_inputs(NC, K, R, scale, seed=100 * R + i)
        for kind, sharpen, temp in ((0, 0, 0.5), (0, 1, 0.25), (0, 1, 0.5), (0, 1, 1.0), (1, 1, 0.5), (2, 0, 1.0)):
            loss, grad, e_loss, e_grad = psm_rows_reference(t, s, roww, temp, sharpen, kind)
            rl, rg = hip.psm_rows(t.cuda(), s.cuda(), roww.cuda(), temp, sharpen, kind)
            rl, rg = rl.cpu(), rg.cpu()
            assert torch.isfinite(rl).all() and torch.isfinite(rg).all()
            assert (rl[roww == 0] == 0).all() and (rg[roww == 0] == 0).all()          # exactly
            wl = worst(rl, loss, 1e-4 * loss.abs() + e_loss + 1e-300)
            wg = worst(rg, grad, 1e-4 * grad.abs() + e_grad + 1e-300)
            assert wl <= 1.0 and wg <= 1.0, (NC, K, R, scale, kind, sharpen, temp, wl, wg)
            worst_l, worst_g = max(worst_l, wl), max(worst_g, wg)
    print("psm_rows R=%d: loss error / bound %.3f, grad error / bound %.3f" % (R, worst_l, worst_g))


@pytest.mark.parametrize("R", [1, 255, 256, 257, 1000])
def test_psm_variance_every_width_and_row_count(hip, R):
    """std over the K views (unbiased), summed over the classes.  std = ||d|| / sqrt(K - 1) with d = q - mean, so an error e in d moves
    it by at most ||e|| / sqrt(K - 1): e = e_q + e_mean + U |d|, e_q = (4 A U + 8 U) q for a softmax of logits up to A (0 without
    the softmax: the values are the inputs), e_mean = mean of e_q + (K + 1) U max |q|; (K + 3) U std for the sum, division and root.
    Beside the project's rtol 1e-4.  Measured on the MI355X: the largest error is 0.021 of rtol |ref| + bound (R = 1000)."""
    worst_v = 0.0
    for i, (NC, K) in enumerate((nc, k) for nc in (2, 3, 7, 16) for k in (2, 3, 8)):
        scale = (1.0, 25.0)[(i + R) % 2]
        t, _, _ = psm_inputs(NC, K, R, scale, seed=200 * R + i)
        for use_softmax in (True, False):
            td = t.double()
            q = F.softmax(td, 2) if use_softmax else td
            ref = q.std(0).sum(1)
            A = td.abs().amax((0, 2))[None, :, None]
            e_q = (4 * A * U + 8 * U) * q if use_softmax else torch.zeros_like(q)
            d = q - q.mean(0, keepdim=True)
            e = e_q + e_q.mean(0, keepdim=True) + (K + 1) * U * q.abs().amax(0, keepdim=True) + U * d.abs()
            bound = ((e * e).sum(0) / (K - 1)).sqrt().sum(1) + (K + 3) * U * ref
            v = hip.psm_variance(t.cuda(), use_softmax=use_softmax).cpu()
            assert torch.isfinite(v).all()
            w = worst(v, ref, 1e-4 * ref + bound + 1e-300)
            assert w <= 1.0, (NC, K, R, scale, use_softmax, w)
            worst_v = max(worst_v, w)
    print("psm_variance R=%d: error / bound %.3f" % (R, worst_v))


def test_psm_refuses_what_it_cannot_take(hip):
    t17, s17, w = torch.randn(2, 5, 17).cuda(), torch.randn(5, 17).cuda(), torch.ones(5).cuda()
    with pytest.raises(RuntimeError):
        hip.psm_rows(t17, s17, w, 0.5, 1, 0)
    with pytest.raises(RuntimeError):
        hip.psm_variance(t17)
    with pytest.raises(RuntimeError):
        hip.psm_variance(torch.randn(1, 5, 3).cuda())       # one view has no deviation
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ EMA / SGD
SIZES = [1, 2, 3, 4, 5, 7, 1023, 4194307]    # below one float4: the tail does everything; 4 194 307: above 4 x 256 x 4096, a tail of 3


@pytest.mark.parametrize("n", SIZES)
def test_ema_update_every_tail_and_alpha(hip, n):
    g = torch.Generator().manual_seed(n)
    for alpha in (0.0, 1.0, 0.999):
        t, s = torch.randn(n, generator=g), torch.randn(n, generator=g)
        want = t.double() * alpha + s.double() * (1 - alpha)
        td = t.cuda()
        hip.ema_update(td, s.cuda(), alpha)
        np.testing.assert_allclose(td.cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-7)
        if alpha in (0.0, 1.0):
            assert torch.equal(td.cpu(), s if alpha == 0.0 else t)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("first", [True, False])
def test_sgd_momentum_three_steps_every_tail(hip, n, first):
    """`first` both ways for the first step: it ignores the buffer (here NaN), or it reads a zero one -- the same update"""
    g = torch.Generator().manual_seed(n + 1)
    a = torch.randn(n, generator=g)
    p = torch.nn.Parameter(a.double())
    opt = torch.optim.SGD([p], lr=0.01, momentum=0.9, weight_decay=1e-4)
    cp = a.clone().cuda()
    buf = torch.full((n,), float("nan")).cuda() if first else torch.zeros(n).cuda()
    for step in range(3):
        gr = torch.randn(n, generator=g)
        p.grad = gr.double()
        opt.step()
        hip.sgd_momentum(cp, gr.cuda(), buf, 0.01, 1e-4, 0.9, first and step == 0)
    np.testing.assert_allclose(cp.cpu().numpy(), p.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(buf.cpu().numpy(), opt.state[p]["momentum_buffer"].numpy(), rtol=1e-5, atol=1e-6)


def test_optimiser_kernels_refuse_a_view_off_the_float4_grid(hip):
    t, s, b = torch.randn(64).cuda(), torch.randn(64).cuda(), torch.randn(64).cuda()
    t0, s0, b0 = t.clone(), s.clone(), b.clone()
    for args in ((t[1:], s[1:]), (t[1:], s[:-1]), (t[:-1], s[1:])):
        with pytest.raises(RuntimeError):
            hip.ema_update(*args, 0.5)
    for args in ((t[1:], s[1:], b[1:]), (t[1:], s[:-1], b[:-1]), (t[:-1], s[1:], b[:-1]), (t[:-1], s[:-1], b[1:])):
        with pytest.raises(RuntimeError):
            hip.sgd_momentum(*args, 0.01, 1e-4, 0.9, False)
    torch.cuda.synchronize()
    assert torch.equal(t, t0) and torch.equal(s, s0) and torch.equal(b, b0)


# ------------------------------------------------------------------------------------------ max pool
def maxpool_inputs(shape, seed):
    """-> [(name, x)]: random; all negative (a zero pad would win); -inf planted on the borders"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    neg = -torch.rand(*shape, generator=g) - 0.01
    inf = neg.clone()
    inf[:, :, 0, ::2] = inf[:, :, -1, 1::3] = inf[:, :, ::3, 0] = inf[:, :, 1::2, -1] = float("-inf")
    inf[:, 0] = float("-inf")    # a whole channel: every window of it
    return [("random", x), ("negative", neg), ("-inf", inf)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 4, 1, 1), (1, 4, 2, 2), (2, 8, 3, 5), (1, 64, 33, 47)])
def test_maxpool_is_padded_with_minus_infinity(hip, shape, dtype):
    """the kernel clamps its taps to the image instead of padding: the same maximum only because a clamped tap repeats a value of
    the window -- a pad of zeros would show on negative data, a skipped tap on -inf"""
    for name, x in maxpool_inputs(shape, sum(shape)):
        x = x.to(dtype)                                     # bf16: rounded inputs; the maximum of bf16 values is one of them
        want = F.max_pool2d(x.float(), 3, 2, 1)
        got = hip.maxpool3x3s2(cl(x))
        assert got.dtype == dtype and got.shape == want.shape
        np.testing.assert_array_equal(got.float().cpu().numpy(), want.numpy(), err_msg=name)


def test_maxpool_beyond_the_grid(hip):
    """(2, 64, 514, 514) -> 257 x 257: 2 113 568 float4s, above the 8192 x 256 grid"""
    g = torch.Generator().manual_seed(5)
    x = -torch.rand(2, 64, 514, 514, generator=g) - 0.01
    got = hip.maxpool3x3s2(cl(x))
    assert torch.equal(got.cpu(), F.max_pool2d(x, 3, 2, 1))


def test_maxpool_refuses_channels_off_the_float4_grid(hip):
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(RuntimeError):
            hip.maxpool3x3s2(cl(torch.randn(1, 6, 4, 4).to(dtype)))
    torch.cuda.synchronize()
