"""CIAM with the reference's normalisations on the device (csrc/relation.hip: mmt_ciam_norm_fwd / _bwd / _bwd_ordered;
MODEL.RELATION_MASK.NORM 1, 2 and PRE_NORM) against the fp64 formulation of tests/ciam_formulations.py, which
tests/test_ciam_formulation.py pins to the reference's own module and whose inputs it holds to the visibility and conditioning
conditions.

Compared are the ATTENTION PARTS, each against its own largest magnitude: out - x, dx - dout (the identity path is exactly x and
dout, 3-18 x larger on these inputs, and would hide an error in them) and dgamma.  Bars: the project's for this module
(tests/test_relation_kernels_gpu.py), 2e-5 forward and 2e-4 gradients.  Every measured deviation is printed (profiles/ciam_norm.txt
keeps a copy)."""
import functools

import pytest
import torch

import ciam_formulations as cf

pytestmark = pytest.mark.gpu


def _cfg(norm, pre):
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    cfg.MODEL.RELATION_MASK.NORM = norm
    cfg.MODEL.RELATION_MASK.PRE_NORM = pre
    return cfg


def _module(norm, pre, gamma=cf.GAMMA):
    from maskrcnn_benchmark.modeling.relation.mask_relation_module import CIAM_Module
    mod = CIAM_Module(_cfg(norm, pre)).cuda()
    with torch.no_grad():
        mod.gamma.fill_(gamma)
    return mod


def _run(norm, pre, x, group, gout):
    """-> out, dx, dgamma of CIAM_Module on the device"""
    mod = _module(norm, pre)
    xg = x.clone().requires_grad_(True)
    out = mod(xg, group)
    out.backward(gout)
    return out.detach(), xg.grad, mod.gamma.grad.clone()


@functools.lru_cache(maxsize=None)
def _case(norm, pre, li):
    """the input of a case on the device and its fp64 expectation, computed once"""
    sizes, hw = cf.LAYOUTS[li]
    x, gout = cf.inputs_for(norm, pre, sizes, hw)
    ref = cf.evaluate(x, cf.GAMMA, gout, sizes, norm, pre)
    return x.cuda(), cf.group_ids(sizes).cuda(), gout.cuda(), ref


@pytest.mark.parametrize("li", range(len(cf.LAYOUTS)))
@pytest.mark.parametrize("norm,pre", cf.VARIANTS)
def test_variant_vs_fp64_formulation(norm, pre, li):
    x, group, gout, ref = _case(norm, pre, li)
    out, dx, dg = _run(norm, pre, x, group, gout)
    got = (out.double() - x.double(), dx.double() - gout.double(), dg.double())
    devs = [cf.rel_dev(a, b) for a, b in zip(got, ref)]
    print("CIAM NORM %d PRE_NORM %s groups %s %dx%d: out - x %.2e (bar %.0e), dx - dout %.2e, dgamma %.2e (bar %.0e)"
          % (norm, pre, cf.LAYOUTS[li][0], cf.LAYOUTS[li][1], cf.LAYOUTS[li][1], devs[0], cf.FWD_BAR, devs[1], devs[2], cf.GRAD_BAR))
    assert devs[0] <= cf.FWD_BAR, ("out - x", devs[0])
    assert devs[1] <= cf.GRAD_BAR, ("dx - dout", devs[1])
    assert devs[2] <= cf.GRAD_BAR, ("dgamma", devs[2])


def _raw(H, norm, pre, x, group, gout, ordered=False):
    """the library called directly on NaN-filled outputs (J on a sentinel) -> out, A, J, dx, dgamma"""
    n, C, hw = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
    L = H.lib()
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    out, A, dx, dg = nan(*x.shape), nan(n, n), nan(*x.shape), nan(1)
    J = torch.full((C, n), -7, dtype=torch.int32, device="cuda")
    saved, ws = nan(L.mmt_ciam_norm_saved_floats(n, C)), nan(L.mmt_ciam_norm_ws_floats(n, C))
    gamma = torch.full((1,), cf.GAMMA, device="cuda")
    kind = H.ciam_norm_kind(norm)
    assert L.mmt_ciam_norm_fwd(H._p(x), H._p(group), n, C, hw, kind, int(pre), H._p(gamma), H._p(saved), H._p(A), H._p(J), H._p(out),
                               H._stream()) == 0
    f = L.mmt_ciam_norm_bwd_ordered if ordered else L.mmt_ciam_norm_bwd
    assert f(H._p(x), H._p(group), n, C, hw, kind, int(pre), H._p(gamma), H._p(saved), H._p(A), H._p(J), H._p(gout), H._p(ws), H._p(dx),
             H._p(dg), H._stream()) == 0
    torch.cuda.synchronize()
    return out, A, J, dx, dg


@pytest.mark.parametrize("norm,pre", cf.VARIANTS)
def test_every_output_element_is_written(norm, pre):
    """workspaces and outputs handed in full of NaN: out, dx, A, dgamma come back finite everywhere, A is zero outside the group and
    a row of it sums to one, J points inside the row's own group"""
    from maskrcnn_benchmark import _hip as H
    x, group, gout, _ = _case(norm, pre, 0)
    sizes = cf.LAYOUTS[0][0]
    for ordered in (False, True):
        out, A, J, dx, dg = _raw(H, norm, pre, x, group, gout, ordered)
        for t in (out, A, dx, dg):
            assert torch.isfinite(t).all()
        same = group[:, None] == group[None, :]
        assert (A[~same] == 0).all()
        assert (A.sum(1) - 1).abs().max().item() < 1e-5
        lo = torch.tensor([sum(sizes[:k]) for k, s in enumerate(sizes) for _ in range(s)], device="cuda")
        hi = torch.tensor([sum(sizes[:k + 1]) for k, s in enumerate(sizes) for _ in range(s)], device="cuda")
        assert ((J >= lo[None]) & (J < hi[None])).all()


@pytest.mark.parametrize("norm,pre", cf.VARIANTS)
def test_groups_do_not_see_each_other(norm, pre):
    """other features in ONE group leave every other group's out and dx bit-identical (NORM 1's sums must not cross groups)"""
    x, group, gout, _ = _case(norm, pre, 0)
    sizes = cf.LAYOUTS[0][0]       # [5, 1, 37, 70]: the third group changes
    st, en = sizes[0] + sizes[1], sizes[0] + sizes[1] + sizes[2]
    x2 = x.clone()
    x2[st:en] = x2[st:en].flip(0) * 1.7 + 0.01
    a = _run(norm, pre, x, group, gout)
    b = _run(norm, pre, x2, group, gout)
    keep = torch.ones(x.shape[0], dtype=torch.bool, device="cuda")
    keep[st:en] = False
    assert torch.equal(a[0][keep], b[0][keep]) and torch.equal(a[1][keep], b[1][keep])
    assert not torch.equal(a[0][~keep], b[0][~keep])


def test_default_pair_is_todays_calls():
    """NORM -1 / PRE_NORM False (and NORM 0, 3: "none" like every value but 1 and 2) through CIAM_Module: the bits of _hip.ciam_fwd /
    _hip.ciam_bwd called directly, from two library calls.  (dgamma is a sum of float atomics in the default mode: its bits are
    compared in deterministic mode, where it is the row-ordered sum.)"""
    from maskrcnn_benchmark import _hip as H
    sizes, hw = cf.LAYOUTS[0]
    x, gout = cf.gaussian_inputs(sizes, hw, seed=9)
    x, gout, group = x.cuda(), gout.cuda(), cf.group_ids(sizes).cuda()
    gamma = torch.full((1,), cf.GAMMA, device="cuda")
    try:
        for det in (False, True):
            H.set_deterministic(det)
            out0, A, J = H.ciam_fwd(x, group, gamma)
            dx0, dg0 = H.ciam_bwd(x, group, gamma, A, J, gout)
            for norm in (-1, 0, 3):
                calls = H.C_CALLS[0]
                out, dx, dg = _run(norm, False, x, group, gout)
                assert H.C_CALLS[0] - calls == 2
                assert torch.equal(out, out0) and torch.equal(dx, dx0)
                if det:
                    assert torch.equal(dg, dg0)
    finally:
        H.set_deterministic(False)


@pytest.mark.parametrize("norm,pre", cf.VARIANTS)
def test_deterministic_mode(norm, pre):
    """two calls in deterministic mode: out, dx, dgamma bit-identical; out and dx are the default mode's bits"""
    from maskrcnn_benchmark import _hip as H
    x, group, gout, ref = _case(norm, pre, 3)          # [200, 56]
    off = _run(norm, pre, x, group, gout)
    try:
        H.set_deterministic(True)
        a = _run(norm, pre, x, group, gout)
        b = _run(norm, pre, x, group, gout)
    finally:
        H.set_deterministic(False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[0], off[0]) and torch.equal(a[1], off[1])
    assert cf.rel_dev(a[2].double(), ref[2]) <= cf.GRAD_BAR


@pytest.mark.parametrize("shape,what", [((513, 16, 2, 2), "n > 512"), ((8, 17, 4, 4), "C > 16"), ((300, 16, 28, 28), "LDS")])
def test_refusals_come_before_any_launch(shape, what):
    """beyond the capacity the module raises and the library answers MMT_EINVAL; no library call that issues work is made"""
    from maskrcnn_benchmark import _hip as H
    n, C, h, w = shape
    x = torch.rand(shape, device="cuda")
    group = torch.zeros(n, dtype=torch.int64, device="cuda")
    if what == "LDS":
        assert n <= 512 and C <= 16 and H.lib().mmt_ciam_norm_lds_bytes(n, C, h * w) > 65536
        assert H.lib().mmt_ciam_norm_lds_bytes(n, C, h * w) == 4 * max(C * h * w + (C + 1) * n, (C + 4) * n)
    for norm, pre in cf.VARIANTS:
        mod = _module(norm, pre)
        calls = H.C_CALLS[0]
        with pytest.raises(RuntimeError, match="CIAM"):
            mod(x, group)
        with pytest.raises(RuntimeError, match="mmt_ciam_norm_fwd"):
            H.ciam_norm_fwd(x, group, mod.gamma.detach(), norm, pre)
        assert H.C_CALLS[0] == calls
    out = torch.zeros_like(x)
    A = torch.zeros(n, n, device="cuda")
    J = torch.zeros(C, n, dtype=torch.int32, device="cuda")
    saved = torch.zeros(H.lib().mmt_ciam_norm_saved_floats(n, C), device="cuda")
    gamma = torch.zeros(1, device="cuda")
    rc = H.lib().mmt_ciam_norm_fwd(H._p(x), H._p(group), n, C, h * w, 1, 1, H._p(gamma), H._p(saved), H._p(A), H._p(J), H._p(out),
                                   H._stream())
    assert rc == -22, rc   # MMT_EINVAL (include/mmtpsm.h)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
