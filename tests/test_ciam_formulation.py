"""tests/ciam_formulations.py, the fp64 statement of CIAM with the reference's normalisations that the GPU tests expect
(tests/test_ciam_norm_gpu.py, tests/test_irnet_norm_gpu.py), held to the reference's own module and its inputs to two conditions.
CPU only.

1. It reproduces tests/golden/ciam_norm.npz -- the reference's CIAM_Module in float64, all six combinations, two slices -- to 1e-10
   of each tensor's largest magnitude (fp64 against fp64, the same operations), and with the default pair it equals
   tests/tensor_formulations.py::ciam.
2. Every input of the GPU test is
   visible:      for every combination and each gradient term of its normalisation (the instance norm, the channel weights, the L2
                 factor), the formulation with that term detached differs from the full one by at least 10 x the gradient bar, in
                 the quantity the GPU test compares: dx - dout against its largest magnitude.  (out and dgamma = <dout, A x> do not
                 see a detached term at all: the forward pass is the same.)  So a kernel that drops a term cannot pass.
                 Exempt, because identically zero: the default pair (no term); the instance norm under NORM 2 (E / F does not change
                 when an instance is rescaled); the layout of singleton groups [1, 1, 1] (a softmax over one entry is constant: no
                 gradient reaches the energies, whatever the normalisation).
   conditioned:  torch's own fp32 evaluation of the formulation on the CPU stays within a quarter of each bar of the fp64 one, so
                 the bars measure the kernels and not the input."""
import os

import numpy as np
import pytest
import torch

import ciam_formulations as cf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ciam_norm.npz")
SLICES = [(5, 7), (9, 14)]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLD)


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("norm,pre", cf.COMBOS)
def test_formulation_reproduces_the_reference(golden, k, norm, pre):
    n, hw = SLICES[k]
    x = torch.from_numpy(golden["x%d" % k]).double().requires_grad_(True)
    gout = torch.from_numpy(golden["gout%d" % k]).double()
    assert x.shape == (n, 16, hw, hw)
    gamma = torch.tensor(float(golden["gamma"]), dtype=torch.float64, requires_grad=True)
    out = cf.ciam(gamma, x, [n], norm, pre)
    out.backward(gout)
    tag = "%d_n%d_p%d" % (k, norm, int(pre))
    for name, v in (("out", out.detach()), ("dx", x.grad)):
        ref, mx = torch.from_numpy(golden[name + tag]), float(golden[name + tag + "_max"])
        got = v.reshape(-1)[cf.sample_index(v.numel(), k)]
        err = (got - ref).abs().max().item() / mx
        assert err <= 1e-10, (name, tag, err)
        assert abs(v.abs().max().item() - mx) <= 1e-10 * mx
        assert abs(v.sum().item() - float(golden[name + tag + "_sum"])) <= 1e-10 * mx * v.numel()
    ref = float(golden["dgamma" + tag][0])
    assert abs(gamma.grad.item() - ref) <= 1e-10 * abs(ref), (tag, gamma.grad.item(), ref)


def test_the_combinations_differ(golden):
    """the golden file holds six different functions, not one six times: every pair of combinations differs in `out` by far more
    than the comparison above allows.  One pair is the same function by its arithmetic: NORM 2 with and without PRE_NORM (E / F does not
    change when an instance is rescaled; only the 1e-10 in the denominator sees the scale)"""
    for k in (0, 1):
        outs = [golden["out%d_n%d_p%d" % (k, norm, int(pre))] for norm, pre in cf.COMBOS]
        for a in range(len(outs)):
            for b in range(a + 1, len(outs)):
                if cf.COMBOS[a][0] == 2 and cf.COMBOS[b][0] == 2:
                    continue
                assert np.abs(outs[a] - outs[b]).max() > 1e-6 * np.abs(outs[a]).max(), (k, cf.COMBOS[a], cf.COMBOS[b])


@pytest.mark.parametrize("sizes,hw", cf.LAYOUTS)
def test_default_pair_is_the_tensor_formulation(sizes, hw):
    import tensor_formulations as tf
    x, gout = cf.gaussian_inputs(sizes, hw, seed=5)
    x, gout = x.double(), gout.double()
    group = cf.group_ids(sizes)
    res = []
    for f in (lambda g, xx: cf.ciam(g, xx, sizes, -1, False), lambda g, xx: tf.ciam(g, xx, group)):
        xx = x.clone().requires_grad_(True)
        g = torch.tensor(cf.GAMMA, dtype=torch.float64, requires_grad=True)
        out = f(g, xx)
        out.backward(gout)
        res.append((out.detach(), xx.grad, g.grad.reshape(1)))
    for a, b in zip(*res):
        assert cf.rel_dev(a, b) <= 1e-10


def test_other_norm_values_mean_none():
    """the reference's else branch: everything but 1 and 2"""
    x, gout = cf.structured_inputs([6], 7, seed=2)
    base = cf.evaluate(x, cf.GAMMA, gout, [6], -1, True)
    for norm in (0, 3):
        for a, b in zip(cf.evaluate(x, cf.GAMMA, gout, [6], norm, True), base):
            assert torch.equal(a, b)


@pytest.mark.parametrize("sizes,hw", cf.LAYOUTS)
@pytest.mark.parametrize("norm,pre", cf.VARIANTS)
def test_gpu_inputs_are_visible_and_conditioned(norm, pre, sizes, hw):
    x, gout = cf.inputs_for(norm, pre, sizes, hw)
    full = cf.evaluate(x, cf.GAMMA, gout, sizes, norm, pre)
    f32 = cf.evaluate(x, cf.GAMMA, gout, sizes, norm, pre, dtype=torch.float32)
    for what, a, b, bar in zip(("out - x", "dx - dout", "dgamma"), f32, full, (cf.FWD_BAR, cf.GRAD_BAR, cf.GRAD_BAR)):
        dev = cf.rel_dev(a, b)
        print("conditioning NORM %d PRE_NORM %s %s %s: fp32 on the CPU %.2e of the maximum (bar %.0e)" % (norm, pre, sizes, what, dev, bar))
        assert dev <= bar / 4, (what, dev)
    if max(sizes) == 1:
        return                       # singleton groups: every term is identically zero (module docstring)
    for term in cf.terms_of(norm, pre):
        cut = cf.evaluate(x, cf.GAMMA, gout, sizes, norm, pre, detach=(term,))
        assert torch.equal(cut[0], full[0]) and torch.equal(cut[2], full[2])      # the forward pass and dgamma do not see it
        dev = cf.rel_dev(cut[1], full[1])
        print("visibility NORM %d PRE_NORM %s %s %s: %.2e of the maximum of dx - dout" % (norm, pre, sizes, term, dev))
        assert dev >= 10 * cf.GRAD_BAR, (term, dev)


def test_the_exempt_terms_are_zero():
    """the instance norm under NORM 2 moves dx by the 1e-10 in the denominator only; in singleton groups no term moves anything"""
    x, gout = cf.structured_inputs([9], 14, seed=3)
    for pre in (True,):
        full = cf.evaluate(x, cf.GAMMA, gout, [9], 2, pre)
        cut = cf.evaluate(x, cf.GAMMA, gout, [9], 2, pre, detach=("instance_norm",))
        assert cf.rel_dev(cut[1], full[1]) <= 1e-8
    x, gout = cf.structured_inputs([1, 1, 1], 14, seed=3)
    for norm, pre in cf.VARIANTS:
        full = cf.evaluate(x, cf.GAMMA, gout, [1, 1, 1], norm, pre)
        cut = cf.evaluate(x, cf.GAMMA, gout, [1, 1, 1], norm, pre, detach=cf.TERMS)
        assert cf.rel_dev(cut[1], full[1]) <= 1e-12


def test_capacity_and_workspace_queries():
    """the library's own expressions (include/mmtpsm.h), host side: no GPU, nothing launched"""
    from maskrcnn_benchmark import _hip as H
    L = H.lib()
    for n, C, hw in ((200, 16, 196), (512, 16, 196), (14, 16, 49), (300, 16, 784), (512, 1, 4)):
        assert L.mmt_ciam_norm_lds_bytes(n, C, hw) == 4 * max(C * hw + (C + 1) * n, (C + 4) * n)
        assert L.mmt_ciam_norm_saved_floats(n, C) == n * C * n + n + n * C
        assert L.mmt_ciam_norm_ws_floats(n, C) == n * n + n + n * C + n
    assert H.ciam_norm_fits(512, 16, 196) and H.ciam_norm_fits(1, 1, 1)
    assert not H.ciam_norm_fits(300, 16, 784) and not H.ciam_norm_fits(513, 16, 4) and not H.ciam_norm_fits(8, 17, 16)
    assert L.mmt_ciam_norm_lds_bytes(0, 16, 196) < 0 and L.mmt_ciam_norm_ws_floats(4, 0) < 0
    assert [H.ciam_norm_kind(v) for v in (-1, 0, 1, 2, 3)] == [0, 0, 1, 2, 0]


def test_module_reads_the_switches_once():
    """construction no longer refuses NORM / PRE_NORM; what stays refused still raises"""
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.relation.mask_relation_module import CIAM_Module, MaskRelationRefineNet
    for norm, pre in cf.COMBOS + [(0, False), (3, True)]:
        cfg = make_default_cfg()
        cfg.MODEL.RELATION_MASK.NORM, cfg.MODEL.RELATION_MASK.PRE_NORM = norm, pre
        m = CIAM_Module(cfg)
        assert (m.norm, m.prenorm) == (norm if norm in (1, 2) else 0, pre)
        assert [k for k, _ in m.named_parameters()] == ["gamma"]
        with pytest.raises(RuntimeError, match="GPU tensors"):
            m(torch.zeros(3, 16, 4, 4))
    cfg = make_default_cfg()
    assert (cfg.MODEL.RELATION_MASK.NORM, cfg.MODEL.RELATION_MASK.PRE_NORM) == (-1, False)
    cfg.MODEL.RELATION_MASK.NORM, cfg.MODEL.RELATION_MASK.TYPE = 1, "CAM"
    with pytest.raises(NotImplementedError):
        MaskRelationRefineNet(cfg)
