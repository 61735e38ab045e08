"""ResNeXt backbones on the GPU: R-50-FPN with NUM_GROUPS 32, WIDTH_PER_GROUP 8, STRIDE_IN_1X1 False, FREEZE_CONV_BODY_AT 2 (all four
group widths appear, layer1 is frozen) against the reference's own CPU backbone, recorded by tests/golden/gen_golden_resnext.py.

Model bar: 1e-4 * max |reference tensor| on pyramid samples and weight-gradient samples -- the project's bar for model taps against
its CPU oracle; the 1x1 layers of a block run on the default two-term fp16 split, which is what that bar was set for, the grouped
3x3 runs exact fp32.  Exact comparisons (forward_pair against the batched pass, repeated passes against the first) are exact.
The measured worst deviations are printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, load_synth

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests"))

BAR = 1e-4
LOSS_KEYS = {"loss_classifier", "loss_box_reg", "loss_seg", "loss_objectness", "loss_rpn_box_reg", "mt_fg_loss", "mt_classifier"}


def _cfg():
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    cfg.merge_from_list(["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8,
                         "MODEL.RESNETS.STRIDE_IN_1X1", False, "MODEL.BACKBONE.FREEZE_CONV_BODY_AT", 2])
    return cfg


@pytest.fixture(scope="module")
def rx_weights():
    shapes = json.load(open(os.path.join(GOLD, "state_shapes_resnext50.json")))["shapes"]
    return load_synth().make_weights(shapes, seed=0)


def _backbone(rx_weights):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.modeling.backbone.backbone import build_backbone
    H.lib()
    bb = build_backbone(_cfg())
    missing, unexpected = bb.load_state_dict({k[len("backbone."):]: v for k, v in rx_weights.items() if k.startswith("backbone.")},
                                             strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return bb.cuda().train()


def _images():
    from maskrcnn_benchmark.structures.image_list import to_image_list
    imgs, _ = load_synth().make_labeled(2, 160, 4, seed=1234)
    return to_image_list(list(imgs), 32).tensors.cuda()


def _nchw(t):
    return t.detach().float().cpu().contiguous().reshape(-1)


def _level_loss(pyr):
    import grouped_formulations as gf
    return sum((p * gf.level_weights(l, p.shape).to(p.device)).sum() for l, p in enumerate(pyr))


def _check(what, got, ref, ref_max, bar=BAR):
    dev = (got.double() - ref.double()).abs().max().item() / max(float(ref_max), 1e-30)
    print("resnext %-44s worst |got - ref| / max |ref| = %.3e" % (what, dev))
    assert dev <= bar, (what, dev)


def test_backbone_matches_the_reference_backbone(rx_weights):
    fx = np.load(os.path.join(GOLD, "resnext160.npz"))
    bb = _backbone(rx_weights)
    pyr = bb(_images())
    assert len(pyr) == 5
    for l, p in enumerate(pyr):
        assert list(p.shape) == list(fx["P%d_shape" % l])
        _check("P%d" % l, _nchw(p)[torch.from_numpy(fx["P%d_idx" % l])], torch.from_numpy(fx["P%d_val" % l]), fx["P%d_max" % l])
    _level_loss(pyr).backward()
    from maskrcnn_benchmark.layers import fused
    fused.join_wgrads()
    params = dict(bb.named_parameters())
    names = sorted(k[2:-4] for k in fx.files if k.startswith("g:") and k.endswith(":val"))
    assert len(names) == 13 and sum(".conv2." in n for n in names) == 3
    for n in names:
        g = params[n].grad
        assert g is not None and list(g.shape) == list(fx["g:%s:shape" % n]), n
        _check("d " + n, _nchw(g)[torch.from_numpy(fx["g:%s:idx" % n])], torch.from_numpy(fx["g:%s:val" % n]), fx["g:%s:max" % n])
    for n, p in params.items():
        if ".layer1." in n or ".stem." in n:
            assert p.grad is None, n   # frozen


@pytest.mark.parametrize("stride_in_1x1", [True, False])
def test_one_block_both_stride_placements(stride_in_1x1):
    """BottleneckWithFixedBatchNorm(256, 512, 512, num_groups=32, stride=2) with downsample against the fp64 formulation of the
    reference's block: output, dx and the four weight gradients"""
    import grouped_formulations as gf
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.modeling.backbone.backbone import BottleneckWithFixedBatchNorm
    H.lib()
    g = torch.Generator().manual_seed(11 + int(stride_in_1x1))
    blk = BottleneckWithFixedBatchNorm(256, 512, 512, num_groups=32, stride_in_1x1=stride_in_1x1, stride=2)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
        for n, m in (("bn1", blk.bn1), ("bn2", blk.bn2), ("bn3", blk.bn3), ("ds", blk.downsample[1])):
            m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5) * (0.4 if n == "bn3" else 1.0))
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.bias.shape, generator=g) * 0.4 + 0.8)
    x = torch.relu(torch.randn((2, 256, 24, 24), generator=g))   # the output of a fused ReLU, like every block input
    gout = torch.randn((2, 512, 12, 12), generator=g)
    bn = []
    for m in (blk.bn1, blk.bn2, blk.bn3, blk.downsample[1]):
        s = m.weight.double() * m.running_var.double().rsqrt()
        bn += [s, m.bias.double() - m.running_mean.double() * s]
    ws = [blk.conv1.weight.detach().clone(), blk.conv2.weight.detach().clone(), blk.conv3.weight.detach().clone(),
          blk.downsample[0].weight.detach().clone()]
    ref = gf.bottleneck_with_grads(x, *ws, bn, 2, 32, stride_in_1x1, gout)

    blk = blk.cuda()
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = blk(xd)
    tag = "1x1" if stride_in_1x1 else "3x3"
    _check("block (stride in %s) out" % tag, _nchw(out), ref[0].reshape(-1), ref[0].abs().max())
    # the conventions of layers/fused.py: the consumer hands over a gradient already masked by (out > 0), the node returns the
    # gradient w.r.t. its ReLU-output input masked by (x > 0)
    out.backward((gout.cuda() * (out.detach() > 0)).contiguous(memory_format=torch.channels_last))
    from maskrcnn_benchmark.layers import fused
    fused.join_wgrads()
    dx_ref = ref[1] * (x > 0)
    _check("block (stride in %s) dx" % tag, _nchw(xd.grad), dx_ref.reshape(-1), dx_ref.abs().max())
    for name, p, r in (("dw1", blk.conv1.weight, ref[2]), ("dw2", blk.conv2.weight, ref[3]), ("dw3", blk.conv3.weight, ref[4]),
                       ("dwd", blk.downsample[0].weight, ref[5])):
        assert p.grad is not None and p.grad.shape == r.shape, name
        _check("block (stride in %s) %s" % (tag, name), _nchw(p.grad), r.reshape(-1), r.abs().max())


def test_forward_pair_equals_batched_forward_and_fills_grouped_gradients(rx_weights):
    from maskrcnn_benchmark.layers import fused
    from maskrcnn_benchmark.modeling.backbone.backbone import forward_pair
    bb = _backbone(rx_weights)
    g = torch.Generator().manual_seed(3)
    xa = (torch.randn((2, 3, 160, 160), generator=g) * 50.0).cuda()
    xb = (torch.randn((2, 3, 160, 160), generator=g) * 50.0).cuda()
    with torch.no_grad():
        cat = bb(torch.cat([xa, xb], 0))
    pa, pb = forward_pair(bb, xa, xb)
    for c, a, b in zip(cat, pa, pb):
        assert torch.equal(c[:2], a.detach()) and torch.equal(c[2:], b.detach())
    assert all(t.requires_grad for t in pa + pb)
    grouped = {n: p for n, p in bb.named_parameters() if ".conv2." in n and p.requires_grad}
    assert len(grouped) == 13 and all(p.shape[1] * 32 == p.shape[0] for p in grouped.values())
    _level_loss(pa).backward()      # half A alone
    fused.join_wgrads()
    got = {n: p.grad.detach().clone() for n, p in grouped.items()}
    assert all(v.abs().max().item() > 0 for v in got.values())
    for p in bb.parameters():
        p.grad = None
    _level_loss(bb(xa)).backward()  # a separate pass over the same images: batch-dependent tiling and atomics change the summation order
    fused.join_wgrads()
    worst = 0.0
    for n, p in grouped.items():
        dev = (got[n].double() - p.grad.double()).abs().max().item() / p.grad.abs().max().item()
        worst = max(worst, dev)
        assert dev <= BAR, (n, dev)
    print("resnext forward_pair half A vs separate pass, grouped weight gradients: worst %.3e" % worst)


def _detector(rx_weights, teacher):
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    m = build_detection_model(_cfg(), is_teacher=True) if teacher else build_detection_model(_cfg(), is_student=True)
    missing, _ = m.load_state_dict(rx_weights, strict=False)
    assert all("cell_anchors" in k for k in missing), missing
    return m.cuda()


def test_repeated_teacher_backbone_passes_are_the_first_pass(rx_weights):
    """five identical no-grad passes of the batched teacher backbone (generalized_rcnn.py::run_backbone: run, recorded into a launch
    plan, replayed): every pass equals the first bit for bit, and the pass without plans"""
    from maskrcnn_benchmark import _hip as H
    m = _detector(rx_weights, True).eval()
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((8, 3, 160, 160), generator=g) * 50.0).cuda()
    keep = H.LAUNCH_PLANS
    try:
        with torch.no_grad():
            H.LAUNCH_PLANS = False
            plain = tuple(t.clone() for t in m.run_backbone(x))
            H.LAUNCH_PLANS = True
            first = None
            for i in range(5):
                got = m.run_backbone(x)
                torch.cuda.synchronize()
                assert len(got) == 5
                if first is None:
                    first = tuple(t.clone() for t in got)
                for a, b, c in zip(got, first, plain):
                    assert a.shape == b.shape and torch.equal(a, b), (i, (a - b).abs().max().item())
                    assert torch.equal(a, c), (i, (a - c).abs().max().item())
    finally:
        H.LAUNCH_PLANS = keep


def _trainer(rx_weights, crop=160, n_inst=4):
    """the bench's trainer (bench.py::build) on the ResNeXt config"""
    from maskrcnn_benchmark.solver import make_optimizer, make_lr_scheduler
    from maskrcnn_benchmark.engine.MTtrainer import MTtrainer, init_teacher_weight
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    from maskrcnn_benchmark.structures.image_list import to_image_list
    synth = load_synth()
    cfg = _cfg()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    student, teacher = _detector(rx_weights, False), _detector(rx_weights, True)
    student.train()
    teacher.eval()
    opt = make_optimizer(cfg, student)
    trainer = MTtrainer(student, teacher, {"source": [None] * cfg.SOLVER.MAX_ITER, "no_label": None}, opt, make_lr_scheduler(cfg, opt),
                        None, None, 10 ** 9, cfg)
    init_teacher_weight(student, teacher)
    imgs, tgs = synth.make_labeled(2, crop, n_inst, seed=1234)
    unl = synth.make_unlabeled(2, crop, cfg.MT.AUG_K + cfg.MT.AUG_S, seed=4321)
    targets = []
    for t in tgs:
        b = BoxList(t["boxes"].to(dev), t["size"], "xyxy")
        b.add_field("labels", t["labels"].to(dev))
        b.add_field("masks", SegmentationMask([[p for p in inst] for inst in t["polys"]], t["size"], mode="poly"))
        targets.append(b)
    imgs, unl = imgs.to(dev), [u.to(dev) for u in unl]

    def batch():
        return (to_image_list(list(imgs), cfg.DATALOADER.SIZE_DIVISIBILITY), targets,
                [to_image_list(list(u), cfg.DATALOADER.SIZE_DIVISIBILITY) for u in unl])
    return cfg, trainer, batch


def test_one_mean_teacher_iteration(rx_weights):
    cfg, trainer, batch = _trainer(rx_weights)
    fs, ft = trainer.flat_s, trainer.flat_t
    before_s, before_t = fs.data.clone(), ft.data.clone()
    losses = trainer.train_step(cfg.MT.START_MT + 400, *batch())
    torch.cuda.synchronize()
    assert set(losses) == LOSS_KEYS, sorted(losses)
    assert all(torch.isfinite(v).item() for v in losses.values()), {k: float(v) for k, v in losses.items()}
    print("resnext step losses:", {k: round(float(v.detach()), 5) for k, v in losses.items()})
    params = dict(trainer.student.named_parameters())
    n_conv2 = 0
    for n, (o, k) in fs.index.items():
        if not n.endswith(".conv2.weight") or ".body." not in n:
            continue
        if ".layer1." in n:   # the frozen stage: no gradient slot, no update
            assert not params[n].requires_grad and params[n].grad is None and o >= fs.n_trainable, n
            assert torch.equal(fs.data[o:o + k], before_s[o:o + k]), n
            continue
        n_conv2 += 1
        assert n in fs.touched or fs.grad[o:o + k].abs().max().item() > 0, n
        assert fs.grad[o:o + k].abs().max().item() > 0, n
        assert torch.isfinite(fs.grad[o:o + k]).all().item(), n
        assert (fs.data[o:o + k] != before_s[o:o + k]).any().item(), "SGD did not move " + n
        ot, kt = ft.index[n]
        assert (ft.data[ot:ot + kt] != before_t[ot:ot + kt]).any().item(), "EMA did not move " + n
    assert n_conv2 == 13
    losses = trainer.train_step(cfg.MT.START_MT + 401, *batch())
    torch.cuda.synchronize()
    assert set(losses) == LOSS_KEYS and all(torch.isfinite(v).item() for v in losses.values())


def test_not_offered_with_bf16_storage(rx_weights):
    from maskrcnn_benchmark import _hip as H
    bb = _backbone(rx_weights)
    prev = H.get_conv_precision()
    H.set_conv_precision(1)
    H.set_bf16_storage(True)
    try:
        with pytest.raises(NotImplementedError, match="bf16 activation storage"):
            with torch.no_grad():
                bb(_images())
    finally:
        H.set_bf16_storage(False)
        H.set_conv_precision(prev)
