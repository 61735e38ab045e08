"""IR-Net's mask refinement with CIAM's normalisations switched on (MODEL.RELATION_MASK.NORM 1, and NORM 2 + PRE_NORM): the detector
builds with the state dict of the default build (the switches add no parameter), `MaskRelationRefineNet.forward_batch` agrees with the
same module at NORM -1 whose CIAM call is replaced by the fp64 formulation of the variant (tests/ciam_formulations.py, pinned to the
reference by tests/test_ciam_formulation.py), and a mean-teacher step runs, bit-identically in deterministic mode."""
import json
import os
import sys

import pytest
import torch

from conftest import GOLD, ROOT
import ciam_formulations as cf

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

CASES = [(1, False), (2, True)]
_DETECTORS = {}


def _detector(synth, norm, pre):
    """a student with IR-Net on and the synthetic weights of tests/test_irnet_gpu.py, one per combination and module run"""
    if (norm, pre) not in _DETECTORS:
        from maskrcnn_benchmark.config import make_default_cfg
        from maskrcnn_benchmark.modeling.detector import build_detection_model
        cfg = make_default_cfg()
        cfg.merge_from_list(["MODEL.RELATION_NMS.USE_RELATION_NMS", True, "MODEL.RELATION_MASK.USE_RELATION", True,
                             "MODEL.RELATION_MASK.NORM", norm, "MODEL.RELATION_MASK.PRE_NORM", pre])
        shapes = json.load(open(os.path.join(GOLD, "state_shapes_irnet.json")))["shapes"]
        m = build_detection_model(cfg, is_student=True).cuda()
        missing, unexpected = m.load_state_dict(synth.make_weights(shapes, seed=0), strict=False)
        assert all("cell_anchors" in k for k in list(missing) + list(unexpected)), (missing, unexpected)
        m.train()
        with torch.no_grad():
            m.mask_heads.mask.mask_relation_module.relation_module.gamma.fill_(cf.GAMMA)
        _DETECTORS[(norm, pre)] = m
    return _DETECTORS[(norm, pre)]


@pytest.mark.parametrize("norm,pre", CASES)
def test_state_dict_is_the_default_builds(synth, norm, pre):
    a, b = _detector(synth, -1, False).state_dict(), _detector(synth, norm, pre).state_dict()
    assert list(a) == list(b)
    assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()}
    rm = _detector(synth, norm, pre).mask_heads.mask.mask_relation_module.relation_module
    assert (rm.norm, rm.prenorm) == (norm, pre)


def _inputs():
    """a two-image batch of ROI features, first mask logits and ranked proposals on 160 x 160 images"""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    g = torch.Generator().manual_seed(77)
    sizes = [12, 9]
    P = sum(sizes)
    feat = torch.relu(torch.randn(P, 256, 14, 14, generator=g)).cuda().contiguous(memory_format=torch.channels_last)
    logits = torch.randn(P, 3, 28, 28, generator=g).cuda()
    props = []
    for n in sizes:
        xy = torch.rand(n, 2, generator=g) * 100
        wh = torch.rand(n, 2, generator=g) * 50 + 8
        b = BoxList(torch.cat((xy, xy + wh), 1).cuda(), (160, 160), mode="xyxy")
        b.add_field("labels", torch.randint(1, 3, (n,), generator=g).cuda())
        b.add_field("objectness", torch.rand(n, generator=g).cuda())
        props.append(b)
    gout = torch.randn(P, 3, 28, 28, generator=g).cuda()
    return feat, logits, props, gout


def _second_logits(mrm, feat, logits, props, gout):
    for p in mrm.parameters():
        p.grad = None
    rel, out = mrm.forward_batch(feat, logits, props)
    (rel * gout).sum().backward()
    return rel.detach(), mrm.appearance_feature_extractor.conv5_mask.weight.grad.clone(), out


@pytest.mark.parametrize("norm,pre", CASES)
def test_forward_batch_vs_fp64_ciam(synth, norm, pre):
    feat, logits, props, gout = _inputs()
    got = _second_logits(_detector(synth, norm, pre).mask_heads.mask.mask_relation_module, feat, logits, props, gout)

    ref_mrm = _detector(synth, -1, False).mask_heads.mask.mask_relation_module
    seen = {}

    def fp64_ciam(x, group):
        sizes = torch.unique_consecutive(group.cpu(), return_counts=True)[1].tolist()
        seen["sizes"] = sizes
        out = cf.ciam(ref_mrm.relation_module.gamma.double().cpu(), x.double().cpu(), sizes, norm, pre)
        return out.to(x.device, x.dtype)

    ref_mrm.relation_module.forward = fp64_ciam
    try:
        ref = _second_logits(ref_mrm, feat, logits, props, gout)
    finally:
        del ref_mrm.relation_module.forward
    assert sum(seen["sizes"]) == feat.shape[0] and max(seen["sizes"]) > 1      # the attention had something to mix
    for a, b in zip(got[2], ref[2]):
        assert torch.equal(a.bbox, b.bbox)
    for what, a, b in (("second logits", got[0], ref[0]), ("d conv5_mask.weight", got[1], ref[1])):
        dev = cf.rel_dev(a, b)
        print("IR-Net NORM %d PRE_NORM %s, %s: %.2e of the maximum (bar 1e-4)" % (norm, pre, what, dev))
        assert dev <= 1e-4, (what, dev)
    # and the variant is not the default function: the default module's own kernels give other logits
    base = _second_logits(ref_mrm, feat, logits, props, gout)
    assert cf.rel_dev(base[0], ref[0]) > 1e-5


def _mt_step(norm, pre):
    """bench.py::build's IR-Net trainer at 160 x 160 from seed 0 with the two keys merged in; one mean-teacher step -> losses"""
    import bench
    import maskrcnn_benchmark.config as C
    keep = C.make_default_cfg
    try:
        def with_keys():
            cfg = keep()
            cfg.merge_from_list(["MODEL.RELATION_MASK.NORM", norm, "MODEL.RELATION_MASK.PRE_NORM", pre])
            return cfg
        C.make_default_cfg = with_keys
        torch.manual_seed(0)
        cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, irnet=True, crop=160, n_inst=4, base_lr=0.005)
    finally:
        C.make_default_cfg = keep
    for m in (trainer.student, trainer.teacher):
        rm = m.mask_heads.mask.mask_relation_module.relation_module
        assert (rm.norm, rm.prenorm) == (norm, pre)
        with torch.no_grad():
            rm.gamma.fill_(cf.GAMMA)          # (zero at initialisation: the attention would not reach the logits)
    trainer.seed_rng(0)
    il, tg, ul = batch()
    losses = trainer.train_step(cfg.MT.START_MT + 400, il, tg, ul)
    torch.cuda.synchronize()
    assert "mt_fg_loss" in losses and "loss_seg" in losses, sorted(losses)
    return {k: v.detach().clone() for k, v in losses.items()}


@pytest.mark.parametrize("norm,pre", CASES)
def test_mean_teacher_step_is_finite(norm, pre):
    losses = _mt_step(norm, pre)
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses


@pytest.mark.parametrize("norm,pre", CASES)
def test_mean_teacher_step_deterministic_mode(norm, pre):
    """the same step twice from the same seed in deterministic mode: every loss bit-identical"""
    from maskrcnn_benchmark import _hip as H
    try:
        H.set_deterministic(True)
        a = _mt_step(norm, pre)
        b = _mt_step(norm, pre)
    finally:
        H.set_deterministic(False)
    assert set(a) == set(b)
    for k in sorted(a):
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), (k, a[k], b[k])
