"""GeneralizedRCNN.forward_teacher(images, targets): the reference's ground-truth branch (generalized_rcnn.py:133-139) on the
160 x 160 synthetic batch and weights of tests/test_model_gpu.py, with polygon targets.  The integral foreground mask is compared
with the oracle's rleFrPoly restatement with equality; the lists by the properties the matcher guarantees."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZE = 160


@pytest.fixture(scope="module")
def models(synth, weights):
    from maskrcnn_benchmark import _hip
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    _hip.lib()
    cfg = make_default_cfg()
    student = build_detection_model(cfg, is_student=True).cuda()
    teacher = build_detection_model(cfg, is_teacher=True).cuda()
    student.load_state_dict(weights, strict=False)
    teacher.load_state_dict(weights, strict=False)
    student.train()
    teacher.eval()
    return cfg, student, teacher


@pytest.fixture(scope="module")
def batch(synth):
    imgs, tgs = synth.make_labeled(2, SIZE, 4, seed=1234)
    return imgs, tgs


def _targets(tgs, dev="cuda", masks=True):
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    out = []
    for t in tgs:
        b = BoxList(t["boxes"].to(dev), t["size"], "xyxy")
        b.add_field("labels", t["labels"].to(dev))
        if masks:
            b.add_field("masks", SegmentationMask([[p for p in inst] for inst in t["polys"]], t["size"], mode="poly"))
        out.append(b)
    return out


def _views(imgs, k=2):
    """k augmented views of the labelled batch (fresh lists: extract_aug_feat mirrors them in place)"""
    from maskrcnn_benchmark.structures.image_list import to_image_list
    return [to_image_list(list(imgs.cuda()), 32) for _ in range(k)]


def _run(teacher, imgs, tgs, seed=5, **kw):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    teacher.set_rng(g)
    try:
        with torch.no_grad():
            return teacher.forward_teacher(_views(imgs), _targets(tgs, **kw))
    finally:
        teacher.set_rng(None)


def _iou(a, b):
    """(n, 4) x (m, 4) -> (n, m), the `+ 1` pixel convention of structures/boxlist_ops.py"""
    area = lambda x: (x[:, 2] - x[:, 0] + 1) * (x[:, 3] - x[:, 1] + 1)   # noqa: E731
    lt, rb = torch.max(a[:, None, :2], b[None, :, :2]), torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area(a)[:, None] + area(b)[None, :] - inter)


@pytest.fixture(scope="module")
def out_targets(models, batch):
    _, _, teacher = models
    teacher.taps = {}
    try:
        out = _run(teacher, *batch)
        props = teacher.taps["teacher_proposals"]
    finally:
        teacher.taps = None
    return out, props


def test_seg_mask_is_the_oracle_sum(out_targets, batch):
    from oracle import native
    out, _ = out_targets
    _, tgs = batch
    assert len(out["seg_mask"]) == len(tgs) == 2
    for t, got in zip(tgs, out["seg_mask"]):
        w, h = t["size"]
        want = np.zeros((h, w), np.int32)
        for inst in t["polys"]:
            want += native.poly_mask([np.asarray(p, dtype=np.float32) for p in inst], h, w)
        assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (h, w)
        assert np.array_equal(got.cpu().numpy(), want)
        assert want.sum() > 0


def test_positive_rows_lie_on_ground_truth_of_their_label(models, out_targets, batch):
    cfg, _, _ = models
    out, _ = out_targets
    thr = cfg.MODEL.ROI_HEADS.FG_IOU_THRESHOLD
    n_pos = 0
    for res, t in zip(out["result_t"], batch[1]):
        lab = res.get_field("labels").cpu()
        pos = lab > 0
        n_pos += int(pos.sum())
        iou = _iou(res.bbox.cpu()[pos], t["boxes"].float())
        same = lab[pos][:, None] == t["labels"][None, :].to(lab.dtype)
        best = torch.where(same, iou, torch.zeros_like(iou)).max(1)[0]
        # (the matcher compares fp32 IoUs computed on the device: 1e-6 is that arithmetic's rounding, not slack)
        assert bool((best >= thr - 1e-6).all()), float(best.min())
        assert set(lab.unique().tolist()) <= set([0] + t["labels"].tolist())
    assert n_pos > 0


def test_class_logits_one_entry_per_view(out_targets):
    out, _ = out_targets
    rows = sum(len(r) for r in out["result_t"])
    assert len(out["class_logit_t"]) == 4                          # two augmented views, each plain and mirrored
    for cl in out["class_logit_t"]:
        assert cl.shape[0] == rows and bool(torch.isfinite(cl).all())
    assert len(out["embedding"]) == 4
    assert out["ffi_boxes"] is None


def test_ground_truth_boxes_among_the_proposals_of_a_training_selector(models, batch):
    """rpn/inference.py:169: the selector appends the ground truth `if self.training and targets is not None`, here as there, so
    an RPN in training mode proposes every annotated box; a teacher in eval mode (engine/MTtrainer.py) proposes what its RPN finds
    -- both are checked"""
    _, _, teacher = models
    imgs, tgs = batch
    seen = {}
    for mode in (True, False):
        teacher.rpn.train(mode)
        teacher.taps = {}
        try:
            _run(teacher, imgs, tgs)
            seen[mode] = teacher.taps["teacher_proposals"]
        finally:
            teacher.taps = None
            teacher.rpn.eval()
    for props, t in zip(seen[True], tgs):
        d = (props.bbox.cpu()[:, None, :] - t["boxes"].float()[None, :, :]).abs().amax(2)
        assert bool((d.min(0)[0] == 0).all())
    for a, b in zip(seen[True], seen[False]):
        assert len(a) > 0 and len(b) > 0


def test_student_losses_and_gradients(models, out_targets, batch):
    from maskrcnn_benchmark.structures.image_list import to_image_list
    _, student, _ = models
    out, _ = out_targets
    imgs, _ = batch
    for p in student.parameters():
        p.grad = None
    losses = student.forward_student([to_image_list(list(imgs.cuda()), 32)], out)
    assert set(losses) == {"mt_fg_loss", "mt_classifier"}
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    assert float(losses["mt_fg_loss"].detach()) > 0
    sum(v.sum() for v in losses.values()).backward()
    named = dict(student.named_parameters())
    for k in ("hint_adaptor.adapter_3.weight", "box_heads.box.predictor.cls_score.weight", "backbone.body.layer2.0.conv1.weight"):
        g = named[k].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    for p in student.parameters():
        p.grad = None


def test_a_target_without_masks_raises(models, batch):
    _, _, teacher = models
    with pytest.raises(RuntimeError, match="masks"):
        _run(teacher, *batch, masks=False)


def test_targets_of_differing_sizes_raise(models, batch):
    _, _, teacher = models
    imgs, tgs = batch
    other = dict(tgs[1], size=(SIZE, SIZE - 32))
    with pytest.raises(RuntimeError, match="differing sizes"):
        _run(teacher, imgs, [tgs[0], other])


def test_without_targets_nothing_changed(models, batch, synth):
    """forward_teacher(images) before and after a call with targets, same seed: the same dict (discrete outcomes equal, values to
    the run-to-run rounding of the convolutions' float atomics, as tests/test_model_gpu.py compares two teacher passes)"""
    from maskrcnn_benchmark.structures.image_list import to_image_list
    _, _, teacher = models
    unl = synth.make_unlabeled(2, SIZE, 3, seed=4321)

    def plain():
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        teacher.set_rng(g)
        try:
            with torch.no_grad():
                return teacher.forward_teacher([to_image_list(list(u.cuda()), 32) for u in unl[:2]])
        finally:
            teacher.set_rng(None)

    a = plain()
    _run(teacher, *batch)
    b = plain()
    assert set(a) == set(b) == {"result_t", "class_logit_t", "embedding", "seg_mask", "ffi_boxes"}
    for x, y in zip(a["result_t"], b["result_t"]):
        assert len(x) == len(y) and (x.bbox - y.bbox).abs().max().item() < 1e-3
        assert torch.equal(x.get_field("labels"), y.get_field("labels"))
    for x, y in zip(a["class_logit_t"], b["class_logit_t"]):
        assert (x - y).abs().max().item() < 1e-5 * max(1.0, x.abs().max().item())
    for ex, ey in zip(a["embedding"], b["embedding"]):
        for x, y in zip(ex, ey):
            assert (x - y).abs().max().item() < 1e-5 * max(1.0, x.abs().max().item())
    for x, y in zip(a["seg_mask"], b["seg_mask"]):
        assert x.dtype == y.dtype and (x != y).float().mean().item() < 1e-4
    assert sum(int(m.sum()) for m in a["seg_mask"]) > 0
