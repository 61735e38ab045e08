"""Bitmap ground truth (BinaryMaskList) through every place a polygon target goes, on the 160 x 160 synthetic batch and weights of
tests/test_model_gpu.py: the mask head's targets for both heads (M = 28, the CSPN head's 25), a supervised step, forward_teacher
with targets, the input transforms, and the PAP evaluator on the device.  Mask targets are compared with the host restatement of
tests/bitmask_formulation.py by equality; the polygon path is shown undisturbed."""
import numpy as np
import pytest
import torch

import bitmask_formulation as bf
import cspn_formulation as cf
from oracle import model as om

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


def _polygon_masks(t):
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    return SegmentationMask([[p for p in inst] for inst in t["polys"]], t["size"], mode="poly")


@pytest.fixture(scope="module")
def bitmaps(batch):
    """the batch's instances as bytes on the host, uint8 (G, h, w) per image: the polygons rasterised once by the existing kernel"""
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    out = [BinaryMaskList.from_polygons(_polygon_masks(t)).get_mask_tensor().cpu() for t in batch[1]]
    assert all(int(m.sum()) > 0 for m in out)
    return out


def _targets(tgs, masks):
    """masks: "poly", or the per-image bytes for BinaryMaskList fields"""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    out = []
    for i, t in enumerate(tgs):
        b = BoxList(t["boxes"].cuda(), t["size"], "xyxy")
        b.add_field("labels", t["labels"].cuda())
        b.add_field("masks", _polygon_masks(t) if isinstance(masks, str) else BinaryMaskList(masks[i], t["size"]))
        out.append(b)
    return out


def _proposals(boxes, tgs):
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    return [BoxList(b.cuda(), t["size"], "xyxy") for b, t in zip(boxes, tgs)]


def _matched(boxes, t):
    """the matcher's (instance or -1 for a non-positive, label) per box, on the host"""
    m = om.matcher(om.box_iou(om.Boxes(t["boxes"], t["size"]), om.Boxes(boxes, t["size"])), 0.5, 0.5, False)
    lab = t["labels"][m.clamp(min=0)].to(torch.int64)
    lab[m < 0] = 0
    return torch.where(lab > 0, m, torch.full_like(m, -1)), lab


def _want(boxes, tgs, bitmaps, M):
    inst = [_matched(b, t) for b, t in zip(boxes, tgs)]
    return (torch.cat([l for _, l in inst]), torch.cat([bf.targets(m, r, b, M) for (r, _), b, m in zip(inst, boxes, bitmaps)]))


# ------------------------------------------------------------------------------------------ 1. the mask head's targets
@pytest.mark.parametrize("M", [28, 25], ids=["mask-rcnn-28", "cspn-25"])
def test_prepare_targets_for_both_heads(batch, bitmaps, M, monkeypatch):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.mask_head import MaskRCNNLossComputation
    _, tgs = batch
    boxes = cf.fixture_boxes(tgs, SIZE)
    le = MaskRCNNLossComputation(Matcher(0.5, 0.5, allow_low_quality_matches=False), M)
    calls = []
    real = H.mask_words_targets
    monkeypatch.setattr(H, "mask_words_targets", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    lab_p, mt_p = le.prepare_targets(_proposals(boxes, tgs), _targets(tgs, "poly"))
    assert calls == []                                                     # polygon targets take the launches they took
    lab_b, mt_b = le.prepare_targets(_proposals(boxes, tgs), _targets(tgs, bitmaps))
    assert len(calls) == len(tgs)                                          # one launch per image
    lab_p2, mt_p2 = le.prepare_targets(_proposals(boxes, tgs), _targets(tgs, "poly"))
    assert torch.equal(lab_p, lab_p2) and torch.equal(mt_p, mt_p2) and len(calls) == len(tgs)   # the polygon path: undisturbed
    want_lab, want = _want(boxes, tgs, bitmaps, M)
    assert torch.equal(lab_b, lab_p) and torch.equal(lab_b.cpu(), want_lab)
    assert mt_b.shape == mt_p.shape == (sum(len(b) for b in boxes), M, M)
    bad = (mt_b.cpu() != want).flatten(1).any(1).nonzero().reshape(-1).tolist()
    print("M %d: %d ROIs, %d positives, %d bits set, ROIs that differ: %s" % (M, len(want), int((want_lab > 0).sum()), int(want.sum()), bad))
    assert torch.equal(mt_b.cpu(), want)
    assert int(want[want_lab == 0].abs().sum()) == 0 and 0 < int((want_lab > 0).sum()) < len(want_lab)
    # the matcher's other form (unequal thresholds: the per-image path) builds the same index for every box above both
    pos = want_lab > 0
    le2 = MaskRCNNLossComputation(Matcher(0.5, 0.4, allow_low_quality_matches=False), M)
    lab_c, mt_c = le2.prepare_targets(_proposals(boxes, tgs), _targets(tgs, bitmaps))
    assert torch.equal(lab_c.cpu()[pos], want_lab[pos]) and torch.equal(mt_c.cpu()[pos], want[pos])


# ------------------------------------------------------------------------------------------ 2. a supervised step
class _Recorder(object):
    def __init__(self, le):
        self.le, self.calls = le, []

    def __call__(self, proposals, logits, targets):
        loss = self.le(proposals, logits, targets)
        labels, _ = self.le.prepare_targets(proposals, targets)
        self.calls.append(([p.bbox.detach().clone() for p in proposals], labels.clone(), logits.detach().clone(),
                           self.le.last_targets.clone(), loss.detach().clone()))
        return loss


def test_supervised_step_with_bitmap_targets(models, batch, bitmaps, monkeypatch):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.modeling.detector import generalized_rcnn as gr
    from maskrcnn_benchmark.structures.image_list import to_image_list
    _, student, _ = models
    imgs, tgs = batch
    il = to_image_list(list(imgs.cuda()), 32)
    monkeypatch.setattr(gr, "_NO_READBACK", True)
    targets = _targets(tgs, bitmaps)
    head = student.mask_heads.mask
    rec = _Recorder(head.loss_evaluator)
    monkeypatch.setattr(head, "loss_evaluator", rec)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    student.set_rng(g)
    reads = []
    tolist, item = torch.Tensor.tolist, torch.Tensor.item

    def spy_tolist(self, _f=tolist):
        if self.is_cuda:
            reads.append("tolist")
        return _f(self)

    def spy_item(self, _f=item):
        if self.is_cuda:
            reads.append("item")
        return _f(self)

    for p in student.parameters():
        p.grad = None
    torch.Tensor.tolist, torch.Tensor.item = spy_tolist, spy_item
    try:
        out = student(il, targets)
        n_reads = list(reads)
        torch.Tensor.tolist, torch.Tensor.item = tolist, item
        sum(out.values()).backward()
        torch.cuda.synchronize()
    finally:
        torch.Tensor.tolist, torch.Tensor.item = tolist, item
        student.set_rng(None)
    assert n_reads == [], n_reads            # as with polygon targets (tests/test_model_gpu.py): no device tensor read by the host
    assert "loss_seg" in out and all(bool(torch.isfinite(v).all()) for v in out.values())
    assert len(rec.calls) >= 1
    M = head.loss_evaluator.le.discretization_size
    for boxes, labels, logits, last, loss in rec.calls:
        boxes = [b.cpu() for b in boxes]
        want_lab, want = _want(boxes, tgs, bitmaps, M)
        assert torch.equal(labels.cpu(), want_lab) and int((want_lab > 0).sum()) > 0
        assert torch.equal(last.cpu(), want)
        again, _ = H.mask_bce(logits, labels, want.cuda())
        # the same kernel on the same inputs; its sum is made with float atomics, so the order of P * M * M fp32 terms may
        # differ from run to run: a few ulp of the sum
        assert float(again) == pytest.approx(float(loss), rel=1e-5)
        assert float(loss) > 0
    named = dict(student.named_parameters())
    grads = [v.grad for k, v in named.items() if k.startswith("mask_heads.mask.") and v.grad is not None]
    assert grads and all(bool(torch.isfinite(x).all()) for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
    assert float(named["mask_heads.mask.predictor.mask_fcn_logits.weight"].grad.abs().max()) > 0
    for p in student.parameters():
        p.grad = None


# ------------------------------------------------------------------------------------------ 3. forward_teacher with targets
def test_forward_teacher_with_bitmap_targets(models, batch):
    from maskrcnn_benchmark.structures.image_list import to_image_list
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    _, _, teacher = models
    imgs, tgs = batch

    def run(targets):
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        teacher.set_rng(g)
        try:
            with torch.no_grad():
                return teacher.forward_teacher([to_image_list(list(imgs.cuda()), 32) for _ in range(2)], targets)
        finally:
            teacher.set_rng(None)

    poly = run(_targets(tgs, "poly"))
    targets = _targets(tgs, "poly")
    for t in targets:
        t.add_field("masks", BinaryMaskList.from_polygons(t.get_field("masks")))
    got = run(targets)
    assert len(got["seg_mask"]) == len(poly["seg_mask"]) == 2
    for a, b in zip(got["seg_mask"], poly["seg_mask"]):
        assert a.dtype == torch.int32 and torch.equal(a, b) and int(a.sum()) > 0
    for x, y in zip(got["result_t"], poly["result_t"]):
        assert len(x) == len(y) and torch.equal(x.get_field("labels"), y.get_field("labels"))
    targets[1] = targets[1].resize((SIZE, SIZE - 32))
    with pytest.raises(RuntimeError, match="differing sizes"):
        run(targets)


# ------------------------------------------------------------------------------------------ 4. the input transforms
def test_transform_pipeline_on_a_bitmap_field(bitmaps, batch):
    from maskrcnn_benchmark.data.transforms import transforms as T
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    t = batch[1][0]
    m = bitmaps[0][:, :120]                                                # a 160 x 120 (w x h) image's instances
    image = T.DeviceImage(torch.randint(0, 256, (120, 160, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)))
    target = BoxList(t["boxes"].cuda(), (160, 120), "xyxy")
    target.add_field("labels", t["labels"].cuda())
    target.add_field("masks", BinaryMaskList(m.contiguous(), (160, 120)))
    pipe = T.Compose([T.Resize(96, 200), T.RandomHorizontalFlip(1.0)])
    image, out = pipe(image, target)
    assert tuple(image.size) == (128, 96) and tuple(out.size) == (128, 96) and image.flip
    f = out.get_field("masks")
    assert isinstance(f, BinaryMaskList) and tuple(f.size) == (128, 96) and len(f) == len(m)
    want = bf.resample(m, (0, 0, 160, 120), 96, 128).flip(2)
    assert torch.equal(f.get_mask_tensor().cpu(), want) and int(want.sum()) > 0
    assert torch.equal(f.mask_words()[0].cpu(), bf.pack(want)[0]) and torch.equal(f.mask_words()[1].cpu(), bf.pack(want)[1])


# ------------------------------------------------------------------------------------------ 5. the evaluator
def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and not isinstance(b, np.ndarray):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.ndarray, float, np.floating)) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f" and b.dtype.kind == "f")
    return a == b


def test_pap_evaluator_on_the_device(batch, bitmaps):
    from maskrcnn_benchmark.data.datasets.evaluation.pap import pap_eval
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
    _, tgs = batch
    ids = [{"file_name": "w%d" % i, "location": (0, 16 * i), "id": i + 1} for i in range(len(tgs))]

    def dataset(bitmap):
        class DS(object):
            maxWS = SIZE
            id_to_img_map = dict(enumerate(ids))
            contiguous_category_id_to_json_id = {1: 1, 2: 2}

            def get_ground_truth(self, original_id):
                t = tgs[original_id["id"] - 1]
                b = BoxList(t["boxes"], t["size"], "xyxy")
                b.add_field("labels", t["labels"])
                sm = _polygon_masks(t)
                b.add_field("masks", BinaryMaskList.from_polygons(sm) if bitmap else sm)
                return b
        return DS()

    preds = {}
    for i, (t, m) in enumerate(zip(tgs, bitmaps)):
        d = torch.stack([m[0], torch.roll(m[1], (3, -2), (0, 1)), m[2] | m[3], torch.roll(m[3], 40, 1)])   # a hit, near hits, a miss
        p = BoxList(torch.zeros((4, 4)), (SIZE, SIZE), "xyxy")
        p.add_field("mask", d[:, None].cuda())
        p.add_field("scores", torch.tensor([0.9, 0.8, 0.7, 0.6], dtype=torch.float64))
        p.add_field("labels", torch.tensor([int(t["labels"][0]), int(t["labels"][1]), int(t["labels"][2]), int(t["labels"][3])]))
        preds[i] = p
    runs = []
    for bitmap in (False, True):
        gts, dts = pap_eval.prepare_for_pap_segmentation(preds, dataset(bitmap), on_device=True)
        assert len(gts) == 8 and len(dts) == 8 and all(isinstance(g["segmentation"]["counts"], str) for g in gts)
        ev = pap_eval.evaluate_predictions_on_pap(gts, dts, on_device=True)
        runs.append((gts, ev.evalImgs, ev.stats))
    assert runs[0][0] == runs[1][0]
    assert _same(runs[0][1], runs[1][1]) and _same(runs[0][2], runs[1][2])
    assert any(e is not None and e["F1"] > 0 for e in runs[1][1])
