"""TEST.MASK_NMS behind the mask head ("Mask NMS at inference") on the small synthetic setup of
tests/test_model_gpu.py: 160 x 160 images, n = 2, the synthetic weights, default arithmetic.  The expected rows are always the plain
formulation (tests/mask_nms_formulation.py) applied to what `Masker.forward_single_image` pastes from the M x M probabilities, so
every comparison is equality."""
import numpy as np
import pytest
import torch

import mask_nms_formulation as F
from test_model_gpu import SIZE

pytestmark = pytest.mark.gpu

ON = {"ENABLED": True, "THRESH": 0.3, "MEASURE": "iomin", "CLASS_AGNOSTIC": True}


def _cfg(keys=None, paste=False):
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    for k, v in (keys or {}).items():
        cfg.TEST.MASK_NMS[k] = v
    cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS = paste
    return cfg


def _model(cfg, weights):
    from maskrcnn_benchmark import _hip
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    _hip.lib()
    m = build_detection_model(cfg).cuda()
    m.load_state_dict(weights, strict=False)
    m.eval()
    return m


@pytest.fixture(scope="module")
def plain(weights):
    """the untouched default config"""
    from maskrcnn_benchmark.config import make_default_cfg
    return _model(make_default_cfg(), weights)


@pytest.fixture(scope="module")
def on(weights):
    return _model(_cfg(ON), weights)


@pytest.fixture(scope="module")
def images(synth):
    from maskrcnn_benchmark.structures.image_list import to_image_list
    imgs, _ = synth.make_labeled(2, SIZE, 4, seed=1234)
    return to_image_list(list(imgs.cuda()), 32)


@pytest.fixture(scope="module")
def plain_out(plain, images):
    """the switch-off detections, computed once and shared"""
    with torch.no_grad():
        out = plain(images)
    torch.cuda.synchronize()
    return out


def _pasted(b, threshold=0.5):
    """the (D, 1, h, w) uint8 stack that Masker.forward_single_image pastes from a list's M x M probabilities"""
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.mask_head import Masker
    return Masker(threshold, 1).forward_single_image(b.get_field("mask"), b)


def _expected_rows(b, keys):
    keep = F.reference(_pasted(b)[:, 0].cpu().numpy() != 0, b.get_field("scores").cpu().numpy(), b.get_field("labels").cpu().numpy(),
                       keys["THRESH"], keys["MEASURE"], keys["CLASS_AGNOSTIC"])
    return torch.from_numpy(np.nonzero(keep)[0]).cuda()


def _assert_selection(out, full, rows, fields=("scores", "labels", "mask")):
    assert len(out) == len(rows) and out.size == full.size and set(out.fields()) == set(full.fields())
    assert torch.equal(out.bbox, full.bbox[rows])
    for f in fields:
        assert torch.equal(out.get_field(f), full.get_field(f)[rows]), f


def _constructed(seed):
    """two images of detections with known duplicates -> (logits (sum D, 3, M, M), the BoxLists with scores and labels)"""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    M = 28
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(M, dtype=torch.float32), torch.arange(M, dtype=torch.float32), indexing="ij")

    def blob(cy, cx, r):   # positive inside a disc, with some seeded texture
        return 3.0 - 6.0 * (((yy - cy) ** 2 + (xx - cx) ** 2) / (r * r)) + 0.2 * torch.randn((M, M), generator=g)

    logits, lists = [], []
    for img in range(2):
        a, b = blob(13, 14, 9 + img), blob(15, 12, 7)
        box_a = torch.tensor([20.0 + 5 * img, 24.0, 84.0 + 5 * img, 90.0])
        box_b = torch.tensor([100.0, 98.0, 150.0, 152.0])
        shift = torch.tensor([3.0, 2.0, 3.0, 2.0])
        #        box            mask  label  score
        rows = [(box_a,         a,    1,     0.90),
                (box_b,         b,    2,     0.85),
                (box_a,         a,    1,     0.80),      # an exact duplicate of row 0
                (box_a + shift, a,    1,     0.75),      # the same mask logits in a shifted box
                (box_a,         a,    2,     0.70),      # a twin of row 0 in another class
                (box_b - shift, b,    2,     0.65),      # the same again for row 1
                (box_b,         b,    2,     0.85)]      # row 1 once more with row 1's score: the lower row wins
        bl = BoxList(torch.stack([r[0] for r in rows]).cuda(), (SIZE, SIZE), "xyxy")
        bl.add_field("labels", torch.tensor([r[2] for r in rows], dtype=torch.int64).cuda())
        bl.add_field("scores", torch.tensor([r[3] for r in rows], dtype=torch.float32).cuda())
        x = torch.randn((len(rows), 3, M, M), generator=g)
        for d, r in enumerate(rows):
            x[d, r[2]] = r[1]
        logits.append(x)
        lists.append(bl)
    return torch.cat(logits).cuda(), lists


@pytest.mark.parametrize("keys", [{"ENABLED": True, "THRESH": 0.5, "MEASURE": "iou", "CLASS_AGNOSTIC": False}, ON], ids=["default", "iomin-agnostic"])
def test_constructed_duplicates(keys):
    from maskrcnn_benchmark.modeling.roi_heads.mask_head import mask_head as mh
    x, lists = _constructed(seed=0)
    off = mh.make_roi_mask_post_processor(_cfg())(x, lists)
    out = mh.make_roi_mask_post_processor(_cfg(keys))(x, lists)
    pasted_out = mh.make_roi_mask_post_processor(_cfg(keys, paste=True))(x, lists)
    for o, po, full in zip(out, pasted_out, off):
        assert len(full) == 7 and tuple(full.get_field("mask").shape) == (7, 1, 28, 28)
        rows = _expected_rows(full, keys)
        _assert_selection(o, full, rows)
        # what the cases are there for: the duplicates go, in either mode; the other class's twin goes only when class-agnostic
        expect = [0, 1] if keys["CLASS_AGNOSTIC"] else [0, 1, 4]
        assert rows.tolist() == expect, rows.tolist()
        # POSTPROCESS_MASKS: the pasted stack has exactly the kept rows
        _assert_selection(po, full, rows, fields=("scores", "labels"))
        stack = po.get_field("mask")
        assert stack.dtype == torch.uint8 and tuple(stack.shape) == (len(rows), 1, SIZE, SIZE)
        assert torch.equal(stack, _pasted(full)[rows])
    # a list without detections comes back as it is, without a launch
    empty = lists[0][torch.zeros((0,), dtype=torch.int64, device="cuda")]
    res = mh.make_roi_mask_post_processor(_cfg(keys))(x[:0], [empty])
    assert len(res[0]) == 0 and tuple(res[0].get_field("mask").shape) == (0, 1, 28, 28)


def test_whole_model_keeps_the_formulations_selection(on, plain_out, images):
    assert on.mask_heads.mask.post_processor.mask_nms is not None
    with torch.no_grad():
        out = on(images)
    torch.cuda.synchronize()
    for o, full in zip(out, plain_out):
        rows = _expected_rows(full, ON)
        print("mask NMS kept %d of %d detections" % (len(rows), len(full)))
        assert 0 < len(rows) < len(full)      # (the formulation drops some of these detections and keeps some)
        _assert_selection(o, full, rows)


def test_switch_off_is_the_default_model_and_never_calls_the_kernel(weights, plain_out, images, monkeypatch):
    from maskrcnn_benchmark import _hip as H

    def refuse(*a, **k):
        raise AssertionError("mmt_mask_nms was called")
    monkeypatch.setattr(H, "mask_nms", refuse)
    off = _model(_cfg(dict(ON, ENABLED=False)), weights)      # every other key set: only ENABLED switches
    assert off.mask_heads.mask.post_processor.mask_nms is None
    with torch.no_grad():
        out = off(images)
        tta = off.forward_tta([images], flip=True)
    torch.cuda.synchronize()
    assert all(t.has_field("mask") for t in tta)
    for o, p in zip(out, plain_out):
        assert len(o) == len(p) and set(o.fields()) == set(p.fields())
        assert torch.equal(o.bbox, p.bbox)
        for f in p.fields():
            assert torch.equal(o.get_field(f), p.get_field(f)), f


def test_teacher_paths_never_call_it(on, plain_out, images, monkeypatch):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    calls = []
    real = H.mask_nms
    monkeypatch.setattr(H, "mask_nms", lambda *a, **k: calls.append(1) or real(*a, **k))
    mask = on.mask_heads.mask

    def boxes(count_dev=False):
        out = []
        for p in plain_out:
            b = BoxList(p.bbox, p.size, "xyxy")
            b.add_field("labels", p.get_field("labels"))
            b.add_field("scores", p.get_field("scores"))
            if count_dev:
                b.count_dev = torch.tensor([len(p)], dtype=torch.int32, device="cuda")
            out.append(b)
        return out
    with torch.no_grad():
        feats = on.backbone(images.tensors)
        try:
            # evaluation (mode None) on lists at fixed capacity: untouched
            res = mask(feats, boxes(count_dev=True), None, images)[1]
            assert not calls and [len(r) for r in res] == [len(p) for p in plain_out]
            # the teacher's two passes: the pseudo-mask generator, then the post-processor in mode "train"
            mask.set_teacher_mode("test")
            res = mask(feats, boxes(), None, images)[1]
            assert not calls and all(hasattr(r.get_field("mask"), "seg") for r in res)
            mask.set_teacher_mode("train")
            res = mask(feats, boxes(), None, images)[1]
            assert not calls and [len(r) for r in res] == [len(p) for p in plain_out]
        finally:
            mask.set_teacher_mode(None)
        # and evaluation on ordinary lists does call it, once per image
        res = mask(feats, boxes(), None, images)[1]
    assert len(calls) == len(plain_out)
    assert [len(r) for r in res] == [len(_expected_rows(p, ON)) for p in plain_out]
    torch.cuda.synchronize()


def test_multi_view_applies_it_once_after_the_merge(on, images, monkeypatch):
    from maskrcnn_benchmark.modeling.roi_heads.mask_head import mask_head as mh
    seen = []
    real = mh.boxlist_mask_nms
    monkeypatch.setattr(mh, "boxlist_mask_nms", lambda b, **k: seen.append((b, k)) or real(b, **k))
    out = on.forward_tta([images], flip=True)
    torch.cuda.synchronize()
    assert len(seen) == len(out) == 2        # once per image, on the merged probabilities of all views
    for o, (full, k) in zip(out, seen):
        assert k == {"thresh": 0.3, "measure": "iomin", "class_agnostic": True, "mask_threshold": 0.5}
        assert tuple(full.get_field("mask").shape[1:]) == (1, 28, 28) and len(full) > 0
        _assert_selection(o, full, _expected_rows(full, ON))


def test_inference_through_the_pap_evaluator_on_the_device(on, images, synth):
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    from maskrcnn_benchmark.engine.inference import inference
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.image_list import to_image_list
    imgs, tgs = synth.make_labeled(2, SIZE, 4, seed=1234)

    def disc(cx, cy, r):
        yy, xx = np.mgrid[0:SIZE, 0:SIZE]
        return np.asfortranarray((((xx - cx) ** 2 + (yy - cy) ** 2) <= r * r).astype(np.uint8))

    class DS(object):
        maxWS = SIZE
        id_to_img_map = {0: {"file_name": "s0", "location": (0, 0), "id": 0}, 1: {"file_name": "s1", "location": (160, 0), "id": 1}}
        contiguous_category_id_to_json_id = {1: 1, 2: 2}

        def __len__(self):
            return 2

        def get_ground_truth(self, original_id):
            t = tgs[original_id["id"]]
            b = BoxList(t["boxes"].clone(), (SIZE, SIZE), "xyxy")
            b.add_field("labels", t["labels"].clone())
            rles = [mask_rle.encode(disc(float(x0 + x1) / 2, float(y0 + y1) / 2, float(x1 - x0) / 2)) for x0, y0, x1, y1 in t["boxes"].tolist()]
            for r in rles:
                r["counts"] = r["counts"].decode("utf-8")
            b.add_field("masks", rles)
            return b

    class Loader(list):
        dataset = DS()

        def __len__(self):
            return 2

    results, pap_results = inference(on, Loader([(to_image_list(list(imgs), 32), None, (0, 1))]), "synthetic", iou_types=("segm",),
                                     eval_on_device=True)
    with torch.no_grad():
        direct = on(images)
    assert len(pap_results) == sum(len(d) for d in direct) > 0
    for m in ("AJI", "F1", "DSC", "mAP", "AP50"):
        assert m in results.results["segm"]
