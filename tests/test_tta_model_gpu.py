"""Multi-view inference (GeneralizedRCNN.forward_tta) on the small synthetic setup of tests/test_model_gpu.py: 160 x 160 images,
n = 2, the synthetic weights, default arithmetic.

Tolerance of (c), (d) and the padded cases.  A pass that batches more views than another runs the same per-image arithmetic, but
the deep, few-tile layers pick their split-K from the tile count, so the summation order differs.  What that is worth was measured
on the path that existed before this feature, with the inputs of tests/test_fullsize_properties.py::
test_teacher_batched_views_equal_unbatched (teacher model, seed 11, 160 x 160, K x flip = 4 views in one batch against four separate
backbone passes): pyramids 4.4e-7 of the level's maximum; ROIBoxHead._forward_single on the batched against the separate pyramids,
class logits MEASURED_REF["logits"] and regression codes MEASURED_REF["regs"] of the tensor's maximum; the mask head's logits on all
four views MEASURED_REF["mask"].  With 2x margin these are EPS_LOGIT, EPS_REG and EPS_MASK, relative to the largest |value| of the
tensor compared.  For the final outputs of (c): softmax and sigmoid do not expand distances, the plain pass takes torch's softmax /
sigmoid and the multi-view pass the kernel's (each within the kernel bound of the exact value), the decoder turns a code error e into
at most e x W / 5 pixels inside a W-pixel image (weights 10 and 5; exp(dw) <= W / w) and rounds four times at magnitude <= W per
coordinate in either pass:
    scores               EPS_LOGIT x max |logit| + 2 box_bound(V, C)
    mask probabilities   EPS_MASK x max |mask logit| + 2 mask_bound(V)
    boxes                EPS_REG x max |code| x W / 5 + 8 x 2^-24 x W
Measured on the MI355X: see MEASURED_C below.  V = 1 gave the plain pass's boxes and scores bit for bit and its mask probabilities to
one ulp (6e-8: the kernel's sigmoid against torch's).

SEED was picked with the CPU oracle (oracle/model.py: the reference's arithmetic in fp32 on the host) among 16 seeds so that the
reference alone satisfies the preconditions of (c): 200 detections on either image, every detection's score 0.0375 or more away from
SCORE_THRESH, every same-class pair of detections 4.8e-4 or more away from NMS in IoU (1e-4 is asserted).  The decisions behind the
lists have room too: no (kept box, lower-scored live candidate) pair of the greedy NMS is within 8.4e-5 of NMS, and the
DETECTIONS_PER_IMG cut falls into a score gap of 2.7e-3 -- both far above what a different summation order moves (IoU ~1e-6)."""
import numpy as np
import pytest
import torch

import tta_formulation as F
from test_model_gpu import SIZE
from test_tta_kernels_gpu import box_bound, mask_bound, reg_bound

pytestmark = pytest.mark.gpu

SEED = 6
U = 2.0 ** -24
# the existing teacher path, batched against separate passes (module docstring), relative to the tensor's maximum
MEASURED_REF = {"logits": 3.03e-6, "regs": 1.88e-6, "mask": 9.19e-7}
EPS_LOGIT, EPS_REG, EPS_MASK = 2 * MEASURED_REF["logits"], 2 * MEASURED_REF["regs"], 2 * MEASURED_REF["mask"]
# largest differences seen on the MI355X between forward_tta([x, x], flip=False) and model(x): scores, boxes (px), mask probabilities
MEASURED_C = {"scores": 1.37e-6, "boxes": 3.05e-5, "mask": 1.67e-6}


def _rel_tol(eps, ref):
    return eps * float(ref.abs().max())


@pytest.fixture(scope="module")
def model(weights):
    from maskrcnn_benchmark import _hip
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    _hip.lib()
    cfg = make_default_cfg()
    m = build_detection_model(cfg).cuda()
    m.load_state_dict(weights, strict=False)
    m.eval()
    return m


@pytest.fixture(scope="module")
def images(synth):
    from maskrcnn_benchmark.structures.image_list import to_image_list
    imgs, _ = synth.make_labeled(2, SIZE, 4, seed=SEED)
    return to_image_list(list(imgs.cuda()), 32)


@pytest.fixture(scope="module")
def plain(model, images):
    """model(x), computed once and shared"""
    with torch.no_grad():
        out = model(images)
    torch.cuda.synchronize()
    return out


def _tapped(model, views, flip):
    model.taps = {}
    try:
        out = model.forward_tta(views, flip=flip)
        return out, model.taps
    finally:
        model.taps = None


def test_merged_taps_equal_the_formulation_and_the_detections_their_postprocessing(model, images, synth):
    """(a) the tapped merged tensors are the formulation of the tapped per-view tensors within the kernels' bounds; (b) the
    detections are post_processor.forward_prob of the tapped merged pair, bit for bit; the mask field likewise"""
    from maskrcnn_benchmark.structures.image_list import to_image_list
    more, _ = synth.make_labeled(2, SIZE, 4, seed=99)
    views = [images, to_image_list(list(more.cuda()), 32)]
    before = [v.tensors.clone() for v in views]
    out, taps = _tapped(model, views, True)
    assert all(torch.equal(v.tensors, b) for v, b in zip(views, before))      # the caller's ImageLists are not mirrored in place
    flips = [False, True, False, True]
    vl, vr = taps["tta_view_logits"], taps["tta_view_regs"]
    V, R, C = vl.shape
    assert V == 4 and vr.shape == (V, R, 4 * C) and R == sum(len(p) for p in taps["infer_proposals"])
    rp, rr = F.merge_box(vl.cpu(), vr.cpu(), flips)
    ep = float((taps["tta_box_prob"].cpu().double() - rp).abs().max())
    er = float((taps["tta_box_reg"].cpu().double() - rr).abs().max())
    print("merged box prob err %.3g (bound %.3g), reg err %.3g (bound %.3g)" % (ep, box_bound(V, C), er, reg_bound(V, vr.cpu())))
    assert ep <= box_bound(V, C) and er <= reg_bound(V, vr.cpu())
    # (the mirrored views really differ: the merge is not one view's output)
    assert float((vl[1] - vl[0]).abs().max()) > 1e-3 and float((vl[2] - vl[0]).abs().max()) > 1e-3
    # (b)
    again = model.box_heads.box.post_processor.forward_prob(taps["tta_box_prob"], taps["tta_box_reg"], taps["infer_proposals"])
    assert [len(a) for a in again] == [len(o) for o in out] and all(len(o) > 0 for o in out)
    for a, o in zip(again, out):
        assert torch.equal(a.bbox, o.bbox) and torch.equal(a.get_field("scores"), o.get_field("scores"))
        assert torch.equal(a.get_field("labels"), o.get_field("labels"))
    # masks
    ml = taps["tta_view_mask_logits"]
    D = sum(len(o) for o in out)
    assert ml.shape == (V, D, C, 28, 28)
    labels = torch.cat([o.get_field("labels") for o in out])
    got = torch.cat([o.get_field("mask") for o in out])
    assert got.shape == (D, 1, 28, 28)
    em = float((got[:, 0].cpu().double() - F.merge_mask(ml.cpu(), labels.cpu(), flips)).abs().max())
    print("merged mask err %.3g (bound %.3g)" % (em, mask_bound(V)))
    assert em <= mask_bound(V)
    # run to run: the same bits
    out2, _ = _tapped(model, views, True)
    for a, o in zip(out2, out):
        assert torch.equal(a.bbox, o.bbox) and torch.equal(a.get_field("mask"), o.get_field("mask"))


def _iou(b):
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    lt = torch.max(b[:, None, :2], b[None, :, :2])
    rb = torch.min(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area[:, None] + area[None, :] - inter)


def test_one_view_and_two_equal_views_reproduce_plain_inference(model, images, plain):
    """(c) forward_tta([x], flip=False) and forward_tta([x, x], flip=False) against model(x): same counts and labels; boxes,
    scores and mask probabilities within the tolerance of the module docstring"""
    pp = model.box_heads.box.post_processor
    for p in plain:      # the preconditions, on the plain result
        assert len(p) >= 1
        assert float((p.get_field("scores") - pp.score_thresh).abs().min()) > 1e-4
        iou, lab = _iou(p.bbox), p.get_field("labels")
        same = (lab[:, None] == lab[None, :]) & ~torch.eye(len(p), dtype=torch.bool, device=lab.device)
        if bool(same.any()):
            assert float((iou[same] - pp.nms).abs().min()) > 1e-4
    for views in ([images], [images, images]):
        out, taps = _tapped(model, views, False)
        V, C = len(views), taps["tta_view_logits"].shape[2]
        tol_p = _rel_tol(EPS_LOGIT, taps["tta_view_logits"]) + 2 * box_bound(V, C)
        tol_m = _rel_tol(EPS_MASK, taps["tta_view_mask_logits"]) + 2 * mask_bound(V)
        tol_b = _rel_tol(EPS_REG, taps["tta_view_regs"]) * SIZE / 5 + 8 * U * SIZE
        assert [len(o) for o in out] == [len(p) for p in plain]
        for o, p in zip(out, plain):
            assert torch.equal(o.get_field("labels"), p.get_field("labels"))
            es = float((o.get_field("scores") - p.get_field("scores")).abs().max())
            eb = float((o.bbox - p.bbox).abs().max())
            em = float((o.get_field("mask") - p.get_field("mask")).abs().max())
            print("V=%d: scores %.3g (tol %.3g) boxes %.3g (tol %.3g) mask %.3g (tol %.3g)" % (len(views), es, tol_p, eb, tol_b, em, tol_m))
            assert es <= tol_p and eb <= tol_b and em <= tol_m
            assert o.get_field("mask").shape == p.get_field("mask").shape and o.size == p.size
            assert set(o.fields()) == set(p.fields())


def test_mirrored_view_of_a_symmetric_image_is_the_plain_network_on_mirrored_rois(model, images):
    """(d) flip=True on x == hflip(x).  Views 0 and 1 are then the same image, so they agree as far as the network is the same
    function: view 1's per-view outputs are what view 0's pyramid gives for the MIRRORED proposals and detections (the network's
    filters are not mirror-symmetric, so the outputs for a proposal and for its mirror image differ; what must agree is the image
    each view saw, its place in the batch and the ROIs it was pooled with).  Checked against the heads run directly on the plain
    single-view pyramid, within the tolerance of the module docstring."""
    from maskrcnn_benchmark.structures.image_list import ImageList
    from maskrcnn_benchmark.utils.miscellaneous import batch_boxlist_hflip
    x = images.tensors
    sym = ImageList(((x + torch.flip(x, (3,))) * 0.5).contiguous(), list(images.image_sizes))
    assert torch.equal(sym.tensors, torch.flip(sym.tensors, (3,)))
    out, taps = _tapped(model, [sym], True)
    box, mask = model.box_heads.box, model.mask_heads.mask
    with torch.no_grad():
        feats = model.backbone(sym.tensors)
        props = taps["infer_proposals"]
        ref = []
        for bl in (props, batch_boxlist_hflip(props)):
            ref.append(box.predictor(box.feature_extractor(feats, bl, istrain=False)))
        dets = taps["detections"]
        mref = [mask.predictor(mask.feature_extractor(feats, bl)[0]) for bl in (dets, batch_boxlist_hflip(dets))]
    vl, vr, vm = taps["tta_view_logits"], taps["tta_view_regs"], taps["tta_view_mask_logits"]
    for v in range(2):
        tl, tr, tm = _rel_tol(EPS_LOGIT, ref[v][0]), _rel_tol(EPS_REG, ref[v][1]), _rel_tol(EPS_MASK, mref[v])
        el, er_ = float((vl[v] - ref[v][0]).abs().max()), float((vr[v] - ref[v][1]).abs().max())
        em = float((vm[v] - mref[v]).abs().max())
        print("view %d: logits %.3g (tol %.3g) regs %.3g (tol %.3g) mask logits %.3g (tol %.3g)" % (v, el, tl, er_, tr, em, tm))
        assert el <= tl and er_ <= tr and em <= tm
    # and the mirrored ROIs matter: view 1 is not view 0
    assert float((vl[1] - vl[0]).abs().max()) > 100 * _rel_tol(EPS_LOGIT, vl[0])


@pytest.mark.parametrize("sizes", [((150, 150), (150, 150)), ((150, 150), (130, 140))], ids=["150x150", "150x150+130x140"])
def test_padded_images_pool_mirrored_views_where_their_content_went(model, synth, sizes):
    """Images whose size is no multiple of 32 (padded to 160 x 160; in the second case two sizes in one batch).  ImageList.hflip()
    mirrors the whole padded tensor, so a mirrored view's content sits pad pixels to the right of its mirror image about the image's
    own width: the ROIs of mirrored views are mirrored about the PADDED width (utils/miscellaneous.py::batch_boxlist_hflip_padded,
    pinned pixel for pixel in tests/test_tta_formulation.py).  View 1's per-view outputs must be the plain network's on the
    mirrored padded tensor with those ROIs, and must NOT be what ROIs mirrored about the image's own width give; the merged
    tensors are the formulation of the per-view ones; boxes, scores and labels stay in the un-mirrored frame of the image."""
    from maskrcnn_benchmark.structures.image_list import to_image_list
    from maskrcnn_benchmark.utils.miscellaneous import batch_boxlist_hflip, batch_boxlist_hflip_padded
    imgs, _ = synth.make_labeled(2, SIZE, 4, seed=SEED)
    il = to_image_list([imgs[i][:, :h, :w].cuda() for i, (h, w) in enumerate(sizes)], 32)
    assert tuple(il.tensors.shape[-2:]) == (SIZE, SIZE) and [tuple(s_) for s_ in il.image_sizes] == [tuple(s_) for s_ in sizes]
    before = il.tensors.clone()
    out, taps = _tapped(model, [il], True)
    assert torch.equal(il.tensors, before)
    box, mask = model.box_heads.box, model.mask_heads.mask
    props, dets = taps["infer_proposals"], taps["detections"]
    with torch.no_grad():
        feats_m = model.backbone(torch.flip(il.tensors, (3,)))
        padded = batch_boxlist_hflip_padded(props, SIZE)
        ref = box.predictor(box.feature_extractor(feats_m, padded, istrain=False))
        own = box.predictor(box.feature_extractor(feats_m, batch_boxlist_hflip(props), istrain=False))
        mref = mask.predictor(mask.feature_extractor(feats_m, batch_boxlist_hflip_padded(dets, SIZE))[0])
        mown = mask.predictor(mask.feature_extractor(feats_m, batch_boxlist_hflip(dets))[0])
    vl, vr, vm = taps["tta_view_logits"], taps["tta_view_regs"], taps["tta_view_mask_logits"]
    tl, tr, tm = _rel_tol(EPS_LOGIT, ref[0]), _rel_tol(EPS_REG, ref[1]), _rel_tol(EPS_MASK, mref)
    el, er_, em = float((vl[1] - ref[0]).abs().max()), float((vr[1] - ref[1]).abs().max()), float((vm[1] - mref).abs().max())
    print("%s view 1: logits %.3g (tol %.3g) regs %.3g (tol %.3g) mask logits %.3g (tol %.3g); own-width mirror: %.3g %.3g %.3g"
          % (sizes, el, tl, er_, tr, em, tm, float((vl[1] - own[0]).abs().max()), float((vr[1] - own[1]).abs().max()),
             float((vm[1] - mown).abs().max())))
    assert el <= tl and er_ <= tr and em <= tm
    # the displacement of 10 (and 20) pixels is visible: ROIs mirrored about the image's own width give other outputs
    assert float((vl[1] - own[0]).abs().max()) > 100 * tl and float((vm[1] - mown).abs().max()) > 100 * tm
    # the merges of what was tapped, and the result in the frame of the image
    flips = [False, True]
    rp, rr = F.merge_box(vl.cpu(), vr.cpu(), flips)
    assert float((taps["tta_box_prob"].cpu().double() - rp).abs().max()) <= box_bound(2, vl.shape[2])
    assert float((taps["tta_box_reg"].cpu().double() - rr).abs().max()) <= reg_bound(2, vr.cpu())
    labels = torch.cat([o.get_field("labels") for o in out])
    got = torch.cat([o.get_field("mask") for o in out])
    assert float((got[:, 0].cpu().double() - F.merge_mask(vm.cpu(), labels.cpu(), flips)).abs().max()) <= mask_bound(2)
    for o, (h, w) in zip(out, sizes):
        assert o.size == (w, h) and len(o) > 0
        assert float(o.bbox[:, 2].max()) <= w - 1 and float(o.bbox[:, 3].max()) <= h - 1 and float(o.bbox.min()) >= 0


def test_plain_inference_never_calls_the_merge_kernels(model, images, monkeypatch):
    """(e)"""
    from maskrcnn_benchmark import _hip as H
    calls = {"box": 0, "mask": 0}
    box, mask = H.tta_merge_box, H.tta_merge_mask
    monkeypatch.setattr(H, "tta_merge_box", lambda *a, **k: calls.__setitem__("box", calls["box"] + 1) or box(*a, **k))
    monkeypatch.setattr(H, "tta_merge_mask", lambda *a, **k: calls.__setitem__("mask", calls["mask"] + 1) or mask(*a, **k))
    with torch.no_grad():
        model(images)
        model(images, tta=False)
        model(images, tta=None)
    assert calls == {"box": 0, "mask": 0}
    with torch.no_grad():
        a = model(images, tta=True)                     # delegates with TEST.TTA_FLIP (True): one launch each
    assert calls == {"box": 1, "mask": 1}
    b = model.forward_tta([images], flip=True)
    for u, v in zip(a, b):
        assert torch.equal(u.bbox, v.bbox) and torch.equal(u.get_field("mask"), v.get_field("mask"))
    # zero detections: empty fields, no mask launch
    pp = model.box_heads.box.post_processor
    monkeypatch.setattr(pp, "score_thresh", 2.0)
    calls["mask"] = 0
    res = model.forward_tta([images], flip=True)
    assert [len(r) for r in res] == [0, 0] and calls["mask"] == 0
    for r in res:
        assert tuple(r.get_field("mask").shape) == (0, 1, 28, 28) and tuple(r.get_field("scores").shape) == (0,)
    torch.cuda.synchronize()


def test_refusals_come_before_any_launch(model, images, monkeypatch):
    """(f) every configuration forward_tta does not offer raises NotImplementedError naming the key, training mode ValueError,
    before the backbone is reached.  (The switches are set on the built model: what forward_tta asks is these attributes, which
    the constructors derive from MODEL.RELATION_NMS.USE_RELATION_NMS, MODEL.RELATION_MASK.USE_RELATION and
    MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR.)"""
    def no_backbone(*a, **k):
        raise AssertionError("the backbone was reached")
    monkeypatch.setattr(model, "extract_aug_feat", no_backbone)
    with monkeypatch.context() as m:
        m.setattr(model.box_heads.box, "use_realation_nms", True)
        with pytest.raises(NotImplementedError, match="RELATION_NMS.USE_RELATION_NMS"):
            model.forward_tta([images])
    with monkeypatch.context() as m:
        m.setattr(model, "relation_nms", torch.nn.Identity())
        with pytest.raises(NotImplementedError, match="RELATION_NMS.USE_RELATION_NMS"):
            model.forward_tta([images])
    with monkeypatch.context() as m:
        m.setattr(model.mask_heads.mask, "use_relation", True)
        with pytest.raises(NotImplementedError, match="RELATION_MASK.USE_RELATION"):
            model.forward_tta([images])
    with monkeypatch.context() as m:
        m.setattr(model.mask_heads.mask, "on_image", True)
        with pytest.raises(NotImplementedError, match="PRCNNFeatureExtractor"):
            model.forward_tta([images])
    with pytest.raises(NotImplementedError, match="TTA_VIEWS"):
        model.forward_tta([images] * 5, flip=True)          # V = 10
    with pytest.raises(NotImplementedError, match="TTA_VIEWS"):
        model.forward_tta([images] * 9, flip=False)
    with pytest.raises(NotImplementedError, match="TTA_VIEWS"):
        model.forward_tta([], flip=True)
    with pytest.raises(NotImplementedError, match="differing shapes"):
        model.forward_tta([images, images.tensors[:, :, :, :128].contiguous()])
    with pytest.raises(NotImplementedError, match="differing shapes"):
        model.forward_tta([images, images.tensors[:1]])
    model.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            model.forward_tta([images])
        with pytest.raises(ValueError, match="eval"):
            model(images, tta=True)
    finally:
        model.eval()
    # the mask head's own entry refuses the same
    with monkeypatch.context() as m:
        m.setattr(model.mask_heads.mask, "use_relation", True)
        with pytest.raises(NotImplementedError, match="RELATION_MASK.USE_RELATION"):
            model.mask_heads.mask.forward_views(None, 2, [False], [], SIZE)


def test_inference_with_tta_through_the_pap_evaluator_on_the_device(model, images, synth):
    """(g) engine/inference.py::inference(tta=True, eval_on_device=True): an ordinary batch (flip-only) and a batch that carries
    two views, predictions scored by the PAP evaluator with the device kernels"""
    from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
    from maskrcnn_benchmark.engine.inference import compute_on_dataset, inference
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.image_list import to_image_list
    imgs, tgs = synth.make_labeled(2, SIZE, 4, seed=SEED)

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

    host = to_image_list(list(imgs), 32)
    results, pap_results = inference(model, Loader([(host, None, (0, 1))]), "synthetic", iou_types=("segm",), tta=True,
                                     eval_on_device=True)
    direct = model.forward_tta([images], flip=True)
    assert len(pap_results) == sum(len(d) for d in direct) > 0
    for m in ("AJI", "F1", "DSC", "mAP", "AP50"):
        assert m in results.results["segm"]
    # a batch that carries its views
    preds = compute_on_dataset(model, [((host, host), None, (0, 1))], torch.device("cuda"), tta=True)
    two = model.forward_tta([images, images], flip=True)
    for i in (0, 1):
        assert preds[i].bbox.device.type == "cpu" and torch.equal(preds[i].bbox, two[i].bbox.cpu())
        assert tuple(preds[i].get_field("mask").shape[1:]) == (1, 28, 28)


def test_tta_views_helper(model):
    """data/transforms::tta_views: K view batches, view 0 un-augmented, the others from the colour chain without erasing; they go
    straight into forward_tta"""
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.data import transforms as T
    from maskrcnn_benchmark.data.transforms import transforms as TT
    cfg = make_default_cfg()
    cfg.TEST.TTA = True
    tr = T.build_transforms(cfg, is_train=False)
    g = torch.Generator().manual_seed(4)
    bases = [T.DeviceImage(torch.randint(0, 256, (96, 128, 3), generator=g, dtype=torch.uint8)) for _ in range(2)]
    views = T.tta_views(bases, tr[1], 3, size_divisible=32)
    assert len(views) == 3 and all(tuple(v.tensors.shape) == (2, 3, 96, 128) for v in views)
    assert views[0].image_sizes == [(96, 128), (96, 128)]
    for i, b in enumerate(bases):
        plain = TT._materialize([T.ToTensor()(b, None)[0]], cfg.INPUT.PIXEL_MEAN, 32)[0]
        assert torch.equal(views[0].tensors[i], plain)
        for k in (1, 2):
            assert not torch.equal(views[k].tensors[i], plain)
    with pytest.raises(ValueError):
        T.tta_views(bases, tr[1], 0)
    out = model.forward_tta(views, flip=True)      # V = 6
    assert len(out) == 2 and all(o.has_field("mask") for o in out)
    torch.cuda.synchronize()
