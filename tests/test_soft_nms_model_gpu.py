"""MODEL.ROI_HEADS.SOFT_NMS in the box head ("Soft-NMS in the box head") on the small synthetic setup of
tests/test_model_gpu.py: 160 x 160 images, n = 2, the synthetic weights, default arithmetic.  The expected lists are the plain
formulation (tests/soft_nms_formulation.py) applied to what the post-processor was handed, so the comparison is equality."""
import numpy as np
import pytest
import torch

import soft_nms_formulation as F
from test_model_gpu import SIZE

pytestmark = pytest.mark.gpu

ON = {"ENABLED": True, "METHOD": "linear", "SIGMA": 0.5, "MIN_SCORE": 0.001}


def _cfg(keys=None):
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    for k, v in (keys or {}).items():
        cfg.MODEL.ROI_HEADS.SOFT_NMS[k] = v
    return cfg


def _model(cfg, weights, **kw):
    from maskrcnn_benchmark import _hip
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    _hip.lib()
    m = build_detection_model(cfg, **kw).cuda()
    m.load_state_dict(weights, strict=False)
    m.eval()
    return m


@pytest.fixture(scope="module")
def plain(weights):
    return _model(_cfg(), weights)


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
    with torch.no_grad():
        out = plain(images)
    torch.cuda.synchronize()
    return out


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) and set(x.fields()) == set(y.fields())
        assert torch.equal(x.bbox, y.bbox)
        for f in y.fields():
            u, v = x.get_field(f), y.get_field(f)
            assert torch.equal(u, v) if torch.is_tensor(u) else u == v, f


def _spy_forward_prob(model, monkeypatch):
    """records (prob, box_regression, boxes, soft_nms) of every PostProcessor.forward_prob call"""
    seen = []
    pp = model.box_heads.box.post_processor
    real = pp.forward_prob

    def spy(prob, reg, boxes, soft_nms=True):
        seen.append((prob, reg, boxes, soft_nms))
        return real(prob, reg, boxes, soft_nms=soft_nms)
    monkeypatch.setattr(pp, "forward_prob", spy)
    return seen


def _expected(model, prob, reg, boxes, keys=ON):
    """the formulation on the post-processor's own decode of what it was handed -> per image (boxes, scores, labels), and the
    decoded boxes"""
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.utils.miscellaneous import dev_const
    pp = model.box_heads.box.post_processor
    per = [len(b) for b in boxes]
    offs = [0]
    for n in per:
        offs.append(offs[-1] + n)
    dec = H.box_decode(reg.reshape(sum(per), -1), torch.cat([b.bbox for b in boxes], 0), pp.box_coder.weights, pp.box_coder.bbox_xform_clip,
                       dev_const(offs, torch.int32, prob.device),
                       dev_const([[b.size[0] - 1, b.size[1] - 1] for b in boxes], torch.float32, prob.device))
    dec = dec.reshape(sum(per), -1).cpu().numpy()
    want = F.filter_results_soft(prob.cpu().numpy(), dec, per, pp.score_thresh, pp.nms, pp.detections_per_img, keys["METHOD"],
                                 keys["SIGMA"], keys["MIN_SCORE"])
    return want, dec, per


def test_switched_off_the_post_processor_never_calls_the_new_wrapper(weights, plain_out, images, monkeypatch):
    from maskrcnn_benchmark import _hip as H

    def refuse(*a, **k):
        raise AssertionError("det_postprocess_soft was called")
    monkeypatch.setattr(H, "det_postprocess_soft", refuse)
    calls = []
    real = H.det_postprocess
    monkeypatch.setattr(H, "det_postprocess", lambda *a, **k: calls.append(k) or real(*a, **k))
    off = _model(_cfg(dict(ON, ENABLED=False, METHOD="gaussian")), weights)      # every other key set: only ENABLED switches
    assert off.box_heads.box.post_processor.soft_nms is None
    with torch.no_grad():
        out = off(images)
    torch.cuda.synchronize()
    assert len(calls) == 1 and "soft" not in calls[0]
    _same_lists(out, plain_out)


def test_enabled_eval_forward_returns_the_formulations_lists(on, plain_out, images, monkeypatch):
    seen = _spy_forward_prob(on, monkeypatch)
    with torch.no_grad():
        out = on(images)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][3] is True
    prob, reg, boxes, _ = seen[0]
    want, dec, per = _expected(on, prob, reg, boxes)
    p, lo, decayed = prob.cpu().numpy(), 0, 0
    for o, pl, (bb, sc, lb), R in zip(out, plain_out, want, per):
        print("soft-NMS returns %d detections, the greedy NMS %d" % (len(o), len(pl)))
        assert len(o) == len(sc) > 0
        assert o.bbox.cpu().numpy().tobytes() == bb.tobytes()
        assert o.get_field("scores").cpu().numpy().tobytes() == sc.tobytes()
        assert o.get_field("labels").cpu().tolist() == lb.tolist()
        assert torch.equal(o.get_field("scores"), o.get_field("objectness"))
        # every detection is a (row, class) of this image, and its score is at most that class probability
        for box, s, j in zip(bb, sc, lb):
            rows = np.flatnonzero((dec[lo:lo + R, 4 * j:4 * j + 4] == box).all(1))
            assert len(rows) > 0 and (s <= p[lo + rows, j]).any()
            decayed += int((s < p[lo + rows, j]).all())
        # the mask head ran on these lists
        assert o.has_field("mask") and o.get_field("mask").shape[0] == len(o)
        lo += R
    # (on these inputs DETECTIONS_PER_IMG cuts both lists at 200, and what survives the cut may well be undecayed: informational)
    print("%d detections carry a decayed score" % decayed)


def test_teacher_passes_are_what_they_are_with_the_flag_off(weights, synth, monkeypatch):
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.structures.image_list import to_image_list
    calls = []
    real = H.det_postprocess_soft
    monkeypatch.setattr(H, "det_postprocess_soft", lambda *a, **k: calls.append(1) or real(*a, **k))
    unl = synth.make_unlabeled(2, SIZE, 3, seed=991)
    outs = []
    for keys in (None, ON):
        teacher = _model(_cfg(keys), weights, is_teacher=True)
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        teacher.set_rng(g)
        with torch.no_grad():
            outs.append(teacher.forward_teacher([to_image_list(list(u.cuda()), 32) for u in unl[:2]]))
        teacher.set_rng(None)
    torch.cuda.synchronize()
    assert not calls
    a, b = outs
    _same_lists(a["result_t"], b["result_t"])
    for x, y in zip(a["class_logit_t"], b["class_logit_t"]):
        assert torch.equal(x, y)
    for x, y in zip(a["seg_mask"], b["seg_mask"]):
        assert torch.equal(x, y)
    for ex, ey in zip(a["embedding"], b["embedding"]):
        for x, y in zip(ex, ey):
            assert torch.equal(x, y)


def test_multi_view_applies_it_after_the_merge(on, images, monkeypatch):
    seen = _spy_forward_prob(on, monkeypatch)
    with torch.no_grad():
        out = on(images, tta=True)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][3] is True          # once, on the probabilities merged over the views
    want, _, _ = _expected(on, *seen[0][:3])
    for o, (bb, sc, lb) in zip(out, want):
        assert o.bbox.cpu().numpy().tobytes() == bb.tobytes() and o.get_field("scores").cpu().numpy().tobytes() == sc.tobytes()
        assert o.has_field("mask") and o.get_field("mask").shape[0] == len(o)


def test_two_runs_give_equal_bits(on, images):
    with torch.no_grad():
        a = on(images)
        b = on(images)
    torch.cuda.synchronize()
    _same_lists(a, b)
