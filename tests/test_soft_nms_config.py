"""MODEL.ROI_HEADS.SOFT_NMS ("Soft-NMS in the box head"): the node's defaults, the refusals when the box head's
post-processor is built, and a disabled node that is not looked at.  CPU only: construction, no kernels."""
import pytest


def _cfg(**keys):
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    for k, v in keys.items():
        cfg.MODEL.ROI_HEADS.SOFT_NMS[k] = v
    return cfg


def _post(cfg):
    from maskrcnn_benchmark.modeling.roi_heads.box_head.box_head import make_roi_box_post_processor
    return make_roi_box_post_processor(cfg)


def test_defaults_of_the_node():
    cfg = _cfg()
    assert dict(cfg.MODEL.ROI_HEADS.SOFT_NMS) == {"ENABLED": False, "METHOD": "linear", "SIGMA": 0.5, "MIN_SCORE": 0.001}
    r = cfg.MODEL.ROI_HEADS                                                        # the node's neighbours stay
    assert r.SCORE_THRESH == 0.05 and r.NMS == 0.5 and r.DETECTIONS_PER_IMG == 200
    cfg.merge_from_list(["MODEL.ROI_HEADS.SOFT_NMS.ENABLED", "True", "MODEL.ROI_HEADS.SOFT_NMS.METHOD", "gaussian",
                         "MODEL.ROI_HEADS.SOFT_NMS.SIGMA", "0.3"])
    n = cfg.MODEL.ROI_HEADS.SOFT_NMS
    assert n.ENABLED is True and n.METHOD == "gaussian" and n.SIGMA == 0.3 and n.MIN_SCORE == 0.001


def test_the_post_processor_takes_the_node():
    assert _post(_cfg()).soft_nms is None
    on = _post(_cfg(ENABLED=True, METHOD="gaussian", SIGMA=0.3, MIN_SCORE=0.01))
    assert on.soft_nms.METHOD == "gaussian" and on.soft_nms.SIGMA == 0.3 and on.soft_nms.MIN_SCORE == 0.01
    assert (on.score_thresh, on.nms, on.detections_per_img) == (0.05, 0.5, 200)
    # MIN_SCORE of exactly 1 is inside
    assert _post(_cfg(ENABLED=True, MIN_SCORE=1.0)).soft_nms is not None
    # and a post-processor built without the node is the one it always was
    from maskrcnn_benchmark.modeling.roi_heads.box_head.box_head import PostProcessor
    assert PostProcessor(0.05, 0.5, 100).soft_nms is None


@pytest.mark.parametrize("keys, match", [({"METHOD": "quadratic"}, "METHOD"), ({"METHOD": "Linear"}, "METHOD"), ({"SIGMA": 0.0}, "SIGMA"),
                                         ({"SIGMA": -0.5}, "SIGMA"), ({"SIGMA": float("inf")}, "SIGMA"), ({"MIN_SCORE": 0.0}, "MIN_SCORE"),
                                         ({"MIN_SCORE": -0.1}, "MIN_SCORE"), ({"MIN_SCORE": 1.5}, "MIN_SCORE")])
def test_bad_method_sigma_or_min_score_raises_when_the_head_is_built(keys, match):
    from maskrcnn_benchmark.modeling.roi_heads.box_head.box_head import build_roi_box_head
    with pytest.raises(ValueError, match="MODEL.ROI_HEADS.SOFT_NMS." + match):
        build_roi_box_head(_cfg(ENABLED=True, **keys))


def test_a_disabled_node_validates_nothing():
    assert _post(_cfg(METHOD="quadratic", SIGMA=-1.0, MIN_SCORE=7.0)).soft_nms is None
    from maskrcnn_benchmark.modeling.roi_heads.box_head.box_head import build_roi_box_head
    assert build_roi_box_head(_cfg(METHOD="quadratic", SIGMA=-1.0, MIN_SCORE=7.0)).post_processor.soft_nms is None


def test_state_dict_names_and_shapes_unchanged(state_shapes):
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    for cfg in (_cfg(), _cfg(ENABLED=True)):
        m = build_detection_model(cfg)
        got = {k: list(v.shape) for k, v in m.state_dict().items() if "cell_anchors" not in k}
        assert got == {k: v for k, v in state_shapes["shapes"].items() if "cell_anchors" not in k}
        assert (m.box_heads.box.post_processor.soft_nms is not None) == cfg.MODEL.ROI_HEADS.SOFT_NMS.ENABLED
