"""TEST.MASK_NMS ("Mask NMS at inference"): the node's defaults, the refusals when the mask head is built, and
the default model left as it was.  CPU only: construction, no kernels."""
import pytest


def _build(cfg):
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    return build_detection_model(cfg)


def _cfg(**keys):
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    for k, v in keys.items():
        cfg.TEST.MASK_NMS[k] = v
    return cfg


def test_defaults_of_the_node():
    cfg = _cfg()
    assert dict(cfg.TEST.MASK_NMS) == {"ENABLED": False, "THRESH": 0.5, "MEASURE": "iou", "CLASS_AGNOSTIC": False}
    assert cfg.TEST.TTA is False and cfg.TEST.TTA_FLIP is True and cfg.TEST.TTA_VIEWS == 1   # the node's neighbours stay
    cfg.merge_from_list(["TEST.MASK_NMS.ENABLED", "True", "TEST.MASK_NMS.THRESH", "0.3", "TEST.MASK_NMS.MEASURE", "iomin"])
    assert cfg.TEST.MASK_NMS.ENABLED is True and cfg.TEST.MASK_NMS.THRESH == 0.3 and cfg.TEST.MASK_NMS.MEASURE == "iomin"


def test_the_post_processor_takes_the_node_and_the_generator_never_does():
    from maskrcnn_benchmark.modeling.roi_heads.mask_head import mask_head as mh
    off = mh.make_roi_mask_post_processor(_cfg())
    assert off.mask_nms is None and off.masker is None
    cfg = _cfg(ENABLED=True, THRESH=0.3, MEASURE="iomin", CLASS_AGNOSTIC=True)
    on = mh.make_roi_mask_post_processor(cfg)
    assert on.mask_nms == {"thresh": 0.3, "measure": "iomin", "class_agnostic": True, "mask_threshold": 0.5}
    assert mh.make_roi_mask_generator(cfg).mask_nms is None
    cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS = True
    cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD = 0.4
    pasted = mh.make_roi_mask_post_processor(cfg)
    assert isinstance(pasted.masker, mh.DetectionMasker) and pasted.mask_nms["mask_threshold"] == 0.4
    # switched off, the other keys are not looked at
    assert mh.make_roi_mask_post_processor(_cfg(MEASURE="dice", THRESH=7.0)).mask_nms is None


@pytest.mark.parametrize("keys, match", [({"MEASURE": "dice"}, "MEASURE"), ({"MEASURE": "IOU"}, "MEASURE"), ({"THRESH": 0.0}, "THRESH"),
                                         ({"THRESH": -0.5}, "THRESH"), ({"THRESH": 1.5}, "THRESH")])
def test_bad_measure_or_threshold_raises_when_the_head_is_built(keys, match):
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.mask_head import build_roi_mask_head
    with pytest.raises(ValueError, match="TEST.MASK_NMS." + match):
        build_roi_mask_head(_cfg(ENABLED=True, **keys))


def test_state_dict_names_and_shapes_unchanged(state_shapes):
    for cfg in (_cfg(), _cfg(ENABLED=True)):
        m = _build(cfg)
        got = {k: list(v.shape) for k, v in m.state_dict().items() if "cell_anchors" not in k}
        assert got == {k: v for k, v in state_shapes["shapes"].items() if "cell_anchors" not in k}
        assert [k for k, _ in m.named_parameters()] == state_shapes["param_order"]
        assert (m.mask_heads.mask.post_processor.mask_nms is not None) == cfg.TEST.MASK_NMS.ENABLED
        assert m.mask_heads.mask.mask_generator.mask_nms is None
