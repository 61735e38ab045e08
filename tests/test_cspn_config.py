"""The CSPN mask head from the reference's own config keys (reference configs/pap/CSPN.yaml,
modeling/roi_heads/mask_head/roi_mask_feature_extractors.py:9-88, roi_mask_predictors.py:39-53): FEATURE_EXTRACTOR / PREDICTOR build
the reference's model -- same state-dict names, shapes, parameter order and trainable set (tests/golden/state_shapes_cspn.json,
written by gen_golden_cspn.py from the reference) --, and the plain-torch restatement the GPU tests take their gradients from
(tests/cspn_formulation.py) reproduces the reference's own outputs (tests/golden/cspn160.npz).  CPU only: construction, no kernels."""
import json
import os

import pytest
import torch

import cspn_formulation as cf
from conftest import GOLD, T, gold


def _build(cfg):
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    return build_detection_model(cfg, is_student=True)


def _cspn_cfg():
    from maskrcnn_benchmark.config import make_default_cfg
    return cf.apply_keys(make_default_cfg())


def _shapes(model):
    return {k: list(v.shape) for k, v in model.state_dict().items() if "cell_anchors" not in k}


@pytest.fixture(scope="module")
def cspn_shapes():
    with open(os.path.join(GOLD, "state_shapes_cspn.json")) as f:
        return json.load(f)


def test_cspn_keys_build_the_reference_state_dict(cspn_shapes):
    m = _build(_cspn_cfg())
    want = {k: v for k, v in cspn_shapes["shapes"].items() if "cell_anchors" not in k}
    got = _shapes(m)
    assert sorted(got) == sorted(want)
    assert got == want
    assert [k for k in m.state_dict() if "cell_anchors" not in k] == [k for k in cspn_shapes["shapes"] if "cell_anchors" not in k]
    assert [k for k, _ in m.named_parameters()] == cspn_shapes["param_order"]
    assert got["mask_heads.mask.feature_extractor.posconv1.weight"] == [256, 480, 3, 3]
    assert got["mask_heads.mask.predictor.mask_fcn_logits.weight"] == [3, 32, 1, 1]
    assert not any(".mask_relation_module.relation_module." in k for k in got)   # TYPE 'LIAM': extractor / classifier / deconv_1 only
    # trainable: the reference leaves the unused relation module trainable (it never gets a gradient there); here it is frozen, as
    # it is in the default model -- every other name agrees
    rel = "mask_heads.mask.mask_relation_module."
    trainable = [k for k, p in m.named_parameters() if p.requires_grad]
    assert trainable == [k for k in cspn_shapes["trainable"] if not k.startswith(rel)]
    assert all(("mask_heads.mask." + n + ".weight") in trainable for n in cf.PRCNN_NAMES)


def test_default_config_is_unchanged(state_shapes):
    from maskrcnn_benchmark.config import make_default_cfg
    m = _build(make_default_cfg())
    assert _shapes(m) == {k: v for k, v in state_shapes["shapes"].items() if "cell_anchors" not in k}
    assert [k for k, _ in m.named_parameters()] == state_shapes["param_order"]
    assert type(m.mask_heads.mask.feature_extractor).__name__ == "MaskRCNNFPNFeatureExtractor"
    assert type(m.mask_heads.mask.predictor).__name__ == "MaskRCNNC4Predictor"


def test_unknown_extractor_or_predictor_raises_key_error():
    cfg = _cspn_cfg()
    cfg.MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR = "ResNet50Conv5ROIFeatureExtractor"
    with pytest.raises(KeyError, match="ResNet50Conv5ROIFeatureExtractor"):
        _build(cfg)
    cfg = _cspn_cfg()
    cfg.MODEL.ROI_MASK_HEAD.PREDICTOR = "NoSuchPredictor"
    with pytest.raises(KeyError, match="NoSuchPredictor"):
        _build(cfg)


def test_liam_with_the_relation_in_use_still_raises():
    cfg = _cspn_cfg()
    cfg.MODEL.RELATION_MASK.USE_RELATION = True
    with pytest.raises(NotImplementedError, match="only TYPE 'CIAM'"):
        _build(cfg)


def test_formulation_reproduces_the_reference(synth, cspn_shapes):
    """the yardstick against the reference, without a GPU: in double, pooled samples and logits to 1e-5 of the tensor's maximum,
    loss_seg to 1e-5 relative"""
    g = gold("cspn160")
    sd = {k: v.double() for k, v in synth.make_weights(cspn_shapes["shapes"], seed=0).items() if k.startswith(cf.PRE)}
    imgs, tgs = synth.make_labeled(2, 160, 4, seed=1234)
    boxes = cf.fixture_boxes(tgs, 160)
    assert torch.equal(torch.stack(boxes), T(g["boxes"]))
    with torch.no_grad():
        pooled, _, logits = cf.head(sd, imgs.double(), [b.double() for b in boxes])
    for name, t in (("pooled", pooled), ("logits", logits)):
        assert list(t.shape) == g[name + "_shape"].tolist()
        err = (t.reshape(-1)[T(g[name + "_idx"])] - T(g[name + "_val"])).abs().max().item()
        print(name, "max err", err, "of", float(g[name + "_max"]))
        assert abs(t.abs().max().item() - float(g[name + "_max"])) <= 1e-5 * float(g[name + "_max"])
        assert err <= 1e-5 * float(g[name + "_max"]), (name, err)
    assert torch.equal(torch.cat(cf.matched_labels(boxes, tgs)), T(g["labels"]))
    loss = cf.mask_loss(logits.float(), boxes, tgs).item()
    print("loss_seg", loss, float(g["loss_seg"]))
    assert abs(loss - float(g["loss_seg"])) <= 1e-5 * abs(float(g["loss_seg"]))
