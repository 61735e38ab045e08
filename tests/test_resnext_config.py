"""ResNeXt backbones from the reference's own config keys (reference modeling/backbone/resnet.py:206-250,
configs/caffe2/e2e_mask_rcnn_X_101_32x8d_FPN_1x_caffe2.yaml): MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP / STRIDE_IN_1X1 build the
reference's model -- same state-dict names and shapes (tests/golden/state_shapes_x101.json, written by gen_golden_resnext.py from
the reference), so its checkpoints load unchanged.  CPU only: construction and checkpoint I/O, no kernels."""
import json
import os

import pytest
import torch

from conftest import GOLD


def _cfg(body="R-50-FPN", groups=32, width=8, in_1x1=False):
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    cfg.MODEL.BACKBONE.CONV_BODY = body
    cfg.MODEL.RESNETS.NUM_GROUPS = groups
    cfg.MODEL.RESNETS.WIDTH_PER_GROUP = width
    cfg.MODEL.RESNETS.STRIDE_IN_1X1 = in_1x1
    return cfg


def _build(cfg):
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    return build_detection_model(cfg, is_student=True)


def _shapes(model):
    return {k: list(v.shape) for k, v in model.state_dict().items() if "cell_anchors" not in k}


def test_x101_32x8d_builds_with_the_reference_state_dict():
    want = json.load(open(os.path.join(GOLD, "state_shapes_x101.json")))["shapes"]
    want = {k: v for k, v in want.items() if "cell_anchors" not in k}
    got = _shapes(_build(_cfg("R-101-FPN")))
    assert sorted(got) == sorted(want)
    assert got == want
    assert got["backbone.body.layer1.0.conv2.weight"] == [256, 8, 3, 3]
    assert got["backbone.body.layer3.22.conv2.weight"] == [1024, 32, 3, 3]
    assert got["backbone.body.layer4.2.conv2.weight"] == [2048, 64, 3, 3]


def test_small_resnext_matches_its_fixture():
    want = json.load(open(os.path.join(GOLD, "state_shapes_resnext50.json")))
    m = _build(_cfg())
    assert _shapes(m) == {k: v for k, v in want["shapes"].items() if "cell_anchors" not in k}
    body = lambda names: [k for k in names if k.startswith("backbone.")]   # noqa: E731
    assert body(k for k, p in m.named_parameters() if p.requires_grad) == body(want["trainable"])   # layer1 frozen, layer2-4 + FPN train


def test_num_groups_is_honoured_with_the_stride_in_the_1x1():
    """NUM_GROUPS 32 with the default STRIDE_IN_1X1 True used to build a dense 256-wide network without complaint"""
    m = _build(_cfg(in_1x1=True))
    assert tuple(m.backbone.body.layer1[0].conv2.weight.shape) == (256, 8, 3, 3)
    blk = m.backbone.body.layer2[0]
    assert blk.conv1.stride == (2, 2) and blk.conv2.stride == (1, 1) and blk.downsample[0].stride == (2, 2)
    blk = _build(_cfg(in_1x1=False)).backbone.body.layer2[0]
    assert blk.conv1.stride == (1, 1) and blk.conv2.stride == (2, 2) and blk.downsample[0].stride == (2, 2)


def test_dense_blocks_with_the_stride_in_the_3x3_still_raise():
    with pytest.raises(NotImplementedError, match="NUM_GROUPS=1 with STRIDE_IN_1X1=False"):
        _build(_cfg(groups=1, width=64, in_1x1=False))


def test_group_widths_without_a_kernel_raise():
    with pytest.raises(NotImplementedError, match="per group"):
        _build(_cfg(groups=32, width=4))   # 32x4d: Cg = 4


def test_default_config_is_unchanged(state_shapes):
    from maskrcnn_benchmark.config import make_default_cfg
    got = _shapes(_build(make_default_cfg()))
    assert got == {k: v for k, v in state_shapes["shapes"].items() if "cell_anchors" not in k}


def test_grouped_weight_round_trips_through_the_checkpointer(tmp_path):
    """a conv2.weight of the reference's shape (width, width // num_groups, 3, 3) is saved and loaded by utils/checkpoint.py"""
    from maskrcnn_benchmark.utils import checkpoint as ck
    from maskrcnn_benchmark.modeling.backbone.backbone import BottleneckWithFixedBatchNorm
    torch.manual_seed(3)
    a = BottleneckWithFixedBatchNorm(256, 512, 512, num_groups=32, stride_in_1x1=False, stride=2)
    assert tuple(a.conv2.weight.shape) == (512, 16, 3, 3)
    with torch.no_grad():
        a.conv2.weight.copy_(torch.randn(512, 16, 3, 3))
    d = str(tmp_path / "ck")
    os.makedirs(d)
    ck.Checkpointer(a, save_dir=d, save_to_disk=True).save("resnext_block")
    saved = torch.load(os.path.join(d, "resnext_block.pth"), map_location="cpu")["model"]
    assert tuple(saved["conv2.weight"].shape) == (512, 16, 3, 3)
    b = BottleneckWithFixedBatchNorm(256, 512, 512, num_groups=32, stride_in_1x1=False, stride=2)
    assert not torch.equal(a.conv2.weight, b.conv2.weight)
    ck.Checkpointer(b, save_dir=d).load(os.path.join(d, "resnext_block.pth"))
    for (n, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(p, q), n
    # a checkpoint as the reference writes it: plain contiguous tensors under the reference's names
    ref_like = {"model": {k: v.clone().contiguous() for k, v in a.state_dict().items()}}
    torch.save(ref_like, os.path.join(d, "ref_like.pth"))
    c = BottleneckWithFixedBatchNorm(256, 512, 512, num_groups=32, stride_in_1x1=False, stride=2)
    ck.Checkpointer(c, save_dir=d).load(os.path.join(d, "ref_like.pth"))
    assert torch.equal(c.conv2.weight, a.conv2.weight)
