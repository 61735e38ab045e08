"""MODEL.BACKBONE.FREEZE_CONV_BODY_AT 0 / 1 / 2 on the host (no GPU): the requires_grad sets are the reference's rule
(modeling/backbone/resnet.py:105-115: stage 0 is the stem, stage k is layerk, the stages below the key are frozen; FrozenBatchNorm
holds buffers), the flat parameter buffer lays the stem weight out with the trainable weights, and the bucketed gradient all-reduce
covers every trainable element exactly once."""
import pytest
import torch

STEM = "backbone.body.stem.conv1.weight"


def _model(freeze_at):
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    cfg = make_default_cfg()
    cfg.merge_from_list(["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", freeze_at])
    torch.manual_seed(0)
    return build_detection_model(cfg, is_student=True)


def _reference_rule(names, freeze_at):
    """the names the reference leaves trainable, from the default's list (state_shapes.json was written by the reference at 2)"""
    frozen = ["backbone.body.stem."] + ["backbone.body.layer%d." % k for k in range(1, 5)]
    return {n for n in names if not any(n.startswith(p) for p in frozen[:freeze_at])}


@pytest.mark.parametrize("freeze_at", [0, 1, 2])
def test_requires_grad_sets_follow_the_reference(state_shapes, freeze_at):
    m = _model(freeze_at)
    params = dict(m.named_parameters())
    assert list(params) == state_shapes["param_order"]
    got = {n for n, p in params.items() if p.requires_grad}
    # (the reference builds mask_relation_module even when it is off, mask_head.py:49; it never receives a gradient there and is
    # kept out of the flat optimiser by freezing it: tests/test_host_logic.py)
    at2 = {n for n in state_shapes["trainable"] if "mask_relation_module" not in n}
    body = {n for n in params if n.startswith("backbone.body.")}
    # outside the body nothing depends on the key; inside it the reference's rule decides
    assert got - body == at2 - body
    assert got & body == _reference_rule(body, freeze_at)
    extra = sorted(got - at2)
    if freeze_at == 2:
        assert extra == []
    else:
        layer1 = sorted(n for n in params if n.startswith("backbone.body.layer1."))
        assert len(layer1) == 10 and all(n.endswith(".weight") and params[n].dim() == 4 for n in layer1)
        assert extra == sorted(layer1 + ([STEM] if freeze_at == 0 else []))
    assert m.backbone.body.stem.follows_updates == (freeze_at == 0)


def test_flat_buffer_and_bucketed_exchange_at_0():
    from maskrcnn_benchmark.engine.flat import FlatParams
    from maskrcnn_benchmark.engine.MTtrainer import BucketedAllReduce
    m = _model(0)
    flat = FlatParams(m)
    o, k = flat.index[STEM]
    assert k == 64 * 3 * 7 * 7 and o + k <= flat.n_weights            # in the trainable weights region
    p = m.backbone.body.stem.conv1.weight
    assert p.grad is not None and p._flat_grad.data_ptr() == flat.grad[o:o + k].data_ptr()
    assert p._flat_ref() is flat
    # the same model at the default keeps it in the frozen region, without a gradient slot
    m2 = _model(2)
    f2 = FlatParams(m2)
    assert f2.index[STEM][0] >= f2.n_trainable and m2.backbone.body.stem.conv1.weight.grad is None
    # stage pieces + fixed remainder: every trainable element exactly once
    b = BucketedAllReduce(flat, m.backbone.body)
    cover = torch.zeros(flat.grad.numel(), dtype=torch.int32)
    for lo, hi in list(b.pieces.values()) + list(b.rest):
        assert 0 <= lo < hi <= cover.numel()
        cover[lo:hi] += 1
    assert bool((cover == 1).all()), (int(cover.min()), int(cover.max()))
    assert cover.numel() == flat.n_trainable
    # the stem and layer1 weights travel in the remainder (no stage hook says when they are final)
    lo1, k1 = flat.index["backbone.body.layer1.0.conv1.weight"]
    assert any(lo <= o and o + k <= hi for lo, hi in b.rest) and any(lo <= lo1 and lo1 + k1 <= hi for lo, hi in b.rest)
