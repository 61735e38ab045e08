"""CPU tests of test-time augmentation: the fp64 formulation of the two merges (tests/tta_formulation.py), the identity the
regression merge rests on, the configuration keys and the host-side refusals that need no GPU."""
import pytest
import torch

import tta_formulation as F


def _boxes(n, W, H, g):
    """n boxes inside a W x H image in the +1 convention: random ones, width-1 and height-1 boxes (x1 == x2), boxes on every
    border, and the whole image"""
    x1 = torch.rand(n, generator=g, dtype=torch.float64) * (W - 1)
    y1 = torch.rand(n, generator=g, dtype=torch.float64) * (H - 1)
    x2 = x1 + torch.rand(n, generator=g, dtype=torch.float64) * (W - 1 - x1)
    y2 = y1 + torch.rand(n, generator=g, dtype=torch.float64) * (H - 1 - y1)
    b = torch.stack((x1, y1, x2, y2), 1)
    b[0:100, 2] = b[0:100, 0]            # width 1
    b[100:150, 3] = b[100:150, 1]        # height 1
    b[150:200, 0] = 0.0                  # left border
    b[200:250, 2] = W - 1.0              # right border
    b[250:275, 0], b[250:275, 2] = 0.0, 0.0                  # width 1 on the left border
    b[275:300, 0], b[275:300, 2] = W - 1.0, W - 1.0          # width 1 on the right border
    b[300] = torch.tensor([0.0, 0.0, W - 1.0, H - 1.0], dtype=torch.float64)
    b = torch.floor(b * 8) / 8           # a 1/8-pixel grid: exact in fp32 too (BoxList's dtype), x2 >= x1 kept
    return b


@pytest.mark.parametrize("size", [(1333, 800), (160, 160), (7, 5)])
def test_negating_dx_is_decoding_on_the_mirrored_proposal(size):
    """the regression merge: for a mirrored view, decoding its code on the mirrored proposal and mirroring the box back equals
    decoding the code with dx negated on the proposal itself -- with the repository's own flip (batch_boxlist_hflip:
    x1' = W - 1 - x2) and box coder, fp64, before clipping, to 1e-9"""
    from maskrcnn_benchmark.modeling.box_coder import BoxCoder
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.utils.miscellaneous import batch_boxlist_hflip
    W, H = size
    g = torch.Generator().manual_seed(7)
    n, C = 1000, 3
    boxes = _boxes(n, W, H, g)
    codes = torch.randn((n, 4 * C), generator=g, dtype=torch.float64) * torch.tensor([3.0, 3.0, 1.5, 1.5], dtype=torch.float64).repeat(C)
    coder = BoxCoder(weights=(10., 10., 5., 5.))
    # BoxList holds fp32: the proposals sit on a 1/8-pixel grid, where batch_boxlist_hflip is exact, so its result IS the fp64
    # mirror image; the decoded boxes (off the grid) are mirrored back by the same expression in fp64
    mirrored = batch_boxlist_hflip([BoxList(boxes, (W, H), "xyxy")])[0].bbox.to(torch.float64)

    def hflip64(b):
        return torch.stack((W - 1 - b[:, 2], b[:, 1], W - 1 - b[:, 0], b[:, 3]), 1)

    assert torch.equal(mirrored, hflip64(boxes))                      # the repository's convention: x1' = W - 1 - x2
    dec_m = coder.decode(codes, mirrored)                             # on the mirrored proposal ...
    back = hflip64(dec_m.reshape(-1, 4)).reshape(n, 4 * C)            # ... and mirrored back
    s = torch.ones(4 * C, dtype=torch.float64)
    s[0::4] = -1.0
    direct = coder.decode(codes * s, boxes)
    assert float((back - direct).abs().max()) <= 1e-9
    # the mutants the kernel tests name are not the identity: no negation, negating dw instead
    assert float((coder.decode(codes, boxes) - back).abs().max()) > 1e-3
    s2 = torch.ones(4 * C, dtype=torch.float64)
    s2[2::4] = -1.0
    assert float((coder.decode(codes * s2, boxes) - back).abs().max()) > 1e-3


@pytest.mark.parametrize("w,h,wpad", [(150, 150, 160), (140, 130, 160), (1000, 1000, 1024), (160, 160, 160)])
def test_padded_mirror_boxes_cover_the_mirrored_pixels(w, h, wpad):
    """ImageList.hflip() mirrors the whole zero-padded batch tensor.  batch_boxlist_hflip_padded gives the boxes that cover, in the
    mirrored tensor, the mirror image of what they cover in the tensor, pixel for pixel; mirroring about the image's own width
    (batch_boxlist_hflip) is off by wpad - w pixels and agrees only without padding"""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.image_list import ImageList
    from maskrcnn_benchmark.utils.miscellaneous import batch_boxlist_hflip, batch_boxlist_hflip_padded
    g = torch.Generator().manual_seed(w + h)
    t = torch.zeros((1, 1, 32 * ((h + 31) // 32), wpad))
    t[:, :, :h, :w] = torch.rand((1, 1, h, w), generator=g) + 1.0           # (content > 0, padding 0)
    il = ImageList(t.clone(), [(h, w)])
    il.hflip()
    x1 = torch.randint(0, w, (64,), generator=g)
    x2 = torch.minimum(x1 + torch.randint(0, 40, (64,), generator=g), torch.tensor(w - 1))
    y1 = torch.randint(0, h, (64,), generator=g)
    y2 = torch.minimum(y1 + torch.randint(0, 40, (64,), generator=g), torch.tensor(h - 1))
    x1[0], x2[0], x1[1], x2[1] = 0, 0, w - 1, w - 1                           # width 1 on either border
    b = BoxList(torch.stack((x1, y1, x2, y2), 1).float(), (w, h), "xyxy")
    b.add_field("scores", torch.arange(64.0))
    m = batch_boxlist_hflip_padded([b], wpad)[0]
    assert m.size == (w, h) and m.mode == "xyxy" and torch.equal(m.get_field("scores"), b.get_field("scores"))
    assert torch.equal(m.bbox[:, 0], wpad - 1 - b.bbox[:, 2]) and torch.equal(m.bbox[:, [1, 3]], b.bbox[:, [1, 3]])
    own = batch_boxlist_hflip([b])[0]
    n_own = 0
    for k in range(64):
        a = [int(v) for v in b.bbox[k]]
        c = [int(v) for v in m.bbox[k]]
        o = [int(v) for v in own.bbox[k]]
        src = t[0, 0, a[1]:a[3] + 1, a[0]:a[2] + 1]
        assert torch.equal(il.tensors[0, 0, c[1]:c[3] + 1, c[0]:c[2] + 1], torch.flip(src, (1,)))
        n_own += int(torch.equal(il.tensors[0, 0, o[1]:o[3] + 1, o[0]:o[2] + 1], torch.flip(src, (1,))))
    assert n_own == (64 if wpad == w else 0)
    assert torch.equal(batch_boxlist_hflip_padded([b.convert("xywh")], wpad)[0].convert("xyxy").bbox, m.bbox)


def test_one_view_and_duplicate_views_are_the_view_itself():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn((1, 37, 3), generator=g, dtype=torch.float64) * 4
    reg = torch.randn((1, 37, 12), generator=g, dtype=torch.float64)
    p1, r1 = F.merge_box(logits, reg, [False])
    assert torch.equal(p1, torch.softmax(logits[0], 1)) and torch.equal(r1, reg[0])
    p2, r2 = F.merge_box(logits.repeat(2, 1, 1), reg.repeat(2, 1, 1), [False, False])
    assert torch.equal(p2, p1) and torch.equal(r2, r1)                 # (a + a) / 2 == a
    ml = torch.randn((1, 5, 3, 7, 7), generator=g, dtype=torch.float64) * 4
    lab = torch.tensor([1, 2, 0, 1, 2])
    m1 = F.merge_mask(ml, lab, [False])
    assert torch.equal(m1, torch.sigmoid(ml[0][torch.arange(5), lab]))
    assert torch.equal(F.merge_mask(ml.repeat(2, 1, 1, 1, 1), lab, [False, False]), m1)
    # a mirrored view is read right to left; a mirrored pair of a symmetric input is again the view
    assert torch.equal(F.merge_mask(ml, lab, [True]), torch.flip(m1, (2,)))
    both = torch.cat([ml, torch.flip(ml, (4,))], 0)
    assert torch.equal(F.merge_mask(both, lab, [False, True]), m1)
    pm, rm = F.merge_box(logits, reg, [True])
    assert torch.equal(pm, p1) and torch.equal(rm[:, 0::4], -reg[0][:, 0::4]) and torch.equal(rm[:, 1::4], reg[0][:, 1::4])


def test_formulation_edges():
    logits = torch.zeros((3, 4, 2), dtype=torch.float64)
    logits[1, 2, 0] = float("nan")
    logits[0, 0] = torch.tensor([100.0, -100.0])
    logits[1, 0] = torch.tensor([100.0, -100.0])
    logits[2, 0] = torch.tensor([100.0, -100.0])
    p, _ = F.merge_box(logits, torch.zeros((3, 4, 8), dtype=torch.float64), [False, True, False])
    assert torch.isnan(p[2]).all() and not torch.isnan(p[[0, 1, 3]]).any()
    assert float(p[0, 0]) == 1.0 and 0.0 <= float(p[0, 1]) < 1e-80
    ml = torch.full((2, 3, 2, 4, 4), 100.0, dtype=torch.float64)
    m = F.merge_mask(ml, torch.tensor([-1, 1, 2]), [False, True])
    assert torch.isnan(m[0]).all() and torch.isnan(m[2]).all() and bool((m[1] == 1.0).all())
    assert bool((F.merge_mask(-ml, torch.tensor([0, 1, 0]), [False, True]) < 1e-40).all())


def test_config_keys_and_binding():
    from maskrcnn_benchmark import _hip
    from maskrcnn_benchmark.config import make_default_cfg
    cfg = make_default_cfg()
    assert cfg.TEST.TTA is False and cfg.TEST.TTA_FLIP is True and cfg.TEST.TTA_VIEWS == 1
    assert {"mmt_tta_merge_box", "mmt_tta_merge_mask"} <= set(_hip.exported_symbols())
    assert _hip.TTA_MAX_VIEWS == 8
    assert _hip._tta_flip_mask([False, True, True], 3) == 6
    with pytest.raises(ValueError):
        _hip._tta_flip_mask([False] * 9, 9)
    with pytest.raises(ValueError):
        _hip._tta_flip_mask([False], 2)
    with pytest.raises(RuntimeError):      # no CPU fall-back
        _hip.tta_merge_box(torch.zeros(1, 2, 3), torch.zeros(1, 2, 12), [False])
    with pytest.raises(RuntimeError):
        _hip.tta_merge_mask(torch.zeros(1, 2, 3, 4, 4), torch.zeros(2, dtype=torch.int64), [False])


def test_forward_tta_refuses_training_mode():
    """eval mode only: ValueError before anything is computed (no GPU needed to be told so)"""
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    model = build_detection_model(make_default_cfg())
    model.train()
    with pytest.raises(ValueError, match="eval"):
        model.forward_tta([torch.zeros(1, 3, 64, 64)])
    with pytest.raises(ValueError, match="eval"):
        model(torch.zeros(1, 3, 64, 64), tta=True)
    model.eval()
    with pytest.raises(NotImplementedError, match="TTA_VIEWS"):
        model.forward_tta([torch.zeros(1, 3, 64, 64)] * 5, flip=True)        # V = 10
    with pytest.raises(NotImplementedError, match="differing shapes"):
        model.forward_tta([torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 96)])
