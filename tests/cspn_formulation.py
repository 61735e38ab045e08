"""Plain-torch restatement of the CSPN mask head (reference modeling/roi_heads/mask_head/roi_mask_feature_extractors.py:9-88,
roi_mask_predictors.py:39-53, configs/pap/CSPN.yaml) on the CPU: `F.conv2d`, `F.max_pool2d` and the oracle's C ROIAlign behind its
autograd function.  tests/test_cspn_config.py checks it against the reference's own outputs (tests/golden/cspn160.npz, which holds
no gradients: the reference's CPU ROIAlign has no backward); tests/test_cspn_model_gpu.py takes its gradients as the yardstick.
Also here: the model keys of CSPN.yaml and the fixed boxes both the fixture generator and the tests pool."""
import torch
import torch.nn.functional as F

from oracle import model as om
from oracle import native

PRE = "mask_heads.mask."
WIDTHS = (32, 64, 128, 256)
SCALES = (1.0, 0.5, 0.25, 0.125)
RES = 25
PRCNN_NAMES = ["feature_extractor.conv%d" % i for i in range(1, 9)] + ["feature_extractor.posconv1", "feature_extractor.posconv2",
                                                                       "predictor.mask_fcn_logits"]

# configs/pap/CSPN.yaml, the MODEL keys that differ from configs/pap/e2e_mask_rcnn_R_50_FPN_1x.yaml
CSPN_KEYS = ["MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "PRCNNFeatureExtractor", "MODEL.ROI_MASK_HEAD.PREDICTOR", "PRCNNPredictor",
             "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 25, "MODEL.ROI_MASK_HEAD.RESOLUTION", 25,
             "MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False,
             "MODEL.RELATION_MASK.TYPE", "LIAM", "MODEL.RELATION_MASK.USE_RELATION", False]


def apply_keys(cfg, keys=CSPN_KEYS):
    """set dotted keys on a config node (the product's or the reference's)"""
    for k, v in zip(keys[0::2], keys[1::2]):
        node = cfg
        parts = k.split(".")
        for p in parts[:-1]:
            node = getattr(node, p)
        setattr(node, parts[-1], v)
    return cfg


def fixture_boxes(targets, size):
    """per image 24 fixed boxes: five shifted / scaled copies of each of the four ground-truth boxes (positives and near misses of
    the 0.5 matcher), three boxes that hang over the image border (one of them larger than the image) and one sub-pixel box"""
    jit = [(0.0, 0.0, 1.0), (1.5, -1.0, 1.1), (-2.0, 0.75, 0.9), (0.25, 2.5, 1.25), (-0.5, -0.5, 0.6)]
    out = []
    for n, t in enumerate(targets):
        bs = []
        for b in t["boxes"].tolist():
            cx, cy, w, h = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2, b[2] - b[0], b[3] - b[1]
            for dx, dy, s in jit:
                bs.append([cx + dx - s * w / 2, cy + dy - s * h / 2, cx + dx + s * w / 2, cy + dy + s * h / 2])
        bs.append([-7.5, -3.25, 21.0 + n, 30.5])
        bs.append([size - 20.5, size - 31.0, size + 9.0, size + 4.5 + n])
        bs.append([-12.0, -9.0, size + 15.0, size + 6.0])
        bs.append([40.3 + n, 71.6, 40.7 + n, 71.9])
        out.append(torch.tensor(bs, dtype=torch.float32))
    return out


def rois_of(boxes):
    return torch.cat([torch.cat([torch.full((len(b), 1), float(i)), b], 1) for i, b in enumerate(boxes)], 0)


def pool_choices(ms):
    """ATen's choice (first maximum in scan order) for every window of the three pools, from the pair outputs `ms`"""
    return [F.max_pool2d(m.detach(), 3, 2, 1, return_indices=True)[1] for m in ms[:3]]


def _pool(x, choice):
    """MaxPool2d(3, 2, 1); with `choice` (flat h * W + w indices per window) the given elements are taken instead, which is allowed
    only where they tie with the window's maximum to within fp32 rounding (2e-6 of the value): the order of two fp32 neighbours is
    a decision the arithmetic does not fix, and a yardstick in double would otherwise take the other side of it than an fp32 run"""
    own, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    if choice is None or torch.equal(choice, idx):
        return own
    taken = x.flatten(2).gather(2, choice.flatten(2)).view_as(own)
    other = choice != idx
    gap = (own - taken).detach()[other]
    assert (gap <= 2e-6 * own.detach()[other].abs()).all(), ("a replayed pool choice that is no fp32 tie", gap.max().item())
    return taken


def maps(sd, x, pre=PRE, choices=None):
    """the four pair outputs of conv1..conv8 on the image batch x (N, 3, H, W); choices: see _pool"""
    fe = pre + "feature_extractor."
    out = []
    for i in range(4):
        if i:
            x = _pool(x, choices[i - 1] if choices is not None else None)
        for j in (2 * i + 1, 2 * i + 2):
            x = F.relu(F.conv2d(x, sd[fe + "conv%d.weight" % j], sd[fe + "conv%d.bias" % j], 1, 1))
        out.append(x)
    return out


def head(sd, x, boxes, sr=2, pre=PRE, choices=None):
    """-> (pooled (K, 480, 25, 25), extractor output (K, 32, 25, 25), logits (K, 3, 25, 25)); differentiable w.r.t. sd's tensors"""
    rois = rois_of(boxes).to(x.dtype)
    pooled = torch.cat([native.roi_align(m, rois, (RES, RES), s, sr) for m, s in zip(maps(sd, x, pre, choices), SCALES)], 1)
    fe = pre + "feature_extractor."
    y = F.relu(F.conv2d(pooled, sd[fe + "posconv1.weight"], sd[fe + "posconv1.bias"], 1, 1))
    y = F.conv2d(y, sd[fe + "posconv2.weight"], sd[fe + "posconv2.bias"], 1, 1)
    p = pre + "predictor.mask_fcn_logits."
    return pooled, y, F.conv2d(F.relu(y), sd[p + "weight"], sd[p + "bias"])


def mask_loss(logits, boxes, targets):
    """mask_head/loss.py:119-180 at 25 x 25 on ALL boxes: the matcher's positives carry the loss"""
    cfg = om.default_cfg(mask_out=RES)
    props = [om.Boxes(b, t["size"]) for b, t in zip(boxes, targets)]
    tg = [om.Boxes(t["boxes"], t["size"], {"labels": t["labels"], "masks": t["polys"]}) for t in targets]
    return om.mask_loss(cfg, props, logits, tg)


def matched_labels(boxes, targets):
    """the matcher's label per box (0: not a positive), per image"""
    out = []
    for b, t in zip(boxes, targets):
        m = om.matcher(om.box_iou(om.Boxes(t["boxes"], t["size"]), om.Boxes(b, t["size"])), 0.5, 0.5, False)
        lab = t["labels"][m.clamp(min=0)].to(torch.int64)
        lab[m == -1] = 0
        out.append(lab)
    return out
