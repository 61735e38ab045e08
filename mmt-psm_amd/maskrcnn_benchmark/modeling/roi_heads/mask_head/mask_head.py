"""Mask head (reference: modeling/roi_heads/mask_head/{mask_head,roi_mask_feature_extractors,
roi_mask_predictors,loss,inference}.py).

Module tree kept: feature_extractor.mask_fcn{1-4}, predictor.conv5_mask (2x2 s2 deconv) / mask_fcn_logits; with the CSPN keys
(configs/pap/CSPN.yaml) feature_extractor.conv{1-8} / posconv{1,2} on the image and predictor.mask_fcn_logits.
The two per-ROI CPU Python loops of the reference are single launches here:
  * mask targets  (project_masks_on_boxes + pycocotools rasteriser)  -> `mmt_polygon_targets`
  * teacher pseudo-mask (Masker.paste_mask_in_image per detection)     -> `mmt_paste_masks`
"""
import torch
from torch import nn

from maskrcnn_benchmark import _hip as H
from maskrcnn_benchmark.layers import Conv2d, ConvTranspose2d, fused
from maskrcnn_benchmark.modeling.matcher import Matcher
from maskrcnn_benchmark.modeling.poolers import Pooler
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.boxlist_ops import boxlist_iou, boxlist_mask_nms
from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList
from maskrcnn_benchmark.utils.miscellaneous import dev_ints
from maskrcnn_benchmark.modeling.relation.mask_relation_module import MaskRelationRefineNet


def keep_only_positive_boxes(boxes):
    pos_boxes, pos_inds = [], []
    for b in boxes:
        m = b.get_field("labels") > 0
        n_pos = getattr(b, "n_pos", None)  # set by the box head's sampler: no blocking nonzero here
        na = getattr(b, "n_pos_async", None)
        if n_pos is None and na is not None:
            # round 6 (SURVEY f-2): the count left the device through a pinned buffer when the sampler ran; everything the box head
            # does with the sampled lists has been queued in between -- the wait here is for work long done
            na[1].synchronize()
            n_pos = int(na[0][na[2]])
        pos_boxes.append(b[torch.nonzero_static(m, size=n_pos).squeeze(1) if n_pos is not None else m.nonzero().squeeze(1)])
        pos_inds.append(m)
    return pos_boxes, pos_inds


class MaskRCNNFPNFeatureExtractor(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        m = cfg.MODEL.ROI_MASK_HEAD
        self.pooler = Pooler((m.POOLER_RESOLUTION, m.POOLER_RESOLUTION), m.POOLER_SCALES, m.POOLER_SAMPLING_RATIO)
        nxt = cfg.MODEL.BACKBONE.OUT_CHANNELS
        self.blocks = []
        for i, ch in enumerate(m.CONV_LAYERS, 1):
            c = Conv2d(nxt, ch, 3, stride=1, padding=1)
            nn.init.kaiming_normal_(c.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(c.bias, 0)
            self.add_module("mask_fcn%d" % i, c)
            self.blocks.append("mask_fcn%d" % i)
            nxt = ch

    def forward(self, x, proposals):
        x = self.pooler(x, proposals)
        pre = x
        for i, name in enumerate(self.blocks):
            # (round 6: a layer's output feeds the next 3x3 layer, its input gradient the previous one's data gradient -- both
            # plane-fed launches: the producing epilogues write the planes)
            x = getattr(self, name)(x, relu=True, input_relu=(i > 0), out_rb=(i + 1 < len(self.blocks)), din_rb=(i > 0))
        return x, pre


class MaskRCNNC4Predictor(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        nc = cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES
        dim = cfg.MODEL.ROI_MASK_HEAD.CONV_LAYERS[-1]
        self.conv5_mask = ConvTranspose2d(dim, dim, 2, 2, 0)
        self.mask_fcn_logits = Conv2d(dim, nc, 1, 1, 0)
        for name, p in self.named_parameters():
            if "bias" in name:
                nn.init.constant_(p, 0)
            else:
                nn.init.kaiming_normal_(p, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        x = self.conv5_mask(x, relu=True, input_relu=True)
        return self.mask_fcn_logits(x, relu=False, input_relu=True)


class PRCNNFeatureExtractor(nn.Module):
    """The CSPN second stage (roi_mask_feature_extractors.py:9-88; configs/pap/CSPN.yaml): four pairs of 3x3 convolutions on the
    normalised IMAGE, a 3x3 / 2 max pool between the pairs, every proposal pooled at 25 x 25 from the four pair outputs (scales 1,
    1/2, 1/4, 1/8; no level mapping) into one 480-channel tensor -- one launch, `fused.RoiAlignMapsFn` --, then posconv1 (+ ReLU) and
    posconv2 (its ReLU belongs to the predictor).  Gradient routing: a pair's output y is a fused-ReLU output with two consumers,
    the pool (whose backward kernel has the (y > 0) mask fused in: fused.MaxPoolFn) and the ROIAlign (reached through
    `fused.relu_grad_mask`), so the convolution nodes receive the masked gradient they expect."""
    WIDTHS = (32, 64, 128, 256)
    RES = 25

    def __init__(self, cfg):
        super().__init__()
        self._refuse_bf16()
        self.sampling_ratio = cfg.MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO
        self.scales = (1.0, 0.5, 0.25, 0.125)
        nxt = 3
        for i, ch in enumerate(self.WIDTHS):
            self.add_module("conv%d" % (2 * i + 1), Conv2d(nxt, ch, 3, stride=1, padding=1))
            self.add_module("conv%d" % (2 * i + 2), Conv2d(ch, ch, 3, stride=1, padding=1))
            nxt = ch
        self.posconv1 = Conv2d(sum(self.WIDTHS), 256, 3, stride=1, padding=1)
        self.posconv2 = Conv2d(256, 32, 3, stride=1, padding=1)
        for i in range(1, 9):
            self._init(getattr(self, "conv%d" % i))
        self._init(self.posconv1)
        self._init(self.posconv2)

    @staticmethod
    def _refuse_bf16():
        """asked at construction and before every forward (the storage mode is a process-wide switch that may come later)"""
        if H.bf16_storage():
            raise NotImplementedError("MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR PRCNNFeatureExtractor is not offered with bf16 "
                                      "activation storage (its ROIAlign reads fp32 maps): set_bf16_storage(False)")

    @staticmethod
    def _init(layer):
        nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(layer.bias, 0)

    def maps(self, x):
        """the four pair outputs for the image batch x (N, 3, H, W)"""
        n, c, h, w = x.shape
        # RGB -> 4 channels with a zero weight slice (the kernels take Cin % 4 == 0); autograd slices conv1's weight gradient back.
        # Per forward this costs a copy of the image (N x H x W x 16 B: 33 MB at 2 x 1024^2, beside the 268 MB conv1 writes), a pad
        # and a layout copy of a 32 x 3 x 3 x 3 weight, and -- the padded weight being a new object every time -- conv1 never
        # finds a kept packed or flipped form (none is used: 4 input channels run on the fp32-input kernel, and the image asks for
        # no data gradient); its weight gradient is a fresh 4.6 KB tensor that autograd slices and adds into the flat buffer
        # instead of the kernel writing there.  Not timed on its own; a padded weight kept in the flat buffer would remove it
        x4 = x.new_zeros((n, h, w, 4))
        x4[..., :3] = x.permute(0, 2, 3, 1)
        w4 = torch.nn.functional.pad(self.conv1.weight, (0, 0, 0, 0, 0, 1)).contiguous(memory_format=torch.channels_last)
        y = fused.conv(x4.permute(0, 3, 1, 2), w4, self.conv1.bias, 1, 1, True, False)
        out = []
        for i in range(4):
            if i:
                y = getattr(self, "conv%d" % (2 * i + 1))(fused.maxpool3x3s2(y), relu=True, input_relu=False)
            y = getattr(self, "conv%d" % (2 * i + 2))(y, relu=True, input_relu=True)
            out.append(y)
        return out

    def forward(self, x, proposals):
        pre = x
        self._refuse_bf16()
        if all(b.mode == "xyxy" for b in proposals) and len(proposals) <= 32 and proposals[0].bbox.is_cuda:
            rois, _ = H.roi_format_levels([b.bbox for b in proposals])   # one launch (modeling/poolers.py)
        else:
            rois = Pooler.convert_to_roi_format(proposals)
        maps = [fused.relu_grad_mask(y) for y in self.maps(x)]
        x = fused.RoiAlignMapsFn.apply(rois, self.RES, self.scales, self.sampling_ratio, *maps)
        x = self.posconv1(x, relu=True, input_relu=False)
        return self.posconv2(x, relu=False, input_relu=True), pre


class PRCNNPredictor(nn.Module):
    """roi_mask_predictors.py:39-53: ReLU, then a 1x1 convolution 32 -> 3 (three classes, as the reference hard-codes them)"""

    def __init__(self, cfg):
        super().__init__()
        self.mask_fcn_logits = Conv2d(32, 3, 1, 1, 0)
        nn.init.constant_(self.mask_fcn_logits.bias, 0)
        nn.init.kaiming_normal_(self.mask_fcn_logits.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        # posconv2's output carries no fused ReLU: the ReLU here is an elementwise pass of torch's own (with its own backward), and
        # the 1x1 layer reads a plain tensor
        return self.mask_fcn_logits(torch.relu(x), relu=False, input_relu=False)


_ROI_MASK_FEATURE_EXTRACTORS = {"MaskRCNNFPNFeatureExtractor": MaskRCNNFPNFeatureExtractor, "PRCNNFeatureExtractor": PRCNNFeatureExtractor}
_ROI_MASK_PREDICTORS = {"MaskRCNNC4Predictor": MaskRCNNC4Predictor, "PRCNNPredictor": PRCNNPredictor}


class MaskRCNNLossComputation(object):
    def __init__(self, proposal_matcher, discretization_size, cfg=None):
        self.proposal_matcher, self.discretization_size, self.cfg = proposal_matcher, discretization_size, cfg

    def prepare_targets(self, proposals, targets):
        """-> labels (cat over images), mask targets (P, M, M) float -- mask_head/loss.py:119-149"""
        labels, mts = [], []
        pm = self.proposal_matcher
        dev = proposals[0].bbox.device
        fused_match = (dev.type == "cuda" and pm.high_threshold == pm.low_threshold and not pm.allow_low_quality_matches
                       and all(len(p) > 0 and len(t) > 0 for p, t in zip(proposals, targets)))
        if fused_match:
            # IoU + Matcher + label lookup of ALL images in one launch (`mmt_match_targets`, the box head's call): with equal
            # thresholds there is no BETWEEN_THRESHOLDS class, so its box-head labels (0 below the threshold, else the matched
            # ground truth's label) are exactly the labels of mask_head/loss.py:119-138
            N = len(proposals)
            A = [len(p) for p in proposals]
            coff, goff = [0], [0]
            for a, t in zip(A, targets):
                coff.append(coff[-1] + a)
                goff.append(goff[-1] + len(t))
            cand = torch.cat([p.bbox for p in proposals], 0) if N > 1 else proposals[0].bbox
            gt = torch.cat([t.bbox.to(dev) for t in targets], 0) if N > 1 else targets[0].bbox.to(dev)
            gl = torch.cat([t.get_field("labels").to(dev) for t in targets], 0) if N > 1 else targets[0].get_field("labels").to(dev)
            mt_all, lab_all, _ = H.match_targets(cand, dev_ints(coff, dev), gt, dev_ints(goff, dev), N,
                                                 pm.high_threshold, pm.low_threshold, False, gt_labels=gl, box_labels=True)
            mi_all = mt_all.clamp(min=0).long()
            pos_all = (lab_all > 0).to(torch.int32)[:, None]
        for i, (p, t) in enumerate(zip(proposals, targets)):
            if fused_match:
                mi, lab = mi_all[coff[i]:coff[i + 1]], lab_all[coff[i]:coff[i + 1]]
            else:
                m = pm(boxlist_iou(t, p))
                mi = m.clamp(min=0)
                lab = t.get_field("labels")[mi].to(torch.int64)
                lab = torch.where(m == Matcher.BELOW_LOW_THRESHOLD, torch.zeros_like(lab), lab)
            labels.append(lab)
            # every box handed to the mask head is already a positive of the same matcher (mask_head.py:74-78),
            # so `positive_inds` is all of them; non-positives (never produced) would get an all-zero range
            gt_masks = t.get_field("masks")
            if isinstance(gt_masks, BinaryMaskList):
                # bitmap ground truth: the matched instance's words cropped to the ROI's window and resampled to M x M in one
                # launch (`mmt_mask_words_targets`); -1 marks a non-positive, built on the device from what is already there
                pos = pos_all[coff[i]:coff[i + 1], 0] if fused_match else (lab > 0).to(torch.int32)
                roi_inst = (mi.to(torch.int32) + 1) * pos - 1
                words, _ = gt_masks.mask_words(p.bbox.device)
                mts.append(H.mask_words_targets(words, roi_inst, p.bbox, gt_masks.size[1], gt_masks.size[0], self.discretization_size))
                continue
            xy, poly_off, inst_rng = gt_masks.packed(p.bbox.device)
            rng = inst_rng[mi] * (pos_all[coff[i]:coff[i + 1]] if fused_match else (lab > 0).to(torch.int32)[:, None])
            mt, ovf = H.polygon_targets(xy, poly_off, rng, p.bbox, self.discretization_size)
            mts.append(mt)
        return torch.cat(labels, 0), torch.cat(mts, 0)

    def __call__(self, proposals, mask_logits, targets):
        labels, mask_targets = self.prepare_targets(proposals, targets)
        if mask_targets.numel() == 0:
            return mask_logits.sum() * 0
        self.last_targets = mask_targets
        return fused.MaskBCEFn.apply(mask_logits, labels, mask_targets)


def make_roi_mask_loss_evaluator(cfg):
    r = cfg.MODEL.ROI_HEADS
    return MaskRCNNLossComputation(Matcher(r.FG_IOU_THRESHOLD, r.BG_IOU_THRESHOLD, allow_low_quality_matches=False),
                                   cfg.MODEL.ROI_MASK_HEAD.RESOLUTION, cfg)


class MaskPostProcessor(nn.Module):
    """mask_head/inference.py:14-65: sigmoid prob of the predicted class, stored per image under 'mask'.
    mask_nms: the TEST.MASK_NMS node, or None.  When it is enabled, every image's detections go through `boxlist_mask_nms` on
    their M x M probabilities before the optional POSTPROCESS_MASKS paste, which then pastes the kept rows only.  Evaluation only:
    the caller says so per call (`mask_nms=`: ROIMaskHead passes False on the teacher's passes), and a pseudo-mask masker or a
    fixed-capacity list (`count_dev`) never takes it."""

    def __init__(self, masker=None, mask_nms=None):
        super().__init__()
        self.masker = masker
        self.mask_nms = None
        if mask_nms is not None and mask_nms.ENABLED:
            if mask_nms.MEASURE not in H.MASK_NMS_MEASURES:
                raise ValueError("TEST.MASK_NMS.MEASURE %r is not one of %s" % (mask_nms.MEASURE, sorted(H.MASK_NMS_MEASURES)))
            if not 0.0 < float(mask_nms.THRESH) <= 1.0:
                raise ValueError("TEST.MASK_NMS.THRESH %r is outside (0, 1]" % (mask_nms.THRESH,))
            self.mask_nms = dict(thresh=float(mask_nms.THRESH), measure=mask_nms.MEASURE, class_agnostic=bool(mask_nms.CLASS_AGNOSTIC),
                                 mask_threshold=getattr(masker, "threshold", 0.5))

    def forward(self, x, boxes, mask_nms=True):
        labels = torch.cat([b.get_field("labels") for b in boxes])
        per = [len(b) for b in boxes]
        if self.masker is not None and not isinstance(self.masker, DetectionMasker):
            return self._with_masks(self.masker(x, labels, boxes), boxes)
        prob = x.sigmoid()[torch.arange(x.shape[0], device=x.device), labels][:, None]
        return self._finish(prob.split(per, 0), boxes, mask_nms)

    def forward_prob(self, prob, boxes, mask_nms=True):
        """forward() from the (D, 1, M, M) probabilities of the predicted class (test-time augmentation merges them over its views)"""
        if self.masker is not None and not isinstance(self.masker, DetectionMasker):
            raise NotImplementedError("the integral pseudo-mask is pasted from logits: probabilities go through the evaluation "
                                      "post-processor only")
        return self._finish(prob.split([len(b) for b in boxes], 0), boxes, mask_nms)

    def _finish(self, segs, boxes, mask_nms):
        """per-image (D, 1, M, M) probabilities -> the lists with their `mask` field: mask NMS when it applies, then the
        POSTPROCESS_MASKS paste (inference.py:62-63: the same rows, pasted into their image)"""
        if self.mask_nms is None or not mask_nms or any(getattr(b, "count_dev", None) is not None for b in boxes):
            if self.masker is not None:
                segs = self.masker(segs, boxes)
            return self._with_masks(segs, boxes)
        out = [boxlist_mask_nms(b, **self.mask_nms) for b in self._with_masks(segs, boxes)]
        if self.masker is not None:
            for b, pasted in zip(out, self.masker([b.get_field("mask") for b in out], out)):
                b.add_field("mask", pasted)
        return out

    @staticmethod
    def _with_masks(segs, boxes):
        out = []
        for s, b in zip(segs, boxes):
            r = BoxList(b.bbox, b.size, "xyxy")
            for f in b.fields():
                r.add_field(f, b.get_field(f))
            r.add_field("mask", s)
            if getattr(b, "count_dev", None) is not None:
                r.count_dev = b.count_dev
            out.append(r)
        return out


class Masker(object):
    """Masker (mask_head/inference.py:209-246) in its only use on the path: the teacher's integral pseudo-mask.
    Returns, per image, an int32 (H, W) map = sum over detections of the pasted binary masks, i.e. exactly
    `t.get_field('mask').sum(0)[0]` of generalized_rcnn.py:129-132, without materialising D canvases."""

    def __init__(self, threshold=0.5, padding=1):
        assert padding == 1
        self.threshold, self.padding = threshold, padding

    def __call__(self, logits, labels, boxes):
        sizes = {b.size for b in boxes}
        if len(sizes) != 1:
            raise NotImplementedError("pseudo-mask paste expects equally sized images in a batch")
        w, h = boxes[0].size
        if all(getattr(b, "count_dev", None) is not None for b in boxes):
            # fixed-capacity detection lists (box_head.py::PostProcessor.forward): rows behind an image's count vote nowhere
            # (image index -1: the paste kernel returns at once)
            cap = len(boxes[0])
            counts = torch.cat([b.count_dev for b in boxes]) if len(boxes) > 1 else boxes[0].count_dev
            rows = torch.arange(cap, device=logits.device, dtype=torch.int32)[None, :]
            ids = torch.arange(len(boxes), device=logits.device, dtype=torch.int32)[:, None]
            img = torch.where(rows < counts[:, None], ids, torch.full_like(ids, -1)).reshape(-1).contiguous()
        else:
            img = torch.cat([torch.full((len(b),), i, dtype=torch.int32, device=logits.device) for i, b in enumerate(boxes)])
        bb = torch.cat([b.bbox for b in boxes], 0)
        seg = H.paste_masks(logits, labels, bb, img, len(boxes), h, w, self.threshold)
        return [IntegralMask(s) for s in seg]


    def forward_single_image(self, masks, boxes):
        """the reference's per-detection form (mask_head/inference.py:221-229), used by the evaluator on predictions whose `mask`
        field is still M x M: masks (n, 1, M, M) probabilities, boxes a BoxList in the target frame -> uint8 (n, 1, H, W)"""
        w, h = boxes.size
        if len(boxes) == 0:
            return torch.zeros((0, 1, h, w), dtype=torch.uint8, device=masks.device)
        return H.paste_mask_stack(masks, boxes.convert("xyxy").bbox, h, w, self.threshold)

    def rle_single_image(self, masks, boxes):
        """the run-length twin of forward_single_image: the list of RLE dicts that mask_rle.encode_device gives for its stack,
        byte for byte, pasted straight into the codec's words (`mmt_paste_mask_words`); zero detections give []"""
        from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
        w, h = boxes.size
        if len(boxes) == 0:
            return []
        return mask_rle.encode_pasted_device(masks, boxes.convert("xyxy").bbox, h, w, self.threshold)


class DetectionMasker(Masker):
    """Masker.__call__ of the reference (mask_head/inference.py:231-246) as MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS uses it: per
    image, the (D, 1, M, M) probabilities of the predicted class -> the uint8 (D, 1, h, w) stack of pasted binary masks, (w, h)
    the BoxList's size.  Images of one batch may differ in size."""

    def __call__(self, probs, boxes):
        return [self.forward_single_image(p, b) for p, b in zip(probs, boxes)]


class IntegralMask(object):
    """stands in for the (D,1,H,W) uint8 stack of the reference: `.sum(0)[0]` gives the integral mask"""

    def __init__(self, seg):
        self.seg = seg

    def sum(self, dim=0):
        assert dim == 0
        return [self.seg]


def make_roi_mask_post_processor(cfg):
    return MaskPostProcessor(DetectionMasker(cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD, 1)
                             if cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS else None,
                             mask_nms=cfg.TEST.MASK_NMS)


def make_roi_mask_generator(cfg):
    return MaskPostProcessor(Masker(cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD, 1))


class ROIMaskHead(nn.Module):
    def __init__(self, cfg, is_student=False):
        super().__init__()
        self.cfg = cfg.clone()
        m = cfg.MODEL.ROI_MASK_HEAD
        # a name that is not built raises KeyError (the reference's own lookup, roi_mask_feature_extractors.py:222-224)
        self.feature_extractor = _ROI_MASK_FEATURE_EXTRACTORS[m.FEATURE_EXTRACTOR](cfg)
        self.predictor = _ROI_MASK_PREDICTORS[m.PREDICTOR](cfg)
        self.on_image = m.FEATURE_EXTRACTOR == "PRCNNFeatureExtractor"   # mask_head.py:82-85: this extractor reads the image
        self.post_processor = make_roi_mask_post_processor(cfg)
        self.mask_generator = make_roi_mask_generator(cfg)
        self.loss_evaluator = make_roi_mask_loss_evaluator(cfg)
        # mask_head.py:49-50 builds the module whatever USE_RELATION says (`if cfg.MODEL.RELATION_MASK:` is a CfgNode),
        # so its keys are in every checkpoint; when unused it never gets a gradient there -> frozen here
        self.use_relation = cfg.MODEL.RELATION_MASK.USE_RELATION
        self.mask_relation_module = MaskRelationRefineNet(cfg, self.predictor)
        if not self.use_relation:
            self.mask_relation_module.requires_grad_(False)
        self.mode = None

    def set_teacher_mode(self, mode):
        self.mode = mode

    def forward(self, features, proposals, targets=None, images=None):
        all_proposals = proposals
        if self.training:
            proposals, _ = keep_only_positive_boxes(proposals)
        x, _ = self.feature_extractor(images.tensors if self.on_image else features, proposals)
        mask_logits = self.predictor(x)
        loss_1 = self.loss_evaluator(proposals, mask_logits, targets) if self.training else None
        if self.use_relation:
            # mask_head.py:98-127: per image, instances sorted per class by objectness, second logits from CIAM
            xr = fused.relu_grad_mask(x)  # x is a fused-ReLU output read by non-fused ops below
            if sum(len(p) for p in proposals) > 0:
                mask_logits, proposals = self.mask_relation_module.forward_batch(xr, mask_logits, proposals)
        if self.training:
            if self.use_relation:
                loss_2 = self.loss_evaluator(proposals, mask_logits, targets)
                loss_1 = 0.5 * (loss_1 + loss_2) if self.cfg.MODEL.RELATION_MASK.DEEP_SUPER else loss_2
            return x, all_proposals, dict(loss_seg=loss_1)
        # D8 of SURVEY.md: the reference hands a tuple to the post-processor here; the only semantics under which
        # the teacher produces a pseudo-mask is the concatenated logits, which is what `mask_logits` already is
        with torch.no_grad():
            if self.mode is None or self.mode == "train":
                # (mask NMS belongs to evaluation: mode "train" is the teacher's second pass)
                result = self.post_processor(mask_logits, proposals, mask_nms=self.mode is None)
            else:
                result = self.mask_generator(mask_logits, proposals)
        return x, result, {}

    def forward_views(self, pyramid, n, flips, detections, padded_width):
        """Eval pass over the views of one batched backbone pass (test-time augmentation): `pyramid` holds len(flips) views of n
        images each, image index = view * n + image; the detections -- for a mirrored view mirrored about `padded_width`, the width
        of the padded batch tensor, where ImageList.hflip() put their content -- are pooled from every view in ONE ROIAlign + mask_fcn + predictor
        pass, and the predicted class's probabilities are averaged over the views by one launch (csrc/tta.hip), mirrored views
        read right to left.
        -> (the detections with their `mask` field, the per-view logits (V, D, C, M, M) or None when nothing was detected)"""
        if self.training:
            raise ValueError("ROIMaskHead.forward_views is an eval-mode pass")
        if self.use_relation:
            raise NotImplementedError("MODEL.RELATION_MASK.USE_RELATION is not offered with test-time augmentation")
        if self.on_image:
            raise NotImplementedError("MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR PRCNNFeatureExtractor is not offered with test-time "
                                      "augmentation")
        from maskrcnn_benchmark.utils.miscellaneous import batch_boxlist_hflip_padded
        V, D = len(flips), sum(len(d) for d in detections)
        if len(detections) != n or pyramid[0].shape[0] != V * n:
            raise ValueError("forward_views: %d detection lists and a pyramid of %d images for %d views of %d images"
                             % (len(detections), pyramid[0].shape[0], V, n))
        M = self.cfg.MODEL.ROI_MASK_HEAD.RESOLUTION
        with torch.no_grad():
            if D == 0:   # nothing to pool: empty fields, no launch
                dev = detections[0].bbox.device
                return self.post_processor.forward_prob(torch.zeros((0, 1, M, M), dtype=torch.float32, device=dev), detections,
                                                        mask_nms=False), None
            mirrored = batch_boxlist_hflip_padded(detections, padded_width) if any(flips) else None
            boxes = []
            for f in flips:
                boxes += list(mirrored if f else detections)
            x, _ = self.feature_extractor(pyramid, boxes)
            logits = self.predictor(x)                                  # (V * D, C, M, M), NHWC memory
            logits = logits.contiguous().view(V, D, logits.shape[1], logits.shape[2], logits.shape[3])
            labels = torch.cat([d.get_field("labels") for d in detections])
            prob = H.tta_merge_mask(logits, labels, flips)
            return self.post_processor.forward_prob(prob, detections, mask_nms=self.mode is None), logits


def build_roi_mask_head(cfg, is_student=False):
    return ROIMaskHead(cfg, is_student)
