"""Golden-vector generator for the CSPN mask head.  BUILD CONTAINER ONLY (needs the reference checkout).

Imports the reference through oracle/refharness/ref_import.py and records, next to this file,

  state_shapes_cspn.json   names and shapes of the detector's state dict, parameter order and trainable names, as the reference
                           builds it with the MODEL keys of configs/pap/CSPN.yaml (tests/cspn_formulation.py: CSPN_KEYS)
  cspn160.npz              the reference's own PRCNNFeatureExtractor + PRCNNPredictor + mask loss on the CPU (double precision) on
                           synthetic.make_labeled(2, 160, 4, seed=1234) with synthetic.make_weights(shapes, seed=0) and the boxes of
                           cspn_formulation.fixture_boxes: fixed index samples of the 480-channel pooled tensor and of the logits,
                           each with the largest magnitude of the whole tensor, the matcher's label per box, and loss_seg.  No
                           gradients: the reference's CPU ROIAlign has no backward.

Weights are never stored: the tests regenerate them from the shapes.  No reference source text is stored.

    python tests/golden/gen_golden_cspn.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from oracle.refharness.ref_import import load_reference  # noqa: E402
import cspn_formulation as cf  # noqa: E402
from gen_golden_resnext import _load_synth, sample_index, shapes_of  # noqa: E402


def main():
    synth = _load_synth()
    mb, make_cfg = load_reference()
    torch.set_num_threads(8)
    cfg = make_cfg(cf.CSPN_KEYS)
    shapes = shapes_of(cfg, "state_shapes_cspn.json", True)

    from maskrcnn_benchmark.modeling.roi_heads.mask_head.roi_mask_feature_extractors import make_roi_mask_feature_extractor
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.roi_mask_predictors import make_roi_mask_predictor
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.loss import make_roi_mask_loss_evaluator
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask
    from maskrcnn_benchmark.structures.image_list import to_image_list
    sd = synth.make_weights(shapes, seed=0)
    fe, pr = make_roi_mask_feature_extractor(cfg), make_roi_mask_predictor(cfg)
    assert type(fe).__name__ == "PRCNNFeatureExtractor" and type(pr).__name__ == "PRCNNPredictor"
    for mod, pre in ((fe, cf.PRE + "feature_extractor."), (pr, cf.PRE + "predictor.")):
        mod.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
    fe, pr = fe.double().eval(), pr.double().eval()
    imgs, tgs = synth.make_labeled(2, 160, 4, seed=1234)
    boxes = cf.fixture_boxes(tgs, 160)
    props = [BoxList(b.double(), t["size"], mode="xyxy") for b, t in zip(boxes, tgs)]
    targets = []
    for t in tgs:
        bl = BoxList(t["boxes"], t["size"], mode="xyxy")
        bl.add_field("labels", t["labels"])
        bl.add_field("masks", SegmentationMask([[p.tolist() for p in inst] for inst in t["polys"]], t["size"], mode="poly"))
        targets.append(bl)
    x = to_image_list(list(imgs), 32).tensors.double()
    for i in range(1, 5):   # (the reference's pooler builds fp32 rois whatever the map's type: widened, exactly, for the double pass)
        getattr(fe, "pooler%d" % i).poolers[0].register_forward_pre_hook(lambda m, a: (a[0], a[1].to(a[0].dtype)))
    pooled = {}
    hook = fe.posconv1.register_forward_pre_hook(lambda m, a: pooled.update(x=a[0].detach()))   # (returns None: the input stays)
    with torch.no_grad():
        feat, _ = fe(x, props)
        logits = pr(feat)
    hook.remove()
    ev = make_roi_mask_loss_evaluator(cfg)
    loss = ev([BoxList(b, t["size"], mode="xyxy") for b, t in zip(boxes, tgs)], logits.float(), targets)
    labels, _ = ev.prepare_targets([BoxList(b, t["size"], mode="xyxy") for b, t in zip(boxes, tgs)], targets)
    labels = torch.cat(labels)   # (per image from the reference)
    out = {"boxes": torch.stack(boxes).numpy(), "labels": labels.numpy(), "loss_seg": np.asarray(loss.item())}
    assert int((labels > 0).sum()) >= 8, labels
    for name, t in (("pooled", pooled["x"]), ("logits", logits)):
        idx = sample_index(t.numel(), "cspn:" + name)
        out[name + "_shape"] = np.asarray(t.shape)
        out[name + "_idx"] = idx.numpy()
        out[name + "_val"] = t.reshape(-1)[idx].numpy()
        out[name + "_max"] = np.asarray(t.abs().max().item())
    np.savez_compressed(os.path.join(HERE, "cspn160.npz"), **out)
    print("wrote cspn160", {k: (v.shape, float(np.abs(v).max())) for k, v in out.items() if k.endswith("val")}, out["loss_seg"], out["labels"])


if __name__ == "__main__":
    main()
