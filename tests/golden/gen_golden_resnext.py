"""Golden-vector generator for the ResNeXt backbones.  BUILD CONTAINER ONLY (needs the reference checkout).

Imports the reference through oracle/refharness/ref_import.py and records, next to this file,

  state_shapes_x101.json       names and shapes of the X-101-32x8d-FPN detector's state dict (R-101-FPN, NUM_GROUPS 32,
                               WIDTH_PER_GROUP 8, STRIDE_IN_1X1 False) as the reference builds it
  state_shapes_resnext50.json  the same for R-50-FPN with the same ResNeXt keys (the small model of the GPU tests), plus parameter
                               order and the trainable names like state_shapes.json
  resnext160.npz               the reference's own CPU backbone (double precision) of the small model on
                               synthetic.make_labeled(2, 160, 4, seed=1234) with synthetic.make_weights(shapes, seed=0): fixed index
                               samples of the five pyramid levels and, for the loss sum_l <P_l, R_l> with R_l = grouped_formulations.level_weights(l, shape),
                               of the gradients of conv1 / conv2 / conv3 / downsample.0 of block 0 of layer2-4 and of fpn_inner2,
                               each with the largest magnitude of the whole tensor (the tolerance is relative to it)

Weights are never stored: the tests regenerate them from the shapes.  No reference source text is stored.

    python tests/golden/gen_golden_resnext.py
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.refharness.ref_import import load_reference  # noqa: E402
from grouped_formulations import level_weights  # noqa: E402

RESNEXT_KEYS = ["MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.STRIDE_IN_1X1", False,
                "MODEL.BACKBONE.FREEZE_CONV_BODY_AT", 2]
N_SAMPLES = 2048
GRAD_NAMES = ["body.layer%d.0.%s.weight" % (l, c) for l in (2, 3, 4) for c in ("conv1", "conv2", "conv3", "downsample.0")] + \
             ["fpn.fpn_inner2.weight"]


def _load_synth():
    spec = importlib.util.spec_from_file_location("synthetic", os.path.join(ROOT, "mmt-psm_amd", "synthetic.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def sample_index(numel, tag):
    """fixed sample of a tensor's flat (NCHW-contiguous) index range"""
    g = torch.Generator().manual_seed(zlib_crc(tag))
    n = min(N_SAMPLES, numel)
    return torch.randperm(numel, generator=g)[:n].sort().values


def zlib_crc(s):
    import zlib
    return zlib.crc32(s.encode()) & 0x7FFFFFFF


def shapes_of(cfg, path, with_order):
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    torch.manual_seed(0)
    m = build_detection_model(cfg, is_student=True)
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    out = {"shapes": shapes}
    if with_order:
        out["param_order"] = [k for k, _ in m.named_parameters()]
        out["trainable"] = [k for k, p in m.named_parameters() if p.requires_grad]
    with open(os.path.join(HERE, path), "w") as f:
        json.dump(out, f)
    print("wrote", path, len(shapes), "entries")
    return shapes


def main():
    synth = _load_synth()
    mb, make_cfg = load_reference()
    torch.set_num_threads(8)
    shapes_of(make_cfg(["MODEL.BACKBONE.CONV_BODY", "R-101-FPN"] + RESNEXT_KEYS), "state_shapes_x101.json", False)
    cfg = make_cfg(RESNEXT_KEYS)
    shapes = shapes_of(cfg, "state_shapes_resnext50.json", True)

    from maskrcnn_benchmark.modeling.backbone import build_backbone
    from maskrcnn_benchmark.structures.image_list import to_image_list
    sd = synth.make_weights(shapes, seed=0)
    bb = build_backbone(cfg)
    missing = bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=False)
    assert not missing.missing_keys, missing
    bb = bb.double().train()
    for n, p in bb.named_parameters():
        p.requires_grad_(n in GRAD_NAMES)
    imgs, _ = synth.make_labeled(2, 160, 4, seed=1234)
    x = to_image_list(list(imgs), 32).tensors.double()
    pyr = bb(x)
    assert len(pyr) == 5
    out = {}
    loss = 0
    for l, p in enumerate(pyr):
        idx = sample_index(p.numel(), "P%d" % l)
        out["P%d_shape" % l] = np.asarray(p.shape)
        out["P%d_idx" % l] = idx.numpy()
        out["P%d_val" % l] = p.detach().reshape(-1)[idx].numpy()
        out["P%d_max" % l] = np.asarray(p.detach().abs().max().item())
        loss = loss + (p * level_weights(l, p.shape).double()).sum()
    loss.backward()
    params = dict(bb.named_parameters())
    for n in GRAD_NAMES:
        g = params[n].grad
        idx = sample_index(g.numel(), n)
        out["g:" + n + ":shape"] = np.asarray(g.shape)
        out["g:" + n + ":idx"] = idx.numpy()
        out["g:" + n + ":val"] = g.reshape(-1)[idx].numpy()
        out["g:" + n + ":max"] = np.asarray(g.abs().max().item())
    np.savez_compressed(os.path.join(HERE, "resnext160.npz"), **out)
    print("wrote resnext160", {k: v.shape for k, v in out.items() if k.endswith("val")})


if __name__ == "__main__":
    main()
