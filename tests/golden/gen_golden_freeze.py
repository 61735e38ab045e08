"""Golden-vector generator for the unfrozen backbone (MODEL.BACKBONE.FREEZE_CONV_BODY_AT 0).  BUILD CONTAINER ONLY (needs the
reference checkout).

Imports the reference through oracle/refharness/ref_import.py and records, next to this file,

  freeze0_160.npz   the reference's own CPU backbone (double precision), default R-50-FPN with FREEZE_CONV_BODY_AT 0, on
                    synthetic.make_labeled(2, 160, 4, seed=1234) with synthetic.make_weights(state_shapes.json, seed=0): for the loss
                    sum_l <P_l, R_l> with R_l = grouped_formulations.level_weights(l, shape), fixed 2 048-element index samples of
                    the gradients of the stem convolution, of conv1 / conv2 / conv3 / downsample.0 of layer1.0, of layer1.2.conv2
                    and of layer2.0.conv1, each with the largest magnitude of the whole tensor (the tolerance is relative to it)

Weights are never stored: the tests regenerate them from the shapes.  No reference source text is stored.

    python tests/golden/gen_golden_freeze.py
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

KEYS = ["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", 0]
N_SAMPLES = 2048
GRAD_NAMES = ["body.stem.conv1.weight"] + ["body.layer1.0.%s.weight" % c for c in ("conv1", "conv2", "conv3", "downsample.0")] + \
             ["body.layer1.2.conv2.weight", "body.layer2.0.conv1.weight"]


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


def main():
    synth = _load_synth()
    mb, make_cfg = load_reference()
    torch.set_num_threads(8)
    cfg = make_cfg(KEYS)
    shapes = json.load(open(os.path.join(HERE, "state_shapes.json")))["shapes"]

    from maskrcnn_benchmark.modeling.backbone import build_backbone
    from maskrcnn_benchmark.structures.image_list import to_image_list
    sd = synth.make_weights(shapes, seed=0)
    bb = build_backbone(cfg)
    missing = bb.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=False)
    assert not missing.missing_keys, missing
    assert all(p.requires_grad for p in bb.parameters())   # FREEZE_CONV_BODY_AT 0 (reference backbone/resnet.py:105-115)
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
    np.savez_compressed(os.path.join(HERE, "freeze0_160.npz"), **out)
    print("wrote freeze0_160", {k: v.shape for k, v in out.items() if k.endswith("val")})


if __name__ == "__main__":
    main()
