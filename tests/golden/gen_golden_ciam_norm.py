"""Golden-vector generator for CIAM's normalisations.  BUILD CONTAINER ONLY (needs the reference checkout).

Imports the reference through oracle/refharness/ref_import.py and records, next to this file,

  ciam_norm.npz   the reference's own CIAM_Module (modeling/relation/mask_relation_module.py:190-242) on the CPU in float64 for
                  the six combinations of MODEL.RELATION_MASK.NORM in (-1, 1, 2) and PRE_NORM in (False, True), on two slices
                  (n = 5, C = 16, 7 x 7 and n = 9, C = 16, 14 x 14; tests/ciam_formulations.py: structured_inputs): per slice the
                  input x, the output gradient gout (float32 as the builder makes them: the float64 pass widens them exactly) and
                  gamma; per (slice, combination) autograd's dgamma and, for the output and dx, a fixed sample of 1024 entries
                  (ciam_formulations.sample_index) with the tensor's largest magnitude and its sum -- float64 noise does not
                  compress, and the file stays a few hundred KiB.

Data only; no reference source text is stored.

    python tests/golden/gen_golden_ciam_norm.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.refharness.ref_import import load_reference  # noqa: E402
import ciam_formulations as cf  # noqa: E402

SLICES = [(5, 7, 11), (9, 14, 12)]     # (n, H = W, seed)
GAMMA = 0.7


def main():
    mb, make_cfg = load_reference()
    from maskrcnn_benchmark.modeling.relation.mask_relation_module import CIAM_Module
    out = {"gamma": np.asarray(GAMMA)}
    for k, (n, hw, seed) in enumerate(SLICES):
        x, gout = cf.structured_inputs([n], hw, seed)
        out["x%d" % k], out["gout%d" % k] = x.numpy(), gout.numpy()
        x, gout = x.double(), gout.double()
        for norm, pre in cf.COMBOS:
            cfg = make_cfg(["MODEL.RELATION_MASK.NORM", norm, "MODEL.RELATION_MASK.PRE_NORM", pre])
            mod = CIAM_Module(cfg).double()
            assert (mod.norm, mod.prenorm) == (norm, pre)
            with torch.no_grad():
                mod.gamma.fill_(GAMMA)
            xx = x.clone().requires_grad_(True)
            y = mod(xx)
            y.backward(gout)
            tag = "%d_n%d_p%d" % (k, norm, int(pre))
            for name, v in (("out", y.detach()), ("dx", xx.grad)):
                out[name + tag] = v.reshape(-1)[cf.sample_index(v.numel(), k)].numpy()
                out[name + tag + "_max"] = np.asarray(v.abs().max().item())
                out[name + tag + "_sum"] = np.asarray(v.sum().item())
            out["dgamma" + tag] = mod.gamma.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "ciam_norm.npz"), **out)
    print("wrote ciam_norm.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
