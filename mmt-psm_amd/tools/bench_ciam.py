"""Timing of CIAM's forward and backward (csrc/relation.hip) for the default pair (mmt_ciam_fwd / _bwd) and the five combinations of
MODEL.RELATION_MASK.NORM 1 / 2 and PRE_NORM (mmt_ciam_norm_fwd / _bwd).  A measurement script: nothing is gated on its numbers; the
default is the yardstick.

Size: IR-Net's at bench scale -- 200 instances in four (image, class) groups of 50, C = 16, 14 x 14 --, ReLU'd Gaussian features.
HIP events around REPS back-to-back calls of the binding (allocations of its outputs included on every side), median of ROUNDS rounds
after a warm-up, one process (the method of tools/bench_gconv.py); the arms take turns, twice, and both passes are printed.  The
output is appended to the file given with --out.

    python mmt-psm_amd/tools/bench_ciam.py [--out profiles/ciam_norm.txt]
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from bench_gconv import REPS, ROUNDS, WARM, timed  # noqa: E402

SIZES, C, HW = [50, 50, 50, 50], 16, 14
COMBOS = [(-1, False), (-1, True), (1, False), (1, True), (2, False), (2, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from maskrcnn_benchmark import _hip as H
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    n = sum(SIZES)
    x = torch.relu(torch.randn((n, C, HW, HW), generator=g, device=dev) * 0.3 + 0.1)
    gout = torch.randn((n, C, HW, HW), generator=g, device=dev)
    group = torch.cat([torch.full((s,), i, dtype=torch.int64) for i, s in enumerate(SIZES)]).to(dev)
    gamma = torch.full((1,), 0.7, device=dev)
    lines = ["CIAM forward / backward, %d instances in groups of %s, C %d, %d x %d; %d calls per event pair, median of %d, %d warm-up"
             % (n, SIZES, C, HW, HW, REPS, ROUNDS, WARM)]
    for rnd in range(2):
        for norm, pre in COMBOS:
            if (norm, pre) == (-1, False):
                fwd = lambda: H.ciam_fwd(x, group, gamma)
                out, A, J = fwd()
                bwd = lambda: H.ciam_bwd(x, group, gamma, A, J, gout)
                launches = "1 + 2 launches"
            else:
                fwd = lambda: H.ciam_norm_fwd(x, group, gamma, norm, pre)
                out, A, J, saved = fwd()
                bwd = lambda: H.ciam_norm_bwd(x, group, gamma, norm, pre, saved, A, J, gout)
                launches = "%d + %d launches" % (1 + int(pre) + int(norm == 1), 2 + int(norm == 1))
            tf, tb = timed(fwd), timed(bwd)
            lines.append("  pass %d  NORM %2d PRE_NORM %-5s  forward %7.1f us   backward %7.1f us   (%s; the backward also clears dgamma)"
                         % (rnd + 1, norm, pre, tf * 1e6, tb * 1e6, launches))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
