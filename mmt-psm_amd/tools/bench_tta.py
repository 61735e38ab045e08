"""Timing of multi-view inference (GeneralizedRCNN.forward_tta) against plain eval-mode inference.  A measurement script: nothing
is gated on its numbers.

Size: the bench's -- n = 2 noise images of 1000 x 1000 (padded to 1024), the synthetic weights, default arithmetic.  Arms: plain
model(x); V = 2 (one batch and its mirror image); V = 4 (two batches, each with its mirror image).  The arms take turns, ROUNDS
rounds after WARM warm-up rounds, wall time around a synchronised pass, the median per arm, in ms per image.  A second pass brackets
the two merge launches (mmt_tta_merge_box, mmt_tta_merge_mask: the binding's allocations included) with events and reports their
device time as a share of the pass.  The expectation that is checked and printed: a V-view pass takes at most V x the plain pass
(the plain path is the parent commit's: forward() without `tta` runs the same launches as before).

    python mmt-psm_amd/tools/bench_tta.py [--out profiles/tta.txt] [--rounds 15]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)

CROP, N, N_INST, WARM = 1000, 2, 12, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--crop", type=int, default=CROP)
    args = ap.parse_args()
    import synthetic
    from maskrcnn_benchmark import _hip as H
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.structures.image_list import to_image_list
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    H.lib()
    cfg = make_default_cfg()
    model = build_detection_model(cfg)
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "state_shapes.json")))["shapes"]
    model.load_state_dict(synthetic.make_weights(shapes, seed=0), strict=False)
    model.to(dev).eval()
    batches = []
    for seed in (1234, 4321):
        imgs, _ = synthetic.make_labeled(N, args.crop, N_INST, seed=seed)
        batches.append(to_image_list(list(imgs.to(dev)), cfg.DATALOADER.SIZE_DIVISIBILITY))
    arms = [("plain", lambda: model(batches[0])),
            ("tta V=2", lambda: model.forward_tta(batches[:1], flip=True)),
            ("tta V=4", lambda: model.forward_tta(batches, flip=True))]
    times = {name: [] for name, _ in arms}
    dets = {}
    with torch.no_grad():
        for rnd in range(WARM + args.rounds):
            for name, fn in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if rnd >= WARM:
                    times[name].append((time.perf_counter() - t0) * 1e3 / N)
                dets[name] = [len(o) for o in out]
        # the merge launches' device time, in a pass of their own
        spans = []
        box, mask = H.tta_merge_box, H.tta_merge_mask

        def bracket(fn):
            def run(*a, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn(*a, **k)
                e1.record()
                spans.append((e0, e1))
                return r
            return run

        H.tta_merge_box, H.tta_merge_mask = bracket(box), bracket(mask)
        merge = {}
        try:
            for name, fn in arms[1:]:
                per = []
                for _ in range(args.rounds):
                    del spans[:]
                    fn()
                    torch.cuda.synchronize()
                    per.append(sum(a.elapsed_time(b) for a, b in spans))
                merge[name] = statistics.median(per)
        finally:
            H.tta_merge_box, H.tta_merge_mask = box, mask
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["multi-view inference, n = %d images of %d x %d, %d rounds after %d warm-up, arms alternating, medians"
             % (N, args.crop, args.crop, args.rounds, WARM)]
    for name, _ in arms:
        v = 1 if name == "plain" else int(name.split("=")[1])
        line = "  %-8s %8.2f ms / image  (min %.2f, max %.2f; detections %s)" % (name, med[name], min(times[name]), max(times[name]),
                                                                                dets[name])
        if v > 1:
            share = merge[name] / (med[name] * N)
            ok = med[name] <= v * med["plain"]
            line += "  = %.2f x plain (expected <= %d x: %s); merge launches %.3f ms = %.2f %% of the pass" % (
                med[name] / med["plain"], v, "holds" if ok else "DOES NOT HOLD", merge[name], 100 * share)
        lines.append(line)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
