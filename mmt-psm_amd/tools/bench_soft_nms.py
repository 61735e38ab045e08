"""Timing of Soft-NMS in the box post-processor (MODEL.ROI_HEADS.SOFT_NMS; csrc/softnms.hip).  A measurement script: nothing is
gated on its numbers, and no time is promised -- the Soft-NMS kernel is a chain of dependent picks and is slower than the
bit-mask NMS it stands in for.  What is reported is that difference, beside the inference pass it sits in.

Part one, the call alone: `_hip.det_postprocess` against `_hip.det_postprocess_soft` (linear and gaussian) on the same synthetic
detections of one image, R = 1000 rows (FPN_POST_NMS_TOP_N_TEST) and three classes, boxes of the bench's sizes (class 1 sides
40 to 160 px, class 2 sides 16 to 40 px at 1000 x 1000):
    crowded   rows around 40 centres per class, four in five above SCORE_THRESH: hundreds of candidates per class that overlap
    sparse    rows scattered over the image, one in twenty above SCORE_THRESH
All arms in one call, alternating repetitions, device events around each call; medians with their range.

Part two, inference: n = 2 noise images of 1000 x 1000, the synthetic weights, default arithmetic; eval-mode `model(x)` with the
switch off and on (one model, the box head's post-processor exchanged), arms in turn, ms per image.

    python mmt-psm_amd/tools/bench_soft_nms.py [--out profiles/soft_nms.txt] [--rounds 25] [--no-model]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)

R, NC, SIZE, WARM = 1000, 3, 1000, 3
SCORE_THRESH, NMS, DETS, SIGMA, MIN_SCORE = 0.05, 0.5, 200, 0.5, 0.001
SIDES = {1: (40.0, 160.0), 2: (16.0, 40.0)}     # synthetic.make_labeled: r in U(20, 80) and U(8, 20)


def detections(dev, crowded, seed=0):
    """-> prob (R, NC), decoded boxes (R, NC * 4) of one image"""
    g = np.random.default_rng(seed)
    prob = np.full((R, NC), 0.01, np.float32)
    dec = np.zeros((R, NC * 4), np.float32)
    for j in range(1, NC):
        lo, hi = SIDES[j]
        if crowded:
            c = g.uniform(100, SIZE - 100, (40, 2))
            ctr = c[g.integers(40, size=R)] + g.normal(0, 0.1 * lo, (R, 2))
        else:
            ctr = g.uniform(100, SIZE - 100, (R, 2))
        wh = g.uniform(lo, hi, (R, 2))
        dec[:, 4 * j:4 * j + 4] = np.clip(np.concatenate([ctr - wh / 2, ctr + wh / 2], 1), 0, SIZE - 1)
        above = g.uniform(size=R) < (0.8 if crowded else 0.05)
        prob[above, j] = g.uniform(SCORE_THRESH, 1.0, int(above.sum())).astype(np.float32)
    return torch.from_numpy(prob).to(dev), torch.from_numpy(dec).to(dev)


def stats(v):
    v = sorted(v)
    q = lambda f: v[min(int(f * len(v)), len(v) - 1)]
    return "%10.3f %10.3f %10.3f %10.3f %10.3f" % (statistics.median(v), v[0], q(0.25), q(0.75), v[-1])


def part_one(H, dev, rounds, lines):
    arms = [("det_postprocess (greedy NMS)", lambda p, d: H.det_postprocess(p, d, [R], SCORE_THRESH, NMS, DETS)),
            ("det_postprocess_soft, linear", lambda p, d: H.det_postprocess_soft(p, d, [R], SCORE_THRESH, NMS, DETS, "linear", SIGMA, MIN_SCORE)),
            ("det_postprocess_soft, gaussian", lambda p, d: H.det_postprocess_soft(p, d, [R], SCORE_THRESH, NMS, DETS, "gaussian", SIGMA, MIN_SCORE))]
    lines.append("one image of R = %d rows, %d classes, SCORE_THRESH %.2f, NMS %.2f, DETECTIONS_PER_IMG %d, SIGMA %.2f, MIN_SCORE %.3f; "
                 "%d alternating repetitions after %d warm-up; device events around each call"
                 % (R, NC, SCORE_THRESH, NMS, DETS, SIGMA, MIN_SCORE, rounds, WARM))
    for crowded in (True, False):
        prob, dec = detections(dev, crowded)
        cand = [(prob[:, j] > SCORE_THRESH).sum().item() for j in range(1, NC)]
        times, counts = {n: [] for n, _ in arms}, {}
        for rnd in range(WARM + rounds):
            for name, fn in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(prob, dec)
                e1.record()
                e1.synchronize()
                if rnd >= WARM:
                    times[name].append(e0.elapsed_time(e1))
                counts[name] = int(out[3].item())
        # with DETECTIONS_PER_IMG out of the way: what each route lets through
        free = [int(H.det_postprocess(prob, dec, [R], SCORE_THRESH, NMS, 0)[3].item()),
                int(H.det_postprocess_soft(prob, dec, [R], SCORE_THRESH, NMS, 0, "linear", SIGMA, MIN_SCORE)[3].item()),
                int(H.det_postprocess_soft(prob, dec, [R], SCORE_THRESH, NMS, 0, "gaussian", SIGMA, MIN_SCORE)[3].item())]
        lines.append("%s image: candidates per class %s; detections without the cut: greedy %d, linear %d, gaussian %d"
                     % ("crowded" if crowded else "sparse", cand, free[0], free[1], free[2]))
        lines.append("ms per call                            median        min        q25        q75        max")
        for name, _ in arms:
            lines.append("%-34s %s   detections %d" % (name, stats(times[name]), counts[name]))
        med = {n: statistics.median(v) for n, v in times.items()}
        lines.append("Soft-NMS costs %.3f ms (linear) and %.3f ms (gaussian) more than the greedy NMS per call"
                     % (med[arms[1][0]] - med[arms[0][0]], med[arms[2][0]] - med[arms[0][0]]))


def part_two(H, dev, rounds, lines):
    import synthetic
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.roi_heads.box_head.box_head import make_roi_box_post_processor
    from maskrcnn_benchmark.structures.image_list import to_image_list
    cfg = make_default_cfg()
    model = build_detection_model(cfg)
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "state_shapes.json")))["shapes"]
    model.load_state_dict(synthetic.make_weights(shapes, seed=0), strict=False)
    model.to(dev).eval()
    pps = {"switch off": model.box_heads.box.post_processor}
    for method in ("linear", "gaussian"):
        on_cfg = make_default_cfg()
        on_cfg.MODEL.ROI_HEADS.SOFT_NMS.ENABLED = True
        on_cfg.MODEL.ROI_HEADS.SOFT_NMS.METHOD = method
        pps["switch on, " + method] = make_roi_box_post_processor(on_cfg)
    n = 2
    imgs, _ = synthetic.make_labeled(n, SIZE, 12, seed=1234)
    batch = to_image_list(list(imgs.to(dev)), cfg.DATALOADER.SIZE_DIVISIBILITY)
    times, dets = {k: [] for k in pps}, {}
    with torch.no_grad():
        for rnd in range(WARM + rounds):
            for name, pp in pps.items():
                model.box_heads.box.post_processor = pp
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model(batch)
                torch.cuda.synchronize()
                if rnd >= WARM:
                    times[name].append((time.perf_counter() - t0) * 1e3 / n)
                dets[name] = [len(o) for o in out]
    model.box_heads.box.post_processor = pps["switch off"]
    lines.append("inference, n = %d noise images of %d x %d, synthetic weights, MODEL.ROI_HEADS.SOFT_NMS defaults but the method; %d rounds "
                 "after %d warm-up, arms in turn; host clock around a device synchronise; ms per image" % (n, SIZE, SIZE, rounds, WARM))
    lines.append("                                       median        min        q25        q75        max")
    for name in pps:
        lines.append("%-34s %s   detections %s" % (name, stats(times[name]), dets[name]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    from maskrcnn_benchmark import _hip as H
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    H.lib()
    lines = ["Soft-NMS in the box post-processor (mmt_det_postprocess_soft, csrc/softnms.hip); tools/bench_soft_nms.py",
             "ran on: %s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)]
    part_one(H, dev, args.rounds, lines)
    if not args.no_model:
        part_two(H, dev, max(args.rounds // 2, 5), lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
