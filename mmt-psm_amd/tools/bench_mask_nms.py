"""Timing of mask NMS at inference (TEST.MASK_NMS; csrc/masknms.hip).  A measurement script: nothing is gated on its numbers.

Part one, the call alone: D = 200 synthetic detections at 1000 x 1000 -- discs of 28 x 28 probabilities in boxes of 40 to 160
pixels around 25 cluster centres, so that many overlap --, pasted into mask words (`mmt_paste_mask_words`) and then
    device   `_hip.mask_nms` (pair launch + sweep launch), the kept count read back
    host     the route one can build from the pieces that were there before: `mask_pair_intersections` over all D x D pairs, the
             matrix and the records read back, the greedy sweep in numpy with the same integer test
The two arms take turns; their keep flags are checked equal; the paste alone is timed beside them.  Host clock around a device
synchronise, medians with their range.  The bytes the pair launch must read are computed from the records (the words of the
overlapping columns of every same-label pair whose boxes overlap, twice).

Part two, inference: n = 2 noise images of 1000 x 1000, the synthetic weights, default arithmetic; eval-mode `model(x)` with the
switch off and on (one model, the mask head's post-processor exchanged), arms in turn, ms per image.

    python mmt-psm_amd/tools/bench_mask_nms.py [--out profiles/mask_nms.txt] [--rounds 25] [--no-model]
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

D, M, SIZE, WARM = 200, 28, 1000, 3
THRESH, MEASURE = 0.5, "iou"
Q = 1 << 20


def detections(dev, seed=0):
    g = np.random.default_rng(seed)
    cx, cy = g.uniform(100, SIZE - 100, 25), g.uniform(100, SIZE - 100, 25)
    k = g.integers(25, size=D)
    w, h = g.uniform(40, 160, D), g.uniform(40, 160, D)
    x0 = np.clip(cx[k] + g.normal(0, 15, D) - w / 2, 0, SIZE - 2)
    y0 = np.clip(cy[k] + g.normal(0, 15, D) - h / 2, 0, SIZE - 2)
    boxes = np.stack([x0, y0, np.minimum(x0 + w, SIZE - 1), np.minimum(y0 + h, SIZE - 1)], 1).astype(np.float32)
    yy, xx = np.mgrid[0:M, 0:M]
    r = g.uniform(0.30, 0.48, D)[:, None, None] * M
    prob = (1.0 / (1.0 + np.exp(((yy - M / 2 + 0.5) ** 2 + (xx - M / 2 + 0.5) ** 2)[None] ** 0.5 - r))).astype(np.float32)
    scores = np.sort(g.uniform(0.05, 1.0, D).astype(np.float32))[::-1].copy()
    labels = g.integers(1, 3, D).astype(np.int64)
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(prob[:, None]), t(boxes), t(scores), t(labels)


def host_sweep(inter, rec, scores, labels, tq, measure):
    order = np.argsort(-scores, kind="stable")
    area = rec[:, 0].astype(np.int64)
    keep = np.zeros(len(order), dtype=np.uint8)
    kept = []
    for j in order:
        ok = True
        for i in kept:
            c = int(inter[i, j])
            if c > 0 and labels[i] == labels[j]:
                den = area[i] + area[j] - c if measure == "iou" else min(area[i], area[j])
                if c * Q >= tq * den:
                    ok = False
                    break
        if ok:
            kept.append(j)
            keep[j] = 1
    return keep


def pair_bytes(rec, labels):
    """bytes of mask words the pair launch reads: both masks' words of the overlapping columns, same-label pairs with overlapping
    record boxes"""
    n, total, pairs = len(rec), 0, 0
    for i in range(n):
        for j in range(i + 1, n):
            a, b = rec[i], rec[j]
            if labels[i] != labels[j] or a[0] == 0 or b[0] == 0:
                continue
            xlo, xhi = max(a[1], b[1]), min(a[2], b[2])
            ylo, yhi = max(0 if a[5] else a[3], 0 if b[5] else b[3]), min(SIZE - 1 if a[5] else a[4], SIZE - 1 if b[5] else b[4])
            if xhi < xlo or yhi < ylo:
                continue
            pairs += 1
            total += 16 * ((((xhi + 1) * SIZE + 63) >> 6) - ((xlo * SIZE) >> 6))
    return pairs, total


def stats(v):
    v = sorted(v)
    q = lambda f: v[min(int(f * len(v)), len(v) - 1)]
    return "%10.3f %10.3f %10.3f %10.3f %10.3f" % (statistics.median(v), v[0], q(0.25), q(0.75), v[-1])


def part_one(H, dev, rounds, lines):
    prob, boxes, scores, labels = detections(dev)
    tq = H.mask_nms_threshold_q20(THRESH)
    s_host, l_host = scores.cpu().numpy(), labels.cpu().numpy()

    def paste():
        return H.paste_mask_words(prob, boxes, SIZE, SIZE, 0.5)

    def device():
        words, rec = paste()
        keep, count = H.mask_nms(words, rec, scores, labels, SIZE, SIZE, THRESH, MEASURE)
        return keep, int(count.item())

    def host():
        words, rec = paste()
        inter = H.mask_pair_intersections(words, rec, words, rec, SIZE, SIZE).cpu().numpy()
        return host_sweep(inter, rec.cpu().numpy(), s_host, l_host, tq, MEASURE)

    arms = [("paste alone", paste), ("paste + mask_nms (device)", device), ("paste + all pairs + host sweep", host)]
    times = {n: [] for n, _ in arms}
    res = {}
    for rnd in range(WARM + rounds):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name] = fn()
            torch.cuda.synchronize()
            if rnd >= WARM:
                times[name].append((time.perf_counter() - t0) * 1e3)
    keep_d, n_d = res[arms[1][0]]
    keep_h = res[arms[2][0]]
    equal = keep_d.cpu().numpy().tolist() == keep_h.tolist() and n_d == int(keep_h.sum())
    rec = res[arms[0][0]][1].cpu().numpy()
    pairs, nbytes = pair_bytes(rec, l_host)
    lines.append("D = %d detections, M = %d, window %d x %d, threshold %.2f (%s), per class; %d alternating repetitions after %d warm-up; "
                 "host clock around a device synchronise" % (D, M, SIZE, SIZE, THRESH, MEASURE, rounds, WARM))
    lines.append("kept %d of %d; keep flags of the two routes: %s" % (n_d, D, "equal" if equal else "DIFFERENT"))
    lines.append("pairs the pair launch reads words for: %d of %d; %.2f MB of mask words (both masks, overlapping columns), "
                 "%.2f MB if every pair read whole masks" % (pairs, D * (D - 1) // 2, nbytes / 1e6, D * (D - 1) // 2 * 2 * 8 * ((SIZE * SIZE + 63) // 64) / 1e6))
    lines.append("ms per call                            median        min        q25        q75        max")
    for name, _ in arms:
        lines.append("%-34s %s" % (name, stats(times[name])))
    med = {n: statistics.median(v) for n, v in times.items()}
    lines.append("behind the paste: device %.3f ms, host route %.3f ms (medians minus the paste's median)"
                 % (med[arms[1][0]] - med[arms[0][0]], med[arms[2][0]] - med[arms[0][0]]))


def part_two(H, dev, rounds, lines):
    import synthetic
    from maskrcnn_benchmark.config import make_default_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.mask_head import make_roi_mask_post_processor
    from maskrcnn_benchmark.structures.image_list import to_image_list
    cfg = make_default_cfg()
    model = build_detection_model(cfg)
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "state_shapes.json")))["shapes"]
    model.load_state_dict(synthetic.make_weights(shapes, seed=0), strict=False)
    model.to(dev).eval()
    on_cfg = make_default_cfg()
    on_cfg.TEST.MASK_NMS.ENABLED = True
    pps = {"switch off": model.mask_heads.mask.post_processor, "switch on": make_roi_mask_post_processor(on_cfg)}
    n = 2
    imgs, _ = synthetic.make_labeled(n, SIZE, 12, seed=1234)
    batch = to_image_list(list(imgs.to(dev)), cfg.DATALOADER.SIZE_DIVISIBILITY)
    times, dets = {k: [] for k in pps}, {}
    with torch.no_grad():
        for rnd in range(WARM + rounds):
            for name, pp in pps.items():
                model.mask_heads.mask.post_processor = pp
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model(batch)
                torch.cuda.synchronize()
                if rnd >= WARM:
                    times[name].append((time.perf_counter() - t0) * 1e3 / n)
                dets[name] = [len(o) for o in out]
    model.mask_heads.mask.post_processor = pps["switch off"]
    lines.append("inference, n = %d noise images of %d x %d, synthetic weights, TEST.MASK_NMS defaults (0.5, iou, per class); %d rounds after "
                 "%d warm-up, arms in turn; ms per image" % (n, SIZE, SIZE, rounds, WARM))
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
    lines = ["Mask NMS at inference (mmt_mask_nms, csrc/masknms.hip); tools/bench_mask_nms.py",
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
