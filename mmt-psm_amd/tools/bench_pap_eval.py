"""PAP evaluation, mask work on the host (numpy run-length codec) against the device path (csrc/maskeval.hip,
`on_device=True`): seeded synthetic 1000 x 1000 windows -- ellipses as in tests/pap_inputs.py, 8 windows, 2 categories, about
100 detections and 30 ground truths per window.  Detections are 28 x 28 probabilities with boxes, so the paste is inside the
timed region.  Per window `prepare_for_pap_segmentation` + `evaluate_predictions_on_pap` run both ways, the arms alternating,
after one warm-up window; the device is synchronised before every clock read.  The two arms' result lists and statistics must
be equal.  Writes profiles/pap_eval_device.txt.

    python mmt-psm_amd/tools/bench_pap_eval.py [--windows 8] [--size 1000]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
from maskrcnn_benchmark.data.datasets.evaluation.pap.pap_eval import evaluate_predictions_on_pap, prepare_for_pap_segmentation
from maskrcnn_benchmark.structures.bounding_box import BoxList

M = 28


def ellipse(size, cx, cy, rx, ry):
    yy, xx = np.mgrid[0:size, 0:size]
    return ((((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) <= 1.0).astype(np.uint8)


def make(windows, size, seed=7):
    """-> (dataset stub, {index: BoxList of predictions})"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:M, 0:M]
    disc = ((((xx - 13.5) / 14.0) ** 2 + ((yy - 13.5) / 14.0) ** 2) <= 1.0).astype(np.float32)   # an ellipse inscribed in its box
    ids, truth, preds = {}, {}, {}
    for w in range(windows):
        ids[w] = {"file_name": "slide%d" % (w % 3), "location": (size * w, 64 * (w % 2)), "id": w + 1}
        g_lab, g_rle, boxes, scores, labels, probs = [], [], [], [], [], []
        for cat in (1, 2):
            for _ in range(15):
                r = rng.uniform(40, 110) if cat == 1 else rng.uniform(25, 60)
                ry = r * rng.uniform(0.7, 1.3)
                cx, cy = rng.uniform(r + 2, size - r - 2), rng.uniform(ry + 2, size - ry - 2)
                rle = mask_rle.encode(ellipse(size, cx, cy, r, ry))
                rle["counts"] = rle["counts"].decode("ascii")
                g_lab.append(cat)
                g_rle.append(rle)
                for _ in range(3):                                     # perturbed copies: matches, duplicates, near misses
                    dx, dy = rng.uniform(-0.25, 0.25, 2) * r
                    sx, sy = rng.uniform(0.8, 1.25, 2)
                    boxes.append([cx + dx - r * sx, cy + dy - ry * sy, cx + dx + r * sx, cy + dy + ry * sy])
                    scores.append(float(rng.rand()))
                    labels.append(cat)
                    probs.append(disc * rng.uniform(0.6, 1.0))
            for _ in range(5):                                         # false positives
                r = rng.uniform(15, 50)
                cx, cy = rng.uniform(r, size - r, 2)
                boxes.append([cx - r, cy - r, cx + r, cy + r])
                scores.append(float(rng.rand()))
                labels.append(cat)
                probs.append(disc * rng.uniform(0.6, 1.0))
        truth[w] = (g_lab, g_rle)
        b = BoxList(torch.tensor(boxes, dtype=torch.float32).clamp_(0, size - 1), (size, size), "xyxy")
        b.add_field("scores", torch.tensor(scores, dtype=torch.float64))
        b.add_field("labels", torch.tensor(labels, dtype=torch.int64))
        b.add_field("mask", torch.from_numpy(np.stack(probs)[:, None]))
        preds[w] = b

    class DS(object):
        maxWS = size
        id_to_img_map = ids
        contiguous_category_id_to_json_id = {1: 1, 2: 2}

        def get_ground_truth(self, original_id):
            lab, rles = truth[original_id["id"] - 1]
            b = BoxList(torch.zeros((len(lab), 4)), (size, size), "xyxy")
            b.add_field("labels", torch.tensor(lab, dtype=torch.int64))
            b.add_field("masks", [dict(r) for r in rles])
            return b

    return DS(), preds


def one(ds, preds, w, on_device):
    """-> (seconds for prepare, seconds for evaluate, result list, stats) of window w"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gts, dts = prepare_for_pap_segmentation({w: preds[w]}, ds, on_device=on_device)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ev = evaluate_predictions_on_pap(gts, dts, None, "segm", on_device=on_device)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, dts, ev.stats


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.ndarray, float, np.floating)):
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pap_eval_device.txt"))
    a = ap.parse_args()
    ds, preds = make(a.windows, a.size)
    for arm in (False, True):                                          # warm-up: one window, both arms
        one(ds, preds, 0, arm)
    t = {False: [0.0, 0.0], True: [0.0, 0.0]}
    n_dt = n_gt = 0
    for w in range(a.windows):
        res = {}
        for arm in ((False, True) if w % 2 == 0 else (True, False)):   # the arms alternate, and so does who goes first
            p, e, dts, stats = one(ds, preds, w, arm)
            t[arm][0] += p
            t[arm][1] += e
            res[arm] = (dts, stats)
        if not (same(res[False][0], res[True][0]) and same(res[False][1], res[True][1])):
            raise SystemExit("window %d: the device path's results differ from the host path's" % w)
        n_dt += len(res[True][0])
        n_gt += len(ds.get_ground_truth(ds.id_to_img_map[w]))
    host, dev = sum(t[False]), sum(t[True])
    lines = [
        "PAP evaluation, mask work on the host vs on the device (tools/bench_pap_eval.py)",
        "%d windows of %d x %d, 2 categories, %d detections (28 x 28 probabilities, pasted inside the timed region), %d ground truths"
        % (a.windows, a.size, a.size, n_dt, n_gt),
        "result lists (run-length strings included) and statistics of the two arms: equal in every window",
        "%-28s %12s %12s %12s" % ("seconds over all windows", "prepare", "evaluate", "total"),
        "%-28s %12.3f %12.3f %12.3f" % ("host (on_device=False)", t[False][0], t[False][1], host),
        "%-28s %12.3f %12.3f %12.3f" % ("device (on_device=True)", t[True][0], t[True][1], dev),
        "%-28s %12.2f %12.2f %12.2f" % ("host / device", t[False][0] / t[True][0], t[False][1] / t[True][1], host / dev),
        "per detection: host %.2f ms, device %.2f ms" % (host / n_dt * 1e3, dev / n_dt * 1e3),
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
