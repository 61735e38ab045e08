"""PAP evaluation, mask work on the host (numpy run-length codec) against the device path (csrc/maskeval.hip,
`on_device=True`): seeded synthetic 1000 x 1000 windows -- ellipses as in tests/pap_inputs.py, 8 windows, 2 categories, about
100 detections and 30 ground truths per window.  Detections are 28 x 28 probabilities with boxes, so the paste is inside the
timed region.  Per window `prepare_for_pap_segmentation` + `evaluate_predictions_on_pap` run three ways, the arms taking turns
at going first, after one warm-up window; the device is synchronised before every clock read:
    host    on_device=False
    stack   on the device, the paste through bytes: Masker.forward_single_image (mmt_paste_mask_stack into a zeroed
            (D, size, size) stack), then the window-sized masks through on_device=True (mmt_mask_pack + transitions)
    fused   on_device=True on the 28 x 28 probabilities: pasted straight into mask words (mmt_paste_mask_words)
The arms' result lists and statistics must be equal.  Writes profiles/pap_eval_device.txt.

Then the paste alone (profiles/paste_words.txt): D = 200 detections (the first windows' boxes and probabilities) into one window,
the stack route against the fused one, to words and to strings; --reps alternating repetitions of --inner calls each after
warm-up, medians and the spread over the repetitions.

    python mmt-psm_amd/tools/bench_pap_eval.py [--windows 8] [--size 1000] [--reps 25]"""
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


ARMS = ("host", "stack", "fused")


def one(ds, preds, w, arm):
    """-> (seconds for prepare, seconds for evaluate, result list, stats) of window w"""
    on_device = arm != "host"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p = preds[w]
    if arm == "stack":
        from maskrcnn_benchmark.modeling.roi_heads.mask_head.mask_head import Masker
        dev = torch.device("cuda", torch.cuda.current_device())
        q = BoxList(p.bbox, p.size, "xyxy")
        for f in p.fields():
            q.add_field(f, p.get_field(f))
        q.add_field("mask", Masker(threshold=0.5, padding=1).forward_single_image(p.get_field("mask").to(dev), p.to(dev)))
        p = q
    gts, dts = prepare_for_pap_segmentation({w: p}, ds, on_device=on_device)
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


def paste_bench(preds, size, D, reps, inner):
    """the paste of D detections into one size x size window, stack route against fused route -> report lines"""
    from maskrcnn_benchmark import _hip as H
    dev = torch.device("cuda", torch.cuda.current_device())
    prob = torch.cat([preds[w].get_field("mask") for w in sorted(preds)])[:D].to(dev)
    boxes = torch.cat([preds[w].bbox for w in sorted(preds)])[:D].to(dev)
    D = int(prob.shape[0])
    arms = {
        ("words", "stack"): lambda: H.mask_pack(H.paste_mask_stack(prob, boxes, size, size, 0.5)[:, 0]),
        ("words", "fused"): lambda: H.paste_mask_words(prob, boxes, size, size, 0.5),
        ("strings", "stack"): lambda: mask_rle.encode_device(H.paste_mask_stack(prob, boxes, size, size, 0.5)),
        ("strings", "fused"): lambda: mask_rle.encode_pasted_device(prob, boxes, size, size, 0.5),
    }
    (ws, rs), (wf, rf) = arms[("words", "stack")](), arms[("words", "fused")]()
    if not (torch.equal(ws, wf) and torch.equal(rs, rf) and arms[("strings", "stack")]() == arms[("strings", "fused")]()):
        raise SystemExit("paste: the fused route's words, records or strings differ from the stack route's")
    for f in arms.values():                                            # warm-up
        for _ in range(3):
            f()
    t = {k: [] for k in arms}
    for r in range(reps):
        for what in ("words", "strings"):
            for route in (("stack", "fused") if r % 2 == 0 else ("fused", "stack")):
                f = arms[(what, route)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    f()
                torch.cuda.synchronize()
                t[(what, route)].append((time.perf_counter() - t0) / inner * 1e3)
    nw = (size * size + 63) // 64
    lines = [
        "Paste of M x M probabilities into a window: through bytes (mmt_paste_mask_stack + mmt_mask_pack) vs straight into mask",
        "words (mmt_paste_mask_words); tools/bench_pap_eval.py",
        "D = %d detections, M = %d, window %d x %d; %d alternating repetitions of %d calls after warm-up; host clock around a device"
        % (D, M, size, size, reps, inner),
        "synchronise; words, records and strings of the two routes: equal",
        "bytes the algorithm moves, from the shapes: stack route %.1f MB cleared + up to %.1f MB written + %.1f MB read back + %.1f MB"
        % (D * size * size / 1e6, D * size * size / 1e6, D * size * size / 1e6, D * nw * 8 / 1e6),
        "of words; fused route %.1f MB of words written once + %.2f MB of probabilities read" % (D * nw * 8 / 1e6, D * M * M * 4 / 1e6),
        "%-34s %10s %10s %10s %10s %10s" % ("ms per call", "median", "min", "q25", "q75", "max"),
    ]
    for what in ("words", "strings"):
        for route in ("stack", "fused"):
            v = np.asarray(t[(what, route)])
            lines.append("%-34s %10.3f %10.3f %10.3f %10.3f %10.3f" % ("to %s, %s route" % (what, route), np.median(v), v.min(),
                                                                         np.percentile(v, 25), np.percentile(v, 75), v.max()))
        a, b = np.asarray(t[(what, "stack")]), np.asarray(t[(what, "fused")])
        lines.append("to %s: stack / fused = %.2f (medians); run-to-run spread (q75 - q25) / median: stack %.1f %%, fused %.1f %%"
                     % (what, np.median(a) / np.median(b), 100 * (np.percentile(a, 75) - np.percentile(a, 25)) / np.median(a),
                        100 * (np.percentile(b, 75) - np.percentile(b, 25)) / np.median(b)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pap_eval_device.txt"))
    ap.add_argument("--paste-out", default=os.path.join(ROOT, "profiles", "paste_words.txt"))
    ap.add_argument("--detections", type=int, default=200)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    ds, preds = make(a.windows, a.size)
    for arm in ARMS:                                                   # warm-up: one window, every arm
        one(ds, preds, 0, arm)
    t = {arm: [0.0, 0.0] for arm in ARMS}
    n_dt = n_gt = 0
    for w in range(a.windows):
        res = {}
        for arm in ARMS[w % 3:] + ARMS[:w % 3]:                        # the arms take turns at going first
            p, e, dts, stats = one(ds, preds, w, arm)
            t[arm][0] += p
            t[arm][1] += e
            res[arm] = (dts, stats)
        for arm in ARMS[1:]:
            if not (same(res["host"][0], res[arm][0]) and same(res["host"][1], res[arm][1])):
                raise SystemExit("window %d: the device path's results (%s) differ from the host path's" % (w, arm))
        n_dt += len(res["fused"][0])
        n_gt += len(ds.get_ground_truth(ds.id_to_img_map[w]))
    host, stack, dev = sum(t["host"]), sum(t["stack"]), sum(t["fused"])
    lines = [
        "PAP evaluation, mask work on the host vs on the device (tools/bench_pap_eval.py)",
        "%d windows of %d x %d, 2 categories, %d detections (28 x 28 probabilities, pasted inside the timed region), %d ground truths"
        % (a.windows, a.size, a.size, n_dt, n_gt),
        "result lists (run-length strings included) and statistics of the three arms: equal in every window",
        "%-34s %12s %12s %12s" % ("seconds over all windows", "prepare", "evaluate", "total"),
        "%-34s %12.3f %12.3f %12.3f" % ("host (on_device=False)", t["host"][0], t["host"][1], host),
        "%-34s %12.3f %12.3f %12.3f" % ("device, paste through a byte stack", t["stack"][0], t["stack"][1], stack),
        "%-34s %12.3f %12.3f %12.3f" % ("device, fused (on_device=True)", t["fused"][0], t["fused"][1], dev),
        "%-34s %12.2f %12.2f %12.2f" % ("host / device, fused", t["host"][0] / t["fused"][0], t["host"][1] / t["fused"][1], host / dev),
        "per detection: host %.2f ms, device through a byte stack %.2f ms, device fused %.2f ms"
        % (host / n_dt * 1e3, stack / n_dt * 1e3, dev / n_dt * 1e3),
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    lines = paste_bench(preds, a.size, a.detections, a.reps, a.inner)
    print("\n".join(lines))
    with open(a.paste_out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
