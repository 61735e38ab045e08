"""Bitmap ground truth on mask words (csrc/bitmasks.hip): the mask head's targets from a BinaryMaskList beside the polygon route's
`polygon_targets` on the polygons the instances came from (informational: the two rasterise by different rules), and the two
transforms of the input pipeline on a whole image's instances.

Input: --instances star polygons of 12-40 vertices with radii of 4-10 % of the side in a --size x --size image, rasterised once by
`polygon_mask_words`; --rois boxes of 40-200 pixels around random instances (jittered copies of their extents), M x M targets.
Arms, each one library call on inputs already on the device:
    targets/words     mmt_mask_words_targets
    targets/polygons  mmt_polygon_targets
    resample          mmt_mask_words_resample, the whole image --size^2 -> --out^2 (its record launch included)
    flip              mmt_mask_words_resample, same size, left-right
After warm-up, --reps repetitions in which the arms take turns (the order rotates); an arm's sample is --inner back-to-back calls
between two device events, divided by --inner.  Medians, with the range.  Byte counts beside the times are what the call must
move (words read once where the window covers them, output written once) at the measured HBM copy rate (--hbm-tbs).

    python mmt-psm_amd/tools/bench_bitmask.py [--size 1000] [--out 800] [--instances 30] [--rois 256] [--M 28] > profiles/bitmask_words.txt"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
from maskrcnn_benchmark import _hip
from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList, SegmentationMask


def star(rng, size):
    nv = int(rng.randint(12, 41))
    r0 = size * rng.uniform(0.04, 0.10)
    cx, cy = rng.uniform(r0, size - r0, 2)
    th = np.sort(rng.uniform(0, 2 * math.pi, nv))
    r = r0 * (1.0 - 0.4 * rng.uniform(0, 1, nv))
    return np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1).astype(np.float32).reshape(-1)


def rois(rng, polys, n, size):
    """n boxes of 40-200 pixels, each the jittered extent of a random instance -> (instance int32 (n,), boxes float32 (n, 4))"""
    inst = rng.randint(0, len(polys), n)
    out = []
    for g in inst:
        p = polys[g].reshape(-1, 2)
        c = 0.5 * (p.min(0) + p.max(0)) + rng.uniform(-6, 6, 2)
        half = 0.5 * np.clip((p.max(0) - p.min(0)) * rng.uniform(0.8, 1.3, 2), 40, 200)
        out.append([c[0] - half[0], c[1] - half[1], c[0] + half[0], c[1] + half[1]])
    return inst.astype(np.int32), np.clip(np.asarray(out, np.float32), 0, size - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--out", type=int, default=800)
    ap.add_argument("--instances", type=int, default=30)
    ap.add_argument("--rois", type=int, default=256)
    ap.add_argument("--M", type=int, default=28)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--hbm-tbs", type=float, default=6.29)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bitmask.py measures on the MI355X; no GPU visible")
    _hip.lib()
    S, O, M, dev = a.size, a.out, a.M, torch.device("cuda", 0)
    rng = np.random.RandomState(11)
    polys = [star(rng, S) for _ in range(a.instances)]
    sm = SegmentationMask([[torch.from_numpy(p)] for p in polys], (S, S), mode="poly")
    masks = BinaryMaskList.from_polygons(sm)
    words, rec = masks.mask_words(dev)
    inst, boxes = rois(rng, polys, a.rois, S)
    roi_inst, boxes = torch.from_numpy(inst).to(dev), torch.from_numpy(boxes).to(dev)
    xy, poly_off, inst_rng = sm.packed(dev)
    roi_poly = inst_rng[roi_inst.long()].contiguous()

    arms = [("targets/words", lambda: _hip.mask_words_targets(words, roi_inst, boxes, S, S, M)),
            ("targets/polygons", lambda: _hip.polygon_targets(xy, poly_off, roi_poly, boxes, M)),
            ("resample", lambda: _hip.mask_words_resample(words, S, S, (0, 0, S, S), 0, O, O)),
            ("flip", lambda: _hip.mask_words_resample(words, S, S, (0, 0, S, S), 1, S, S))]
    for _, f in arms:                       # warm-up: code objects loaded, the allocator holds every size
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t_b, t_p = arms[0][1](), arms[1][1]()[0]
    agree = float((t_b == t_p).float().mean())
    times = {n: [] for n, _ in arms}
    for r in range(a.reps):
        for k in range(len(arms)):
            n, f = arms[(k + r) % len(arms)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    nw, nwo = (S * S + 63) // 64, (O * O + 63) // 64
    G, P = a.instances, a.rois
    area = float(((boxes[:, 2] - boxes[:, 0]).round().clamp(min=1) * (boxes[:, 3] - boxes[:, 1]).round().clamp(min=1)).sum())
    bound = {"targets/words": area / 8 + 4 * P * M * M, "targets/polygons": None,
             "resample": 8 * G * (nw + 2 * nwo), "flip": 8 * G * (nw + 2 * nw)}
    p = torch.cuda.get_device_properties(0)
    print("box: %s (%s), %d compute units, torch %s, HIP %s" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count,
                                                                 torch.__version__, torch.version.hip))
    print("%d instances in %d x %d (%d pixels set), %d ROIs of %.0f pixels a side on average, M = %d; resample to %d x %d"
          % (G, S, S, int(rec[:, 0].sum()), P, math.sqrt(area / P), M, O, O))
    print("us per call by device events over %d back-to-back calls, %d repetitions, arms in turn: median (min .. max)" % (a.inner, a.reps))
    for n, _ in arms:
        v = times[n]
        b = bound[n]
        tail = ("   moves %.2f MB: %.2f us at %.2f TB/s" % (b / 1e6, b / (a.hbm_tbs * 1e12) * 1e6, a.hbm_tbs)) if b else \
            "   (informational: the polygon route's rasteriser on the same instances and boxes)"
        print("  %-17s %9.2f  (%.2f .. %.2f)%s" % (n, float(np.median(v)), min(v), max(v), tail))
    print("targets of the two routes agree on %.2f %% of the %d x %d x %d elements (different rules: the outline scaled and filled "
          "against the filled image resampled)" % (100 * agree, P, M, M))
    print("resample and flip include the record launch (one block per mask over the output words); every call also allocates its "
          "outputs from torch's caching allocator")


if __name__ == "__main__":
    main()
