"""Polygon ground truth decoded at image size (csrc/polyfill.hip): `SegmentationMask.decode` on the device against the host
route it replaces, and the two library calls against the bytes they must move.

Input: --images images of --size x --size with --instances annotated instances each, seeded star polygons of 12-40 vertices and
radii of 3-9 % of the side (every fifth instance has two overlapping polygons), vertices in float32 as SegmentationMask keeps
them.  After warm-up, --reps repetitions; the arms take turns; the device is synchronised before every clock read.
    device  polygon_mask_words (clear, walk, block parities, fill, records) + mask_words_integral per image, vertices already on
            the device (SegmentationMask.packed is cached; the words' cache is dropped for every repetition)
    host    mask_rle.frPolygons (numpy boundary walk), mask_rle.decode, sum over instances, upload of the int32 map
The two maps must be equal.  Then each library call alone, by device events, next to its byte bound at the measured HBM copy rate
(--hbm-tbs, 6.29 TB/s): toggle planes cleared and read once, G * H * W / 8 bytes of words written; the words read once and
4 * N * H * W bytes of map written.

    python mmt-psm_amd/tools/bench_polyfill.py [--size 1000] [--images 2] [--instances 40] [--reps 15] > profiles/polygon_words.txt"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
from maskrcnn_benchmark import _hip
from maskrcnn_benchmark.data.datasets.evaluation.pap import mask_rle
from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask


def star(rng, size):
    nv = int(rng.randint(12, 41))
    r0 = size * rng.uniform(0.03, 0.09)
    cx, cy = rng.uniform(r0, size - r0, 2)
    th = np.sort(rng.uniform(0, 2 * math.pi, nv))
    r = r0 * (1.0 - 0.4 * rng.uniform(0, 1, nv))
    return np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1).astype(np.float32).reshape(-1)


def make(images, size, instances, seed=11):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(images):
        inst = []
        for g in range(instances):
            p = star(rng, size)
            inst.append([p, (p + rng.uniform(-4, 4)).astype(np.float32)] if g % 5 == 4 else [p])
        out.append(inst)
    return out


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--instances", type=int, default=40)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--hbm-tbs", type=float, default=6.29)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_polyfill.py measures on the MI355X; no GPU visible")
    _hip.lib()
    S, dev = a.size, torch.device("cuda", 0)
    polys = make(a.images, S, a.instances)
    masks = [SegmentationMask([[torch.from_numpy(p) for p in inst] for inst in im], (S, S), mode="poly") for im in polys]
    for m in masks:
        m.packed(dev)

    def device():
        out = []
        for m in masks:
            m._words = None
            out.append(m.decode(S, S, dev))
        torch.cuda.synchronize()
        return out

    def host():
        out = []
        for im in polys:
            rles = mask_rle.frPolygons(im, S, S)
            out.append(torch.from_numpy(mask_rle.decode(rles).astype(np.int32).sum(2)).to(dev))
        torch.cuda.synchronize()
        return out

    d, h = device(), host()
    assert all(torch.equal(x, y) for x, y in zip(d, h)), "device and host maps differ"
    device()
    t_dev, t_host = [], []
    for r in range(a.reps):
        for arm in ((device, host) if r % 2 == 0 else (host, device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            (t_dev if arm is device else t_host).append((time.perf_counter() - t0) * 1e3)
    n_poly = sum(len(i) for im in polys for i in im)
    n_vert = sum(len(p) // 2 for im in polys for i in im for p in i)
    print("decode of %d images of %d x %d, %d instances each (%d polygons, %d vertices; %d pixels covered at least once)"
          % (a.images, S, S, a.instances, n_poly, n_vert, int(sum((x > 0).sum() for x in d))))
    print("wall ms per batch of %d images, %d alternating repetitions, synchronised: median (min .. max)" % (a.images, a.reps))
    print("  device  %9.3f  (%.3f .. %.3f)" % (med(t_dev), min(t_dev), max(t_dev)))
    print("  host    %9.3f  (%.3f .. %.3f)   numpy frPolygons + decode + sum + upload" % (med(t_host), min(t_host), max(t_host)))
    print("  host / device = %.1f" % (med(t_host) / med(t_dev)))

    # the two library calls alone, all images' instances in one call each, by device events
    xy, off, rng = [], [0], []
    for im in polys:
        for inst in im:
            b = len(off) - 1
            for p in inst:
                xy.append(p)
                off.append(off[-1] + len(p) // 2)
            rng.append([b, len(off) - 1])
    xy = torch.from_numpy(np.concatenate(xy)).to(dev)
    off = torch.tensor(off, dtype=torch.int32, device=dev)
    rng = torch.tensor(rng, dtype=torch.int32, device=dev)
    G, NP, nw = rng.shape[0], off.numel() - 1, (S * S + 63) // 64
    img_off = [i * a.instances for i in range(a.images + 1)]
    words, _ = _hip.polygon_mask_words(xy, off, rng, S, S)
    _hip.mask_words_integral(words, img_off, S, S)
    torch.cuda.synchronize()
    t_w, t_i = [], []
    for _ in range(a.reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        words, _ = _hip.polygon_mask_words(xy, off, rng, S, S)
        e[1].record()
        _hip.mask_words_integral(words, img_off, S, S)
        e[2].record()
        torch.cuda.synchronize()
        t_w.append(e[0].elapsed_time(e[1]) * 1e3)
        t_i.append(e[1].elapsed_time(e[2]) * 1e3)
    b_w = 2 * NP * nw * 8 + G * nw * 8
    b_i = G * nw * 8 + 4 * a.images * S * S
    rate = a.hbm_tbs * 1e12
    print("library calls alone (G = %d instances, NP = %d polygons in one call), device events, us: median (min .. max)" % (G, NP))
    print("  mmt_polygon_mask_words   %9.1f  (%.1f .. %.1f)   byte bound %6.1f us: %.1f MB = planes cleared and read once + words "
          "written, at %.2f TB/s -> %.1f %% of the bound's rate"
          % (med(t_w), min(t_w), max(t_w), b_w / rate * 1e6, b_w / 1e6, a.hbm_tbs, 100 * (b_w / rate * 1e6) / med(t_w)))
    print("    (five launches and an allocation of the workspace; the call reads the polygon ranges back once, so the span holds one "
          "wait for the stream)")
    print("  mmt_mask_words_integral  %9.1f  (%.1f .. %.1f)   byte bound %6.1f us: %.1f MB = words read once + int32 map written "
          "-> %.1f %% of the bound's rate"
          % (med(t_i), min(t_i), max(t_i), b_i / rate * 1e6, b_i / 1e6, 100 * (b_i / rate * 1e6) / med(t_i)))


if __name__ == "__main__":
    main()
