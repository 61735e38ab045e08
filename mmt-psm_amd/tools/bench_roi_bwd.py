"""Isolated device time of the ROIAlign backward: the scatter form (fp32 atomics, plus the clear it needs) against the ordered tile-gather
form of deterministic mode (mmt_roi_align_backward_ordered), on calls shaped like the bench's box head (1024 ROIs, 7 x 7) and mask head
(256 ROIs, 14 x 14) over a 256-channel pyramid of 2 images (256^2 ... 32^2), with the ROIs spread over the image and with 80 % of them
clustered in one 160 x 160-pixel window.  10 launches per event pair, median of 20 (as tools/bench_gconv.py).
  python bench_roi_bwd.py"""
import os
import statistics
import sys

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
from maskrcnn_benchmark import _hip as H

N, C = 2, 256
shapes = [(N, C, 256 >> l, 256 >> l) for l in range(4)]
scales = [0.25 / (1 << l) for l in range(4)]


def rois_of(K, clustered, g):
    xy = torch.rand(K, 2, generator=g) * 900
    wh = torch.rand(K, 2, generator=g) * 300 + 8
    n = int(0.8 * K) if clustered else 0
    xy[:n] = 400 + torch.rand(n, 2, generator=g) * 100
    wh[:n] = 16 + torch.rand(n, 2, generator=g) * 44
    boxes = torch.cat([xy, xy + wh], 1)
    img = (torch.arange(K) % N).float()
    img[:n] = 0.
    area = (wh[:, 0] * wh[:, 1]).sqrt()
    lv = torch.floor(4 + torch.log2(area / 224 + 1e-6)).clamp(2, 5).long() - 2
    return torch.cat([img[:, None], boxes], 1).cuda(), lv.int().cuda()


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    return statistics.median(ms)


g = torch.Generator().manual_seed(0)
for name, K, res in (("box head", 1024, 7), ("mask head", 256, 14)):
    for clustered in (False, True):
        rois, lv = rois_of(K, clustered, g)
        go = torch.randn(K, C, res, res, generator=g).cuda().contiguous(memory_format=torch.channels_last)
        H.set_deterministic(False)
        t_sc = timed(lambda: H.roi_align_backward(go, shapes, scales, rois, lv, res, res, 2))
        H.set_deterministic(True)
        t_or = timed(lambda: H.roi_align_backward(go, shapes, scales, rois, lv, res, res, 2))
        H.set_deterministic(False)
        print("%-9s K=%4d %2dx%-2d %-9s  scatter (clear + atomics) %.3f ms   ordered tile gather %.3f ms"
              % (name, K, res, res, "clustered" if clustered else "spread", t_sc, t_or), flush=True)
