"""ms/step of the bench's full-size mean-teacher step with MT.AUG_S = 1 and AUG_S = 2, alternating in one process, and the MGD
launches per step for each value (C-ABI calls by symbol: mmt_mgd_level_* for AUG_S = 1, mmt_mgd_views_* beyond).
  python aug_s_steps.py [rounds] [--no-timing]
--no-timing: two steps per value and the call counts only (the form to run under `rocprofv3 --kernel-trace --stats`)."""
import collections
import os
import statistics
import sys
import time

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
import bench
import synthetic
from maskrcnn_benchmark import _hip as H
from maskrcnn_benchmark.structures.image_list import to_image_list

args = [a for a in sys.argv[1:] if not a.startswith("--")]
timing = "--no-timing" not in sys.argv
rounds = int(args[0]) if args else 10
dev = torch.device("cuda", 0)
cfg, trainer, batch = bench.build(dev, 0, base_lr=bench.BENCH_BASE_LR)
unl2 = [u.to(dev) for u in synthetic.make_unlabeled(bench.N_UNLAB, bench.CROP, cfg.MT.AUG_K + 2, seed=4321)]
it0 = cfg.MT.START_MT + cfg.MT.RAMPUP_STEP + 100


def step(s, it):
    cfg.MT.AUG_S = trainer.student_bs = s
    il, tg, ul = batch()
    if s != 1:
        ul = [to_image_list(list(u), cfg.DATALOADER.SIZE_DIVISIBILITY) for u in unl2]
    return trainer.train_step(it, il, tg, ul)


hist = collections.Counter()
_orig = H._check


def _counting(code, what):
    if "mgd" in what or what == "mmt_mask_pool":
        hist[what] += 1
    return _orig(code, what)


it = it0
for s in (1, 2) * (2 if timing else 1):   # warm-up: plans, planes, allocator
    step(s, it)
    it += 1
torch.cuda.synchronize()
H._check = _counting
for s in (1, 2):
    hist.clear()
    step(s, it)
    it += 1
    torch.cuda.synchronize()
    print("AUG_S=%d MGD-related C-ABI calls per step: %s" % (s, dict(sorted(hist.items()))))
H._check = _orig
if not timing:
    sys.exit(0)
ms = {1: [], 2: []}
for r in range(rounds):
    for s in ((1, 2) if r % 2 == 0 else (2, 1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(s, it)
        torch.cuda.synchronize()
        ms[s].append((time.perf_counter() - t0) * 1e3)
        it += 1
for s, v in ms.items():
    print("AUG_S=%d ms/step over %d steps: median %.2f  min %.2f  max %.2f  (spread max-min %.2f)"
          % (s, len(v), statistics.median(v), min(v), max(v), max(v) - min(v)))
