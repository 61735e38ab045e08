"""ms/step of the bench's full-size mean-teacher step with MODEL.BACKBONE.FREEZE_CONV_BODY_AT 2 (the default), 1 and 0: three
trainers in one process, the arms alternating.
  python freeze_steps.py [rounds]
The arm at 2 is the step bench.py times; what 1 and 0 cost beyond it is the backward of layer1 and of the stem.  Whether the arm at
2 is still the parent commit's step is a comparison of two checkouts: tools/bench_ab.py, run in the same session; the outputs of both
make up profiles/freeze_at_steps.txt."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
import bench
import maskrcnn_benchmark.config as C
from maskrcnn_benchmark import _hip as H

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda", 0)
_default = C.make_default_cfg
arms = {}
for fa in (2, 1, 0):
    def with_key(fa=fa):
        cfg = _default()
        cfg.merge_from_list(["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", fa])
        return cfg
    C.make_default_cfg = with_key
    try:
        arms[fa] = bench.build(dev, 0, base_lr=bench.BENCH_BASE_LR)
    finally:
        C.make_default_cfg = _default
cfg = arms[2][0]
it = cfg.MT.START_MT + cfg.MT.RAMPUP_STEP + 100


def step(fa, it):
    _, trainer, batch = arms[fa]
    il, tg, ul = batch()
    return trainer.train_step(it, il, tg, ul)


for _ in range(4):   # warm-up: plans, planes, allocator
    for fa in (2, 1, 0):
        step(fa, it)
        it += 1
torch.cuda.synchronize()
for fa in (2, 1, 0):
    n0 = H.C_CALLS[0]
    step(fa, it)
    it += 1
    torch.cuda.synchronize()
    print("FREEZE_CONV_BODY_AT=%d library calls per step: %d" % (fa, H.C_CALLS[0] - n0))
ms = {2: [], 1: [], 0: []}
orders = ((2, 1, 0), (0, 1, 2), (1, 0, 2), (2, 0, 1))
for r in range(rounds):
    for fa in orders[r % len(orders)]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(fa, it)
        torch.cuda.synchronize()
        ms[fa].append((time.perf_counter() - t0) * 1e3)
        it += 1
for fa, v in ms.items():
    print("FREEZE_CONV_BODY_AT=%d ms/step over %d steps: median %.2f  min %.2f  max %.2f  (spread max-min %.2f)"
          % (fa, len(v), statistics.median(v), min(v), max(v), max(v) - min(v)))
