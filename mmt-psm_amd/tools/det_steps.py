"""Deterministic mode at bench size: is a run repeatable, and what does the mode cost?
  python det_steps.py [steps] [timed] [--set KEY VALUE]...
--set merges configuration keys into the defaults of both parts (the children are then tests/det_cfg_worker.py, which takes the same
pairs): `--set MODEL.BACKBONE.FREEZE_CONV_BODY_AT 0` measures the mode with a trainable stem.  A configuration the mode refuses ends
part 1 with the refusal's message.
1. tests/det_worker.py -- the bench's trainer (2 + 2 crops of 1000 x 1000, BASE_LR 0.005, seed 0), `steps` (10) mean-teacher steps with the
   mode on -- twice, as fresh child processes one after the other; the per-step SHA-256 digests of the student's flat buffer, its
   momentum, the teacher's flat buffer and the losses side by side, and the first step that differs, if any.  Acceptance: none.
2. One trainer in this process (the bench's learning rate of 0: every step is the same step), the mode switched off / on from step to
   step: `timed` (12) steps of each, median and spread of the wall time per step."""
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
argv, keys = sys.argv[1:], []
while "--set" in argv:
    i = argv.index("--set")
    if len(argv) < i + 3:
        raise SystemExit("--set takes a key and a value")
    keys += argv[i + 1:i + 3]
    del argv[i:i + 3]
steps = int(argv[0]) if len(argv) > 0 else 10
timed = int(argv[1]) if len(argv) > 1 else 12

worker = [os.path.join(ROOT, "tests", "det_cfg_worker.py")] + [a for k, v in zip(keys[0::2], keys[1::2]) for a in ("--set", k, v)] if keys \
    else [os.path.join(ROOT, "tests", "det_worker.py")]
runs = []
for r in range(2):
    out = subprocess.run([sys.executable] + worker + ["--crop", "0", "--n-inst", "0", "--steps", str(steps)],
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:   # (the second child is not started after a first that failed)
        raise SystemExit("run %d ended with exit status %d:\n%s" % (r, out.returncode, out.stderr[-3000:]))
    runs.append([l.split()[1:] for l in out.stdout.splitlines() if l.startswith("DIGEST ")])
first = None
for a, b in zip(*runs):
    same = a == b
    if a[2] == "loss-names":
        print("step %2s %-10s %s" % (a[1], a[2], a[3] if same else "%s | %s" % (a[3], b[3])))
    else:
        print("step %2s %-10s %s %s %s" % (a[1], a[2], a[3][:16], b[3][:16], "==" if same else "DIFFERENT"))
    if not same and first is None:
        first = int(a[1])
print("two fresh processes, %d steps at bench size, mode on: %s" % (steps, "identical" if first is None and len(runs[0]) == len(runs[1]) == 5 * steps
                                                                   else "FIRST DIFFERENCE at step %s" % first), flush=True)

import bench
from det_cfg_worker import default_cfg_with
from maskrcnn_benchmark import _hip as H
with default_cfg_with(keys):
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, base_lr=bench.BENCH_BASE_LR)
it0 = cfg.MT.START_MT + cfg.MT.RAMPUP_STEP + 100
ms = {False: [], True: []}
calls = {}
for i in range(2 * (timed + 4)):
    on = bool(i % 2)
    H.set_deterministic(on)
    il, tg, ul = batch()
    torch.cuda.synchronize()
    c0, t0 = H.C_CALLS[0], time.perf_counter()
    trainer.train_step(it0 + i, il, tg, ul)
    torch.cuda.synchronize()
    if i >= 8:                      # four warm-up steps of each arm (launch plans: plain, recorded, replayed)
        ms[on].append((time.perf_counter() - t0) * 1e3)
        calls[on] = H.C_CALLS[0] - c0
H.set_deterministic(False)
for on in (False, True):
    v = ms[on]
    print("mode %-3s ms/step over %d alternating steps: median %.2f  min %.2f  max %.2f  (spread max-min %.2f); library calls per step %d"
          % ("on" if on else "off", len(v), statistics.median(v), min(v), max(v), max(v) - min(v), calls[on]))
print("cost of the mode: %+.2f ms/step (difference of the medians); consistency branch skipped in %d steps" %
      (statistics.median(ms[True]) - statistics.median(ms[False]), trainer.skipped_pairs))
