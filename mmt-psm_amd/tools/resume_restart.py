"""What a checkpoint costs the steps behind it in deterministic mode ("Resuming a run"): there `save_model` makes the
checkpoint a restart point -- it drops the adaptive arithmetic state (`_hip.reset_adaptive_state`), so the next steps run the split
passes of a site's first step again and the teacher's launch plan is run plain, plain, recorded before it is replayed.
  python resume_restart.py [reps] [out]
The bench's trainer at full size (2 + 2 crops of 1000 x 1000, learning rate 0: every step is the same step), the mode on.  `reps` (4)
repetitions, the two arms alternating: ten timed steps, `save_model` into a temporary directory, three timed steps.  Per repetition the
median of the ten steps before and each of the three after; then the medians over the repetitions.  The time of the save itself
(state dicts, device-to-host copies, the file) is printed beside them, not mixed in.  `out`: a file the lines are also written to."""
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, ROOT)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
out_path = sys.argv[2] if len(sys.argv) > 2 else None
BEFORE, AFTER, WARMUP = 10, 3, 6

import bench
from maskrcnn_benchmark import _hip as H
from maskrcnn_benchmark.utils.checkpoint import Checkpointer

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


H.set_deterministic(True)
cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, base_lr=bench.BENCH_BASE_LR)
save_dir = tempfile.mkdtemp(prefix="resume_restart_")
trainer.ckpt_s = Checkpointer(trainer.student, trainer.optimizer, trainer.scheduler, save_dir=save_dir, save_to_disk=True)
trainer.ckpt_t = Checkpointer(trainer.teacher, save_dir=save_dir, save_to_disk=True)
it = [cfg.MT.START_MT + cfg.MT.RAMPUP_STEP + 100]


def step():
    il, tg, ul = batch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train_step(it[0], il, tg, ul)
    torch.cuda.synchronize()
    it[0] += 1
    return (time.perf_counter() - t0) * 1e3


try:
    for _ in range(WARMUP):      # (launch plans: plain, plain, recorded, replayed)
        step()
    before, after, saves = [], [[] for _ in range(AFTER)], []
    for r in range(reps):
        b = [step() for _ in range(BEFORE)]
        t0 = time.perf_counter()
        trainer.save_model(it[0] - 1)
        torch.cuda.synchronize()
        saves.append(time.perf_counter() - t0)
        a = [step() for _ in range(AFTER)]
        before.append(statistics.median(b))
        for k, v in enumerate(a):
            after[k].append(v)
        say("repetition %d: ten steps before the save: median %.2f ms (min %.2f, max %.2f); save_model %.2f s; steps after: %s ms"
            % (r, before[-1], min(b), max(b), saves[-1], "  ".join("%.2f" % v for v in a)))
        for f in os.listdir(save_dir):
            os.remove(os.path.join(save_dir, f))
    base = statistics.median(before)
    say("deterministic mode, bench size, %d repetitions: step before a save %.2f ms (median of the repetitions' medians)" % (reps, base))
    for k in range(AFTER):
        m = statistics.median(after[k])
        say("  step %d after the save: median %.2f ms (min %.2f, max %.2f): %+.2f ms" % (k + 1, m, min(after[k]), max(after[k]), m - base))
    say("  the three steps together: %+.2f ms per checkpoint; save_model itself: median %.2f s; consistency branch skipped in %d steps"
        % (sum(statistics.median(after[k]) - base for k in range(AFTER)), statistics.median(saves), trainer.skipped_pairs))
finally:
    H.set_deterministic(False)
    shutil.rmtree(save_dir, ignore_errors=True)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
