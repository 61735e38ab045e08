"""What the guarded optimiser step (SOLVER.GRAD_GUARD) costs at bench size.
  python mmt-psm_amd/tools/grad_guard_steps.py [--timed 25] [--max-norm 0.0] [--out profiles/grad_guard.txt]
1. One trainer (the bench's: 2 + 2 crops of 1000 x 1000, the bench's learning rate of 0 -- every step is the same step), the guard
   switched off / on from step to step after four warm-up steps of each arm: --timed steps of each, host clock around a device
   synchronise; median, minimum, quartiles, maximum, and the library calls per step.
2. The guard's own two launches alone on that trainer's flat gradient: device time between events around 10 calls, 20 repetitions,
   against the time one read of the gradient takes at the 6.3 TB/s a copy reaches (profiles/paste_words.txt).  The buffer is the one
   the step's backward has just written; a 176 MB gradient read over and over can be served in part by the 256 MB last-level cache.
3. The plain and the guarded SGD kernel alone on the weight region, the same way.
Prints the report and writes it to --out.
  rocprofv3 --kernel-trace --stats -d DIR -- python mmt-psm_amd/tools/grad_guard_steps.py --kernels 12
--kernels N: nothing is timed or written; N rounds of grad_guard, sgd_momentum, sgd_momentum_guarded on the trainer's flat gradient, for a
kernel trace (a run of its own)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, ROOT)
COPY_TBS = 6.3   # profiles/paste_words.txt

ap = argparse.ArgumentParser()
ap.add_argument("--timed", type=int, default=25)
ap.add_argument("--max-norm", type=float, default=0.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard.txt"))
ap.add_argument("--kernels", type=int, default=0)
args = ap.parse_args()

import bench
from maskrcnn_benchmark import _hip as H

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def row(name, v):
    q = statistics.quantiles(v, n=4)
    say("%-34s %10.3f %10.3f %10.3f %10.3f %10.3f" % (name, statistics.median(v), min(v), q[0], q[2], max(v)))


cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, base_lr=bench.BENCH_BASE_LR)
opt, flat = trainer.optimizer, trainer.flat_s
opt.enable_guard(max_norm=args.max_norm)
guard = opt.guard
if args.kernels:
    flat.grad.normal_()
    nw = flat.n_weights
    p, buf = flat.data[:nw].clone(), flat.momentum[:nw].clone()    # copies: the trainer's weights stay as they are
    for _ in range(args.kernels):
        H.grad_guard(flat.grad, guard["state"], guard["ws"], args.max_norm)
        H.sgd_momentum(p, flat.grad[:nw], buf, 0.0, 1e-4, 0.9, False)
        H.sgd_momentum_guarded(p, flat.grad[:nw], buf, 0.0, 1e-4, 0.9, False, guard["state"])
    torch.cuda.synchronize()
    print("%d rounds on %d fp32: %s" % (args.kernels, flat.grad.numel(), opt.guard_stats()))
    raise SystemExit(0)
it0 = cfg.MT.START_MT + cfg.MT.RAMPUP_STEP + 100
ms, calls = {False: [], True: []}, {}
for i in range(2 * (args.timed + 4)):
    on = bool(i % 2)
    opt.guard = guard if on else None
    il, tg, ul = batch()
    torch.cuda.synchronize()
    c0, t0 = H.C_CALLS[0], time.perf_counter()
    trainer.train_step(it0 + i, il, tg, ul)
    torch.cuda.synchronize()
    if i >= 8:                      # four warm-up steps of each arm (launch plans: plain, recorded, replayed)
        ms[on].append((time.perf_counter() - t0) * 1e3)
        calls[on] = H.C_CALLS[0] - c0
opt.guard = guard
stats = opt.guard_stats()
n = flat.grad.numel()
say("Guarded optimiser step (SOLVER.GRAD_GUARD, MAX_NORM %g) against the plain one; tools/grad_guard_steps.py" % args.max_norm)
say("one MI355X, the bench's trainer (2 + 2 crops of 1000 x 1000, learning rate 0), flat gradient of %d fp32 = %.1f MB; the guard "
    "switched" % (n, n * 4 / 1e6))
say("off / on from step to step, %d timed steps of each after 4 warm-up steps of each; host clock around a device synchronise" % args.timed)
say("guard after the run: %d steps seen, %d skipped, %d clipped, last norm %.6g; consistency branch skipped in %d steps"
    % (stats["seen"], stats["skipped"], stats["clipped"], stats["norm"], trainer.skipped_pairs))
say("%-34s %10s %10s %10s %10s %10s" % ("ms per step", "median", "min", "q25", "q75", "max"))
row("guard off (%d library calls)" % calls[False], ms[False])
row("guard on  (%d library calls)" % calls[True], ms[True])
m0, m1 = statistics.median(ms[False]), statistics.median(ms[True])
spread = lambda v: 100.0 * (statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0]) / statistics.median(v)
say("guard on - off = %+.3f ms/step (medians, %+.2f %%); run-to-run spread (q75 - q25) / median: off %.1f %%, on %.1f %%"
    % (m1 - m0, 100.0 * (m1 - m0) / m0, spread(ms[False]), spread(ms[True])))


def device_us(fn, inner=10, reps=20):
    """-> per-call device times in us: events around `inner` calls, `reps` times, after a warm-up round"""
    out = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        if r:
            out.append(a.elapsed_time(b) * 1e3 / inner)
    return out


bound = n * 4 / (COPY_TBS * 1e12) * 1e6
say("the guard's two launches alone (device time between events, 10 calls, 20 repetitions); bytes the algorithm reads: %.1f MB = "
    "%.1f us at %.1f TB/s" % (n * 4 / 1e6, bound, COPY_TBS))
say("%-34s %10s %10s %10s %10s %10s" % ("us per call", "median", "min", "q25", "q75", "max"))
v = device_us(lambda: H.grad_guard(flat.grad, guard["state"], guard["ws"], args.max_norm))
row("grad_guard (sum of squares + finish)", v)
say("grad_guard / byte bound = %.2f (median); %.2f TB/s read" % (statistics.median(v) / bound, n * 4 / statistics.median(v) / 1e6))
nw = flat.n_weights
p, g, buf = flat.data[:nw].clone(), flat.grad[:nw], flat.momentum[:nw].clone()    # copies: the trainer's weights stay as they are
plain = device_us(lambda: H.sgd_momentum(p, g, buf, 0.0, 1e-4, 0.9, False))
guarded = device_us(lambda: H.sgd_momentum_guarded(p, g, buf, 0.0, 1e-4, 0.9, False, guard["state"]))
row("sgd_momentum, %.1f MB x 5" % (nw * 4 / 1e6), plain)
row("sgd_momentum_guarded, the same", guarded)
say("guarded - plain SGD kernel = %+.1f us (medians)" % (statistics.median(guarded) - statistics.median(plain)))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
