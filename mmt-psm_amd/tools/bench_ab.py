"""`python bench.py` of two checkouts of this repository measured ALTERNATELY in one session (each run a fresh child process), to
compare a commit's headline step with its parent's: both built beforehand, one of them this checkout.
  python bench_ab.py OTHER_CHECKOUT [rounds] [steps] [warmup]
Prints every run's median ms/step and, per checkout, the median over its runs and their run-to-run spread (max - min).  A change
that is meant to leave the default step alone shows a median of this checkout inside the other's spread."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
other = os.path.abspath(sys.argv[1])
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 10
arms = (("other", other), ("this", HERE))
ms = {name: [] for name, _ in arms}
for r in range(rounds):
    for name, root in (arms if r % 2 == 0 else arms[::-1]):
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=root,
                             capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit("bench.py failed in %s:\n%s" % (root, out.stderr[-2000:]))
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        ms[name].append(line["median_ms_per_step"])
        print("round %d  %-5s median %.3f ms/step  mean %.3f  p10..p90 %s  (%d steps after %d)"
              % (r, name, line["median_ms_per_step"], line["ms_per_step"], line["p10_p90_ms_per_step"], steps, warmup), flush=True)
for name, _ in arms:
    v = ms[name]
    print("%-5s checkout: median of %d runs %.3f ms/step, min %.3f, max %.3f, run-to-run spread (max - min) %.3f"
          % (name, len(v), statistics.median(v), min(v), max(v), max(v) - min(v)))
