"""Worker of tests/test_deterministic_step_gpu.py and tools/det_steps.py: ONE fresh process that builds the bench's trainer from seed 0,
switches deterministic mode on (unless --off), takes a few mean-teacher steps and prints a SHA-256 of the student's flat buffer, its
momentum buffer, the teacher's flat buffer and the loss dict after every step -- two runs of it are compared line by line.

Usage: python tests/det_worker.py [--crop 160] [--n-inst 4] [--steps 3] [--mode 3] [--irnet] [--off]
(MMT_OVERLAP_TEACHER=0 in the environment selects the serial schedule, as everywhere)"""
import argparse
import hashlib
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, ROOT)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def state_digests(trainer, losses):
    """-> [(name, sha256)] of everything the guarantee covers"""
    blob = b"".join(k.encode() + struct.pack("<f", float(v)) for k, v in sorted(losses.items()))
    return [("student", digest(trainer.flat_s.data)), ("momentum", digest(trainer.flat_s.momentum)),
            ("teacher", digest(trainer.flat_t.data)), ("losses", hashlib.sha256(blob).hexdigest())]


def run(crop, n_inst, steps, mode, irnet, on, base_lr=0.005):
    """-> per step [(name, sha256)] (and the names of the step's losses: was the mean-teacher branch active?): a trainer built from
    seed 0, `steps` steps from iteration START_MT + 400"""
    import bench
    from maskrcnn_benchmark import _hip as H
    H.set_deterministic(on)
    H.set_conv_precision(mode)
    torch.manual_seed(0)
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, irnet=irnet, crop=crop, n_inst=n_inst, base_lr=base_lr)
    trainer.seed_rng(0)
    out = []
    for i in range(steps):
        il, tg, ul = batch()
        losses = trainer.train_step(cfg.MT.START_MT + 400 + i, il, tg, ul)
        torch.cuda.synchronize()
        out.append(state_digests(trainer, losses) + [("loss-names", ",".join(sorted(losses)))])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crop", type=int, default=160)
    ap.add_argument("--n-inst", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--mode", type=int, default=3)
    ap.add_argument("--irnet", action="store_true")
    ap.add_argument("--off", action="store_true", help="the default mode (for comparison: do two runs differ?)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for i, row in enumerate(run(a.crop if a.crop else None, a.n_inst if a.n_inst else None, a.steps, a.mode, a.irnet, not a.off)):
        for name, h in row:
            print("DIGEST step %d %s %s" % (i, name, h), flush=True)


if __name__ == "__main__":
    main()
