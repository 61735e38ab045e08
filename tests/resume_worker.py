"""Worker of tests/test_resume_gpu.py: ONE fresh process, deterministic mode, the bench's trainer at 160 x 160 with checkpointers on DIR.
  straight   steps 1..4 from iteration START_MT + 400, `save_model` after step 2
  resume     a trainer seeded differently calls `resume()` on DIR and takes steps 3 and 4
Both print, per step, the SHA-256 lines of det_worker.py (student, momentum, teacher, losses): the lines of steps 3 and 4 are compared.

Usage: python tests/resume_worker.py DIR straight|resume [--irnet]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS, SAVE_AFTER = 4, 2


def build(save_dir, irnet):
    import bench
    from maskrcnn_benchmark.utils.checkpoint import Checkpointer
    cfg, trainer, batch = bench.build(torch.device("cuda", 0), 0, irnet=irnet, crop=160, n_inst=4, base_lr=0.005)
    trainer.ckpt_s = Checkpointer(trainer.student, trainer.optimizer, trainer.scheduler, save_dir=save_dir, save_to_disk=True)
    trainer.ckpt_t = Checkpointer(trainer.teacher, save_dir=save_dir, save_to_disk=True)
    return cfg, trainer, batch


def main():
    from det_worker import state_digests
    from maskrcnn_benchmark import _hip as H
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("phase", choices=("straight", "resume"))
    ap.add_argument("--irnet", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    H.set_deterministic(True)
    first = cfg = None
    if a.phase == "straight":
        torch.manual_seed(0)
        cfg, trainer, batch = build(a.dir, a.irnet)
        trainer.seed_rng(0)
        first, step0 = cfg.MT.START_MT + 400, 1
    else:
        torch.manual_seed(123)
        cfg, trainer, batch = build(a.dir, a.irnet)
        trainer.seed_rng(7)
        at = trainer.resume()
        assert at == cfg.MT.START_MT + 400 + SAVE_AFTER - 1 and trainer.start_iter == at + 1, (at, trainer.start_iter)
        first, step0 = cfg.MT.START_MT + 400, SAVE_AFTER + 1
    for step in range(step0, STEPS + 1):
        il, tg, ul = batch()
        iteration = first + step - 1
        losses = trainer.train_step(iteration, il, tg, ul)
        torch.cuda.synchronize()
        for name, h in state_digests(trainer, losses) + [("loss-names", ",".join(sorted(losses)))]:
            print("DIGEST step %d %s %s" % (step, name, h), flush=True)
        if a.phase == "straight" and step == SAVE_AFTER:
            trainer.save_model(iteration)


if __name__ == "__main__":
    main()
